// fused_emit_v2.hip -- V2 (nerf_mlp.NeRFMLP, pos_freq 10): the renderer that also emits each sample's raw head outputs (fused_impl.hpp: render_emit_kernel)
#include "fused_impl.hpp"

namespace nrf {

int NRF_TU_NAME(render_emit_v2)(const DeviceNet& net, int mode, const RenderArgs& a, float* raw4, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_render_emit, NRF_NET_V2_10, 10, net, mode, a, raw4, s, err) }

}  // namespace nrf
