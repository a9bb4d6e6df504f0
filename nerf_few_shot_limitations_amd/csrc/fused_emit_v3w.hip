// fused_emit_v3w.hip -- V3 with 128-d (multi-scale) features: the renderer that also emits each sample's raw head outputs (fused_impl.hpp: render_emit_kernel)
#include "fused_impl.hpp"

namespace nrf {

int NRF_TU_NAME(render_emit_v3w)(const DeviceNet& net, int mode, const RenderArgs& a, float* raw4, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_render_emit, NRF_NET_V3_12_128, 12, net, mode, a, raw4, s, err) }

}  // namespace nrf
