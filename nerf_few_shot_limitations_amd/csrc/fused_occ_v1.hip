// fused_occ_v1.hip -- V1 (nerf_model.NeRFMLP, pos_freq 10): the ray-queue renderer with empty-space skipping (fused_impl.hpp: render_queue_occ_kernel)
#include "fused_impl.hpp"

namespace nrf {

int NRF_TU_NAME(render_occ_v1)(const DeviceNet& net, int mode, const RenderArgs& a, const OccDev& g, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_render_occ, NRF_NET_V1_10, 10, net, mode, a, g, s, err) }

}  // namespace nrf
