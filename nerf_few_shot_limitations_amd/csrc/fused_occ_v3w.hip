// fused_occ_v3w.hip -- V3 with 128-d (multi-scale) features: the ray-queue renderer with empty-space skipping (fused_impl.hpp: render_queue_occ_kernel)
#include "fused_impl.hpp"

namespace nrf {

int NRF_TU_NAME(render_occ_v3w)(const DeviceNet& net, int mode, const RenderArgs& a, const OccDev& g, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_render_occ, NRF_NET_V3_12_128, 12, net, mode, a, g, s, err) }

}  // namespace nrf
