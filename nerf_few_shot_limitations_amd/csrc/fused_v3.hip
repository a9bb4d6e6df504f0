// fused_v3.hip -- V3 (NeRFWithDINO, pos_freq 12, 64-d features) instantiations
#include "fused_impl.hpp"

namespace nrf {

int NRF_TU_NAME(render_v3)(const DeviceNet& net, int mode, const RenderArgs& a, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_render, NRF_NET_V3_12_64, 12, net, mode, a, s, err) }
int NRF_TU_NAME(forward_v3)(const DeviceNet& net, int mode, ForwardKArgs k, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_forward, NRF_NET_V3_12_64, 12, net, mode, k, s, err) }
NRF_DEFINE_HOLD(v3, NRF_NET_V3_12_64, 12)

}  // namespace nrf
