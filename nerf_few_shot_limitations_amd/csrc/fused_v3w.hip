// fused_v3w.hip -- V3 with 128-d (multi-scale) features
#include "fused_impl.hpp"

namespace nrf {

int NRF_TU_NAME(render_v3w)(const DeviceNet& net, int mode, const RenderArgs& a, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_render, NRF_NET_V3_12_128, 12, net, mode, a, s, err) }
int NRF_TU_NAME(forward_v3w)(const DeviceNet& net, int mode, ForwardKArgs k, hipStream_t s, std::string& err) { NRF_DISPATCH_MODE(run_forward, NRF_NET_V3_12_128, 12, net, mode, k, s, err) }
NRF_DEFINE_HOLD(v3w, NRF_NET_V3_12_128, 12)

}  // namespace nrf
