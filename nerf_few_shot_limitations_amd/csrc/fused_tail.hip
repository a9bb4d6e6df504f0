// fused_tail.hip -- tail mode: the split-f16 launch that adds every ray's last sample to the state a 16-bit prefix launch carried
// (fused_impl.hpp: render_march<kTail>), one instantiation per network family
#include "fused_impl.hpp"

namespace nrf {

#define NRF_DEFINE_TAIL(fam, NETT, LP)                                                                                   \
    int render_tail_##fam(const DeviceNet& net, const RenderArgs& a, float* carry, hipStream_t s, std::string& err) {     \
        return run_render_tail<NETT(ModeF16X3, 1), ModeF16X3, 1, 4, LP, 4>(net, NRF_MMA_F16X3, a, carry, s, err);         \
    }
NRF_DEFINE_TAIL(v1, NRF_NET_V1_10, 10)
NRF_DEFINE_TAIL(v2, NRF_NET_V2_10, 10)
NRF_DEFINE_TAIL(v3, NRF_NET_V3_12_64, 12)
NRF_DEFINE_TAIL(v3w, NRF_NET_V3_12_128, 12)

}  // namespace nrf
