// fused_inst.hip -- every instantiation of the fused renderer / staged forward.  build.py compiles this file once per (kind, family,
// half): -DNRF_KIND=<kind> picks one of the bodies below, -DNRF_FAMILY=<name> the row of the family table (fused_impl.hpp) it is
// expanded with, the half's flags NRF_TU_HALF.  The tail kind is built with -DNRF_FAMILY=all: one object (fused_tail) holds all four.
#include "fused_impl.hpp"

namespace nrf {

// plain + ray queue (run_render picks by ert_eps) and the staged forward; in the 16-bit half also the tail mode's prefix launch
#if NRF_TU_HALF == 16
#define NRF_DEFINE_HOLD(fam, NETT, LP)                                                                                              \
    int render_hold_##fam##_16(const DeviceNet& net, int mode, const RenderArgs& a, float* carry, hipStream_t s, std::string& err) { \
        NRF_DISPATCH_MODE(run_render_hold, NETT, LP, net, mode, a, carry, s, err)                                                   \
    }
#else
#define NRF_DEFINE_HOLD(fam, NETT, LP)
#endif
#define NRF_KIND_plain(fam, NETT, LP, ...)                                                                                          \
    int NRF_TU_NAME(render_##fam)(const DeviceNet& net, int mode, const RenderArgs& a, hipStream_t s, std::string& err) {            \
        NRF_DISPATCH_MODE(run_render, NETT, LP, net, mode, a, s, err)                                                               \
    }                                                                                                                               \
    int NRF_TU_NAME(forward_##fam)(const DeviceNet& net, int mode, ForwardKArgs k, hipStream_t s, std::string& err) {                \
        NRF_DISPATCH_MODE(run_forward, NETT, LP, net, mode, k, s, err)                                                              \
    }                                                                                                                               \
    NRF_DEFINE_HOLD(fam, NETT, LP)
// the ray-queue renderer with empty-space skipping (render_queue_occ_kernel)
#define NRF_KIND_occ(fam, NETT, LP, ...)                                                                                                        \
    int NRF_TU_NAME(render_occ_##fam)(const DeviceNet& net, int mode, const RenderArgs& a, const OccDev& g, hipStream_t s, std::string& err) {   \
        NRF_DISPATCH_MODE(run_render_occ, NETT, LP, net, mode, a, g, s, err)                                                                    \
    }
// the renderer that also emits each sample's raw head outputs (render_emit_kernel)
#define NRF_KIND_emit(fam, NETT, LP, ...)                                                                                                       \
    int NRF_TU_NAME(render_emit_##fam)(const DeviceNet& net, int mode, const RenderArgs& a, float* raw4, hipStream_t s, std::string& err) {      \
        NRF_DISPATCH_MODE(run_render_emit, NETT, LP, net, mode, a, raw4, s, err)                                                                \
    }
// tail mode: the split-f16 launch that adds every ray's last sample to the state a 16-bit prefix launch carried (render_march<kTail>)
#define NRF_KIND_tail(fam, NETT, LP, ...)                                                                                \
    int render_tail_##fam(const DeviceNet& net, const RenderArgs& a, float* carry, hipStream_t s, std::string& err) {     \
        return run_render_tail<NETT(ModeF16X3, 1), ModeF16X3, 1, 4, LP, 4>(net, NRF_MMA_F16X3, a, carry, s, err);         \
    }

#define NRF_FAMILY_all(X) NRF_FAMILIES(X)
NRF_CAT(NRF_FAMILY_, NRF_FAMILY)(NRF_CAT(NRF_KIND_, NRF_KIND))

}  // namespace nrf
