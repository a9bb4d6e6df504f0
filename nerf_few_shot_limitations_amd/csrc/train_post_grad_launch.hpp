// train_post_grad_launch.hpp -- the host side shared by the launchers of the post-chain gradient kernels
// (train_dino_grad.hip, train_input_grad.hip, train_input_grad_v3.hip): the opening of a launch_* function, the mode switch and
// the launch itself.  Device side: train_post_grad_core.hpp.
#pragma once
#include "train_post_grad_core.hpp"

namespace nrf {

namespace {

// What the opening of a launch_* function leaves: the mode's rider stream, the context's slot offsets for n samples and the
// 32-sample tiles that hold a sample (0: nothing to do).
struct PostGradOpening {
    const void* wstream = nullptr;
    TrainKArgs k{};
    int64_t n_tiles = 0;
};

// The opening of launch_*: the training path's own checks, the family's (`refusal`: its message, or NULL), the rider streams of
// the three modes (`unprepared`: the message where the mode's is missing), n <= 0, the slot offsets.
int open_post_grad(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, const char* refusal, const void* const (&streams)[3],
                   const char* unprepared, PostGradOpening& o, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return NRF_EINVAL;
    if (refusal) { err = refusal; return NRF_EINVAL; }
    if (!streams[mode]) { err = unprepared; return NRF_EINVAL; }
    if (n <= 0) return NRF_OK;
    if (!fill_slots(t, mode, n, o.k, err)) return NRF_EINVAL;
    o.wstream = streams[mode];
    o.n_tiles = (n + 31) / 32;          // not tiles32(n): that is the context's layout, whole 256-sample groups, and would walk dead tiles
    return NRF_OK;
}

template <class M>
struct ModeTag {
    typedef M Mode;
};

// f(ModeTag<Mode>{}) for the MFMA mode of the call
template <class F>
int dispatch_post_grad(int mode, F&& f) {
    switch (mode) {
        case NRF_MMA_BF16: return f(ModeTag<ModeBF16>{});
        case NRF_MMA_F16:  return f(ModeTag<ModeF16>{});
        default:           return f(ModeTag<ModeF32>{});
    }
}

// Persistent workgroups of kPostGradWaves waves over a.n_tiles 32-sample tiles, one tile per wave and trip: two workgroups per CU
// where two sets of resident fragments fit in the LDS comfortably, one where the fragments take most of it.  A template per
// kernel, so that each keeps its own once-per-device attribute cache (prepare).
template <auto kernel, int LDS, class Args>
int run_post_grad(const DeviceNet& net, const Args& a, hipStream_t s, const char* what, std::string& err) {
    static unsigned char done[64] = {};
    const int prepared = prepare(kernel, net.device, done, err, LDS);
    if (prepared != NRF_OK) return prepared;
    const int64_t want = (a.n_tiles + kPostGradWaves - 1) / kPostGradWaves;
    const int64_t room = (int64_t)net.cu_count * (LDS <= 64 * 1024 ? 2 : 1);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(want < room ? want : room)), dim3(kPostGradWaves * 64), LDS, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string(what) + " launch: " + hipGetErrorString(e); return NRF_EHIP; }
    return NRF_OK;
}

}  // namespace

}  // namespace nrf
