// train_dino_grad.hip -- host entry point of dino_grad_kernel (train_dino_grad_impl.hpp): the V3 network's gradient with
// respect to its per-sample DINO features
#include "train_dino_grad_impl.hpp"

namespace nrf {

namespace {

template <class Mode, int DT>
int run_dino_grad(const DeviceNet& net, const DinoGradArgs& a, hipStream_t s, std::string& err) {
    static unsigned char done[64] = {};
    constexpr int lds = dino_grad_lds_bytes<Mode, DT>();
    const int prepared = prepare(dino_grad_kernel<Mode, DT>, net.device, done, err, lds);
    if (prepared != NRF_OK) return prepared;
    // persistent workgroups: one per CU where the fragments take most of the LDS, two where two fit comfortably
    const int64_t want = (a.n_tiles + kDinoGradWaves - 1) / kDinoGradWaves;
    const int64_t room = (int64_t)net.cu_count * (lds <= 64 * 1024 ? 2 : 1);
    hipLaunchKernelGGL((dino_grad_kernel<Mode, DT>), dim3((unsigned)(want < room ? want : room)), dim3(kDinoGradWaves * 64), lds, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("dino grad launch: ") + hipGetErrorString(e); return NRF_EHIP; }
    return NRF_OK;
}

template <int DT>
int dispatch_dino_grad(const DeviceNet& net, int mode, const DinoGradArgs& a, hipStream_t s, std::string& err) {
    switch (mode) {
        case NRF_MMA_BF16: return run_dino_grad<ModeBF16, DT>(net, a, s, err);
        case NRF_MMA_F16:  return run_dino_grad<ModeF16, DT>(net, a, s, err);
        default:           return run_dino_grad<ModeF32, DT>(net, a, s, err);
    }
}

}  // namespace

int launch_dino_grad(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, void* ctx, float* d_dino, hipStream_t s, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return NRF_EINVAL;
    if (net.arch.net != NRF_NET_V3 || (net.arch.dino_dim != 64 && net.arch.dino_dim != 128)) {
        err = "the DINO feature gradient needs a V3 model with dino_dim 64 or 128";
        return NRF_EINVAL;
    }
    if (!t.gstream[mode]) { err = "model not prepared for the DINO feature gradient"; return NRF_EINVAL; }
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const SlotsV3 S{net.arch.n_layers};
    if (S.dz_fusion0(1) >= t.n_slots || t.slot_tiles[S.dz_fusion0(0)] != 8 || t.slot_tiles[S.dz_fusion0(1)] != 8) {
        err = "training plan: unexpected fusion.0 gradient slots";
        return NRF_EINVAL;
    }
    DinoGradArgs a{};
    a.wstream = t.gstream[mode];
    a.ctx = (const char*)ctx;
    a.dz1_off = k.slot_off[S.dz_fusion0(0)];
    a.dz2_off = k.slot_off[S.dz_fusion0(1)];
    a.aux_off = k.aux_off;
    a.n = n;
    a.n_tiles = (n + 31) / 32;
    a.d_dino = d_dino;
    return net.arch.dino_dim == 64 ? dispatch_dino_grad<2>(net, mode, a, s, err) : dispatch_dino_grad<4>(net, mode, a, s, err);
}

}  // namespace nrf
