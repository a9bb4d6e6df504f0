// train_input_grad.hip -- host entry point of input_grad_kernel (train_input_grad_impl.hpp): the V1 and V2 networks' gradient
// with respect to their encoded inputs, positions and directions
#include "train_input_grad_impl.hpp"

namespace nrf {

namespace {

template <class Mode, bool V2>
int run_input_grad(const DeviceNet& net, const InputGradArgs& a, hipStream_t s, std::string& err) {
    static unsigned char done[64] = {};
    constexpr int lds = input_grad_lds_bytes<Mode, V2>();
    const int prepared = prepare(input_grad_kernel<Mode, V2>, net.device, done, err, lds);
    if (prepared != NRF_OK) return prepared;
    // persistent workgroups: two per CU where two fragment sets fit in the LDS, one otherwise
    const int64_t want = (a.n_tiles + kInputGradWaves - 1) / kInputGradWaves;
    const int64_t room = (int64_t)net.cu_count * (lds <= 64 * 1024 ? 2 : 1);
    hipLaunchKernelGGL((input_grad_kernel<Mode, V2>), dim3((unsigned)(want < room ? want : room)), dim3(kInputGradWaves * 64), lds, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("input grad launch: ") + hipGetErrorString(e); return NRF_EHIP; }
    return NRF_OK;
}

template <bool V2>
int dispatch_input_grad(const DeviceNet& net, int mode, const InputGradArgs& a, hipStream_t s, std::string& err) {
    switch (mode) {
        case NRF_MMA_BF16: return run_input_grad<ModeBF16, V2>(net, a, s, err);
        case NRF_MMA_F16:  return run_input_grad<ModeF16, V2>(net, a, s, err);
        default:           return run_input_grad<ModeF32, V2>(net, a, s, err);
    }
}

}  // namespace

int launch_input_grad(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, void* ctx, const float* positions, const float* directions,
                      float* d_x_enc, float* d_positions, float* d_directions, hipStream_t s, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return NRF_EINVAL;
    const bool v2 = net.arch.net == NRF_NET_V2;
    if (net.arch.net != NRF_NET_V1 && !v2) { err = "the input gradient is built for the V1 and V2 networks"; return NRF_EINVAL; }
    if (net.arch.pos_freq != kInputGradPosFreq || (v2 && (net.arch.dir_freq < 1 || net.arch.dir_freq > 4))) {
        err = "the input gradient is built for pos_freq 10 and dir_freq 1..4";
        return NRF_EINVAL;
    }
    if (!t.istream[mode]) { err = "model not prepared for the input gradient"; return NRF_EINVAL; }
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const int n_layers = net.arch.n_layers;
    const int dz0 = v2 ? SlotsV2{n_layers}.dz_trunk(0) : SlotsV1{n_layers}.dz_trunk(0);
    const int dzc = v2 ? SlotsV2{n_layers}.colour().dz_c0() : dz0;
    if (dz0 >= t.n_slots || dzc >= t.n_slots || t.slot_tiles[dz0] != 8 || (v2 && t.slot_tiles[dzc] != 4)) {
        err = "training plan: unexpected first-layer gradient slots";
        return NRF_EINVAL;
    }
    InputGradArgs a{};
    a.wstream = t.istream[mode];
    a.ctx = (const char*)ctx;
    a.dz0_off = k.slot_off[dz0];
    a.dzc_off = k.slot_off[dzc];
    a.n = n;
    a.n_tiles = (n + 31) / 32;
    a.positions = positions; a.directions = directions;
    a.d_x_enc = d_x_enc; a.d_positions = d_positions; a.d_directions = d_directions;
    a.dir_freq = net.arch.dir_freq;
    return v2 ? dispatch_input_grad<true>(net, mode, a, s, err) : dispatch_input_grad<false>(net, mode, a, s, err);
}

}  // namespace nrf
