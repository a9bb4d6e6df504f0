// train_input_grad_v3.hip -- host entry point of input_grad_v3_kernel (train_input_grad_v3_impl.hpp): the V3 network's gradient
// with respect to positions and directions through the positional encodings
#include "train_input_grad_v3_impl.hpp"

namespace nrf {

namespace {

template <class Mode, bool POS, bool DIR>
int run_input_grad_v3(const DeviceNet& net, const InputGradV3Args& a, hipStream_t s, std::string& err) {
    static unsigned char done[64] = {};
    constexpr int lds = input_grad_v3_lds_bytes<Mode>();
    const int prepared = prepare(input_grad_v3_kernel<Mode, POS, DIR>, net.device, done, err, lds);
    if (prepared != NRF_OK) return prepared;
    // persistent workgroups: two per CU where two fragment sets fit in the LDS, one otherwise
    const int64_t want = (a.n_tiles + kInputGradWaves - 1) / kInputGradWaves;
    const int64_t room = (int64_t)net.cu_count * (lds <= 64 * 1024 ? 2 : 1);
    hipLaunchKernelGGL((input_grad_v3_kernel<Mode, POS, DIR>), dim3((unsigned)(want < room ? want : room)), dim3(kInputGradWaves * 64), lds, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("V3 input grad launch: ") + hipGetErrorString(e); return NRF_EHIP; }
    return NRF_OK;
}

template <class Mode>
int run3(const DeviceNet& net, const InputGradV3Args& a, hipStream_t s, std::string& err) {
    if (a.d_positions && a.d_directions) return run_input_grad_v3<Mode, true, true>(net, a, s, err);
    if (a.d_positions) return run_input_grad_v3<Mode, true, false>(net, a, s, err);
    return run_input_grad_v3<Mode, false, true>(net, a, s, err);
}

}  // namespace

int launch_input_grad_v3(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, void* ctx, const float* positions, const float* directions,
                         float* d_positions, float* d_directions, hipStream_t s, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return NRF_EINVAL;
    if (net.arch.net != NRF_NET_V3) { err = "this input gradient is built for the V3 network"; return NRF_EINVAL; }
    if (net.arch.pos_freq != kInputGradV3PosFreq || net.arch.dir_freq < 1 || net.arch.dir_freq > 4) {
        err = "the V3 input gradient is built for pos_freq 12 and dir_freq 1..4";
        return NRF_EINVAL;
    }
    if (!t.istream[mode]) { err = "model not prepared for the input gradient"; return NRF_EINVAL; }
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const SlotsV3 S{net.arch.n_layers};
    const int dz1 = S.dz_fusion0(0), dz2 = S.dz_fusion0(1), dzc = S.colour().dz_c0();
    if (dz1 >= t.n_slots || dz2 >= t.n_slots || dzc >= t.n_slots || t.slot_tiles[dz1] != 8 || t.slot_tiles[dz2] != 8 || t.slot_tiles[dzc] != 4) {
        err = "training plan: unexpected fusion.0 / color_layers.0 gradient slots";
        return NRF_EINVAL;
    }
    InputGradV3Args a{};
    a.wstream = t.istream[mode];
    a.ctx = (const char*)ctx;
    a.dz1_off = k.slot_off[dz1];
    a.dz2_off = k.slot_off[dz2];
    a.dzc_off = k.slot_off[dzc];
    a.aux_off = k.aux_off;
    a.n = n;
    a.n_tiles = (n + 31) / 32;
    a.positions = positions; a.directions = directions;
    a.d_positions = d_positions; a.d_directions = d_directions;
    a.dir_freq = net.arch.dir_freq;
    switch (mode) {
        case NRF_MMA_BF16: return run3<ModeBF16>(net, a, s, err);
        case NRF_MMA_F16:  return run3<ModeF16>(net, a, s, err);
        default:           return run3<ModeF32>(net, a, s, err);
    }
}

}  // namespace nrf
