// train_input_grad_v3.hip -- host entry point of input_grad_v3_kernel (train_input_grad_v3_impl.hpp): the V3 network's gradient
// with respect to positions and directions through the positional encodings
#include "train_input_grad_v3_impl.hpp"
#include "train_post_grad_launch.hpp"

namespace nrf {

int launch_input_grad_v3(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, void* ctx, const float* positions, const float* directions,
                         float* d_positions, float* d_directions, hipStream_t s, std::string& err) {
    const char* refusal = nullptr;
    if (net.arch.net != NRF_NET_V3) refusal = "this input gradient is built for the V3 network";
    else if (net.arch.pos_freq != kInputGradV3PosFreq || net.arch.dir_freq < 1 || net.arch.dir_freq > 4)
        refusal = "the V3 input gradient is built for pos_freq 12 and dir_freq 1..4";
    PostGradOpening o;
    const int opened = open_post_grad(net, t, mode, n, refusal, t.istream, "model not prepared for the input gradient", o, err);
    if (opened != NRF_OK || !o.n_tiles) return opened;
    const SlotsV3 S{net.arch.n_layers};
    const int dz1 = S.dz_fusion0(0), dz2 = S.dz_fusion0(1), dzc = S.colour().dz_c0();
    if (dz1 >= t.n_slots || dz2 >= t.n_slots || dzc >= t.n_slots || t.slot_tiles[dz1] != 8 || t.slot_tiles[dz2] != 8 || t.slot_tiles[dzc] != 4) {
        err = "training plan: unexpected fusion.0 / color_layers.0 gradient slots";
        return NRF_EINVAL;
    }
    InputGradV3Args a{};
    a.wstream = o.wstream;
    a.ctx = (const char*)ctx;
    a.dz1_off = o.k.slot_off[dz1];
    a.dz2_off = o.k.slot_off[dz2];
    a.dzc_off = o.k.slot_off[dzc];
    a.aux_off = o.k.aux_off;
    a.n = n;
    a.n_tiles = o.n_tiles;
    a.positions = positions; a.directions = directions;
    a.d_positions = d_positions; a.d_directions = d_directions;
    a.dir_freq = net.arch.dir_freq;
    return dispatch_post_grad(mode, [&](auto tag) {
        typedef typename decltype(tag)::Mode Mode;
        constexpr int lds = post_grad_lds_bytes<Mode, kInputGradV3PT, true>();
        const char* what = "V3 input grad";
        if (a.d_positions && a.d_directions) return run_post_grad<input_grad_v3_kernel<Mode, true, true>, lds>(net, a, s, what, err);
        if (a.d_positions) return run_post_grad<input_grad_v3_kernel<Mode, true, false>, lds>(net, a, s, what, err);
        return run_post_grad<input_grad_v3_kernel<Mode, false, true>, lds>(net, a, s, what, err);
    });
}

}  // namespace nrf
