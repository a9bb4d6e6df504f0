// train_input_grad.hip -- host entry point of input_grad_kernel (train_input_grad_impl.hpp): the V1 and V2 networks' gradient
// with respect to their encoded inputs, positions and directions
#include "train_input_grad_impl.hpp"
#include "train_post_grad_launch.hpp"

namespace nrf {

int launch_input_grad(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, void* ctx, const float* positions, const float* directions,
                      float* d_x_enc, float* d_positions, float* d_directions, hipStream_t s, std::string& err) {
    const bool v2 = net.arch.net == NRF_NET_V2;
    const char* refusal = nullptr;
    if (net.arch.net != NRF_NET_V1 && !v2) refusal = "the input gradient is built for the V1 and V2 networks";
    else if (net.arch.pos_freq != kInputGradPosFreq || (v2 && (net.arch.dir_freq < 1 || net.arch.dir_freq > 4)))
        refusal = "the input gradient is built for pos_freq 10 and dir_freq 1..4";
    PostGradOpening o;
    const int opened = open_post_grad(net, t, mode, n, refusal, t.istream, "model not prepared for the input gradient", o, err);
    if (opened != NRF_OK || !o.n_tiles) return opened;
    const int n_layers = net.arch.n_layers;
    const int dz0 = v2 ? SlotsV2{n_layers}.dz_trunk(0) : SlotsV1{n_layers}.dz_trunk(0);
    const int dzc = v2 ? SlotsV2{n_layers}.colour().dz_c0() : dz0;
    if (dz0 >= t.n_slots || dzc >= t.n_slots || t.slot_tiles[dz0] != 8 || (v2 && t.slot_tiles[dzc] != 4)) {
        err = "training plan: unexpected first-layer gradient slots";
        return NRF_EINVAL;
    }
    InputGradArgs a{};
    a.wstream = o.wstream;
    a.ctx = (const char*)ctx;
    a.dz0_off = o.k.slot_off[dz0];
    a.dzc_off = o.k.slot_off[dzc];
    a.n = n;
    a.n_tiles = o.n_tiles;
    a.positions = positions; a.directions = directions;
    a.d_x_enc = d_x_enc; a.d_positions = d_positions; a.d_directions = d_directions;
    a.dir_freq = net.arch.dir_freq;
    return dispatch_post_grad(mode, [&](auto tag) {
        typedef typename decltype(tag)::Mode Mode;
        constexpr int PT = kInputGradPT;
        return v2 ? run_post_grad<input_grad_kernel<Mode, true>, post_grad_lds_bytes<Mode, PT, true>()>(net, a, s, "input grad", err)
                  : run_post_grad<input_grad_kernel<Mode, false>, post_grad_lds_bytes<Mode, PT, false>()>(net, a, s, "input grad", err);
    });
}

}  // namespace nrf
