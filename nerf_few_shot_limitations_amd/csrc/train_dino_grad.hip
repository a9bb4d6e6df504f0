// train_dino_grad.hip -- host entry point of dino_grad_kernel (train_dino_grad_impl.hpp): the V3 network's gradient with
// respect to its per-sample DINO features
#include "train_dino_grad_impl.hpp"
#include "train_post_grad_launch.hpp"

namespace nrf {

int launch_dino_grad(const DeviceNet& net, const TrainDev& t, int mode, int64_t n, void* ctx, float* d_dino, hipStream_t s, std::string& err) {
    const bool family = net.arch.net == NRF_NET_V3 && (net.arch.dino_dim == 64 || net.arch.dino_dim == 128);
    PostGradOpening o;
    const int opened = open_post_grad(net, t, mode, n, family ? nullptr : "the DINO feature gradient needs a V3 model with dino_dim 64 or 128", t.gstream,
                                      "model not prepared for the DINO feature gradient", o, err);
    if (opened != NRF_OK || !o.n_tiles) return opened;
    const SlotsV3 S{net.arch.n_layers};
    if (S.dz_fusion0(1) >= t.n_slots || t.slot_tiles[S.dz_fusion0(0)] != 8 || t.slot_tiles[S.dz_fusion0(1)] != 8) {
        err = "training plan: unexpected fusion.0 gradient slots";
        return NRF_EINVAL;
    }
    DinoGradArgs a{};
    a.wstream = o.wstream;
    a.ctx = (const char*)ctx;
    a.dz1_off = o.k.slot_off[S.dz_fusion0(0)];
    a.dz2_off = o.k.slot_off[S.dz_fusion0(1)];
    a.aux_off = o.k.aux_off;
    a.n = n;
    a.n_tiles = o.n_tiles;
    a.d_dino = d_dino;
    return dispatch_post_grad(mode, [&](auto tag) {
        typedef typename decltype(tag)::Mode Mode;
        return net.arch.dino_dim == 64 ? run_post_grad<dino_grad_kernel<Mode, 2>, post_grad_lds_bytes<Mode, 2, false>()>(net, a, s, "dino grad", err)
                                       : run_post_grad<dino_grad_kernel<Mode, 4>, post_grad_lds_bytes<Mode, 4, false>()>(net, a, s, "dino grad", err);
    });
}

}  // namespace nrf
