// train_v2_impl.hpp -- training kernels of the V2 network (the one src/training/train.py:82-89 builds with
// use_dino=False: PE(pos) -> DensityMLP -> ColorMLP(cat[feature, PE(dir)]), nerf_mlp.py:41-84).  Same machinery as
// train_impl.hpp (V1); the chain is longer on both sides.  Slots and planes: train_slots.hpp (SlotsV2).
// Backward stream order (packing.cpp:make_backward_plan): color_layers.4^T, .2^T, .0^T (feature columns only),
// [feature_head | density_head]^T (K = 8 + 1 tiles), density_layers.{n-1..1}^T.
#pragma once
#include "train_impl.hpp"

namespace nrf {

template <class Mode, int WAVES, int LP, int LD, class Src>
__device__ __forceinline__ void train_forward_v2_body(const typename Src::KArgs& P) {
    typedef typename Mode::Act Act;
    constexpr int KT0 = pe_tiles(LP);
    const TrainRaysDev* rays = nullptr;
    const int32_t* index = nullptr;
    if constexpr (Src::kRays) rays = &P.rays;
    if constexpr (Src::kIndexed) index = P.index;
    chain_kernel<Mode, WAVES, true>(P, [&](ChainTile<Mode, WAVES>& T) {
        const SlotsV2 S{P.net.n_layers};
        Act A[8][1], B[8][1];
        {
            float p[3];
            if constexpr (Src::kIndexed) {
                const int64_t id = P.index[T.sid];
                RaySample(P.rays, id).position_kept(P.rays, id, p);
            } else if constexpr (Src::kRays) {
                RaySample(P.rays, T.sid).position(P.rays, T.sid, T.h == 0 && T.raw < P.n, p);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = P.pos[T.sid * 3 + k];
            }
            Act e1[KT0], enc[KT0][1];
            encode3<Mode, LP>(p, T.h, e1);
#pragma unroll
            for (int t = 0; t < KT0; ++t) {
                enc[t][0] = e1[t];
                T.save(S.input(), t, e1[t]);
            }
            T.relu_layer(enc, A, S.trunk(0), S.plane(0), 0);
        }
        float dens_raw = 0.0f, logit[3];
        int boff = 32 * 8;
        T.trunk_forward(S, 1, S.n, A, B, boff, [&](const Act (&X)[8][1]) { T.template colour_forward<LD, Src>(S.colour(), X, boff, dens_raw, logit, rays, index); });
        T.write_rgb_density(dens_raw, logit);
    });
}

template <class Mode, int WAVES, int LP, int LD>
__global__ void __launch_bounds__(WAVES * 64) train_forward_v2_kernel(const TrainKArgs P) {
    train_forward_v2_body<Mode, WAVES, LP, LD, StagedInputs>(P);
}

template <class Mode, int WAVES, int LP, int LD>
__global__ void __launch_bounds__(WAVES * 64) train_forward_v2_rays_kernel(const TrainRayKArgs P) {
    train_forward_v2_body<Mode, WAVES, LP, LD, RayInputs>(P);
}

template <class Mode, int WAVES, int LP, int LD>
__global__ void __launch_bounds__(WAVES * 64) train_forward_v2_rays_indexed_kernel(const TrainRayIndexKArgs P) {
    train_forward_v2_body<Mode, WAVES, LP, LD, IndexedRayInputs>(P);
}

template <class Mode, int WAVES, int LP>
__global__ void __launch_bounds__(WAVES * 64) train_backward_v2_kernel(const TrainKArgs P) {
    typedef typename Mode::Act Act;
    chain_kernel<Mode, WAVES, false>(P, [&](ChainTile<Mode, WAVES>& T) {
        const SlotsV2 S{P.net.n_layers};
        Act in9[9][1];
        T.colour_backward(S.colour(), S.plane(S.n - 1), in9);
        Act A[8][1], B[8][1];
        T.trunk_backward(S, S.n, in9, A, B, [](const Act (&)[8][1], const Act (&)[8][1]) {});
    });
}

}  // namespace nrf
