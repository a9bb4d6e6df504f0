// train_v3_impl.hpp -- training kernels of the V3 network (nerf_mlp.py:86-158 NeRFWithDINO with lora_dino.py:146-193
// NeRFDINOFusion in front of the V2 body).  Same machinery as train_impl.hpp / train_v2_impl.hpp.
//
//   fused = fusion(cat[pe, dino]);  (w0, w1) = softmax(attention(fused));
//   x     = output_proj(fusion(cat[pe * w0, dino * w1]))          -- the SAME fusion weights, twice
//   then DensityMLP(x) and ColorMLP as in V2.
// No gradient with respect to positions or directions.  The gradient with respect to the per-sample DINO features is a kernel
// of its own behind this chain (train_dino_grad_impl.hpp), from the two dZ(fusion.0) slots and the gate saved here.
//
// Slots and planes: train_slots.hpp (SlotsV3).
#pragma once
#include "train_impl.hpp"

namespace nrf {

// operand tile -> fp32 registers (element r of the result = accumulator-row order of the tile)
template <class Mode> struct ActF32;
template <>
struct ActF32<ModeBF16> {
    __device__ static __forceinline__ f32x16 get(const ModeBF16::Act& a) {
        f32x16 o;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const i32x4 q = __builtin_bit_cast(i32x4, a.f[s]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = q[j];
                o[8 * s + 2 * j] = __builtin_bit_cast(float, d << 16);
                o[8 * s + 2 * j + 1] = __builtin_bit_cast(float, (int)((uint32_t)d & 0xffff0000u));
            }
        }
        return o;
    }
};
template <>
struct ActF32<ModeF16> {
    __device__ static __forceinline__ f32x16 get(const ModeF16::Act& a) {
        f32x16 o;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) o[8 * s + j] = (float)a.f[s][j];
        return o;
    }
};
template <>
struct ActF32<ModeF32> {
    __device__ static __forceinline__ f32x16 get(const ModeF32::Act& a) {
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = a.r[r];
        return o;
    }
};

__device__ __forceinline__ float2* gate_ptr(const TrainKArgs& P, int64_t sample) { return (float2*)(P.ctx + P.aux_off) + sample; }

template <class Mode, int WAVES, int LP, int LD, int DT, class Src>
__device__ __forceinline__ void train_forward_v3_body(const typename Src::KArgs& P) {
    typedef typename Mode::Act Act;
    constexpr int PT = pe_tiles(LP), KT0 = PT + DT;
    const TrainRaysDev* rays = nullptr;
    const int32_t* index = nullptr;
    if constexpr (Src::kRays) rays = &P.rays;
    if constexpr (Src::kIndexed) index = P.index;
    chain_kernel<Mode, WAVES, true>(P, [&](ChainTile<Mode, WAVES>& T) {
        const SlotsV3 S{P.net.n_layers};
        const int h = T.h;
        float p[3];
        if constexpr (Src::kIndexed) {
            const int64_t id = P.index[T.sid];
            RaySample(P.rays, id).position_kept(P.rays, id, p);
        } else if constexpr (Src::kRays) {
            RaySample(P.rays, T.sid).position(P.rays, T.sid, h == 0 && T.raw < P.n, p);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = P.pos[T.sid * 3 + k];
        }
        // first-layer operand tiles [pe * w0 | dino * w1], saved into `slot` (lora_dino.py:181,187-191)
        auto inputs = [&](float w0, float w1, Act (&x)[KT0][1], int slot) {
            if constexpr (Src::kRays) {
                // The renderer's gather (nets.hpp: dino_taps, DinoRaw) from the source view's map, once per fusion pass and one operand
                // tile at a time: a pass rounds round16(e * w1) from the fp32 blend as the staged route does (never a rescaled 16-bit
                // tile: nets.hpp:DinoHeld), and neither the taps (8 registers) nor the channels (16 DT) are held across the layers
                // between the passes -- the map is a few hundred KB and stays in L2.  The first tile's 16 loads fly during the
                // positional encoding, every later tile's during the conversion of the one before.
                const DinoTaps tp = dino_taps(P.rays.dino, p);
                DinoRaw<1> raw;
                raw.issue(P.rays.dino.features, tp, h);
                Act e1[PT];
                encode3<Mode, LP>(p, h, e1, w0);
#pragma unroll
                for (int t = 0; t < PT; ++t) x[t][0] = e1[t];
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    float e[16];
                    raw.finish(tp, e);
                    if (t + 1 < DT) raw.issue(P.rays.dino.features + 32 * (t + 1), tp, h);
                    Act d1[1];
                    dino_scaled_tiles<Mode, 1>(e, w1, d1);
                    x[PT + t][0] = d1[0];
                }
            } else {
                Act e1[PT];
                encode3<Mode, LP>(p, h, e1, w0);
#pragma unroll
                for (int t = 0; t < PT; ++t) x[t][0] = e1[t];
                const float* f = P.dino + T.sid * (32 * DT);
#pragma unroll
                for (int t = 0; t < DT; ++t) {
                    f32x16 e;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 v = *(const f32x4*)(f + 32 * t + 8 * g + 4 * h);
#pragma unroll
                        for (int q = 0; q < 4; ++q) e[4 * g + q] = v[q] * w1;
                    }
                    x[PT + t][0] = Mode::template to_act<false>(e);
                }
            }
#pragma unroll
            for (int t = 0; t < KT0; ++t) T.save(slot, t, x[t][0]);
        };

        Act A[8][1], B[8][1];
        int boff = 0;
        {
            Act x[KT0][1];
            inputs(1.0f, 1.0f, x, S.input(0));
            T.relu_layer(x, A, S.fusion0(0), S.plane_fusion0(0), boff); boff += 32 * 8;
        }
        T.relu_layer(A, B, S.fusion2(0), S.plane_fusion2(0), boff); boff += 32 * 8;
        float w0, w1;
        {   // attention: Linear(256->64)+ReLU, Linear(64->2), softmax (lora_dino.py:162-167,184)
            Act a0[2][1];
            T.relu_layer(B, a0, S.attention0(), S.plane_attention0(), boff); boff += 8 * 8;
            f32x16 lg[1];
            dense_head<Mode, 2, 1>(T.pipe, T.bias + boff, h, a0, lg); boff += 32;
            const float d = lg[0][1] - lg[0][0];
            w0 = 1.0f / (1.0f + (Mode::FAST_EXP ? __expf(d) : expf(d)));
            w1 = 1.0f - w0;
            if (h == 0) *gate_ptr(P, T.raw) = make_float2(w0, w1);          // padded samples included: the context is padded
        }
        {
            Act x[KT0][1];
            inputs(w0, w1, x, S.input(1));
            T.relu_layer(x, A, S.fusion0(1), S.plane_fusion0(1), boff); boff += 32 * 8;
        }
        T.relu_layer(A, B, S.fusion2(1), S.plane_fusion2(1), boff); boff += 32 * 8;
        T.template linear<8>(B, A, S.proj(), boff);                        // output_proj: no activation
        boff += 32 * 8;

        float dens_raw = 0.0f, logit[3];
        T.trunk_forward(S, 0, S.n, A, B, boff, [&](const Act (&X)[8][1]) { T.template colour_forward<LD, Src>(S.colour(), X, boff, dens_raw, logit, rays, index); });
        T.write_rgb_density(dens_raw, logit);
    });
}

template <class Mode, int WAVES, int LP, int LD, int DT>
__global__ void __launch_bounds__(WAVES * 64) train_forward_v3_kernel(const TrainKArgs P) {
    train_forward_v3_body<Mode, WAVES, LP, LD, DT, StagedInputs>(P);
}

template <class Mode, int WAVES, int LP, int LD, int DT>
__global__ void __launch_bounds__(WAVES * 64) train_forward_v3_rays_kernel(const TrainRayKArgs P) {
    train_forward_v3_body<Mode, WAVES, LP, LD, DT, RayInputs>(P);
}

template <class Mode, int WAVES, int LP, int LD, int DT>
__global__ void __launch_bounds__(WAVES * 64) train_forward_v3_rays_indexed_kernel(const TrainRayIndexKArgs P) {
    train_forward_v3_body<Mode, WAVES, LP, LD, DT, IndexedRayInputs>(P);
}

template <class Mode, int WAVES, int LP, int DT>
__global__ void __launch_bounds__(WAVES * 64) train_backward_v3_kernel(const TrainKArgs P) {
    typedef typename Mode::Act Act;
    typedef ActIO<Mode> IO;
    constexpr int PT = pe_tiles(LP), KT0 = PT + DT;
    chain_kernel<Mode, WAVES, false>(P, [&](ChainTile<Mode, WAVES>& T) {
        const SlotsV3 S{P.net.n_layers};
        const int h = T.h;
        Act in9[9][1];
        T.colour_backward(S.colour(), S.plane(S.n - 1), in9);
        Act A[8][1], B[8][1];
        // below the trunk: X = dZ of trunk layer 0, Y = scratch
        T.trunk_backward(S, S.n, in9, A, B, [&](Act (&X)[8][1], Act (&Y)[8][1]) {
            T.template linear<8>(X, Y, S.dz_proj(), 0);                                   // trunk 0^T -> d output_proj
            T.mcur = T.bits(S.plane_fusion2(1));
            T.masked_layer(Y, X, S.dz_fusion2(1));                                        // output_proj^T -> dZ fusion.2 p2
            T.mcur = T.bits(S.plane_fusion0(1));
            T.masked_layer(X, Y, S.dz_fusion0(1));                                        // fusion.2^T -> dZ fusion.0 p2
            // fusion.0^T: d [pe*w0 | dino*w1]; its dot products with the unscaled inputs are d w0, d w1 (lora_dino.py:187-190)
            float dw0 = 0.0f, dw1 = 0.0f;
            dense<Mode, 8, KT0, 1>(T.pipe, T.bias, h, Y, [&](auto m_, f32x16(&acc)[1]) {
                constexpr int m = decltype(m_)::value;
                const f32x16 xin = ActF32<Mode>::get(IO::template load_g<Act>(tile_ptr<Mode>(P, S.input(0), T.st, m, T.lane)));
                float s = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s = __builtin_fmaf(acc[0][r], xin[r], s);
                if constexpr (m < PT) dw0 += s; else dw1 += s;
            });
            dw0 += __shfl_xor(dw0, 32, 64);                              // the two lane halves hold different features of the same sample
            dw1 += __shfl_xor(dw1, 32, 64);
            Act G2[1][1], da0[2][1];
            {
                const float2 w = *gate_ptr(P, T.raw);
                const float s = w.x * dw0 + w.y * dw1;                   // softmax': d logit_i = w_i (d w_i - sum_j w_j d w_j)
                f32x16 e = {};
                if (h == 0) { e[0] = w.x * (dw0 - s); e[1] = w.y * (dw1 - s); }
                G2[0][0] = Mode::template to_act<false>(e);
                T.save(S.d_gate(), 0, G2[0][0]);
            }
            T.mcur = T.bits(S.plane_attention0());
            T.masked_layer(G2, da0, S.dz_attention0());                                   // attention.2^T
            T.mcur = T.bits(S.plane_fusion2(0));
            T.masked_layer(da0, X, S.dz_fusion2(0));                                      // attention.0^T -> dZ fusion.2 p1
            T.mcur = T.bits(S.plane_fusion0(0));
            T.masked_layer(X, Y, S.dz_fusion0(0));                                        // fusion.2^T -> dZ fusion.0 p1
        });
    });
}

}  // namespace nrf
