// train_dino_grad_impl.hpp -- dL/d (per-sample DINO features) of the V3 network, from what a finished dZ chain
// (train_v3_impl.hpp: train_backward_v3_kernel) left in the context.  Notation of train_slots.hpp: fusion.0 has weight W0
// (256 x (PE + C)), W0d = its C columns that multiply the DINO channels; the chain saved
//     d1 = dZ(fusion.0, pass 1)  in slot SlotsV3::dz_fusion0(0)   (it already contains the whole gate path)
//     d2 = dZ(fusion.0, pass 2)  in slot SlotsV3::dz_fusion0(1)
// and the gate (w0, w1) per sample, because the weight-gradient jobs need them.  With the inputs [pe | f] (pass 1) and
// [pe w0 | f w1] (pass 2),
//     dL/df = W0d^T d1 + w1 (W0d^T d2)                                  (C values per sample)
// The A operand W0d^T is one small fragment stream of the packer (packing.cpp:make_dino_grad_plan: DT x 8 tile pairs, 32 .. 128
// KiB), which fits in LDS whole; the kernel needs 2 * DT accumulator tiles and two operand tiles in flight.  The two products are
// kept apart down to the fp32 epilogue acc1 + w1 * acc2 (forming d1 + w1 d2 in front of the MFMA would round a gradient to 16
// bits a second time).  HBM-bound: 2 x 8 saved tiles read and 4 C bytes written per sample.  Built from
// train_post_grad_core.hpp.
#pragma once
#include "train_post_grad_core.hpp"

namespace nrf {

struct DinoGradArgs {
    const void* wstream;        // DT * 8 * Mode::SUB fragments: W0d^T, (m, t, s) order (mlp_core.hpp)
    const char* ctx;
    int64_t dz1_off, dz2_off;   // context offsets of the two dZ slots (8 feature tiles per sample tile)
    int64_t aux_off;            // the gate
    int64_t n;                  // samples
    int64_t n_tiles;            // 32-sample tiles that hold a sample
    float* d_dino;              // (n, 32 * DT), rows >= n not written
};

template <class Mode, int DT>
__global__ void __launch_bounds__(kPostGradWaves * 64) dino_grad_kernel(const DinoGradArgs P) {
    constexpr int64_t TB = tile_bytes<Mode>();
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const NRF_LDS char* frags = post_grad_resident<post_grad_frags<Mode, DT, false>()>(P.wstream, lane, wave);
    for (int64_t st = (int64_t)blockIdx.x * kPostGradWaves + wave; st < P.n_tiles; st += (int64_t)gridDim.x * kPostGradWaves) {
        f32x16 acc1[DT], acc2[DT];
        post_grad_walk<Mode, DT>(frags, P.ctx + P.dz1_off + st * 8 * TB + lane * 16, P.ctx + P.dz2_off + st * 8 * TB + lane * 16, acc1, acc2);
        const int64_t raw = st * 32 + c;
        if (raw < P.n) {
            const float w1 = ((const float2*)(P.ctx + P.aux_off))[raw].y;
            float* out = P.d_dino + raw * (32 * DT) + 4 * h;
#pragma unroll
            for (int m = 0; m < DT; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = acc1[m][4 * g + q] + w1 * acc2[m][4 * g + q];
                    *(f32x4*)(out + 32 * m + 8 * g) = v;
                }
        }
    }
}

}  // namespace nrf
