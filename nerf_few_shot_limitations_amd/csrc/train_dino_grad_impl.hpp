// train_dino_grad_impl.hpp -- dL/d (per-sample DINO features) of the V3 network, from what a finished dZ chain
// (train_v3_impl.hpp: train_backward_v3_kernel) left in the context.  Notation of train_slots.hpp: fusion.0 has weight W0
// (256 x (PE + C)), W0d = its C columns that multiply the DINO channels; the chain saved
//     d1 = dZ(fusion.0, pass 1)  in slot SlotsV3::dz_fusion0(0)   (it already contains the whole gate path)
//     d2 = dZ(fusion.0, pass 2)  in slot SlotsV3::dz_fusion0(1)
// and the gate (w0, w1) per sample, because the weight-gradient jobs need them.  With the inputs [pe | f] (pass 1) and
// [pe w0 | f w1] (pass 2),
//     dL/df = W0d^T d1 + w1 (W0d^T d2)                                  (C values per sample)
// A kernel of its own, not a tail of the dZ chain: that kernel sits at the register limit, this one needs 2 * DT accumulator
// tiles and two operand tiles in flight.  The saved tiles are B-operand images as they lie (train_core.hpp); the A operand
// W0d^T is one more small fragment stream of the packer (packing.cpp:make_dino_grad_plan: DT x 8 tile pairs, 32 .. 128 KiB),
// which fits in LDS whole: loaded once per workgroup, persistent workgroups over the 32-sample tiles, one tile per wave.
// The two products are kept apart down to the fp32 epilogue acc1 + w1 * acc2 (forming d1 + w1 d2 in front of the MFMA would
// round a gradient to 16 bits a second time).  HBM-bound: 2 x 8 saved tiles read and 4 C bytes written per sample.
#pragma once
#include "train_impl.hpp"

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

constexpr int kDinoGradWaves = 4;

template <class Mode, int DT>
constexpr int dino_grad_lds_bytes() { return DT * 8 * Mode::SUB * kFragBytes; }

template <class Mode, int DT>
__global__ void __launch_bounds__(kDinoGradWaves * 64) dino_grad_kernel(const DinoGradArgs P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename Mode::Act Act;
    typedef typename Mode::frag_t frag_t;
    typedef ActIO<Mode> IO;
    constexpr int SUB = Mode::SUB, NF = DT * 8 * SUB, TB = tile_bytes<Mode>();
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int f = wave; f < NF; f += kDinoGradWaves)
        *(i32x4*)(smem + f * kFragBytes + lane * 16) = *(const i32x4*)((const char*)P.wstream + f * kFragBytes + lane * 16);
    __syncthreads();
    const NRF_LDS char* frags = (const NRF_LDS char*)smem + lane * 16;
    for (int64_t st = (int64_t)blockIdx.x * kDinoGradWaves + wave; st < P.n_tiles; st += (int64_t)gridDim.x * kDinoGradWaves) {
        const char* z1 = P.ctx + P.dz1_off + st * 8 * (int64_t)TB + lane * 16;
        const char* z2 = P.ctx + P.dz2_off + st * 8 * (int64_t)TB + lane * 16;
        f32x16 acc1[DT], acc2[DT];
#pragma unroll
        for (int m = 0; m < DT; ++m) { acc1[m] = f32x16{}; acc2[m] = f32x16{}; }
        // K tile t multiplied while tile t + 1 is in flight.  A rolled loop: unrolled, the compiler hoists every fragment read
        // and every tile load to the top and spills
        Act b1 = IO::template load_g<Act>(z1), b2 = IO::template load_g<Act>(z2);
#pragma unroll 1
        for (int t = 0; t < 8; ++t) {
            Act n1 = b1, n2 = b2;
            if (t < 7) {
                n1 = IO::template load_g<Act>(z1 + (t + 1) * TB);
                n2 = IO::template load_g<Act>(z2 + (t + 1) * TB);
            }
#pragma unroll
            for (int m = 0; m < DT; ++m)
#pragma unroll
                for (int s = 0; s < SUB; ++s) {
                    const frag_t a = *(const NRF_LDS frag_t*)(frags + ((m * 8 + t) * SUB + s) * kFragBytes);
                    Mode::mma(acc1[m], a, b1, s);
                    Mode::mma(acc2[m], a, b2, s);
                }
            b1 = n1;
            b2 = n2;
        }
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
