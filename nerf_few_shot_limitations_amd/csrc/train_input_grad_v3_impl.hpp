// train_input_grad_v3_impl.hpp -- dL/d (positions, directions) of the V3 network through the positional encodings, from what a
// finished dZ chain (train_v3_impl.hpp: train_backward_v3_kernel) left in the context.  Notation of train_slots.hpp and
// train_dino_grad_impl.hpp: fusion.0 has weight W0 = [W0p | W0d] (256 x (PE + C)) and runs twice, on [pe | f] and on
// [pe w0 | f w1]; the chain saved
//     d1 = dZ(fusion.0, pass 1)   in slot SlotsV3::dz_fusion0(0)   (it already contains the whole gate path)
//     d2 = dZ(fusion.0, pass 2)   in slot SlotsV3::dz_fusion0(1)
//     dZc = dZ(color_layers.0)    in slot ColourSlots::dz_c0()     (4 tiles)
// and the gate (w0, w1) per sample, so that
//     dL/d e(p) = W0p^T d1 + w0 (W0p^T d2)          dL/d e(d) = C0[:, 256 + pe]^T dZc
// and the epilogue applies the adjoint of the encoding (train_input_grad_impl.hpp: encoding_adjoint, L = 12 over three
// accumulator tiles for the positions, the run-time dir_freq over one for the directions).  The two products are kept apart down
// to the fp32 join acc1 + w0 * acc2: forming d1 + w0 d2 in front of the MFMA would round a gradient to 16 bits a second time.
// This is the share of dL/d positions that flows through the encoding only; the share through the fetched features -- the
// adjoint of the projection and of the bilinear fetch applied to nrf_mlp_backward_dino's dL/df -- is
// fetch_points_backward_kernel (staged_kernels.hip), which adds onto this kernel's output.
// Built like input_grad_kernel and dino_grad_kernel: the A operands are two small fragment streams of the packer
// (packing.cpp:make_input_grad_v3_plan: 3 x 8 and 1 x 4 tile pairs, 48 + 8 KiB in the 16-bit modes, twice that in fp32 -- the
// second is padded to a whole chunk in the stream but only its fragments are copied), resident in LDS: loaded once per workgroup,
// persistent waves over the 32-sample tiles.  HBM-bound: 2 x 8 + 4 saved tiles, the gate and 24 bytes of coordinates read, 24 B
// written per sample.
#pragma once
#include "train_input_grad_impl.hpp"

namespace nrf {

struct InputGradV3Args {
    const void* wstream;        // (3 * 8 + 4) * Mode::SUB fragments: W0p^T, then color_layers.0^T's direction tile, (m, t, s) order
    const char* ctx;
    int64_t dz1_off, dz2_off;   // context offsets of the two fusion.0 dZ slots (8 feature tiles per sample tile)
    int64_t dzc_off;            // ... of color_layers.0's (4)
    int64_t aux_off;            // the gate
    int64_t n;                  // samples
    int64_t n_tiles;            // 32-sample tiles that hold a sample
    const float* positions;     // (n,3), read when d_positions is asked for
    const float* directions;    // (n,3), read when d_directions is asked for
    float* d_positions;         // (n,3) or NULL
    float* d_directions;        // (n,3) or NULL
    int dir_freq;               // 1..4
};

constexpr int kInputGradV3PosFreq = 12;                         // the V3 training path's pos_freq (check_train_common)
constexpr int kInputGradV3PT = pe_tiles(kInputGradV3PosFreq);   // 3

template <class Mode>
constexpr int input_grad_v3_frags() { return (kInputGradV3PT * 8 + 4) * Mode::SUB; }
template <class Mode>
constexpr int input_grad_v3_lds_bytes() { return input_grad_v3_frags<Mode>() * kFragBytes; }

// encoding_adjoint (train_input_grad_impl.hpp) one accumulator tile at a time: slots 16 M .. 16 M + 15 added onto this lane half's
// three sums, in slot order.  Three tiles in ONE unrolled loop are more than the unroller takes (48 inlined sincosf): the
// accumulators would be indexed at run time and land in scratch.
template <int M>
__device__ __forceinline__ void encoding_adjoint_tile(const f32x16& acc, const float (&p)[3], int L, int h, float (&d)[3]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        constexpr int u0 = 16 * M;
        const int u = u0 + r;
        const float a = acc[r];
        const int f = u / 3, c = u % 3;
        if (f < 15) {
            const float scale = (float)(1u << f);
            float sn, cs;
            sincosf(__fmul_rn(p[c], scale), &sn, &cs);
            const float t = __fadd_rn(d[c], __fmul_rn(__fmul_rn(scale, h ? -sn : cs), a));
            d[c] = u < 3 * L ? t : d[c];
        }
        if (c == 0) {                                    // u == 3L: x | z
            const float t0 = __fadd_rn(d[0], a), t2 = __fadd_rn(d[2], a);
            d[0] = (u == 3 * L && !h) ? t0 : d[0];
            d[2] = (u == 3 * L && h) ? t2 : d[2];
        }
        if (c == 1) {                                    // u == 3L + 1: y | unused
            const float t1 = __fadd_rn(d[1], a);
            d[1] = (u == 3 * L + 1 && !h) ? t1 : d[1];
        }
    }
}

template <class Mode, bool POS, bool DIR>
__global__ void __launch_bounds__(kInputGradWaves * 64) input_grad_v3_kernel(const InputGradV3Args P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename Mode::Act Act;
    typedef typename Mode::frag_t frag_t;
    typedef ActIO<Mode> IO;
    constexpr int SUB = Mode::SUB, PT = kInputGradV3PT, NF = input_grad_v3_frags<Mode>(), TB = tile_bytes<Mode>();
    constexpr int DF0 = (PT * 8 * SUB + 15) / 16 * 16;   // first fragment of the direction layer: the next chunk boundary
    static_assert(DF0 == PT * 8 * SUB, "the position layer must end on a chunk boundary");
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int f = wave; f < NF; f += kInputGradWaves)
        *(i32x4*)(smem + f * kFragBytes + lane * 16) = *(const i32x4*)((const char*)P.wstream + f * kFragBytes + lane * 16);
    __syncthreads();
    const NRF_LDS char* frags = (const NRF_LDS char*)smem + lane * 16;
    for (int64_t st = (int64_t)blockIdx.x * kInputGradWaves + wave; st < P.n_tiles; st += (int64_t)gridDim.x * kInputGradWaves) {
        const int64_t raw = st * 32 + c;
        const bool live = raw < P.n;
        const int64_t sid = live ? raw : P.n - 1;              // rows past the end read the last sample and write nothing
        if constexpr (POS) {
            const char* z1 = P.ctx + P.dz1_off + st * 8 * (int64_t)TB + lane * 16;
            const char* z2 = P.ctx + P.dz2_off + st * 8 * (int64_t)TB + lane * 16;
            f32x16 acc1[PT], acc2[PT];
#pragma unroll
            for (int m = 0; m < PT; ++m) { acc1[m] = f32x16{}; acc2[m] = f32x16{}; }
            // K tile t multiplied while tile t + 1 is in flight; rolled, as in dino_grad_kernel
            Act b1 = IO::template load_g<Act>(z1), b2 = IO::template load_g<Act>(z2);
#pragma unroll 1
            for (int t = 0; t < 8; ++t) {
                Act n1 = b1, n2 = b2;
                if (t < 7) {
                    n1 = IO::template load_g<Act>(z1 + (t + 1) * TB);
                    n2 = IO::template load_g<Act>(z2 + (t + 1) * TB);
                }
#pragma unroll
                for (int m = 0; m < PT; ++m)
#pragma unroll
                    for (int s = 0; s < SUB; ++s) {
                        const frag_t a = *(const NRF_LDS frag_t*)(frags + ((m * 8 + t) * SUB + s) * kFragBytes);
                        Mode::mma(acc1[m], a, b1, s);
                        Mode::mma(acc2[m], a, b2, s);
                    }
                b1 = n1;
                b2 = n2;
            }
            const float w0 = ((const float2*)(P.ctx + P.aux_off))[sid].x;
#pragma unroll
            for (int m = 0; m < PT; ++m) acc1[m] = acc1[m] + acc2[m] * w0;        // (two roundings: the build sets -ffp-contract=off)
            const float p[3] = {P.positions[sid * 3], P.positions[sid * 3 + 1], P.positions[sid * 3 + 2]};
            float d[3];
            d[0] = d[1] = d[2] = 0.0f;
            static_assert(PT == 3, "one call per accumulator tile");
            encoding_adjoint_tile<0>(acc1[0], p, kInputGradV3PosFreq, h, d);
            encoding_adjoint_tile<1>(acc1[1], p, kInputGradV3PosFreq, h, d);
            encoding_adjoint_tile<2>(acc1[2], p, kInputGradV3PosFreq, h, d);
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = __fadd_rn(d[k], __shfl_xor(d[k], 32, 64));      // the cross-half add
            if (live && h == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) P.d_positions[raw * 3 + k] = d[k];
            }
        }
        if constexpr (DIR) {
            const char* z = P.ctx + P.dzc_off + st * 4 * (int64_t)TB + lane * 16;
            f32x16 acc[1];
            acc[0] = f32x16{};
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                const Act b = IO::template load_g<Act>(z + t * TB);
#pragma unroll
                for (int s = 0; s < SUB; ++s) {
                    const frag_t a = *(const NRF_LDS frag_t*)(frags + (DF0 + t * SUB + s) * kFragBytes);
                    Mode::mma(acc[0], a, b, s);
                }
            }
            const float p[3] = {P.directions[sid * 3], P.directions[sid * 3 + 1], P.directions[sid * 3 + 2]};
            float d[3];
            encoding_adjoint<1>(acc, p, P.dir_freq, h, d);
            if (live && h == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) P.d_directions[raw * 3 + k] = d[k];
            }
        }
    }
}

}  // namespace nrf
