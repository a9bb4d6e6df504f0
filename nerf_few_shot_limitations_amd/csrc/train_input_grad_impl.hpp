// train_input_grad_impl.hpp -- dL/d (inputs of the field) of the V1 and V2 networks, from what a finished dZ chain
// (train_impl.hpp: train_backward_kernel, train_v2_impl.hpp) left in the context.  Notation of train_slots.hpp: the first Linear
// has weight W0 (256 x pe_dim), color_layers.0 has weight C0 (128 x (256 + dir pe_dim)); the chain saved
//     dZ0 = dZ(first Linear)      in slot dz_trunk(0)           (8 tiles)
//     dZc = dZ(color_layers.0)    in slot ColourSlots::dz_c0()  (4 tiles, V2)
// so that, with the encodings e(p) and e(d) of feature_map.hpp,
//     dL/d e(p) = W0[:, pe]^T dZ0          dL/d e(d) = C0[:, 256 + pe]^T dZc
// and the epilogue applies the adjoint of the encoding.  The kernel order gives lane half 0 the sine and lane half 1 the cosine of
// the same (frequency, coordinate): half 0 adds 2^f cos(2^f p_c) acc over its slots, half 1 adds -2^f sin(2^f p_c) acc, the raw
// coordinates sit in slots 3L (x | z) and 3L+1 (y | -), and one cross-half add joins them.  The sum runs in slot order and the
// trigonometry is the precise sincosf of the exact product p * 2^f in every mode, so a sample's gradient is bit-reproducible and
// independent of the batch around it.
// A kernel of its own, in the manner of dino_grad_kernel (train_dino_grad_impl.hpp): the chain kernels sit at the register limit.
// The A operands are two small fragment streams of the packer (packing.cpp:make_input_grad_plan: PT x 8 and 1 x 4 tile pairs,
// 32 + 8 KiB in the 16-bit modes, twice that in fp32 -- the second is padded to a whole chunk in the stream but only its
// fragments are copied), resident in LDS: loaded once per workgroup, persistent waves over the 32-sample tiles.
// HBM-bound: 8 (+ 4) saved tiles and 12 (+ 12) bytes of coordinates read, 12 .. 24 B (or 4 pe_dim B) written per sample.
#pragma once
#include "feature_map.hpp"
#include "train_impl.hpp"

namespace nrf {

struct InputGradArgs {
    const void* wstream;        // (PT * 8 + 4) * Mode::SUB fragments: W0^T, then (V2) C0^T's direction tile, (m, t, s) order
    const char* ctx;
    int64_t dz0_off, dzc_off;   // context offsets of the two dZ slots (8 | 4 feature tiles per sample tile)
    int64_t n;                  // samples
    int64_t n_tiles;            // 32-sample tiles that hold a sample
    const float* positions;     // (n,3), read when d_positions is asked for
    const float* directions;    // (n,3), read when d_directions is asked for
    float* d_x_enc;             // V1: (n, pe_dim) in the reference's column order, or NULL
    float* d_positions;         // (n,3) or NULL
    float* d_directions;        // V2: (n,3) or NULL
    int dir_freq;               // V2: 1..4
};

constexpr int kInputGradWaves = 4;
constexpr int kInputGradPosFreq = 10;                       // the training path's pos_freq (check_train_common)
constexpr int kInputGradPT = pe_tiles(kInputGradPosFreq);   // 2

template <class Mode, bool V2>
constexpr int input_grad_frags() { return (kInputGradPT * 8 + (V2 ? 4 : 0)) * Mode::SUB; }
template <class Mode, bool V2>
constexpr int input_grad_lds_bytes() { return input_grad_frags<Mode, V2>() * kFragBytes; }

// The adjoint of one encoding over NT accumulator tiles: this lane half's share of dL/d x (three sums, slot order), then the
// cross-half add.  Written with selects, not branches, on the frequency count: L is a run-time value for the directions, and a
// branch per slot around the (inlined) sincosf parks an exec mask each.
template <int NT>
__device__ __forceinline__ void encoding_adjoint(const f32x16 (&acc)[NT], const float (&p)[3], int L, int h, float (&d)[3]) {
    d[0] = d[1] = d[2] = 0.0f;
#pragma unroll
    for (int u = 0; u < 16 * NT; ++u) {
        const float a = acc[u >> 4][u & 15];
        const int f = u / 3, c = u % 3;
        if (f < 15) {                                    // (a compile-time bound: 1 << f; no encoding here has more frequencies)
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
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = __fadd_rn(d[k], __shfl_xor(d[k], 32, 64));
}

template <class Mode, bool V2>
__global__ void __launch_bounds__(kInputGradWaves * 64) input_grad_kernel(const InputGradArgs P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename Mode::Act Act;
    typedef typename Mode::frag_t frag_t;
    typedef ActIO<Mode> IO;
    constexpr int SUB = Mode::SUB, PT = kInputGradPT, NF = input_grad_frags<Mode, V2>(), TB = tile_bytes<Mode>();
    constexpr int DF0 = PT * 8 * SUB;          // first fragment of the direction layer (the position layer is whole chunks)
    static_assert(DF0 % 16 == 0, "the position layer must end on a chunk boundary");
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
        {
            const char* z = P.ctx + P.dz0_off + st * 8 * (int64_t)TB + lane * 16;
            f32x16 acc[PT];
#pragma unroll
            for (int m = 0; m < PT; ++m) acc[m] = f32x16{};
            // K tile t multiplied while tile t + 1 is in flight; rolled, as in dino_grad_kernel
            Act b = IO::template load_g<Act>(z);
#pragma unroll 1
            for (int t = 0; t < 8; ++t) {
                Act nb = b;
                if (t < 7) nb = IO::template load_g<Act>(z + (t + 1) * TB);
#pragma unroll
                for (int m = 0; m < PT; ++m)
#pragma unroll
                    for (int s = 0; s < SUB; ++s) {
                        const frag_t a = *(const NRF_LDS frag_t*)(frags + ((m * 8 + t) * SUB + s) * kFragBytes);
                        Mode::mma(acc[m], a, b, s);
                    }
                b = nb;
            }
            if constexpr (!V2) {
                if (P.d_x_enc && live) {
                    float* out = P.d_x_enc + raw * pe_dim(kInputGradPosFreq);
#pragma unroll
                    for (int u = 0; u < 16 * PT; ++u) {
                        const int idx = pe_ref_index(kInputGradPosFreq, u, h);
                        if (idx >= 0) out[idx] = acc[u >> 4][u & 15];
                    }
                }
            }
            if (P.d_positions) {
                const float p[3] = {P.positions[sid * 3], P.positions[sid * 3 + 1], P.positions[sid * 3 + 2]};
                float d[3];
                encoding_adjoint<PT>(acc, p, kInputGradPosFreq, h, d);
                if (live && h == 0) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) P.d_positions[raw * 3 + k] = d[k];
                }
            }
        }
        if constexpr (V2) {
            if (P.d_directions) {
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
}

}  // namespace nrf
