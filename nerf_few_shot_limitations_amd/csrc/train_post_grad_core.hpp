// train_post_grad_core.hpp -- the parts shared by the kernels that run behind a finished dZ chain and turn what it saved in the
// context into gradients with respect to the network's inputs: dino_grad_kernel (train_dino_grad_impl.hpp), input_grad_kernel
// (train_input_grad_impl.hpp) and input_grad_v3_kernel (train_input_grad_v3_impl.hpp).  Kernels of their own, not tails of the
// chain: the chain kernels sit at the register limit.  All three are built alike: the A operands are one or two small fragment
// streams of the packer (packing.cpp: first_linear_T, colour0_direction_T), (m, t, s) order (mlp_core.hpp), resident in LDS --
// loaded once per workgroup (post_grad_resident) -- and persistent waves walk the 32-sample tiles, one tile per wave and trip.  The
// saved dZ tiles are B-operand images as they lie (train_core.hpp), read straight from the context (post_grad_walk); a second
// layer, where there is one, is padded to a whole chunk in the stream but only its fragments are copied.  No atomics and one fixed
// order of every sum: a sample's gradient is bit-reproducible and independent of the batch around it.
#pragma once
#include "feature_map.hpp"
#include "train_impl.hpp"

namespace nrf {

constexpr int kPostGradWaves = 4;

// fragments of the resident stream: MT x 8 tile pairs of the first Linear^T, then (DIR) 1 x 4 of color_layers.0^T's direction tile
template <class Mode, int MT, bool DIR>
constexpr int post_grad_frags() { return (MT * 8 + (DIR ? 4 : 0)) * Mode::SUB; }
template <class Mode, int MT, bool DIR>
constexpr int post_grad_lds_bytes() { return post_grad_frags<Mode, MT, DIR>() * kFragBytes; }
// first fragment of the direction layer: every layer of a stream starts on a chunk boundary (packing.cpp:stream_sources)
template <class Mode, int MT>
constexpr int post_grad_dir_frag0() {
    static_assert(MT * 8 * Mode::SUB % 16 == 0, "the position layer must end on a chunk boundary");
    return MT * 8 * Mode::SUB;
}

// The first NF fragments of `wstream` copied into LDS by the whole workgroup -> this lane's 16 bytes of fragment 0.
template <int NF>
__device__ __forceinline__ const NRF_LDS char* post_grad_resident(const void* wstream, int lane, int wave) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int f = wave; f < NF; f += kPostGradWaves)
        *(i32x4*)(smem + f * kFragBytes + lane * 16) = *(const i32x4*)((const char*)wstream + f * kFragBytes + lane * 16);
    __syncthreads();
    return (const NRF_LDS char*)smem + lane * 16;
}

// Row `c` of 32-sample tile `st`: rows past the end read the last sample and write nothing.
struct PostGradRow {
    int64_t raw, sid;
    bool live;
    __device__ __forceinline__ PostGradRow(int64_t st, int c, int64_t n) : raw(st * 32 + c), sid(raw < n ? raw : n - 1), live(raw < n) {}
};

// acc1[m] (and, NS = 2, acc2[m]) = (fragments (m, 0..7, s) of the resident layer) x (the eight saved tiles at z1 (z2)): one or two
// saved streams that share their A fragments; z1, z2 point at this lane's 16 bytes of tile 0.  K tile t is multiplied while tile
// t + 1 is in flight.  A rolled loop: unrolled, the compiler hoists every fragment read and every tile load to the top and
// spills.  Per (m, s) the MFMAs run stream 1, then stream 2.  The streams are two arrays and two pointers by value, not one
// [NS][MT] array and an array of pointers: in that form dino_grad_kernel holds four scalar registers more.
template <class Mode, int MT, int NS>
__device__ __forceinline__ void post_grad_walk_n(const NRF_LDS char* frags, const char* z1, const char* z2, f32x16 (&acc1)[MT], f32x16 (&acc2)[MT]) {
    typedef typename Mode::Act Act;
    typedef typename Mode::frag_t frag_t;
    typedef ActIO<Mode> IO;
    constexpr int SUB = Mode::SUB, TB = tile_bytes<Mode>();
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        acc1[m] = f32x16{};
        if constexpr (NS == 2) acc2[m] = f32x16{};
    }
    Act b1 = IO::template load_g<Act>(z1), b2 = b1;
    if constexpr (NS == 2) b2 = IO::template load_g<Act>(z2);
#pragma unroll 1
    for (int t = 0; t < 8; ++t) {
        Act n1 = b1, n2 = b2;
        if (t < 7) {
            n1 = IO::template load_g<Act>(z1 + (t + 1) * TB);
            if constexpr (NS == 2) n2 = IO::template load_g<Act>(z2 + (t + 1) * TB);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int s = 0; s < SUB; ++s) {
                const frag_t a = *(const NRF_LDS frag_t*)(frags + ((m * 8 + t) * SUB + s) * kFragBytes);
                Mode::mma(acc1[m], a, b1, s);
                if constexpr (NS == 2) Mode::mma(acc2[m], a, b2, s);
            }
        b1 = n1;
        if constexpr (NS == 2) b2 = n2;
    }
}
template <class Mode, int MT>
__device__ __forceinline__ void post_grad_walk(const NRF_LDS char* frags, const char* z, f32x16 (&acc)[MT]) {
    post_grad_walk_n<Mode, MT, 1>(frags, z, z, acc, acc);
}
template <class Mode, int MT>
__device__ __forceinline__ void post_grad_walk(const NRF_LDS char* frags, const char* z1, const char* z2, f32x16 (&acc1)[MT], f32x16 (&acc2)[MT]) {
    post_grad_walk_n<Mode, MT, 2>(frags, z1, z2, acc1, acc2);
}

// The adjoint of one encoding (feature_map.hpp), one accumulator tile at a time: slots 16 M .. 16 M + 15 added onto this lane
// half's three sums, in slot order.  The kernel order gives lane half 0 the sine and lane half 1 the cosine of the same (frequency,
// coordinate): half 0 adds 2^f cos(2^f p_c) acc over its slots, half 1 adds -2^f sin(2^f p_c) acc, and the raw coordinates sit in
// slots 3L (x | z) and 3L+1 (y | -).  The trigonometry is the precise sincosf of the exact product p * 2^f in every mode.  Written
// with selects, not branches, on the frequency count: L is a run-time value for the directions, and a branch per slot around the
// (inlined) sincosf parks an exec mask each.
template <int M>
__device__ __forceinline__ void encoding_adjoint_tile(const f32x16& acc, const float (&p)[3], int L, int h, float (&d)[3]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        constexpr int u0 = 16 * M;
        const int u = u0 + r;
        const float a = acc[r];
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
}

// ... over NT tiles: a compile-time chain of per-tile calls.  Three tiles in ONE unrolled loop are more than the unroller takes (48
// inlined sincosf): the accumulators would be indexed at run time and land in scratch.
template <int NT, int M = 0>
__device__ __forceinline__ void encoding_adjoint_tiles(const f32x16 (&acc)[NT], const float (&p)[3], int L, int h, float (&d)[3]) {
    if constexpr (M < NT) {
        encoding_adjoint_tile<M>(acc[M], p, L, h, d);
        encoding_adjoint_tiles<NT, M + 1>(acc, p, L, h, d);
    }
}

// dL/d x of row `row` from dL/d e(x) in `acc`: the row's coordinates read from `x` (n,3), this lane half's share of the three
// sums, one cross-half add to join them, and lane half 0's store to `out` (n,3).
template <int NT>
__device__ __forceinline__ void encoding_adjoint_store(const f32x16 (&acc)[NT], const float* x, int L, const PostGradRow& row, int h, float* out) {
    const float p[3] = {x[row.sid * 3], x[row.sid * 3 + 1], x[row.sid * 3 + 2]};
    float d[3];
    d[0] = d[1] = d[2] = 0.0f;
    encoding_adjoint_tiles<NT>(acc, p, L, h, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = __fadd_rn(d[k], __shfl_xor(d[k], 32, 64));
    if (row.live && h == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[row.raw * 3 + k] = d[k];
    }
}

// dL/d directions of the V2 and V3 networks: the four saved tiles of dZ(color_layers.0) at `z` (this lane's 16 bytes of tile 0)
// against the direction layer's fragments DF0 .., then the adjoint of the direction encoding with its run-time frequency count.
template <class Mode, int DF0>
__device__ __forceinline__ void post_grad_directions(const NRF_LDS char* frags, const char* z, const float* directions, int dir_freq,
                                                     const PostGradRow& row, int h, float* d_directions) {
    typedef typename Mode::Act Act;
    typedef typename Mode::frag_t frag_t;
    constexpr int SUB = Mode::SUB, TB = tile_bytes<Mode>();
    f32x16 acc[1];
    acc[0] = f32x16{};
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        const Act b = ActIO<Mode>::template load_g<Act>(z + t * TB);
#pragma unroll
        for (int s = 0; s < SUB; ++s) {
            const frag_t a = *(const NRF_LDS frag_t*)(frags + (DF0 + t * SUB + s) * kFragBytes);
            Mode::mma(acc[0], a, b, s);
        }
    }
    encoding_adjoint_store<1>(acc, directions, dir_freq, row, h, d_directions);
}

}  // namespace nrf
