// sample_pdf_impl.hpp -- the inverse-cdf resampling of one ray per wave (ray_utils.py:86-143, intent): the body of sample_pdf_kernel
// (staged_kernels.hip) and of sample_pdf_sorted_kernel (hier_kernels.hip), which also hands out the ascending row of new samples.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nerfhip.h"

namespace nrf {
namespace {

// ---- a3: ray_utils.py:86-143 (intent) --------------------------------------------------------
// One WAVE per ray, LANE <-> sample: the rows of z, weights, the new samples and the union are read and written as contiguous
// 64-element segments; the cdf is a wave prefix sum; every search (inverse cdf, merge ranks) is a branch-free binary search over
// the wave's private LDS rows.  HBM-bound: 8 S + 4 Ni + 4 (S + Ni) bytes per ray.  The coarse depths z must ascend (they are a
// depth ladder); the new samples may arrive in any order (perturbed u) and are ranked before the merge.
__device__ __forceinline__ float wave_incl_sum(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_up(v, d, 64);
        if (lane >= d) v = __fadd_rn(v, u);
    }
    return v;
}
// number of leading elements of the ascending row a[0..n) that are <= x (upper bound) / < x (lower bound)
__device__ __forceinline__ int count_le(const float* a, int n, int top, float x) {
    int pos = 0;
    for (int step = top; step > 0; step >>= 1)
        if (pos + step <= n && a[pos + step - 1] <= x) pos += step;
    return pos;
}
__device__ __forceinline__ int count_lt(const float* a, int n, int top, float x) {
    int pos = 0;
    for (int step = top; step > 0; step >>= 1)
        if (pos + step <= n && a[pos + step - 1] < x) pos += step;
    return pos;
}
__host__ __device__ inline int top_pow2(int n) { int t = 1; while (t * 2 <= n) t *= 2; return t; }

// ---- the two reductions of ray_utils.py:107-109 in the order PyTorch's CPU kernels use (what "the reference's CPU renderer" computes) ----
// `weights.sum(-1)` (:107) is ATen's cascade_sum (aten/src/ATen/native/cpu/SumKernel.cpp): the contiguous row is read as vectors of
// 8 floats (also on AVX-512 hosts: checked bit for bit against torch 2.10 for S = 16 ... 4096 in the build container), four
// interleaved vector accumulators (ILP), each a cascade of 16-vector blocks over up to four levels; then the scalar tail, then the
// eight lanes left to right.  Lane l < 8 of the wave plays vector lane l; the result is broadcast.
__device__ __forceinline__ int ceil_log2_i(int x) { int l = 0; while ((1 << l) < x) ++l; return l; }

__device__ float torch_cpu_row_sum(const float* x, int S, int lane) {
    constexpr int V = 8, ILP = 4, LEVELS = 4;
    const int vec_size = S / V, size_ilp = vec_size / ILP;
    const int l = lane & (V - 1);
    float acc[LEVELS][ILP];
#pragma unroll
    for (int j = 0; j < LEVELS; ++j)
#pragma unroll
        for (int k = 0; k < ILP; ++k) acc[j][k] = 0.0f;
    const int quarter = ceil_log2_i(size_ilp) / LEVELS;
    const int level_power = quarter > 4 ? quarter : 4;
    const int level_step = 1 << level_power, level_mask = level_step - 1;
    int i = 0;
    while (i + level_step <= size_ilp) {
        for (int j = 0; j < level_step; ++j, ++i)
#pragma unroll
            for (int k = 0; k < ILP; ++k) acc[0][k] = __fadd_rn(acc[0][k], x[(i * ILP + k) * V + l]);
        bool go = true;
#pragma unroll
        for (int j = 1; j < LEVELS; ++j) {
            if (go) {
#pragma unroll
                for (int k = 0; k < ILP; ++k) { acc[j][k] = __fadd_rn(acc[j][k], acc[j - 1][k]); acc[j - 1][k] = 0.0f; }
                if ((i & (level_mask << (j * level_power))) != 0) go = false;
            }
        }
    }
    for (; i < size_ilp; ++i)
#pragma unroll
        for (int k = 0; k < ILP; ++k) acc[0][k] = __fadd_rn(acc[0][k], x[(i * ILP + k) * V + l]);
#pragma unroll
    for (int j = 1; j < LEVELS; ++j)
#pragma unroll
        for (int k = 0; k < ILP; ++k) acc[0][k] = __fadd_rn(acc[0][k], acc[j][k]);
    for (int v = size_ilp * ILP; v < vec_size; ++v) acc[0][0] = __fadd_rn(acc[0][0], x[v * V + l]);
#pragma unroll
    for (int k = 1; k < ILP; ++k) acc[0][0] = __fadd_rn(acc[0][0], acc[0][k]);
    float fin = 0.0f;
    for (int k = vec_size * V; k < S; ++k) fin = __fadd_rn(fin, x[k]);
#pragma unroll
    for (int k = 0; k < V; ++k) fin = __fadd_rn(fin, __shfl(acc[0][0], k, 64));
    return fin;
}

// `torch.cumsum` (:108) on the CPU accumulates in DOUBLE and rounds every prefix to float (ReduceOpsKernel.cpp: acc_type<float,
// false>; verified against torch 2.10).  For compositing weights (pdf >= 2^-18, sums < 2) every partial sum is a multiple of 2^-41
// below 2, i.e. exact in a double: the wave-parallel scan below then equals the sequential one bit for bit.
__device__ __forceinline__ double wave_incl_sum_f64(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double u = __shfl_up(v, d, 64);
        if (lane >= d) v = v + u;
    }
    return v;
}

// (the body of sample_pdf_kernel and of sample_pdf_sorted_kernel, which also hands out the ascending row `ssort`)
__device__ __forceinline__ void sample_pdf_rows(const float* __restrict__ z, const float* __restrict__ w, int64_t n_rays, int S, int Ni,
                                                const float* __restrict__ u_in, int64_t u_ray_stride, float* __restrict__ samples,
                                                float* __restrict__ z_union, float* __restrict__ samples_sorted) {
    extern __shared__ float lds_rows[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row_len = 3 * S + 3 * Ni + 1;
    float* cdf = lds_rows + (size_t)wave * row_len;         // S + 1 knots
    float* zl = cdf + S + 1;                                // S coarse depths
    float* smp = zl + S;                                    // Ni new samples, in the order of u
    float* ssort = smp + Ni;                                // Ni new samples, ascending
    float* uni = ssort + Ni;                                // S + Ni merged depths
    const int64_t wave0 = blockIdx.x * (int64_t)(blockDim.x >> 6) + wave;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int topS1 = top_pow2(S + 1), topS = top_pow2(S), topN = top_pow2(Ni);
    const float ustep = Ni > 1 ? 1.0f / (float)(Ni - 1) : 0.0f;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        const float* zr = z + r * S;
        const float* wr = w + r * S;
        // weights + 1e-5 (:104), parked in the cdf row; their sum (:107) in PyTorch's CPU order
        for (int s = lane; s < S; s += 64) {
            cdf[s + 1] = __fadd_rn(wr[s], 1e-5f);
            zl[s] = zr[s];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const float total = torch_cpu_row_sum(cdf + 1, S, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // cdf = [0, cumsum(pdf)] (:108-109): double-precision prefix sums of 64-sample segments, carried from segment to segment,
        // every knot rounded to float -- torch.cumsum's CPU arithmetic, so that the `denom < 1e-5` guard (:131) decides alike
        double carry = 0.0;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const float pdf = s < S ? cdf[s + 1] / total : 0.0f;
            const double incl = carry + wave_incl_sum_f64((double)pdf, lane);
            if (s < S) cdf[s + 1] = (float)incl;
            carry = __shfl(incl, 63, 64);
        }
        if (lane == 0) cdf[0] = 0.0f;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // inverse cdf (:112-133)
        for (int j = lane; j < Ni; j += 64) {
            float u;
            if (u_in) u = u_in[r * u_ray_stride + j];
            else u = Ni == 1 ? 0.0f : ((j < Ni / 2) ? __fmul_rn(ustep, (float)j) : __fsub_rn(1.0f, __fmul_rn(ustep, (float)(Ni - 1 - j))));
            const int idx = count_le(cdf, S + 1, topS1, u);          // searchsorted(cdf, u, right=True)  (:120)
            const int below = idx - 1 > 0 ? idx - 1 : 0;
            const int above = idx < S ? idx : S;
            // bin edges [z0, mids.., z_{S-1}]: the stratification intervals of ray_utils.py:73-75
            auto edge = [&](int k) -> float {
                if (k == 0) return zl[0];
                if (k == S) return zl[S - 1];
                return __fmul_rn(0.5f, __fadd_rn(zl[k], zl[k - 1]));
            };
            float denom = __fsub_rn(cdf[above], cdf[below]);
            if (denom < 1e-5f) denom = 1.0f;                                                 // (:131)
            const float t = __fsub_rn(u, cdf[below]) / denom;
            const float eb = edge(below), ea = edge(above);
            const float v = __fadd_rn(eb, __fmul_rn(t, __fsub_rn(ea, eb)));                  // (:133)
            smp[j] = v;
            if (samples) samples[r * Ni + j] = v;
        }
        if (!z_union && !samples_sorted) continue;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        // sorted union (:136): rank the new samples among themselves (stable), then merge ranks by binary search -- a coarse
        // depth goes in front of an equal new sample
        for (int j = lane; j < Ni; j += 64) {
            const float v = smp[j];
            int rank = 0;
            for (int i = 0; i < Ni; ++i) {
                const float o = smp[i];                                                      // same address in every lane: broadcast
                rank += (o < v || (o == v && i < j)) ? 1 : 0;
            }
            ssort[rank] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        if (samples_sorted)
            for (int k = lane; k < Ni; k += 64) samples_sorted[r * Ni + k] = ssort[k];
        if (!z_union) {                                          // (the fence: the next ray's ranking overwrites ssort)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            continue;
        }
        for (int k = lane; k < Ni; k += 64) {
            const float v = ssort[k];
            uni[k + count_le(zl, S, topS, v)] = v;
        }
        for (int a = lane; a < S; a += 64) {
            const float v = zl[a];
            uni[a + count_lt(ssort, Ni, topN, v)] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        float* out = z_union + r * (S + Ni);
        for (int k = lane; k < S + Ni; k += 64) out[k] = uni[k];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
}

// launch geometry of both kernels: waves per workgroup (one LDS row set each), workgroups, dynamic LDS bytes
struct SamplePdfGrid {
    int waves;
    int64_t blocks;
    size_t lds_bytes;
};
inline bool sample_pdf_grid(int64_t n_rays, int S, int Ni, SamplePdfGrid& g) {
    const int row_bytes = (3 * S + 3 * Ni + 1) * 4;          // one wave's LDS rows (cdf, depths, samples, sorted samples, union)
    g.waves = 4;
    while (g.waves > 1 && g.waves * row_bytes > 60 * 1024) g.waves >>= 1;
    if (g.waves * row_bytes > 60 * 1024) return false;
    g.blocks = (n_rays + g.waves - 1) / g.waves;
    if (g.blocks > 256 * 16) g.blocks = 256 * 16;            // grid-stride over the rays beyond that
    g.lds_bytes = (size_t)g.waves * row_bytes;
    return true;
}

}  // namespace
}  // namespace nrf
