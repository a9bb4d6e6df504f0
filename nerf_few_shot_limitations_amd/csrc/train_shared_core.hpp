// train_shared_core.hpp -- the bodies train_shared.hip's re-pack and weight-gradient reduce share with their masked variants
// (freq_mask.hip): the operand conversion, the re-pack's argument block and the reduce's summation and scatter.
#pragma once
#include "train_impl.hpp"

namespace nrf {

// out element i = convert(flat[src[i]]) (0 where src < 0); mode selects the operand type
// one 16-bit operand pair of the stream: bf16, f16, or the split mode's hi / lo part (pair i lies in fragment i/256; odd
// fragments carry the low parts: packing.cpp:pack_stream)
__device__ __forceinline__ uint32_t convert_pair(float a, float b, int mode, int64_t pair) {
    if (mode == NRF_MMA_BF16) return (uint32_t)pack_pair<bf16x2, false>(a, b);
    a = __builtin_amdgcn_fmed3f(a, -65504.0f, 65504.0f);      // f16-typed streams saturate (packing.cpp:pack_stream does the same on the host)
    b = __builtin_amdgcn_fmed3f(b, -65504.0f, 65504.0f);
    if (mode == NRF_MMA_F16X3 && ((pair >> 8) & 1)) {
        const f32x2 ab = {a, b};
        const f32x2 hf = __builtin_convertvector(__builtin_convertvector(ab, f16x2), f32x2);
        return (uint32_t)pack_pair<f16x2, false>(__fsub_rn(a, hf[0]), __fsub_rn(b, hf[1]));
    }
    return (uint32_t)pack_pair<f16x2, false>(a, b);
}

// forward stream, backward stream and bias table in ONE launch (an optimisation step re-packs all three): segment k holds
// n[k] work items -- pairs of 16-bit elements, or single fp32 values when mode[k] is NRF_MMA_F32
struct Repack3Args {
    const int32_t* src[3];
    void* out[3];
    int64_t n[3];
    int mode[3];
};

// weight_grad_reduce_kernel's body (train_shared.hip).  scale(flat index, sum) is what a weight's finished sum becomes in front of
// its add into the gradient vector: the identity there, the column's scale in freq_mask.hip.  Bias sums never pass through it.
struct NoScale {
    __device__ __forceinline__ float operator()(int, float v) const { return v; }
};
template <class Scale>
__device__ __forceinline__ void weight_grad_reduce_body(const GradKArgs& P, const Scale& scale) {
    const int job = blockIdx.x >> 6, wt = blockIdx.x & 63, wave = wt >> 3, tile = wt & 7;
    const GradJob J = P.jobs[job];
    constexpr int RT = 2, CT = 4;
    const int i = tile / CT, j = tile % CT;
    const int row0 = (wave & 3) * RT, col0 = (wave >> 2) * CT;
    const int b0 = P.first_block[job], b1 = P.first_block[job + 1];
    const int32_t* row_w = P.maps + J.map_off;
    const int32_t* row_b = row_w + 320;
    const int32_t* colm = row_b + 320;
    if (row0 + i < J.MT && col0 + j < J.KT) {
        // thread t: register group q = t >> 6, lane = t & 63: the 16 bytes that lane stored for registers 4q .. 4q+3
        const int q = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
        const f32x4* src = (const f32x4*)(P.partial + (int64_t)b0 * kPartialFloats + (wave * 8 + tile) * 16 * 64) + threadIdx.x;
        // the partial sums are added in workgroup order (fixed: bit-reproducible), but LOADED sixteen at a time: one load per
        // iteration and a wait on it is 32 HBM latencies in a row at the reference's batch (25 us for 61 MB, round-3 trace)
        f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
        constexpr int64_t kStep = kPartialFloats / 4;
        int b = b0;
        for (; b + 16 <= b1; b += 16, src += 16 * kStep) {
            f32x4 v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = src[k * kStep];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += v[k];
        }
        for (; b + 4 <= b1; b += 4, src += 4 * kStep) {
            f32x4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = src[k * kStep];
#pragma unroll
            for (int k = 0; k < 4; ++k) s += v[k];
        }
        for (; b < b1; ++b, src += kStep) s += *src;
        const int col = colm[32 * (col0 + j) + c];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int r = 4 * q + sub;
            const int o = 32 * (row0 + i) + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int w = row_w[o];
            if (w >= 0 && col >= 0) unsafeAtomicAdd(P.grad + w + col, scale(w + col, s[sub]));
        }
    }
    if (tile == 0 && wave < J.MT && threadIdx.x < 32) {
        const float* src = P.partial + (int64_t)b0 * kPartialFloats + 8 * 8 * 16 * 64 + 32 * wave + threadIdx.x;
        float s = 0.0f;
        int b = b0;
        for (; b + 16 <= b1; b += 16, src += 16 * (int64_t)kPartialFloats) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = src[k * (int64_t)kPartialFloats];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += v[k];
        }
        for (; b < b1; ++b, src += kPartialFloats) s += *src;
        const int bo = row_b[32 * wave + threadIdx.x];
        if (bo >= 0) unsafeAtomicAdd(P.grad + bo, s);
    }
}

}  // namespace nrf
