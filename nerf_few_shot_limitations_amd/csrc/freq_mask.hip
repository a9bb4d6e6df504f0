// freq_mask.hip -- the frequency mask on the positional encodings (nerfhip.h: nrf_model_set_freq_mask; freq_mask.hpp), in the two
// places that run once per step and see every weight:
//
//   repack3_masked_kernel            : repack3_kernel (train_shared.hip) with a masked element converted from
//                                      __fmul_rn(flat[src], scale[id]): the streams a re-pack would produce from a flat vector that
//                                      already holds the fp32 products.  Every render and chain kernel reads those streams, so the
//                                      forward, the dZ chain and the input gradients (their transposed tiles ride in the backward
//                                      stream) are the masked field's with no further code.
//   weight_grad_reduce_masked_kernel : weight_grad_reduce_kernel with each finished sum of a masked column multiplied by its scale
//                                      in front of the add -- dW = (dZ enc^T) diag m, and the saved enc is unmasked.  At the
//                                      scatter, not in a pass over the gradient vector: that vector accumulates across calls.
//
// The scale id of an element follows from its flat parameter index through one device table (int8, -1 = none), the scales
// themselves travel by value.  Elements without an id are bit for bit what the plain kernels write.
#include "freq_mask_launch.hpp"

namespace nrf {

namespace {

__device__ __forceinline__ float masked_load(const float* __restrict__ flat, int sidx, const FreqMaskArgs& F) {
    if (sidx < 0) return 0.0f;
    const float x = flat[sidx];
    const int id = F.ids[sidx];
    return id >= 0 ? __fmul_rn(x, F.scale[id]) : x;
}

__global__ void __launch_bounds__(256) repack3_masked_kernel(const float* __restrict__ flat, const Repack3Args a, const FreqMaskArgs F) {
    const int64_t total = a.n[0] + a.n[1] + a.n[2];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int k = 0;
        int64_t j = i;
        if (j >= a.n[0]) { j -= a.n[0]; k = 1; if (j >= a.n[1]) { j -= a.n[1]; k = 2; } }
        if (a.mode[k] == NRF_MMA_F32) {
            ((float*)a.out[k])[j] = masked_load(flat, a.src[k][j], F);
        } else {
            const int2 sp = *(const int2*)(a.src[k] + 2 * j);
            ((uint32_t*)a.out[k])[j] = convert_pair(masked_load(flat, sp.x, F), masked_load(flat, sp.y, F), a.mode[k], j);
        }
    }
}

struct ColumnScale {
    const FreqMaskArgs& F;
    __device__ __forceinline__ float operator()(int flat_index, float v) const {
        const int id = F.ids[flat_index];
        return id >= 0 ? __fmul_rn(v, F.scale[id]) : v;
    }
};

__global__ void __launch_bounds__(256) weight_grad_reduce_masked_kernel(const GradKArgs P, const FreqMaskArgs F) {
    weight_grad_reduce_body(P, ColumnScale{F});
}

}  // namespace

void launch_repack3_masked(const float* flat, const Repack3Args& a, unsigned grid, const FreqMaskArgs& f, hipStream_t s) {
    hipLaunchKernelGGL(repack3_masked_kernel, dim3(grid), dim3(256), 0, s, flat, a, f);
}

void launch_weight_grad_reduce_masked(const GradKArgs& g, const FreqMaskArgs& f, hipStream_t s) {
    hipLaunchKernelGGL(weight_grad_reduce_masked_kernel, dim3((unsigned)(64 * g.n_jobs)), dim3(256), 0, s, g, f);
}

}  // namespace nrf
