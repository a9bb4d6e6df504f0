// train_shared.hip -- what the training paths of all network families share: parameter re-pack, Adam, the weight gradients
// (train_impl.hpp: weight_grad_kernel) and the size of the saved-tensor context
#include "train_shared_core.hpp"
#include "freq_mask_launch.hpp"

namespace nrf {

// ---------------------------------------------------------------------------------------------
// parameter re-pack and Adam
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) repack3_kernel(const float* __restrict__ flat, const Repack3Args a) {
    const int64_t total = a.n[0] + a.n[1] + a.n[2];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int k = 0;
        int64_t j = i;
        if (j >= a.n[0]) { j -= a.n[0]; k = 1; if (j >= a.n[1]) { j -= a.n[1]; k = 2; } }
        if (a.mode[k] == NRF_MMA_F32) {
            const int sidx = a.src[k][j];
            ((float*)a.out[k])[j] = sidx >= 0 ? flat[sidx] : 0.0f;
        } else {
            const int2 sp = *(const int2*)(a.src[k] + 2 * j);
            const float x = sp.x >= 0 ? flat[sp.x] : 0.0f, y = sp.y >= 0 ? flat[sp.y] : 0.0f;
            ((uint32_t*)a.out[k])[j] = convert_pair(x, y, a.mode[k], j);
        }
    }
}

// Sum of x[0..n) by one 256-thread workgroup in a fixed order (thread t: elements t, t + 256, ...; one butterfly; four partial
// sums): reproducible run to run, the same value in every thread.  `part`: four floats of LDS, not reused before a barrier.
__device__ __forceinline__ float block_sum_fixed(const float* __restrict__ x, int64_t n, float* part) {
    float t = 0.0f;
    int64_t r = threadIdx.x;
    for (; r + 7 * 256 < n; r += 8 * 256) {               // eight loads in flight, added in order
        float q[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = x[r + k * 256];
#pragma unroll
        for (int k = 0; k < 8; ++k) t += q[k];
    }
    for (; r < n; r += 256) t += x[r];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// torch.optim.Adam (train.py:113-118; no amsgrad, weight decay added to the gradient, bias-corrected moments):
//   g += wd*p; m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// Side job (FusedStep): the loss VALUE of the step, loss_weight * mean over 3 n_rays values = loss_weight * sum(ray_loss) / (3 n_rays)
// with the rays' squared errors left by composite_loss_backward_kernel, added by one workgroup more than the update needs in a
// fixed order (block_sum_fixed).
// EXT (train_multiscale.py:259-266: clip_grad_norm_(params, max_norm) then optim.AdamW):
//   * every workgroup adds the <= 1024 partial sums of squares of grad_sqnorm_partials_kernel in the same fixed order, so all of
//     them hold the identical coefficient min(1, max_norm / (norm + 1e-6)) (torch's formula) with no grid-wide synchronisation
//     and no read-back; it scales g on load;
//   * decoupled decay: p *= 1 - lr wd in front of the moment update (torch.optim.AdamW), nothing added to the gradient;
//   * the side job sums the three rows of ray_terms: losses[4] = total, rgb (mse), depth (l1), reg (mean w^2).
template <bool EXT>
__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                  float wd, float bc1, float bc2_sqrt, const float* __restrict__ ray_loss, int64_t n_rays,
                                                  float loss_weight, float* __restrict__ loss, const AdamExt ext, int n_partials, float keep) {
    const int extra = ray_loss ? 1 : 0;
    if (extra && blockIdx.x == 0) {                       // one workgroup more than the update needs, the first to start: it does nothing else
        if constexpr (EXT) {
            __shared__ float parts[3][4];
            const float sq = block_sum_fixed(ray_loss, n_rays, parts[0]);
            const float w2 = block_sum_fixed(ray_loss + n_rays, n_rays, parts[1]);
            const float ad = block_sum_fixed(ray_loss + 2 * n_rays, n_rays, parts[2]);
            if (threadIdx.x == 0) {
                const float rgb = sq / (3.0f * (float)n_rays), depth = ad / (float)n_rays, reg = w2 / ((float)n_rays * (float)ext.n_samples);
                float total = ext.rgb_weight * rgb;                                       // nerf_mlp.py:249-255, in its order
                total += ext.depth_weight * depth;
                total += ext.reg_weight * reg;
                loss[0] = total; loss[1] = rgb; loss[2] = depth; loss[3] = reg;
            }
        } else {
            __shared__ float part[4];
            const float t = block_sum_fixed(ray_loss, n_rays, part);
            if (threadIdx.x == 0) *loss = loss_weight * t / (3.0f * (float)n_rays);
        }
        return;
    }
    float coef = 1.0f;
    if constexpr (EXT) {
        if (ext.partials) {
            __shared__ float npart[4];
            const float norm = sqrtf(block_sum_fixed(ext.partials, n_partials, npart));
            if (ext.max_norm > 0.0f) coef = fminf(1.0f, ext.max_norm / (norm + 1e-6f));
            if (ext.grad_norm && blockIdx.x == extra && threadIdx.x == 0) *ext.grad_norm = norm;
        }
    }
    const int64_t stride = (int64_t)(gridDim.x - extra) * blockDim.x;
    for (int64_t i = (blockIdx.x - extra) * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        float gi = g[i];
        float pi = p[i];
        if constexpr (EXT) {
            gi = __fmul_rn(gi, coef);
            if (ext.decoupled) pi = __fmul_rn(pi, keep);
            else if (wd != 0.0f) gi = __fadd_rn(gi, __fmul_rn(wd, pi));
        } else {
            if (wd != 0.0f) gi = __fadd_rn(gi, __fmul_rn(wd, pi));
        }
        const float mi = __fadd_rn(__fmul_rn(b1, m[i]), __fmul_rn(1.0f - b1, gi));
        const float vi = __fadd_rn(__fmul_rn(b2, v[i]), __fmul_rn(__fmul_rn(1.0f - b2, gi), gi));
        m[i] = mi; v[i] = vi;
        const float denom = __fadd_rn(sqrtf(vi) / bc2_sqrt, eps);
        p[i] = __fsub_rn(pi, __fmul_rn(lr / bc1, mi / denom));
    }
}

// Partial sums of squares of the flat gradient vector for the clip coefficient: workgroup b leaves the sum over its elements
// (b * 256 + t, + gridDim * 256, ...) in partials[b].  Fixed order, no atomics: bit-reproducible.  A thread's serial chain is in
// double (any n); behind it are a 6-level butterfly and 3 adds in float, and in the optimiser <= 4 + 6 + 3 more: (L + d) 2^-24
// stays below 1e-5 relative (the terms are non-negative).
__global__ void __launch_bounds__(256) grad_sqnorm_partials_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials) {
    __shared__ float part[4];
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {         // four loads in flight, added in order
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = g[i + k * stride];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)q[k] * (double)q[k];
    }
    for (; i < n; i += stride) { const float q = g[i]; acc += (double)q * (double)q; }
    float t = (float)acc;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) t += __shfl_xor(t, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// Second stage of the weight gradients: sum the workgroups' partial sums of a job in a fixed order and scatter them
// through the job's row / column maps into the flat gradient vector.  One block per (job, wave, tile) = 16 registers x 64
// lanes.  The only atomics left are the adds into `grad` (a weight shared by two jobs -- the fusion block of V3 -- receives
// two of them; a + b = b + a, so the result does not depend on their order): gradients are bit-reproducible run to run.
__global__ void __launch_bounds__(256) weight_grad_reduce_kernel(const GradKArgs P) {
    weight_grad_reduce_body(P, NoScale{});
}

namespace {

template <class Mode> constexpr int mode_of() { return NRF_MMA_F32; }
template <> constexpr int mode_of<ModeBF16>() { return NRF_MMA_BF16; }
template <> constexpr int mode_of<ModeF16>() { return NRF_MMA_F16; }

template <class Mode, int ST>
int run_weight_grad(const DeviceNet& net, const TrainDev& t, const TrainKArgs& k, float* grad, hipStream_t s, std::string& err) {
    auto kernel = weight_grad_kernel<Mode, ST>;
    constexpr int kLds = 2 * ST * 16 * tile_bytes<Mode>();
    static_assert(kLds <= 160 * 1024, "weight-gradient staging exceeds the LDS");
    static unsigned char done[64] = {};
    const int prepared = prepare(kernel, net.device, done, err, kLds);
    if (prepared != NRF_OK) return prepared;
    GradKArgs g{};
    g.ctx = k.ctx; g.grad = grad; g.maps = t.maps; g.n_jobs = t.n_jobs; g.n_tiles32 = tiles32(k.n);
    for (int j = 0; j < t.n_jobs; ++j) {
        g.jobs[j].x_off = k.slot_off[t.job_x_slot[j]];
        g.jobs[j].dz_off = k.slot_off[t.job_dz_slot[j]];
        g.jobs[j].KT = t.job_KT[j]; g.jobs[j].MT = t.job_MT[j];
        g.jobs[j].x_stride = t.slot_tiles[t.job_x_slot[j]]; g.jobs[j].dz_stride = t.slot_tiles[t.job_dz_slot[j]];
        g.jobs[j].x_first = t.job_x_first[j];
        g.jobs[j].map_off = j * kMapStride;
    }
    const unsigned grid = (unsigned)wgrad_grid(t, mode_of<Mode>(), g.n_tiles32, g.first_block);
    g.partial = (float*)(k.ctx + k.partial_off);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(512), kLds, s, g);
    if (const FreqMaskArgs* f = t.freq[mode_of<Mode>()]) launch_weight_grad_reduce_masked(g, *f, s);     // the mode's streams were packed under a mask
    else hipLaunchKernelGGL(weight_grad_reduce_kernel, dim3((unsigned)(64 * t.n_jobs)), dim3(256), 0, s, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = std::string("weight gradient launch: ") + hipGetErrorString(e); return NRF_EHIP; }
    return NRF_OK;
}

}  // namespace

int64_t train_ctx_bytes(const TrainDev& t, int mode, int64_t n) {
    int64_t tiles = 0;
    for (int i = 0; i < t.n_slots; ++i) tiles += t.slot_tiles[i];
    if (n <= 0) return 0;
    const int64_t nt = tiles32(n);
    return nt * (tiles * tile_bytes_of(mode) + (int64_t)t.n_mask_slots * kFragBytes + 32 * (int64_t)t.aux_floats * 4) +
           (int64_t)wgrad_grid(t, mode, nt, nullptr) * kPartialFloats * 4;
}

int launch_weight_grad(const DeviceNet& net, const TrainDev& t, int mode, const TrainKArgs& k, float* grad, hipStream_t s, std::string& err) {
    switch (mode) {
        case NRF_MMA_BF16: return run_weight_grad<ModeBF16, 2>(net, t, k, grad, s, err);
        case NRF_MMA_F16:  return run_weight_grad<ModeF16, 2>(net, t, k, grad, s, err);
        default:           return run_weight_grad<ModeF32, 1>(net, t, k, grad, s, err);
    }
}

int launch_repack3(const float* flat, const int32_t* const src[3], const int64_t n_elems[3], const int modes[3], void* const out[3], hipStream_t s,
                   const FreqMaskArgs* freq) {
    Repack3Args a{};
    int64_t total = 0;
    for (int k = 0; k < 3; ++k) {
        a.src[k] = src[k]; a.out[k] = out[k]; a.mode[k] = modes[k];
        a.n[k] = src[k] ? (modes[k] == NRF_MMA_F32 ? n_elems[k] : n_elems[k] / 2) : 0;
        total += a.n[k];
    }
    if (total <= 0) return NRF_OK;
    const int64_t blocks = (total + 255) / 256;
    if (freq) launch_repack3_masked(flat, a, (unsigned)(blocks < 4096 ? blocks : 4096), *freq, s);
    else hipLaunchKernelGGL(repack3_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, flat, a);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

static unsigned adam_blocks(int64_t n) { return (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096); }

int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd, int step,
                const float* ray_loss, int64_t n_rays, float loss_weight, float* loss, hipStream_t s) {
    if (n <= 0) return NRF_OK;
    const float bc1 = 1.0f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(b2, (float)step));
    const unsigned blocks = adam_blocks(n) + (ray_loss ? 1u : 0u);
    hipLaunchKernelGGL(adam_kernel<false>, dim3(blocks), dim3(256), 0, s, p, g, m, v, n, lr, b1, b2, eps,
                       wd, bc1, bc2_sqrt, ray_loss, n_rays, loss_weight, loss, AdamExt{}, 0, 1.0f);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_grad_sqnorm_partials(const float* g, int64_t n, float* partials, hipStream_t s) {
    if (n <= 0) return NRF_EINVAL;
    hipLaunchKernelGGL(grad_sqnorm_partials_kernel, dim3((unsigned)sqnorm_partials(n)), dim3(256), 0, s, g, n, partials);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd, int step,
                 const AdamExt& ext, hipStream_t s) {
    if (n <= 0) return NRF_OK;
    const float bc1 = 1.0f - powf(b1, (float)step);
    const float bc2_sqrt = sqrtf(1.0f - powf(b2, (float)step));
    const float keep = (float)(1.0 - (double)lr * (double)wd);          // torch.optim.AdamW: param.mul_(1 - lr * weight_decay)
    const unsigned blocks = adam_blocks(n) + (ext.ray_terms ? 1u : 0u);
    hipLaunchKernelGGL(adam_kernel<true>, dim3(blocks), dim3(256), 0, s, p, g, m, v, n, lr, b1, b2, eps,
                       wd, bc1, bc2_sqrt, ext.ray_terms, ext.n_rays, 0.0f, ext.losses, ext, sqnorm_partials(n), keep);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
