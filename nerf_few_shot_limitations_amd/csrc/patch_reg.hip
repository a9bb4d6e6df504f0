// patch_reg.hip -- the fused training step's loss launch with RegNeRF's depth-smoothness term on patches of unseen views (nerfhip.h:
// nrf_composite_patch_loss_backward, nrf_patch_terms_finish).  A batch of R rays is R_s supervised rays followed by N_p patches of
// P x P rays, patch-major, row-major inside a patch: ray (i, j) of patch p is row R_s + p P^2 + i P + j.
//
//   patch_loss_backward_kernel<false, *> : reg_loss_backward_kernel<false> (ray_reg.hip) on the supervised rays, one WAVE per ray; then
//                                       one WORKGROUP per patch: its four waves composite the patch's rays and leave their depths
//                                       in LDS, a barrier, every wave forms dL/d depth of its rays from the neighbours' depths and
//                                       runs the compositor backward with it (zero colour gradient, the target-free terms as on any
//                                       ray), one wave sums the patch's squared differences.  Both kinds of item go through ONE
//                                       walk per workgroup (see there), the barriers under its block-uniform `patch` flag.
//   patch_loss_backward_kernel<true, *>  : the same on the compacted rows of a step under an occupancy grid.
//   <*, true> is launched with N_p > 0: the compositor bodies with composite_core.hpp's FINE, whose transmittance behind a nearly
//   opaque sample and whose suffix sums keep their digits -- the float64 bars on the patch rows need them; <*, false> with N_p = 0:
//   the parent's instantiations, for the parent's bits.
//   patch_terms_finish_kernel         : one workgroup forms the step's seven loss values from ray_terms and patch_terms.
//
// The exchange between the compositor forward and its backward is the P^2 floats of LDS: no second launch, no atomics, two runs
// give the same bits.  The supervised rays' arithmetic is the parent's with R_s where the colour and depth terms divide, so with
// N_p = 0 every output is the parent's bits.  The pointers touched once per ray, the regularisers' values and the patch geometry
// ride in vector registers as in the parent: the scalar file has no room for them next to the scans' masks.
#include <algorithm>

#include "kernels.hpp"
#include "composite_core.hpp"

namespace nrf {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPatch = 16;         // P <= 16: P^2 floats of LDS, at most 64 rays per wave

inline unsigned grid_for(int64_t n, int block, int64_t cap) {
    int64_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// The patch term as the kernel takes it (nerfhip.h: nrf_patch_reg)
struct PatchArgs {
    int64_t n_sup;                    // R_s
    int64_t n_patches;                // N_p
    int P;
    float gd_scale;                   // 2 depth_smooth_weight / (N_p (P-1)^2)
    float* patch_terms;               // (N_p): DS_p
    float* patch_depth;               // (N_p, P, P) or NULL
};

// ray_loss (5,R): squared rgb error | sum of w^2 | |depth - target_depth| | D_r | O_r; rows 0 and 2 of a patch ray are 0
// FINE (composite_core.hpp; launched with N_p > 0): the transmittance factor from e itself and the true exclusive suffix.  Without
// it (N_p = 0) the compositor bodies are the parent's instantiations and the outputs the parent's bits.
template <bool IDX, bool FINE>
__global__ void __launch_bounds__(kBlock) patch_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                     int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                     int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                     float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                     int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                     float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                     const LossExt ext, const RayReg reg, const int32_t* __restrict__ slot,
                                                                     const PatchArgs pa) {
    __shared__ float seg[kWaves][3 * kMaxSegments];               // per wave: seg_T | the two prefix carries of the distortion scans
    __shared__ float dep[kMaxPatch * kMaxPatch];                  // the depths of the workgroup's patch
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t gtid = blockIdx.x * (int64_t)kBlock + threadIdx.x, n_threads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = gtid; i < zero_n; i += n_threads) zero_buf[i] = 0.0f;
    const float* tdepth = ext.target_depth;
    asm volatile("" : "+v"(target), "+v"(pred), "+v"(ray_loss), "+v"(tdepth));
    RayReg rr = reg;
    float gd_scale = ext.gd_scale;
    asm volatile("" : "+v"(rr.dist_scale), "+v"(rr.kappa), "+v"(rr.occ_scale), "+v"(rr.occ_inv), "+v"(rr.occ_m), "+v"(gd_scale));
    NoiseSrc ns = ext.noise;
    float gw_scale = ext.gw_scale;
    asm volatile("" : "+v"(ns.std), "+v"(ns.n), "+v"(ns.seed), "+v"(gw_scale));
    int64_t n_sup = pa.n_sup, n_patches = pa.n_patches;
    int P = pa.P;
    float* patch_terms = pa.patch_terms;
    float* patch_depth = pa.patch_depth;
    float smooth_scale = pa.gd_scale;
    asm volatile("" : "+v"(patch_terms), "+v"(patch_depth), "+v"(smooth_scale), "+v"(n_sup), "+v"(n_patches), "+v"(P));
    // (and, with the walk's state on top of the parent's, the strides, the row count and three more pointers)
    asm volatile("" : "+v"(n_rays), "+v"(white_bkgd), "+v"(rgb_stride), "+v"(sigma_stride), "+v"(d_rgb_stride), "+v"(d_sigma_stride));
    asm volatile("" : "+v"(d_rgb), "+v"(d_sigma), "+v"(rays_d), "+v"(z));
    const float count = 3.0f * (float)n_sup;
    const float scale = 2.0f * weight / count;
    const int PP = P * P;
    // One walk per workgroup over its items, so that each compositor body is instantiated once (two copies of each: 25 - 29 spilled
    // SGPRs): first its groups of kWaves supervised rays -- wave w takes ray sup + w of the group, the parent's one wave per ray, and
    // keeps the ray's loss gradient in registers between its forward and its backward -- then its patches.  `patch`, sup, p, kn are
    // block-uniform and k is wave-uniform: the two barriers stand under `patch` alone, a supervised ray meets none.
    int64_t sup = (int64_t)blockIdx.x * kWaves;          // the first ray of the workgroup's next supervised group
    int64_t p = blockIdx.x;                              // its next patch
    int64_t sup_step = (int64_t)gridDim.x * kWaves, p_step = gridDim.x;
    asm volatile("" : "+v"(sup), "+v"(p), "+v"(sup_step), "+v"(p_step));          // (the walk's state rides in vector registers too)
    for (;;) {
        const bool patch = sup >= n_sup;
        if (patch && p >= n_patches) break;
        const int64_t base = patch ? n_sup + p * PP : sup;
        const int kn = patch ? PP : (int)std::min<int64_t>(kWaves, n_sup - sup);
        float gr = 0.0f, gg = 0.0f, gb = 0.0f, gd_own = 0.0f;        // a supervised ray's dL/d rgb_map, dL/d depth
        // phase 1: wave w composites rays w, w + 4, ... of the item; a patch leaves their depths in LDS
        for (int k = wv; k < kn; k += kWaves) {
            const int64_t r = base + k;
            RaySums o = composite_ray<true, IDX, FINE>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, nullptr, ns, slot);
            if (white_bkgd) {
                const float bg = __fsub_rn(1.0f, o.acc);
                o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
            }
            float se = 0.0f, ad = 0.0f;                  // the ray's squared colour error and |depth error|: 0 on a patch ray
            if (!patch) {
                const float dr = o.r - target[r * 3], dg = o.g - target[r * 3 + 1], db = o.b - target[r * 3 + 2];
                const float dd = tdepth ? __fsub_rn(o.depth, tdepth[r]) : 0.0f;
                gd_own = dd > 0.0f ? gd_scale : (dd < 0.0f ? -gd_scale : 0.0f);          // l1_loss: sign(0) = 0
                gr = scale * dr; gg = scale * dg; gb = scale * db;
                se = dr * dr + dg * dg + db * db; ad = fabsf(dd);
            }
            if (lane == 0) {
                if (patch) {
                    dep[k] = o.depth;
                    if (patch_depth) patch_depth[p * PP + k] = o.depth;
                }
                ray_loss[n_rays + r] = o.w2; ray_loss[2 * n_rays + r] = ad;
                if (pred) { pred[r * 3] = o.r; pred[r * 3 + 1] = o.g; pred[r * 3 + 2] = o.b; }
                ray_loss[r] = se;
            }
        }
        if (patch) __syncthreads();
        // phase 2: the compositor backward; dL/d depth of patch ray (i, j) comes from its own anchor and from the anchors to its left
        // and above
        for (int k = wv; k < kn; k += kWaves) {
            const int64_t r = base + k;
            float gd = gd_own;
            if (patch) {
                const int i = k / P, j = k - i * P;
                const float c = dep[k];
                float t = 0.0f;
                if (i < P - 1 && j < P - 1) t = __fadd_rn(__fsub_rn(c, dep[k + 1]), __fsub_rn(c, dep[k + P]));
                if (i < P - 1 && j > 0) t = __fsub_rn(t, __fsub_rn(dep[k - 1], c));
                if (i > 0 && j < P - 1) t = __fsub_rn(t, __fsub_rn(dep[k - P], c));
                gd = __fmul_rn(smooth_scale, t);
            }
            float terms[2];                              // D_r, O_r
            composite_backward_ray<true, false, IDX, true, FINE>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, white_bkgd, gr, gg, gb, gd,
                                                           nullptr, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, seg[wv], ns, gw_scale, nullptr,
                                                           nullptr, slot, rr, terms);
            if (lane == 0) { ray_loss[3 * n_rays + r] = terms[0]; ray_loss[4 * n_rays + r] = terms[1]; }
        }
        if (patch) {
            // DS_p: wave 0, lane l adds up anchors l, l + 64, ... in that order, then the wave's fixed tree
            if (wv == 0) {
                const int Q = P - 1;
                float ds = 0.0f;
                for (int a = lane; a < Q * Q; a += 64) {
                    const int i = a / Q, j = a - i * Q, k = i * P + j;
                    const float c = dep[k];
                    const float da = __fsub_rn(c, dep[k + 1]), db = __fsub_rn(c, dep[k + P]);
                    ds = __fadd_rn(ds, __fadd_rn(__fmul_rn(da, da), __fmul_rn(db, db)));
                }
                ds = wave_sum(ds);
                if (lane == 0) patch_terms[p] = ds;
            }
            __syncthreads();                             // the next patch overwrites dep
            p += p_step;
        } else {
            sup += sup_step;
        }
    }
}

// losses7 = [total, rgb, depth, reg, dist, occ, smooth] with the divisors of the batch layout: rgb 3 R_s, depth R_s, reg R S, dist
// and occ R, smooth N_p (P-1)^2.  One workgroup, every partial sum in a fixed order.
struct FinishArgs {
    int64_t n_rays, n_sup, n_patches;
    float rgb_div, depth_div, reg_div, ray_div, smooth_div;           // the divisors, 0 where a term has none (smooth with N_p = 0)
    float rgb_weight, depth_weight, reg_weight, dist_weight, occ_weight, smooth_weight;
};
__global__ void __launch_bounds__(1024) patch_terms_finish_kernel(const float* __restrict__ ray_terms, const float* __restrict__ patch_terms,
                                                                  const FinishArgs a, float* __restrict__ losses7) {
    __shared__ float part[6][16];
    float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t i = threadIdx.x; i < a.n_sup; i += 1024) {
        s[0] = __fadd_rn(s[0], ray_terms[i]);
        s[1] = __fadd_rn(s[1], ray_terms[2 * a.n_rays + i]);
    }
    for (int64_t i = threadIdx.x; i < a.n_rays; i += 1024) {
        s[2] = __fadd_rn(s[2], ray_terms[a.n_rays + i]);
        s[3] = __fadd_rn(s[3], ray_terms[3 * a.n_rays + i]);
        s[4] = __fadd_rn(s[4], ray_terms[4 * a.n_rays + i]);
    }
    for (int64_t i = threadIdx.x; i < a.n_patches; i += 1024) s[5] = __fadd_rn(s[5], patch_terms[i]);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        s[k] = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            t[k] = 0.0f;
            for (int w = 0; w < 16; ++w) t[k] = __fadd_rn(t[k], part[k][w]);
        }
        const float l_rgb = t[0] / a.rgb_div, l_depth = t[1] / a.depth_div, l_reg = t[2] / a.reg_div;
        const float l_dist = t[3] / a.ray_div, l_occ = t[4] / a.ray_div;
        const float l_smooth = a.smooth_div > 0.0f ? t[5] / a.smooth_div : 0.0f;
        float total = __fmul_rn(a.rgb_weight, l_rgb);
        total = __fadd_rn(total, __fmul_rn(a.depth_weight, l_depth));
        total = __fadd_rn(total, __fmul_rn(a.reg_weight, l_reg));
        total = __fadd_rn(total, __fmul_rn(a.dist_weight, l_dist));
        total = __fadd_rn(total, __fmul_rn(a.occ_weight, l_occ));
        total = __fadd_rn(total, __fmul_rn(a.smooth_weight, l_smooth));
        losses7[0] = total; losses7[1] = l_rgb; losses7[2] = l_depth; losses7[3] = l_reg;
        losses7[4] = l_dist; losses7[5] = l_occ; losses7[6] = l_smooth;
    }
}

}  // namespace

int launch_composite_patch_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                                         int64_t n_rays, int S, int white_bkgd, const float* target, const LossTerms& lt, const RayRegTerms& rt,
                                         const PatchRegTerms& pt, const int32_t* slot, float* pred, float* d_rgb, int d_rgb_stride, float* d_sigma,
                                         int d_sigma_stride, float* ray_terms, float* zero_buf, int64_t zero_n, float* patch_terms,
                                         float* patch_depth, hipStream_t s) {
    const int P = pt.patch_size;
    if (P < 2 || P > kMaxPatch || pt.n_patches < 0) return NRF_EINVAL;
    const int64_t n_sup = n_rays - pt.n_patches * P * P;
    if (n_rays <= 0 || n_sup < 1 || S < 1 || S > 64 * kMaxSegments) return NRF_EINVAL;
    if (pt.n_patches > 0 && !patch_terms) return NRF_EINVAL;
    // the target-free terms divide by R as in the parent; the colour and depth terms by R_s
    LossExt ext = loss_ext_of(lt, n_rays, S);
    ext.gd_scale = lt.target_depth ? lt.depth_weight / (float)n_sup : 0.0f;
    RayReg reg{};
    if (rt.dist_weight > 0.0f) {
        reg.dist_scale = rt.dist_weight / (float)n_rays;
        reg.kappa = rt.dist_inv_span;
    }
    if (rt.occ_weight > 0.0f) {
        reg.occ_m = std::min(rt.occ_samples, S);
        reg.occ_inv = 1.0f / (float)reg.occ_m;
        reg.occ_scale = rt.occ_weight / ((float)n_rays * (float)reg.occ_m);
    }
    PatchArgs pa{};
    pa.n_sup = n_sup; pa.n_patches = pt.n_patches; pa.P = P;
    pa.gd_scale = pt.n_patches > 0 ? 2.0f * pt.depth_smooth_weight / ((float)pt.n_patches * (float)((P - 1) * (P - 1))) : 0.0f;
    pa.patch_terms = patch_terms; pa.patch_depth = patch_depth;
    const int64_t work = std::max(std::max(n_sup * 64, (zero_n + 3) / 4), pt.n_patches * kBlock);
    const dim3 grid(grid_for(work, kBlock, 16384)), block(kBlock);
    // with patches the compositor bodies of better conditioning; without, the parent's, for the parent's bits
    auto* kernel = slot ? (pt.n_patches > 0 ? patch_loss_backward_kernel<true, true> : patch_loss_backward_kernel<true, false>)
                        : (pt.n_patches > 0 ? patch_loss_backward_kernel<false, true> : patch_loss_backward_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, rgb, rgb_stride, sigma, sigma_stride, z, rays_d, n_rays, S, white_bkgd, target, lt.rgb_weight, pred,
                       d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, ext, reg, slot, pa);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_patch_terms_finish(const float* ray_terms, int64_t n_rays, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                              const float* patch_terms, float* losses7, hipStream_t s) {
    const int P = pt.patch_size;
    if (P < 2 || P > kMaxPatch || pt.n_patches < 0) return NRF_EINVAL;
    const int64_t n_sup = n_rays - pt.n_patches * P * P;
    if (n_rays <= 0 || n_sup < 1 || S < 1) return NRF_EINVAL;
    FinishArgs a{};
    a.n_rays = n_rays; a.n_sup = n_sup; a.n_patches = pt.n_patches;
    a.rgb_div = 3.0f * (float)n_sup; a.depth_div = (float)n_sup; a.reg_div = (float)n_rays * (float)S; a.ray_div = (float)n_rays;
    a.smooth_div = (float)pt.n_patches * (float)((P - 1) * (P - 1));
    a.rgb_weight = lt.rgb_weight; a.depth_weight = lt.target_depth ? lt.depth_weight : 0.0f; a.reg_weight = lt.reg_weight;
    a.dist_weight = rt.dist_weight; a.occ_weight = rt.occ_weight; a.smooth_weight = pt.depth_smooth_weight;
    hipLaunchKernelGGL(patch_terms_finish_kernel, dim3(1), dim3(1024), 0, s, ray_terms, patch_terms, a, losses7);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
