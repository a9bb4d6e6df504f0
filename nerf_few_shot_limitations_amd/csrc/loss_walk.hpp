// loss_walk.hpp -- what the fused training step's regularised loss launches share (ray_reg.hip, patch_reg.hip, info_reg.hip): the walk
// of a workgroup over a batch of supervised rays and patches, the body of the finish kernels, and the host's derivations of the
// kernels' arguments from the term structs of kernels.hpp.
//
// A batch of R rays is R_s supervised rays followed by N_p patches of P x P rays, patch-major, row-major inside a patch: ray (i, j)
// of patch p is row R_s + p P^2 + i P + j.  loss_walk runs reg_loss_backward_kernel's (ray_reg.hip) arithmetic on the supervised
// rays, one WAVE per ray; then one WORKGROUP per patch: its four waves composite the patch's rays and leave their depths in LDS, a
// barrier, every wave forms dL/d depth of its rays from the neighbours' depths and runs the compositor backward with it (zero
// colour gradient, the target-free terms as on any ray), one wave sums the patch's squared differences.  The exchange between the
// compositor forward and its backward is the P^2 floats of LDS: no second launch, no atomics, two runs give the same bits.  The
// supervised rays' arithmetic is ray_reg.hip's with R_s where the colour and depth terms divide, so with N_p = 0 every output is
// that kernel's bits.
#pragma once

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

// What the walk reads.  rgb, sigma, S and slot stay the kernel's arguments, in scalar registers; everything else -- the pointers
// touched once per ray, the regularisers' values, the noise source, the two scales of the multi-term loss, the patch geometry, the
// strides, the row count and the walk's own state -- rides in vector registers (loss_walk_prologue pins it there): the scalar file
// has no room for it next to the scans' masks.
struct LossWalk {
    const float *rgb, *sigma;
    const int32_t* slot;
    int S, lane, wv;
    const float *z, *rays_d, *target, *tdepth;
    float *pred, *ray_loss, *d_rgb, *d_sigma;
    int64_t n_rays;
    int white_bkgd, rgb_stride, sigma_stride, d_rgb_stride, d_sigma_stride;
    RayReg rr;
    NoiseSrc ns;
    float gd_scale, gw_scale;
    int64_t n_sup, n_patches;
    int P, PP;
    float *patch_terms, *patch_depth;
    float smooth_scale;               // PatchArgs::gd_scale
    float scale;                      // 2 rgb_weight / (3 R_s)
    int64_t gtid, n_threads;
    int64_t sup, p;                   // the first ray of the workgroup's first supervised group; its first patch
    int64_t sup_step, p_step;
};

// The head of a kernel that walks: the flat gradient vector's zero fill, and the walk's values pinned into vector registers
__device__ __forceinline__ void loss_walk_prologue(LossWalk& w, const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z,
                                                   const float* rays_d, int64_t n_rays, int S, int white_bkgd, const float* target, float weight,
                                                   float* pred, float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_loss,
                                                   float* zero_buf, int64_t zero_n, const LossExt& ext, const RayReg& reg, const int32_t* slot,
                                                   const PatchArgs& pa) {
    w.rgb = rgb; w.sigma = sigma; w.slot = slot; w.S = S;
    w.lane = threadIdx.x & 63; w.wv = threadIdx.x >> 6;
    w.gtid = blockIdx.x * (int64_t)kBlock + threadIdx.x; w.n_threads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = w.gtid; i < zero_n; i += w.n_threads) zero_buf[i] = 0.0f;
    w.target = target; w.pred = pred; w.ray_loss = ray_loss; w.tdepth = ext.target_depth;
    asm volatile("" : "+v"(w.target), "+v"(w.pred), "+v"(w.ray_loss), "+v"(w.tdepth));
    w.rr = reg; w.gd_scale = ext.gd_scale;
    asm volatile("" : "+v"(w.rr.dist_scale), "+v"(w.rr.kappa), "+v"(w.rr.occ_scale), "+v"(w.rr.occ_inv), "+v"(w.rr.occ_m), "+v"(w.gd_scale));
    w.ns = ext.noise; w.gw_scale = ext.gw_scale;
    asm volatile("" : "+v"(w.ns.std), "+v"(w.ns.n), "+v"(w.ns.seed), "+v"(w.gw_scale));
    w.n_sup = pa.n_sup; w.n_patches = pa.n_patches; w.P = pa.P;
    w.patch_terms = pa.patch_terms; w.patch_depth = pa.patch_depth; w.smooth_scale = pa.gd_scale;
    asm volatile("" : "+v"(w.patch_terms), "+v"(w.patch_depth), "+v"(w.smooth_scale), "+v"(w.n_sup), "+v"(w.n_patches), "+v"(w.P));
    w.n_rays = n_rays; w.white_bkgd = white_bkgd;
    w.rgb_stride = rgb_stride; w.sigma_stride = sigma_stride; w.d_rgb_stride = d_rgb_stride; w.d_sigma_stride = d_sigma_stride;
    asm volatile("" : "+v"(w.n_rays), "+v"(w.white_bkgd), "+v"(w.rgb_stride), "+v"(w.sigma_stride), "+v"(w.d_rgb_stride), "+v"(w.d_sigma_stride));
    w.d_rgb = d_rgb; w.d_sigma = d_sigma; w.rays_d = rays_d; w.z = z;
    asm volatile("" : "+v"(w.d_rgb), "+v"(w.d_sigma), "+v"(w.rays_d), "+v"(w.z));
    w.PP = w.P * w.P;
    w.scale = 2.0f * weight / (3.0f * (float)w.n_sup);
    w.sup = (int64_t)blockIdx.x * kWaves;
    w.p = blockIdx.x;
    w.sup_step = (int64_t)gridDim.x * kWaves; w.p_step = gridDim.x;
    asm volatile("" : "+v"(w.sup), "+v"(w.p), "+v"(w.sup_step), "+v"(w.p_step));
}

// One walk per workgroup over its items, so that each compositor body is instantiated once (two copies of each: 25 - 29 spilled
// SGPRs): first its groups of kWaves supervised rays -- wave w takes ray sup + w of the group, one wave per ray, and keeps the
// ray's loss gradient in registers between its forward and its backward -- then its patches.  `patch`, sup, p, kn are block-uniform
// and k is wave-uniform: the two barriers stand under `patch` alone, a supervised ray meets none.
// ray_loss (5,R): squared rgb error | sum of w^2 | |depth - target_depth| | D_r | O_r; rows 0 and 2 of a patch ray are 0.
// FINE (composite_core.hpp; launched with N_p > 0): the transmittance factor from e itself and the true exclusive suffix -- the
// float64 bars on the patch rows need their digits.  Without it (N_p = 0) the compositor bodies are reg_loss_backward_kernel's
// instantiations and the outputs its bits.
// UNIFORM_EXIT: the exit test through readfirstlane, for a kernel that goes on behind the walk -- a uniform branch needs no saved
// exec mask behind the loop: two scalar registers that a kernel which ends with the walk never holds.
// seg: per wave seg_T | the two prefix carries of the distortion scans; dep: the depths of the workgroup's patch.  w by value: by
// reference the dense kernels of info_reg.hip hold one vector register more.
template <bool IDX, bool FINE, bool UNIFORM_EXIT>
__device__ __forceinline__ void loss_walk(const LossWalk w, float (*seg)[3 * kMaxSegments], float* dep) {
    const int lane = w.lane, wv = w.wv, S = w.S, P = w.P, PP = w.PP;
    int64_t sup = w.sup, p = w.p;
    for (;;) {
        const bool patch = sup >= w.n_sup;
        if constexpr (UNIFORM_EXIT) {
            if (__builtin_amdgcn_readfirstlane((int)(patch && p >= w.n_patches))) break;
        } else {
            if (patch && p >= w.n_patches) break;
        }
        const int64_t base = patch ? w.n_sup + p * PP : sup;
        const int kn = patch ? PP : (int)std::min<int64_t>(kWaves, w.n_sup - sup);
        float gr = 0.0f, gg = 0.0f, gb = 0.0f, gd_own = 0.0f;        // a supervised ray's dL/d rgb_map, dL/d depth
        // phase 1: wave w composites rays w, w + 4, ... of the item; a patch leaves their depths in LDS
        for (int k = wv; k < kn; k += kWaves) {
            const int64_t r = base + k;
            RaySums o = composite_ray<true, IDX, FINE>(w.rgb, w.rgb_stride, w.sigma, w.sigma_stride, w.z, w.rays_d, r, S, lane, nullptr, w.ns, w.slot);
            if (w.white_bkgd) {
                const float bg = __fsub_rn(1.0f, o.acc);
                o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
            }
            float se = 0.0f, ad = 0.0f;                  // the ray's squared colour error and |depth error|: 0 on a patch ray
            if (!patch) {
                const float dr = o.r - w.target[r * 3], dg = o.g - w.target[r * 3 + 1], db = o.b - w.target[r * 3 + 2];
                const float dd = w.tdepth ? __fsub_rn(o.depth, w.tdepth[r]) : 0.0f;
                gd_own = dd > 0.0f ? w.gd_scale : (dd < 0.0f ? -w.gd_scale : 0.0f);          // l1_loss: sign(0) = 0
                gr = w.scale * dr; gg = w.scale * dg; gb = w.scale * db;
                se = dr * dr + dg * dg + db * db; ad = fabsf(dd);
            }
            if (lane == 0) {
                if (patch) {
                    dep[k] = o.depth;
                    if (w.patch_depth) w.patch_depth[p * PP + k] = o.depth;
                }
                w.ray_loss[w.n_rays + r] = o.w2; w.ray_loss[2 * w.n_rays + r] = ad;
                if (w.pred) { w.pred[r * 3] = o.r; w.pred[r * 3 + 1] = o.g; w.pred[r * 3 + 2] = o.b; }
                w.ray_loss[r] = se;
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
                gd = __fmul_rn(w.smooth_scale, t);
            }
            float terms[2];                              // D_r, O_r
            composite_backward_ray<true, false, IDX, true, FINE>(w.rgb, w.rgb_stride, w.sigma, w.sigma_stride, w.z, w.rays_d, r, S, lane, w.white_bkgd, gr,
                                                                 gg, gb, gd, nullptr, w.d_rgb, w.d_rgb_stride, w.d_sigma, w.d_sigma_stride, seg[wv], w.ns,
                                                                 w.gw_scale, nullptr, nullptr, w.slot, w.rr, terms);
            if (lane == 0) { w.ray_loss[3 * w.n_rays + r] = terms[0]; w.ray_loss[4 * w.n_rays + r] = terms[1]; }
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
                if (lane == 0) w.patch_terms[p] = ds;
            }
            __syncthreads();                             // the next patch overwrites dep
            p += w.p_step;
        } else {
            sup += w.sup_step;
        }
    }
}

// The step's loss values with the divisors of the batch layout: rgb 3 R_s, depth R_s, reg R S, dist, occ and entropy R, smooth and
// kl N_p (P-1)^2.
struct FinishArgs {
    int64_t n_rays, n_sup, n_patches;
    float rgb_div, depth_div, reg_div, ray_div, patch_div;            // patch_div = 0 with N_p = 0: a patch term is 0 then
    float rgb_weight, depth_weight, reg_weight, dist_weight, occ_weight, smooth_weight, ent_weight, kl_weight;
};

// losses[N + 1] = [total, rgb, depth, reg, dist, occ, smooth (, entropy, kl: N = 8)] from N running sums per thread.  One workgroup
// of BLOCK threads, every partial sum in a fixed order.
template <int N, int BLOCK>
__device__ __forceinline__ void terms_finish(const float* ray_terms, const float* patch_terms, const float* info_terms, const float* patch_kl,
                                             const FinishArgs& a, float* losses) {
    static_assert(N == 6 || N == 8, "six sums, or eight with the two information terms");
    __shared__ float part[N][BLOCK / 64];
    float s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0f;
    for (int64_t i = threadIdx.x; i < a.n_sup; i += BLOCK) {
        s[0] = __fadd_rn(s[0], ray_terms[i]);
        s[1] = __fadd_rn(s[1], ray_terms[2 * a.n_rays + i]);
    }
    for (int64_t i = threadIdx.x; i < a.n_rays; i += BLOCK) {
        if constexpr (N == 8) {
            if (info_terms) s[6] = __fadd_rn(s[6], info_terms[i]);
        }
        s[2] = __fadd_rn(s[2], ray_terms[a.n_rays + i]);
        s[3] = __fadd_rn(s[3], ray_terms[3 * a.n_rays + i]);
        s[4] = __fadd_rn(s[4], ray_terms[4 * a.n_rays + i]);
    }
    for (int64_t i = threadIdx.x; i < a.n_patches; i += BLOCK) {
        s[5] = __fadd_rn(s[5], patch_terms[i]);
        if constexpr (N == 8) {
            if (patch_kl) s[7] = __fadd_rn(s[7], patch_kl[i]);
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        s[k] = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            t[k] = 0.0f;
            for (int w = 0; w < BLOCK / 64; ++w) t[k] = __fadd_rn(t[k], part[k][w]);
        }
        const float l_rgb = t[0] / a.rgb_div, l_depth = t[1] / a.depth_div, l_reg = t[2] / a.reg_div;
        const float l_dist = t[3] / a.ray_div, l_occ = t[4] / a.ray_div;
        const float l_smooth = a.patch_div > 0.0f ? t[5] / a.patch_div : 0.0f;
        float l_ent = 0.0f, l_kl = 0.0f;
        if constexpr (N == 8) {
            l_ent = t[6] / a.ray_div;
            l_kl = a.patch_div > 0.0f ? t[7] / a.patch_div : 0.0f;
        }
        float total = __fmul_rn(a.rgb_weight, l_rgb);
        total = __fadd_rn(total, __fmul_rn(a.depth_weight, l_depth));
        total = __fadd_rn(total, __fmul_rn(a.reg_weight, l_reg));
        total = __fadd_rn(total, __fmul_rn(a.dist_weight, l_dist));
        total = __fadd_rn(total, __fmul_rn(a.occ_weight, l_occ));
        total = __fadd_rn(total, __fmul_rn(a.smooth_weight, l_smooth));
        if constexpr (N == 8) {
            total = __fadd_rn(total, __fmul_rn(a.ent_weight, l_ent));
            total = __fadd_rn(total, __fmul_rn(a.kl_weight, l_kl));
        }
        losses[0] = total; losses[1] = l_rgb; losses[2] = l_depth; losses[3] = l_reg;
        losses[4] = l_dist; losses[5] = l_occ; losses[6] = l_smooth;
        if constexpr (N == 8) { losses[7] = l_ent; losses[8] = l_kl; }
    }
}

// ---- the host's side: the kernels' arguments from the term structs (kernels.hpp) ----

inline RayReg ray_reg_of(const RayRegTerms& rt, int64_t n_rays, int S) {
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
    return reg;
}

// R_s of a batch whose last N_p P^2 rays are patch rays, or -1 where the layout or the sizes are refused
inline int64_t batch_n_sup(const PatchRegTerms& pt, int64_t n_rays, int S) {
    const int P = pt.patch_size;
    if (P < 2 || P > kMaxPatch || pt.n_patches < 0) return -1;
    const int64_t n_sup = n_rays - pt.n_patches * P * P;
    if (n_rays <= 0 || n_sup < 1 || S < 1 || S > 64 * kMaxSegments) return -1;
    return n_sup;
}

inline float patch_div_of(const PatchRegTerms& pt) { return (float)pt.n_patches * (float)((pt.patch_size - 1) * (pt.patch_size - 1)); }

// the target-free terms divide by R as in ray_reg.hip; the colour and depth terms by R_s
inline LossExt patch_loss_ext_of(const LossTerms& lt, int64_t n_rays, int64_t n_sup, int S) {
    LossExt ext = loss_ext_of(lt, n_rays, S);
    ext.gd_scale = lt.target_depth ? lt.depth_weight / (float)n_sup : 0.0f;
    return ext;
}

inline PatchArgs patch_args_of(const PatchRegTerms& pt, int64_t n_sup, float* patch_terms, float* patch_depth) {
    PatchArgs pa{};
    pa.n_sup = n_sup; pa.n_patches = pt.n_patches; pa.P = pt.patch_size;
    pa.gd_scale = pt.n_patches > 0 ? 2.0f * pt.depth_smooth_weight / patch_div_of(pt) : 0.0f;
    pa.patch_terms = patch_terms; pa.patch_depth = patch_depth;
    return pa;
}

// it == NULL: the seven values of the patch step
inline FinishArgs finish_args_of(int64_t n_rays, int64_t n_sup, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                                 const InfoRegTerms* it) {
    FinishArgs a{};
    a.n_rays = n_rays; a.n_sup = n_sup; a.n_patches = pt.n_patches;
    a.rgb_div = 3.0f * (float)n_sup; a.depth_div = (float)n_sup; a.reg_div = (float)n_rays * (float)S; a.ray_div = (float)n_rays;
    a.patch_div = patch_div_of(pt);
    a.rgb_weight = lt.rgb_weight; a.depth_weight = lt.target_depth ? lt.depth_weight : 0.0f; a.reg_weight = lt.reg_weight;
    a.dist_weight = rt.dist_weight; a.occ_weight = rt.occ_weight; a.smooth_weight = pt.depth_smooth_weight;
    if (it) { a.ent_weight = it->ent_weight; a.kl_weight = it->kl_weight; }
    return a;
}

}  // namespace

}  // namespace nrf
