// info_reg.hip -- the fused training step's loss launch with InfoNeRF's two terms on the per-sample distribution of a ray (nerfhip.h:
// nrf_composite_info_loss_backward, nrf_info_terms_finish): the ray entropy on every ray and the KL divergence between neighbouring
// rays of a patch.  The batch layout, the walk and every other term are patch_reg.hip's.
//
// Per ray, over the S - 1 samples with a finite interval (the last sample's dist is 1e10 |d|: excluded), eps = 1e-10:
//   x_i = relu(sigma_i) dist_i,  a_i = -expm1(-x_i),  A = sum a_i,  p_i = a_i / (A + eps),  m = [A > tau]
//   H = -sum p_i ln(p_i + eps),  KL(p || q) = sum p_i (ln(p_i + eps) - ln(q_i + eps))
// (sigma_i the density the ReLU sees: behind the noise, -inf for a skipped sample; dist_i as the compositor forms it).  a_i comes
// from expm1, not from the compositor's 1 - e: next to e = 1 the subtraction leaves a_i three digits, and p_i G_i needs seven.
//
//   info_loss_backward_kernel<IDX, FINE> : patch_loss_backward_kernel<IDX, FINE>'s walk, then -- with a term on -- the same walk
//                                          once more for the two terms, every ray on the wave and lanes that ran its compositor
//                                          backward.  Phase 1 of a patch leaves every ray's a_i and A in (dynamic) LDS when the KL
//                                          term is on; a barrier; in phase 2 the ray's wave, LANE <-> sample, forms
//                                            G_i = dL/dp_i   (entropy: -ln(p_i+eps) - p_i/(p_i+eps); KL as the first argument:
//                                                             ln(p_i+eps) - ln(q_i+eps) + p_i/(p_i+eps); as the second: -p'_i/(p_i+eps))
//                                          summed over the ray's roles, M = sum p_i G_i (a wave reduction per 64-sample segment, the
//                                          segments added front to back) and adds dist_i e_i (G_i - M) / (A + eps) to the d_sigma
//                                          entry the compositor backward of the same lane has stored.
//   info_terms_finish_kernel             : one workgroup forms the step's nine loss values.
//
// No atomics, no second launch: two runs give the same bits.  With both weights 0 the first walk is the parent's, the second is not
// taken, the launch carries no dynamic LDS and every output is the parent's bits.  Every barrier stands under a block-uniform flag:
// `patch` in the first walk, `patch` and the KL weight in the second.
#include <algorithm>

#include "kernels.hpp"
#include "composite_core.hpp"

namespace nrf {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxPatch = 16;         // P <= 16
constexpr float kEps = 1e-10f;

inline unsigned grid_for(int64_t n, int block, int64_t cap) {
    int64_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// The patch term as the kernel takes it (nerfhip.h: nrf_patch_reg), as in patch_reg.hip
struct PatchArgs {
    int64_t n_sup;                    // R_s
    int64_t n_patches;                // N_p
    int P;
    float gd_scale;                   // 2 depth_smooth_weight / (N_p (P-1)^2)
    float* patch_terms;               // (N_p): DS_p
    float* patch_depth;               // (N_p, P, P) or NULL
};

// The two terms as the kernel takes them (nerfhip.h: nrf_info_reg).  A term whose weight is 0 has scale 0: it is not computed.
struct InfoArgs {
    float ent_scale;                  // ent_weight / R
    float tau;                        // ent_threshold
    float kl_scale;                   // kl_weight / (N_p (P-1)^2)
    float* info_terms;                // (R): m_r H_r, or NULL
    float* patch_kl;                  // (N_p): K_p, or NULL
};

// The lane's sample s < S - 1 of ray r: a = -expm1(-x); de = dist e where the density passes the ReLU, else 0; o = the sample's
// row of d_sigma, -1 where it has none (a skipped sample).  The arithmetic of x and e is composite_backward_ray's `sample`.
template <bool IDX>
__device__ __forceinline__ void info_sample(const float* __restrict__ sigma, int sigma_stride, const float* __restrict__ z, float norm, int64_t r,
                                            int S, int s, const NoiseSrc& ns, const int32_t* __restrict__ slot, float& a, float& de, int64_t& o) {
    const int64_t i = r * S + s;
    const float dist = __fmul_rn(__fsub_rn(z[i + 1], z[i]), norm);
    int64_t row = i;
    float sg;
    if constexpr (IDX) {
        row = slot[i];
        sg = row < 0 ? -__builtin_huge_valf() : sigma_eff<true>(sigma[row * sigma_stride], ns, i, r, s);
    } else {
        sg = sigma_eff<true>(sigma[i * sigma_stride], ns, i, r, s);
    }
    const float nx = __fmul_rn(-fmaxf(sg, 0.0f), dist);
    a = -expm1f(nx);
    de = sg > 0.0f ? __fmul_rn(dist, expf(nx)) : 0.0f;
    o = sg > 0.0f ? row : -1;
}

// A of ray r: the segments' wave sums added front to back; `row` != NULL: the a_i are left there (LDS, S - 1 floats)
template <bool IDX>
__device__ __forceinline__ float info_ray_sum(const float* __restrict__ sigma, int sigma_stride, const float* __restrict__ z,
                                              const float* __restrict__ rays_d, int64_t r, int S, int lane, const NoiseSrc& ns,
                                              const int32_t* __restrict__ slot, float* row) {
    const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
    const float norm = ray_norm(d);
    float A = 0.0f;
    for (int s0 = 0; s0 < S - 1; s0 += 64) {
        const int s = s0 + lane;
        float a = 0.0f, de;
        int64_t o;
        if (s < S - 1) {
            info_sample<IDX>(sigma, sigma_stride, z, norm, r, S, s, ns, slot, a, de, o);
            if (row) row[s] = a;
        }
        A = __fadd_rn(A, wave_sum(a));
    }
    return A;
}

// The two terms of one ray on one wave, behind its compositor backward: adds their dL/dsigma to d_sigma and returns m H (`ent`) and
// the masked KLs of the ray's own anchor (`kl`).  rows != NULL: a patch ray k = (i, j) of a P x P patch whose a_i stand in
// rows[k' (S-1) + s] and whose A in sums[k'] -- the KL roles are read from there; rows == NULL: a ray with the entropy alone.
template <bool IDX>
__device__ __forceinline__ void info_backward_ray(const float* __restrict__ sigma, int sigma_stride, const float* __restrict__ z,
                                                  const float* __restrict__ rays_d, int64_t r, int S, int lane, float* __restrict__ d_sigma,
                                                  int d_sigma_stride, const NoiseSrc& ns, const int32_t* __restrict__ slot, float ent_scale,
                                                  float tau, float kl_scale, const float* rows, const float* sums, int k, int P, float& ent,
                                                  float& kl) {
    ent = 0.0f; kl = 0.0f;
    const int nd = S - 1;
    if (nd < 1) return;
    float A = rows ? sums[k] : info_ray_sum<IDX>(sigma, sigma_stride, z, rays_d, r, S, lane, ns, slot, nullptr);
    // The ray's roles, wave-uniform -- bit 0: the entropy; bits 1, 2: first argument of its own anchor's KLs against the right and the
    // lower neighbour; bits 3, 4: second argument of the left and of the upper anchor's.  Neighbour q stands nb(q) rows away.
    auto nb = [&](int q) { return q == 0 ? k + 1 : (q == 1 ? k + P : (q == 2 ? k - 1 : k - P)); };
    int roles = 0;
    float Ae_nb[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (A > tau) {
        if (ent_scale > 0.0f) roles = 1;
        if (rows) {
            const int i = k / P, j = k - i * P;
            const bool can[4] = {i < P - 1 && j < P - 1, i < P - 1 && j < P - 1, i < P - 1 && j > 0, i > 0 && j < P - 1};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (can[q]) {
                    const float An = sums[nb(q)];
                    if (An > tau) roles |= 2 << q;
                    Ae_nb[q] = __fadd_rn(An, kEps);
                }
            }
        }
    }
    if (roles == 0) return;
    float Ae = __fadd_rn(A, kEps);
    const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
    float norm = ray_norm(d);
    // (once-per-ray values in vector registers, the roles as one integer: the scalar file is the compositor's)
    asm volatile("" : "+v"(roles), "+v"(Ae), "+v"(norm), "+v"(Ae_nb[0]), "+v"(Ae_nb[1]), "+v"(Ae_nb[2]), "+v"(Ae_nb[3]));
    // sample s < nd with its a: G = dL/dp (scaled), p, and the lane's shares of H and of the anchor's KLs
    auto grad = [&](int s, float a, float& p, float& hs, float& ks) {
        p = a / Ae;
        const float pe = __fadd_rn(p, kEps);
        const float lp = logf(pe), rp = p / pe;
        float G = 0.0f;
        hs = 0.0f; ks = 0.0f;
        if (roles & 1) {
            hs = __fmul_rn(p, lp);
            G = -__fmul_rn(ent_scale, __fadd_rn(lp, rp));
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (roles & (2 << q)) {
                const float lq = logf(__fadd_rn(rows[nb(q) * nd + s] / Ae_nb[q], kEps));
                const float dl = __fsub_rn(lp, lq);
                G = __fadd_rn(G, __fmul_rn(kl_scale, __fadd_rn(dl, rp)));
                ks = __fadd_rn(ks, __fmul_rn(p, dl));
            }
        }
#pragma unroll
        for (int q = 2; q < 4; ++q) {
            if (roles & (2 << q)) G = __fsub_rn(G, __fmul_rn(kl_scale, (rows[nb(q) * nd + s] / Ae_nb[q]) / pe));
        }
        return G;
    };
    auto apply = [&](float G, float M, float de, int64_t o) {
        if (o >= 0) {
            const float da = __fsub_rn(G, M) / Ae;
            d_sigma[o * d_sigma_stride] = __fadd_rn(d_sigma[o * d_sigma_stride], __fmul_rn(de, da));
        }
    };
    float M = 0.0f, H = 0.0f, K = 0.0f;
    if (nd <= 64) {
        // one segment: a and G stay in registers between the reduction and the store
        float a = 0.0f, de = 0.0f, G = 0.0f, p = 0.0f, hs = 0.0f, ks = 0.0f;
        int64_t o = -1;
        if (lane < nd) {
            info_sample<IDX>(sigma, sigma_stride, z, norm, r, S, lane, ns, slot, a, de, o);
            G = grad(lane, a, p, hs, ks);
        }
        M = wave_sum(__fmul_rn(p, G)); H = wave_sum(hs); K = wave_sum(ks);
        apply(G, M, de, o);
    } else {
        // the sums cross segments: one walk for M, H and the KLs, one more for the stores
        for (int s0 = 0; s0 < nd; s0 += 64) {
            const int s = s0 + lane;
            float a, de, G = 0.0f, p = 0.0f, hs = 0.0f, ks = 0.0f;
            int64_t o;
            if (s < nd) {
                if (rows) a = rows[k * nd + s];
                else info_sample<IDX>(sigma, sigma_stride, z, norm, r, S, s, ns, slot, a, de, o);
                G = grad(s, a, p, hs, ks);
            }
            M = __fadd_rn(M, wave_sum(__fmul_rn(p, G))); H = __fadd_rn(H, wave_sum(hs)); K = __fadd_rn(K, wave_sum(ks));
        }
        for (int s0 = 0; s0 < nd; s0 += 64) {
            const int s = s0 + lane;
            if (s < nd) {
                float a, de, p, hs, ks;
                int64_t o;
                info_sample<IDX>(sigma, sigma_stride, z, norm, r, S, s, ns, slot, a, de, o);
                apply(grad(s, a, p, hs, ks), M, de, o);
            }
        }
    }
    ent = (roles & 1) ? -H : 0.0f;
    kl = K;
}

// ray_loss (5,R) as in patch_reg.hip.  dyn (the launch's dynamic LDS; present only with the KL term on): P^2 rows of S - 1 floats
// a_i | P^2 floats A | P^2 floats: the anchors' KLs.
template <bool IDX, bool FINE>
__global__ void __launch_bounds__(kBlock) info_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                    int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                    int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                    float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                    int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                    float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                    const LossExt ext, const RayReg reg, const int32_t* __restrict__ slot,
                                                                    const PatchArgs pa, const InfoArgs ia) {
    __shared__ float seg[kWaves][3 * kMaxSegments];               // per wave: seg_T | the two prefix carries of the distortion scans
    __shared__ float dep[kMaxPatch * kMaxPatch];                  // the depths of the workgroup's patch
    extern __shared__ __attribute__((aligned(16))) float dyn[];
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
    asm volatile("" : "+v"(n_rays), "+v"(white_bkgd), "+v"(rgb_stride), "+v"(sigma_stride), "+v"(d_rgb_stride), "+v"(d_sigma_stride));
    asm volatile("" : "+v"(d_rgb), "+v"(d_sigma), "+v"(rays_d), "+v"(z));
    // (the two terms' scalars and pointers ride in vector registers like the parent's)
    float ent_scale = ia.ent_scale, tau = ia.tau, kl_scale = ia.kl_scale;
    float* info_terms = ia.info_terms;
    float* patch_kl = ia.patch_kl;
    asm volatile("" : "+v"(ent_scale), "+v"(tau), "+v"(kl_scale), "+v"(info_terms), "+v"(patch_kl));
    const float count = 3.0f * (float)n_sup;
    const float scale = 2.0f * weight / count;
    const int PP = P * P;
    // The parent's walk: `patch`, sup, p, kn are block-uniform and k is wave-uniform; every barrier stands under `patch` alone.
    int64_t sup = (int64_t)blockIdx.x * kWaves;
    int64_t p = blockIdx.x;
    int64_t sup_step = (int64_t)gridDim.x * kWaves, p_step = gridDim.x;
    asm volatile("" : "+v"(sup), "+v"(p), "+v"(sup_step), "+v"(p_step));
    int64_t n_thr = n_threads;
    asm volatile("" : "+v"(n_thr));
    const int64_t sup0 = sup, p0 = p;                    // (for the second walk, with the stride of its zero fills)
    for (;;) {
        const bool patch = sup >= n_sup;
        // (the exit test through readfirstlane: a uniform branch needs no saved exec mask behind the loop -- two scalar registers the
        // parent, whose kernel ends there, never held)
        if (__builtin_amdgcn_readfirstlane((int)(patch && p >= n_patches))) break;
        const int64_t base = patch ? n_sup + p * PP : sup;
        const int kn = patch ? PP : (int)std::min<int64_t>(kWaves, n_sup - sup);
        float gr = 0.0f, gg = 0.0f, gb = 0.0f, gd_own = 0.0f;
        // phase 1: wave w composites rays w, w + 4, ... of the item; a patch leaves their depths -- and with the KL term their a_i
        // and A -- in LDS
        for (int k = wv; k < kn; k += kWaves) {
            const int64_t r = base + k;
            RaySums o = composite_ray<true, IDX, FINE>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, nullptr, ns, slot);
            if (white_bkgd) {
                const float bg = __fsub_rn(1.0f, o.acc);
                o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
            }
            float se = 0.0f, ad = 0.0f;
            if (!patch) {
                const float dr = o.r - target[r * 3], dg = o.g - target[r * 3 + 1], db = o.b - target[r * 3 + 2];
                const float dd = tdepth ? __fsub_rn(o.depth, tdepth[r]) : 0.0f;
                gd_own = dd > 0.0f ? gd_scale : (dd < 0.0f ? -gd_scale : 0.0f);
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
        // phase 2: the compositor backward with the stencil's dL/d depth
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
    // The two terms: the same walk once more -- every ray on the wave and the lanes that ran its compositor backward, so the d_sigma
    // entry a lane adds to is the one it stored itself.  A walk of its own keeps the compositor bodies' scalar registers and these
    // apart (one walk with both spills 36 of them).  kl_on and info_on are kernel arguments' values: block-uniform.
    const bool kl_on = kl_scale > 0.0f, info_on = kl_on || ent_scale > 0.0f;
    if (!info_on) {
        // a term that is off: its output is 0
        if (info_terms) for (int64_t i = gtid; i < n_rays; i += n_thr) info_terms[i] = 0.0f;
        if (patch_kl) for (int64_t i = gtid; i < n_patches; i += n_thr) patch_kl[i] = 0.0f;
        return;
    }
    if (!kl_on && patch_kl) for (int64_t i = gtid; i < n_patches; i += n_thr) patch_kl[i] = 0.0f;
    float* const rows = dyn;                               // kl_on: (PP, S-1) a_i
    float* const sums = dyn + PP * (S - 1);                //        (PP) A
    float* const kls = sums + PP;                          //        (PP) the anchors' KLs
    sup = sup0;
    p = p0;
    for (;;) {
        const bool patch = sup >= n_sup;
        if (__builtin_amdgcn_readfirstlane((int)(patch && p >= n_patches))) break;
        const int64_t base = patch ? n_sup + p * PP : sup;
        const int kn = patch ? PP : (int)std::min<int64_t>(kWaves, n_sup - sup);
        const bool lds = patch && kl_on;                 // block-uniform: the three barriers stand under it
        // phase 1: the patch's a_i and A into LDS
        if (lds) {
            for (int k = wv; k < kn; k += kWaves) {
                const float A = info_ray_sum<IDX>(sigma, sigma_stride, z, rays_d, base + k, S, lane, ns, slot, rows + k * (S - 1));
                if (lane == 0) sums[k] = A;
            }
            __syncthreads();
        }
        // phase 2: G, M and the addition to d_sigma; a patch leaves its anchors' KLs in LDS
        for (int k = wv; k < kn; k += kWaves) {
            const int64_t r = base + k;
            float ent, kl;                               // m_r H_r and the anchor's masked KLs
            info_backward_ray<IDX>(sigma, sigma_stride, z, rays_d, r, S, lane, d_sigma, d_sigma_stride, ns, slot, ent_scale, tau, kl_scale,
                                   lds ? rows : nullptr, sums, k, P, ent, kl);
            if (lane == 0) {
                if (info_terms) info_terms[r] = ent;
                if (lds) kls[k] = kl;
            }
        }
        if (lds) {
            __syncthreads();
            // K_p: wave 0, lane l adds up anchors l, l + 64, ... in that order, then the wave's fixed tree
            if (wv == 0) {
                const int Q = P - 1;
                float ks = 0.0f;
                for (int a = lane; a < Q * Q; a += 64) {
                    const int i = a / Q, j = a - i * Q;
                    ks = __fadd_rn(ks, kls[i * P + j]);
                }
                ks = wave_sum(ks);
                if (lane == 0) patch_kl[p] = ks;
            }
            __syncthreads();                             // the next patch overwrites the LDS
        }
        if (patch) p += p_step;
        else sup += sup_step;
    }
}

// losses9 = [total, rgb, depth, reg, dist, occ, smooth, entropy, kl] with the divisors of the batch layout: rgb 3 R_s, depth R_s,
// reg R S, dist, occ and entropy R, smooth and kl N_p (P-1)^2.  One workgroup, every partial sum in a fixed order.
constexpr int kFinish = 512;          // eight running sums per thread: 512 threads leave them their registers
struct FinishArgs {
    int64_t n_rays, n_sup, n_patches;
    float rgb_div, depth_div, reg_div, ray_div, patch_div;            // patch_div = 0 with N_p = 0
    float rgb_weight, depth_weight, reg_weight, dist_weight, occ_weight, smooth_weight, ent_weight, kl_weight;
};
__global__ void __launch_bounds__(kFinish) info_terms_finish_kernel(const float* __restrict__ ray_terms, const float* __restrict__ patch_terms,
                                                                 const float* __restrict__ info_terms, const float* __restrict__ patch_kl,
                                                                 const FinishArgs a, float* __restrict__ losses9) {
    __shared__ float part[8][kFinish / 64];
    float s[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t i = threadIdx.x; i < a.n_sup; i += kFinish) {
        s[0] = __fadd_rn(s[0], ray_terms[i]);
        s[1] = __fadd_rn(s[1], ray_terms[2 * a.n_rays + i]);
    }
    for (int64_t i = threadIdx.x; i < a.n_rays; i += kFinish) {
        s[2] = __fadd_rn(s[2], ray_terms[a.n_rays + i]);
        s[3] = __fadd_rn(s[3], ray_terms[3 * a.n_rays + i]);
        s[4] = __fadd_rn(s[4], ray_terms[4 * a.n_rays + i]);
        if (info_terms) s[6] = __fadd_rn(s[6], info_terms[i]);
    }
    for (int64_t i = threadIdx.x; i < a.n_patches; i += kFinish) {
        s[5] = __fadd_rn(s[5], patch_terms[i]);
        if (patch_kl) s[7] = __fadd_rn(s[7], patch_kl[i]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        s[k] = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            t[k] = 0.0f;
            for (int w = 0; w < kFinish / 64; ++w) t[k] = __fadd_rn(t[k], part[k][w]);
        }
        const float l_rgb = t[0] / a.rgb_div, l_depth = t[1] / a.depth_div, l_reg = t[2] / a.reg_div;
        const float l_dist = t[3] / a.ray_div, l_occ = t[4] / a.ray_div, l_ent = t[6] / a.ray_div;
        const float l_smooth = a.patch_div > 0.0f ? t[5] / a.patch_div : 0.0f;
        const float l_kl = a.patch_div > 0.0f ? t[7] / a.patch_div : 0.0f;
        float total = __fmul_rn(a.rgb_weight, l_rgb);
        total = __fadd_rn(total, __fmul_rn(a.depth_weight, l_depth));
        total = __fadd_rn(total, __fmul_rn(a.reg_weight, l_reg));
        total = __fadd_rn(total, __fmul_rn(a.dist_weight, l_dist));
        total = __fadd_rn(total, __fmul_rn(a.occ_weight, l_occ));
        total = __fadd_rn(total, __fmul_rn(a.smooth_weight, l_smooth));
        total = __fadd_rn(total, __fmul_rn(a.ent_weight, l_ent));
        total = __fadd_rn(total, __fmul_rn(a.kl_weight, l_kl));
        losses9[0] = total; losses9[1] = l_rgb; losses9[2] = l_depth; losses9[3] = l_reg;
        losses9[4] = l_dist; losses9[5] = l_occ; losses9[6] = l_smooth; losses9[7] = l_ent; losses9[8] = l_kl;
    }
}

}  // namespace

int launch_composite_info_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                                        int64_t n_rays, int S, int white_bkgd, const float* target, const LossTerms& lt, const RayRegTerms& rt,
                                        const PatchRegTerms& pt, const InfoRegTerms& it, const int32_t* slot, float* pred, float* d_rgb,
                                        int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf, int64_t zero_n,
                                        float* patch_terms, float* patch_depth, float* info_terms, float* patch_kl, hipStream_t s) {
    const int P = pt.patch_size;
    if (P < 2 || P > kMaxPatch || pt.n_patches < 0) return NRF_EINVAL;
    const int64_t n_sup = n_rays - pt.n_patches * P * P;
    if (n_rays <= 0 || n_sup < 1 || S < 1 || S > 64 * kMaxSegments) return NRF_EINVAL;
    if (pt.n_patches > 0 && !patch_terms) return NRF_EINVAL;
    const bool ent_on = it.ent_weight > 0.0f, kl_on = it.kl_weight > 0.0f;
    if ((ent_on && !info_terms) || (kl_on && (!patch_kl || pt.n_patches < 1))) return NRF_EINVAL;
    if (kl_on && (int64_t)P * P * S > NRF_INFO_KL_MAX_LDS_FLOATS) return NRF_EINVAL;
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
    const float patch_div = (float)pt.n_patches * (float)((P - 1) * (P - 1));
    pa.gd_scale = pt.n_patches > 0 ? 2.0f * pt.depth_smooth_weight / patch_div : 0.0f;
    pa.patch_terms = patch_terms; pa.patch_depth = patch_depth;
    InfoArgs ia{};
    ia.ent_scale = ent_on ? it.ent_weight / (float)n_rays : 0.0f;
    ia.tau = it.ent_threshold;
    ia.kl_scale = kl_on ? it.kl_weight / patch_div : 0.0f;
    ia.info_terms = info_terms; ia.patch_kl = patch_kl;
    const int64_t work = std::max(std::max(n_sup * 64, (zero_n + 3) / 4), pt.n_patches * kBlock);
    const dim3 grid(grid_for(work, kBlock, 16384)), block(kBlock);
    // the KL term's exchange: P^2 rows of S - 1 floats, P^2 sums, P^2 anchor values; nothing without it
    const size_t lds = kl_on ? (size_t)P * P * (S + 1) * sizeof(float) : 0;
    auto* kernel = slot ? (pt.n_patches > 0 ? info_loss_backward_kernel<true, true> : info_loss_backward_kernel<true, false>)
                        : (pt.n_patches > 0 ? info_loss_backward_kernel<false, true> : info_loss_backward_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, lds, s, rgb, rgb_stride, sigma, sigma_stride, z, rays_d, n_rays, S, white_bkgd, target, lt.rgb_weight, pred,
                       d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, ext, reg, slot, pa, ia);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_info_terms_finish(const float* ray_terms, int64_t n_rays, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                             const InfoRegTerms& it, const float* patch_terms, const float* info_terms, const float* patch_kl, float* losses9,
                             hipStream_t s) {
    const int P = pt.patch_size;
    if (P < 2 || P > kMaxPatch || pt.n_patches < 0) return NRF_EINVAL;
    const int64_t n_sup = n_rays - pt.n_patches * P * P;
    if (n_rays <= 0 || n_sup < 1 || S < 1) return NRF_EINVAL;
    FinishArgs a{};
    a.n_rays = n_rays; a.n_sup = n_sup; a.n_patches = pt.n_patches;
    a.rgb_div = 3.0f * (float)n_sup; a.depth_div = (float)n_sup; a.reg_div = (float)n_rays * (float)S; a.ray_div = (float)n_rays;
    a.patch_div = (float)pt.n_patches * (float)((P - 1) * (P - 1));
    a.rgb_weight = lt.rgb_weight; a.depth_weight = lt.target_depth ? lt.depth_weight : 0.0f; a.reg_weight = lt.reg_weight;
    a.dist_weight = rt.dist_weight; a.occ_weight = rt.occ_weight; a.smooth_weight = pt.depth_smooth_weight;
    a.ent_weight = it.ent_weight; a.kl_weight = it.kl_weight;
    hipLaunchKernelGGL(info_terms_finish_kernel, dim3(1), dim3(kFinish), 0, s, ray_terms, patch_terms, it.ent_weight > 0.0f ? info_terms : nullptr,
                       it.kl_weight > 0.0f ? patch_kl : nullptr, a, losses9);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
