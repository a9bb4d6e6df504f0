// info_reg.hip -- the fused training step's loss launch with InfoNeRF's two terms on the per-sample distribution of a ray (nerfhip.h:
// nrf_composite_info_loss_backward, nrf_info_terms_finish): the ray entropy on every ray and the KL divergence between neighbouring
// rays of a patch.  The batch layout, the walk, every other term and the finish body are loss_walk.hpp's.
//
// Per ray, over the S - 1 samples with a finite interval (the last sample's dist is 1e10 |d|: excluded), eps = 1e-10:
//   x_i = relu(sigma_i) dist_i,  a_i = -expm1(-x_i),  A = sum a_i,  p_i = a_i / (A + eps),  m = [A > tau]
//   H = -sum p_i ln(p_i + eps),  KL(p || q) = sum p_i (ln(p_i + eps) - ln(q_i + eps))
// (sigma_i the density the ReLU sees: behind the noise, -inf for a skipped sample; dist_i as the compositor forms it).  a_i comes
// from expm1, not from the compositor's 1 - e: next to e = 1 the subtraction leaves a_i three digits, and p_i G_i needs seven.
//
//   info_loss_backward_kernel<IDX, FINE> : loss_walk.hpp's walk, then -- with a term on -- the same walk
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
#include "loss_walk.hpp"

namespace nrf {

namespace {

constexpr float kEps = 1e-10f;
// the walk's geometry is loss_walk.hpp's (kBlock = 256, kWaves = kBlock / 64): the second walk below deals rays to waves by it
static_assert(kBlock == 256 && kWaves == kBlock / 64, "the second walk deals a group's rays to the four waves of a workgroup");

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

// dyn (the launch's dynamic LDS; present only with the KL term on): P^2 rows of S - 1 floats a_i | P^2 floats A | P^2 floats: the
// anchors' KLs.
template <bool IDX, bool FINE>
__global__ void __launch_bounds__(kBlock) info_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                    int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                    int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                    float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                    int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                    float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                    const LossExt ext, const RayReg reg, const int32_t* __restrict__ slot,
                                                                    const PatchArgs pa, const InfoArgs ia) {
    __shared__ float seg[kWaves][3 * kMaxSegments];
    __shared__ float dep[kMaxPatch * kMaxPatch];
    extern __shared__ __attribute__((aligned(16))) float dyn[];
    LossWalk w;
    loss_walk_prologue(w, rgb, rgb_stride, sigma, sigma_stride, z, rays_d, n_rays, S, white_bkgd, target, weight, pred, d_rgb, d_rgb_stride, d_sigma,
                       d_sigma_stride, ray_loss, zero_buf, zero_n, ext, reg, slot, pa);
    // (the two terms' scalars and pointers ride in vector registers like the walk's, and so does the stride of the zero fills below)
    float ent_scale = ia.ent_scale, tau = ia.tau, kl_scale = ia.kl_scale;
    float* info_terms = ia.info_terms;
    float* patch_kl = ia.patch_kl;
    asm volatile("" : "+v"(ent_scale), "+v"(tau), "+v"(kl_scale), "+v"(info_terms), "+v"(patch_kl));
    int64_t n_thr = w.n_threads;
    asm volatile("" : "+v"(n_thr));
    loss_walk<IDX, FINE, true>(w, seg, dep);
    // The two terms: the same walk once more -- every ray on the wave and the lanes that ran its compositor backward, so the d_sigma
    // entry a lane adds to is the one it stored itself.  A walk of its own keeps the compositor bodies' scalar registers and these
    // apart (one walk with both spills 36 of them).  kl_on and info_on are kernel arguments' values: block-uniform.
    const int lane = w.lane, wv = w.wv, P = w.P, PP = w.PP;
    const bool kl_on = kl_scale > 0.0f, info_on = kl_on || ent_scale > 0.0f;
    if (!info_on) {
        // a term that is off: its output is 0
        if (info_terms) for (int64_t i = w.gtid; i < w.n_rays; i += n_thr) info_terms[i] = 0.0f;
        if (patch_kl) for (int64_t i = w.gtid; i < w.n_patches; i += n_thr) patch_kl[i] = 0.0f;
        return;
    }
    if (!kl_on && patch_kl) for (int64_t i = w.gtid; i < w.n_patches; i += n_thr) patch_kl[i] = 0.0f;
    float* const rows = dyn;                               // kl_on: (PP, S-1) a_i
    float* const sums = dyn + PP * (S - 1);                //        (PP) A
    float* const kls = sums + PP;                          //        (PP) the anchors' KLs
    int64_t sup = w.sup, p = w.p;
    for (;;) {
        const bool patch = sup >= w.n_sup;
        if (__builtin_amdgcn_readfirstlane((int)(patch && p >= w.n_patches))) break;
        const int64_t base = patch ? w.n_sup + p * PP : sup;
        const int kn = patch ? PP : (int)std::min<int64_t>(kWaves, w.n_sup - sup);
        const bool lds = patch && kl_on;                 // block-uniform: the three barriers stand under it
        // phase 1: the patch's a_i and A into LDS
        if (lds) {
            for (int k = wv; k < kn; k += kWaves) {
                const float A = info_ray_sum<IDX>(sigma, w.sigma_stride, w.z, w.rays_d, base + k, S, lane, w.ns, slot, rows + k * (S - 1));
                if (lane == 0) sums[k] = A;
            }
            __syncthreads();
        }
        // phase 2: G, M and the addition to d_sigma; a patch leaves its anchors' KLs in LDS
        for (int k = wv; k < kn; k += kWaves) {
            const int64_t r = base + k;
            float ent, kl;                               // m_r H_r and the anchor's masked KLs
            info_backward_ray<IDX>(sigma, w.sigma_stride, w.z, w.rays_d, r, S, lane, w.d_sigma, w.d_sigma_stride, w.ns, slot, ent_scale, tau, kl_scale,
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
        if (patch) p += w.p_step;
        else sup += w.sup_step;
    }
}

// losses9 = [total, rgb, depth, reg, dist, occ, smooth, entropy, kl]
constexpr int kFinish = 512;          // eight running sums per thread: 512 threads leave them their registers
__global__ void __launch_bounds__(kFinish) info_terms_finish_kernel(const float* __restrict__ ray_terms, const float* __restrict__ patch_terms,
                                                                 const float* __restrict__ info_terms, const float* __restrict__ patch_kl,
                                                                 const FinishArgs a, float* __restrict__ losses9) {
    terms_finish<8, kFinish>(ray_terms, patch_terms, info_terms, patch_kl, a, losses9);
}

}  // namespace

int launch_composite_info_loss_backward(const LossLaunch& a, const RayRegTerms& rt, const PatchRegTerms& pt, const InfoRegTerms& it,
                                        float* patch_terms, float* patch_depth, float* info_terms, float* patch_kl) {
    const int64_t n_sup = batch_n_sup(pt, a.n_rays, a.S);
    if (n_sup < 0) return NRF_EINVAL;
    if (pt.n_patches > 0 && !patch_terms) return NRF_EINVAL;
    const int P = pt.patch_size, S = a.S;
    const bool ent_on = it.ent_weight > 0.0f, kl_on = it.kl_weight > 0.0f;
    if ((ent_on && !info_terms) || (kl_on && (!patch_kl || pt.n_patches < 1))) return NRF_EINVAL;
    if (kl_on && (int64_t)P * P * S > NRF_INFO_KL_MAX_LDS_FLOATS) return NRF_EINVAL;
    InfoArgs ia{};
    ia.ent_scale = ent_on ? it.ent_weight / (float)a.n_rays : 0.0f;
    ia.tau = it.ent_threshold;
    ia.kl_scale = kl_on ? it.kl_weight / patch_div_of(pt) : 0.0f;
    ia.info_terms = info_terms; ia.patch_kl = patch_kl;
    // a wave per supervised ray, the zero fill's share, a workgroup per patch until the cap
    const int64_t work = std::max(std::max(n_sup * 64, (a.zero_n + 3) / 4), pt.n_patches * kBlock);
    const dim3 grid(grid_for(work, kBlock, 16384)), block(kBlock);
    // the KL term's exchange: P^2 rows of S - 1 floats, P^2 sums, P^2 anchor values; nothing without it
    const size_t lds = kl_on ? (size_t)P * P * (S + 1) * sizeof(float) : 0;
    auto* kernel = a.slot ? (pt.n_patches > 0 ? info_loss_backward_kernel<true, true> : info_loss_backward_kernel<true, false>)
                          : (pt.n_patches > 0 ? info_loss_backward_kernel<false, true> : info_loss_backward_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, lds, a.s, a.rgb, a.rgb_stride, a.sigma, a.sigma_stride, a.z, a.rays_d, a.n_rays, S, a.white_bkgd, a.target,
                       a.lt.rgb_weight, a.pred, a.d_rgb, a.d_rgb_stride, a.d_sigma, a.d_sigma_stride, a.ray_terms, a.zero_buf, a.zero_n,
                       patch_loss_ext_of(a.lt, a.n_rays, n_sup, S), ray_reg_of(rt, a.n_rays, S), a.slot,
                       patch_args_of(pt, n_sup, patch_terms, patch_depth), ia);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_info_terms_finish(const float* ray_terms, int64_t n_rays, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                             const InfoRegTerms& it, const float* patch_terms, const float* info_terms, const float* patch_kl, float* losses9,
                             hipStream_t s) {
    const int64_t n_sup = batch_n_sup(pt, n_rays, S);
    if (n_sup < 0) return NRF_EINVAL;
    hipLaunchKernelGGL(info_terms_finish_kernel, dim3(1), dim3(kFinish), 0, s, ray_terms, patch_terms, it.ent_weight > 0.0f ? info_terms : nullptr,
                       it.kl_weight > 0.0f ? patch_kl : nullptr, finish_args_of(n_rays, n_sup, S, lt, rt, pt, &it), losses9);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
