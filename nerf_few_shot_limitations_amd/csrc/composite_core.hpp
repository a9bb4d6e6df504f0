// composite_core.hpp -- the volume compositor's per-ray bodies (volume_renderer.py:4-43, nerf_mlp.py:165-215 and their autograd): one ray
// on one wave, LANE <-> sample, 64-sample segments.  Shared by the staged kernels (staged_kernels.hip) and the regularised loss
// launch (ray_reg.hip); each unit instantiates what it launches.
#pragma once

#include "kernels.hpp"

namespace nrf {

namespace {

__device__ __forceinline__ float wave_incl_prod(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_up(v, d, 64);
        if (lane >= d) v = __fmul_rn(v, u);
    }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = __fadd_rn(v, __shfl_xor(v, d, 64));
    return v;
}

// Density noise of a training render (nerf_mlp.py:188-190: density + randn_like(density) * noise_std in front of the ReLU): the
// caller's (R,S) standard normals, or -- n == NULL -- the counter RNG keyed by (seed, ray index in the call, sample).
struct NoiseSrc { float std; const float* n; uint64_t seed; };
// EXT = false: the density as it is (every caller but the multi-term loss kernel; these instantiations are the code the kernels
// had before the noise existed)
template <bool EXT>
__device__ __forceinline__ float sigma_eff(float sigma, const NoiseSrc& ns, int64_t i, int64_t r, int s) {
    if constexpr (EXT) {
        if (ns.std > 0.0f) return __fadd_rn(sigma, __fmul_rn(ns.n ? ns.n[i] : counter_normal(ns.seed, (uint64_t)r, (uint32_t)s), ns.std));
    }
    return sigma;
}

// One ray on one wave (LANE <-> sample, 64-sample segments front to back): every lane returns the ray's sums
// (w2 = sum of squared weights, the regulariser of nerf_mlp.py:245: EXT only)
// IDX (training under an occupancy grid, nerfhip.h: nrf_composite_loss_backward_indexed): rgb / sigma hold the rows of the evaluated
// samples alone, sample i of the (R,S) ladder reads row slot[i]; slot[i] < 0 is a skipped sample, composited as colour (0,0,0) and
// effective density -inf -- behind the noise, so that no draw brings it back.  The instantiations without IDX are the code the
// kernels had before it existed.
// FINE (the loss launch with patches, patch_reg.hip): the factor a sample leaves of the transmittance is formed as e + 1e-10 from
// e = exp(-relu(sigma) dist) itself, not as (1 - alpha) + 1e-10 from alpha = 1 - e rounded to fp32 -- the same number in exact
// arithmetic, but behind a nearly opaque sample (e = 1e-5) the rounding of alpha costs everything later 6e-3 of its value.  The
// instantiations without FINE are the code the kernels had before it existed.
struct RaySums { float r, g, b, depth, acc, w2; };
template <bool EXT = false, bool IDX = false, bool FINE = false>
__device__ __forceinline__ RaySums composite_ray(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma, int sigma_stride,
                                                 const float* __restrict__ z, const float* __restrict__ rays_d, int64_t r, int S, int lane,
                                                 float* __restrict__ out_w, const NoiseSrc ns = NoiseSrc{},
                                                 const int32_t* __restrict__ slot = nullptr) {
    const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
    const float norm = ray_norm(d);
    float T_in = 1.0f;                                   // transmittance entering this 64-sample segment
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sd = 0.0f, sa = 0.0f, sw2 = 0.0f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < S;
        const int64_t i = r * S + (valid ? s : S - 1);
        const float zc = z[i];
        float zn = __shfl_down(zc, 1, 64);
        if (lane == 63 && s + 1 < S) zn = z[i + 1];
        const bool last = (s + 1 == S);
        const float dist = last ? __fmul_rn(1e10f, norm) : __fmul_rn(__fsub_rn(zn, zc), norm);
        float alpha = 0.0f;
        float e_fine = 1.0f;                             // FINE: exp(-relu(sigma) dist), 1 beyond the ray
        int64_t row = i;                                 // the sample's row of rgb / sigma
        if constexpr (IDX) row = slot[i];
        if constexpr (FINE) {
            if (valid) {
                float sg;
                if constexpr (IDX) sg = row < 0 ? -__builtin_huge_valf() : sigma_eff<EXT>(sigma[row * sigma_stride], ns, i, r, s);
                else sg = sigma_eff<EXT>(sigma[i * sigma_stride], ns, i, r, s);
                e_fine = expf(__fmul_rn(-fmaxf(sg, 0.0f), dist));
                alpha = __fsub_rn(1.0f, e_fine);
            }
        } else if constexpr (IDX) {
            if (valid) {
                const float sg = row < 0 ? -__builtin_huge_valf() : sigma_eff<EXT>(sigma[row * sigma_stride], ns, i, r, s);
                alpha = __fsub_rn(1.0f, expf(__fmul_rn(-fmaxf(sg, 0.0f), dist)));
            }
        } else {
            if (valid) alpha = __fsub_rn(1.0f, expf(__fmul_rn(-fmaxf(sigma_eff<EXT>(sigma[i * sigma_stride], ns, i, r, s), 0.0f), dist)));
        }
        const float f = valid ? __fadd_rn(FINE ? e_fine : __fsub_rn(1.0f, alpha), 1e-10f) : 1.0f;
        const float incl = wave_incl_prod(f, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        const float w = __fmul_rn(alpha, __fmul_rn(T_in, excl));
        if (valid) {
            if (out_w) out_w[i] = w;
            if constexpr (IDX) {
                const bool ev = row >= 0;
                sr = __fadd_rn(sr, __fmul_rn(w, ev ? rgb[row * rgb_stride] : 0.0f));
                sg = __fadd_rn(sg, __fmul_rn(w, ev ? rgb[row * rgb_stride + 1] : 0.0f));
                sb = __fadd_rn(sb, __fmul_rn(w, ev ? rgb[row * rgb_stride + 2] : 0.0f));
            } else {
                sr = __fadd_rn(sr, __fmul_rn(w, rgb[i * rgb_stride]));
                sg = __fadd_rn(sg, __fmul_rn(w, rgb[i * rgb_stride + 1]));
                sb = __fadd_rn(sb, __fmul_rn(w, rgb[i * rgb_stride + 2]));
            }
            sd = __fadd_rn(sd, __fmul_rn(w, zc));
            sa = __fadd_rn(sa, w);
            if constexpr (EXT) sw2 = __fadd_rn(sw2, __fmul_rn(w, w));
        }
        T_in = __fmul_rn(T_in, __shfl(incl, 63, 64));
    }
    RaySums o;
    o.r = wave_sum(sr); o.g = wave_sum(sg); o.b = wave_sum(sb); o.depth = wave_sum(sd); o.acc = wave_sum(sa);
    o.w2 = EXT ? wave_sum(sw2) : 0.0f;
    return o;
}

// ---- backward of a9 (autograd through nerf_mlp.py:181-212) -------------------------
// With v_i = g_rgb . c_i + g_depth * z_i + g_w[i] - [white_bkgd] * sum(g_rgb)  (so that dL = sum_i v_i dw_i):
//   dL/dc_i     = w_i * g_rgb
//   dL/dalpha_i = T_i * v_i - (sum_{j>i} w_j v_j) / (1 - alpha_i + 1e-10)
//   dL/dsigma_i = dL/dalpha_i * dist_i * exp(-relu(sigma_i) dist_i) * [sigma_i > 0]
// (under density noise sigma_i stands for sigma_i + noise_std * n_i throughout: the compositor's ReLU acts on the noisy density)
// The suffix sum is a true reverse scan (segments walked back to front): "total - prefix" would lose every digit behind
// an opaque sample, where the reference's +1e-10 makes the divisor 1e-10.  One WAVE per ray, LANE <-> sample.
__device__ __forceinline__ float wave_incl_sum_rev(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_down(v, d, 64);
        if (lane + d < 64) v = __fadd_rn(v, u);
    }
    return v;
}

__device__ __forceinline__ float wave_incl_sum_fwd(float v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float u = __shfl_up(v, d, 64);
        if (lane >= d) v = __fadd_rn(v, u);
    }
    return v;
}

constexpr int kMaxSegments = 64;     // S <= 4096

// The two per-ray regularisers of few-shot training (composite_backward_ray: REG; nerfhip.h: nrf_ray_reg), as the kernel takes them.
// A term whose weight is 0 has scale 0 here: it is not computed, its row of ray_terms is 0 and the d rows are the bits they were.
struct RayReg {
    float dist_scale;                 // dist_weight / R, 0 = no distortion term
    float kappa;                      // dist_inv_span
    float occ_scale;                  // occ_weight / (R M'), 0 = no occlusion term
    float occ_inv;                    // 1 / M'
    int occ_m;                        // M' = min(occ_samples, S)
};

// One ray on one wave; gr, gg, gb, gd = dL/d rgb_map, dL/d depth of the ray (wave-uniform), g_w = dL/d weights or NULL;
// seg_T = the wave's LDS row of kMaxSegments floats.  EXT: the density noise `ns`, and the regulariser's dL/d weights formed in
// registers, g_w[i] = gw_scale * w_i (no (R,S) tensor).  GEOM: the geometric terms of the same autograd as well --
//   dL/d dist_i = dL/dalpha_i * relu(sigma_i) * e_i                      (dist_i = (z_{i+1} - z_i) |d|, the last one 1e10 |d|)
//   dL/d z_i    = g_depth * w_i + |d| (dL/d dist_{i-1} - [i < S-1] dL/d dist_i)              -> d_z (R,S)
//   dL/d |d|    = sum_{i<S-1} dL/d dist_i (z_{i+1} - z_i) + dL/d dist_{S-1} * 1e10,   d_rays_d (R,3) = dL/d |d| * d / |d|
// The neighbour term of a segment's first sample waits for the segment in front of it (walked later), as the suffix sum's carry
// travels the other way.  The instantiations without GEOM are the code the kernels had before it existed.
// IDX: as in composite_ray; d_rgb / d_sigma address the evaluated rows too, a skipped sample stores nothing (its d_sigma is masked
// to 0 by [-inf > 0] and its d_rgb is w g = 0: there is no row to leave them in).
// REG (the regularised loss launch, ray_reg.hip; seg_T is then the wave's row of 3 kMaxSegments floats): two more per-ray terms, with
//   m_i = kappa (z_i + z_{i+1}) / 2, delta_i = kappa (z_{i+1} - z_i) for i < S-1, m_{S-1} = kappa z_{S-1}, delta_{S-1} = 0
//   D = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i           (mip-NeRF 360's distortion loss)  -> reg_out[0]
//   O = (1/M') sum_{i<M'} relu(sigma_i)                                   (FreeNeRF's occlusion penalty)    -> reg_out[1]
// (sigma_i the density the ReLU sees: behind the noise, -inf for a skipped sample).  dL/dw_i gains dist_scale (2 t_i + (2/3) w_i
// delta_i), t_i = sum_j w_j |m_i - m_j|, where gw_scale w_i enters v_i; dL/dsigma_i gains occ_scale [sigma_i > 0] for i < M'.  The
// depths ascend, so t_i = (m_i A_i - B_i) + (Dm_i - m_i C_i) with the exclusive prefix sums A, B of w, w m and their exclusive suffix
// sums C, Dm: O(S).  Pass 1 leaves the prefix sums entering every segment beside seg_T (rays of one segment have none: it skips the
// two sums), pass 2 carries the suffix sums as it carries `carry`; both sides are true scans.  The instantiations without REG are
// the code the kernels had before it existed.
// FINE: as in composite_ray, and the sum over the strictly later samples is the neighbour's inclusive sum, not `inclusive - own`:
// behind an opaque sample the later samples' w v (1e-11) vanish in that subtraction against the own (1e-1), and the divisor there is
// 1e-10.  The instantiations without FINE are the code the kernels had before it existed.
template <bool EXT = false, bool GEOM = false, bool IDX = false, bool REG = false, bool FINE = false>
__device__ __forceinline__ void composite_backward_ray(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                       int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                       int64_t r, int S, int lane, int white_bkgd, float gr, float gg, float gb, float gd,
                                                       const float* __restrict__ g_w, float* __restrict__ d_rgb, int d_rgb_stride,
                                                       float* __restrict__ d_sigma, int d_sigma_stride, float* seg_T,
                                                       const NoiseSrc ns = NoiseSrc{}, float gw_scale = 0.0f, float* __restrict__ d_z = nullptr,
                                                       float* __restrict__ d_rays_d = nullptr, const int32_t* __restrict__ slot = nullptr,
                                                       const RayReg rr = RayReg{}, float* reg_out = nullptr) {
    const int n_seg = (S + 63) / 64;
    const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
    const float norm = ray_norm(d);
    const float bg = white_bkgd ? __fadd_rn(__fadd_rn(gr, gg), gb) : 0.0f;
    int64_t row = 0;                                     // IDX: the row of rgb / sigma / d_rgb / d_sigma of the lane's sample, < 0 = skipped
    auto sample = [&](int s0, float& alpha, float& e, float& dist, float& f, float& zc, bool& valid, int64_t& i, float& sg) {
        const int s = s0 + lane;
        valid = s < S;
        i = r * S + (valid ? s : S - 1);
        zc = z[i];
        float zn = __shfl_down(zc, 1, 64);
        if (lane == 63 && s + 1 < S) zn = z[i + 1];
        const bool last = (s + 1 == S);
        dist = last ? __fmul_rn(1e10f, norm) : __fmul_rn(__fsub_rn(zn, zc), norm);
        if constexpr (IDX) {
            row = slot[i];
            sg = row < 0 ? -__builtin_huge_valf() : sigma_eff<EXT>(sigma[row * sigma_stride], ns, i, r, s);
        } else {
            sg = sigma_eff<EXT>(sigma[i * sigma_stride], ns, i, r, s);
        }
        e = valid ? expf(__fmul_rn(-fmaxf(sg, 0.0f), dist)) : 1.0f;
        alpha = valid ? __fsub_rn(1.0f, e) : 0.0f;
        f = valid ? __fadd_rn(FINE ? e : __fsub_rn(1.0f, alpha), 1e-10f) : 1.0f;
    };
    // REG: m_i and delta_i of the lane's sample from (z_{i+1} - z_i) as `sample` formed it
    auto interval = [&](int s0, float zc, int64_t i, float& m, float& delta) {
        float zn = __shfl_down(zc, 1, 64);
        if (lane == 63 && s0 + lane + 1 < S) zn = z[i + 1];
        const bool last = (s0 + lane + 1 >= S);
        m = __fmul_rn(rr.kappa, last ? zc : __fmul_rn(0.5f, __fadd_rn(zc, zn)));
        delta = last ? 0.0f : __fmul_rn(rr.kappa, __fsub_rn(zn, zc));
    };
    const bool dist_on = REG && rr.dist_scale > 0.0f;                       // wave-uniform
    float* const seg_A = seg_T + kMaxSegments;
    float* const seg_B = seg_T + 2 * kMaxSegments;
    // pass 1, front to back: transmittance entering every 64-sample segment
    float T_in = 1.0f;
    float pre_A = 0.0f, pre_B = 0.0f;                    // REG: sums of w_j, w_j m_j over all earlier segments
    for (int k = 0; k < n_seg; ++k) {
        float alpha, e, dist, f, zc, sg; bool valid; int64_t i;
        sample(64 * k, alpha, e, dist, f, zc, valid, i, sg);
        if (lane == 0) seg_T[k] = T_in;
        const float incl = wave_incl_prod(f, lane);
        if constexpr (REG) {
            if (dist_on && n_seg > 1) {
                float excl = __shfl_up(incl, 1, 64);
                if (lane == 0) excl = 1.0f;
                const float w = __fmul_rn(alpha, __fmul_rn(T_in, excl));
                float m, delta;
                interval(64 * k, zc, i, m, delta);
                if (lane == 0) { seg_A[k] = pre_A; seg_B[k] = pre_B; }
                pre_A = __fadd_rn(pre_A, wave_sum(w));
                pre_B = __fadd_rn(pre_B, wave_sum(__fmul_rn(w, m)));
            }
        }
        T_in = __fmul_rn(T_in, __shfl(incl, 63, 64));
    }
    // pass 2, back to front
    float carry = 0.0f;                                  // sum of w_j v_j over all later segments
    float pend_z = 0.0f, s_norm = 0.0f;                  // GEOM: dL/d z of the later segment's first sample without its neighbour term; dL/d |d|
    float suf_C = 0.0f, suf_D = 0.0f, acc_D = 0.0f, acc_O = 0.0f;      // REG: sums of w_j, w_j m_j over all later segments; the lane's share of D, M' O
    for (int k = n_seg - 1; k >= 0; --k) {
        float alpha, e, dist, f, zc, sg; bool valid; int64_t i;
        sample(64 * k, alpha, e, dist, f, zc, valid, i, sg);
        const float incl = wave_incl_prod(f, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        const float T = __fmul_rn(seg_T[k], excl);
        const float w = __fmul_rn(alpha, T);
        float g_dist = 0.0f;                             // REG: the distortion term's dL/dw_i (+0 keeps v's bits when the term is off)
        if constexpr (REG) {
            if (dist_on) {
                float m, delta;
                interval(64 * k, zc, i, m, delta);
                const float wm = __fmul_rn(w, m);        // (w = 0 beyond the ray: alpha = 0 there)
                const float pa = wave_incl_sum_fwd(w, lane), pb = wave_incl_sum_fwd(wm, lane);
                const float sc = wave_incl_sum_rev(w, lane), sd = wave_incl_sum_rev(wm, lane);
                float A = __shfl_up(pa, 1, 64), B = __shfl_up(pb, 1, 64), Cs = __shfl_down(sc, 1, 64), Ds = __shfl_down(sd, 1, 64);
                if (lane == 0) { A = 0.0f; B = 0.0f; }
                if (lane == 63) { Cs = 0.0f; Ds = 0.0f; }
                if (n_seg > 1) { A = __fadd_rn(A, seg_A[k]); B = __fadd_rn(B, seg_B[k]); }
                Cs = __fadd_rn(Cs, suf_C); Ds = __fadd_rn(Ds, suf_D);
                suf_C = __fadd_rn(suf_C, __shfl(sc, 0, 64)); suf_D = __fadd_rn(suf_D, __shfl(sd, 0, 64));
                const float t = __fadd_rn(__fsub_rn(__fmul_rn(m, A), B), __fsub_rn(Ds, __fmul_rn(m, Cs)));
                const float wd = __fmul_rn(w, delta);
                g_dist = __fmul_rn(rr.dist_scale, __fadd_rn(__fmul_rn(2.0f, t), __fmul_rn(2.0f / 3.0f, wd)));
                if (valid) acc_D = __fadd_rn(acc_D, __fadd_rn(__fmul_rn(w, t), __fmul_rn(1.0f / 3.0f, __fmul_rn(w, wd))));
            }
        }
        float v = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
        if (valid) {
            if constexpr (IDX) {
                if (row >= 0) { cr = rgb[row * rgb_stride]; cg = rgb[row * rgb_stride + 1]; cb = rgb[row * rgb_stride + 2]; }
            } else {
                cr = rgb[i * rgb_stride]; cg = rgb[i * rgb_stride + 1]; cb = rgb[i * rgb_stride + 2];
            }
            v = __fadd_rn(__fadd_rn(__fmul_rn(gr, cr), __fmul_rn(gg, cg)), __fmul_rn(gb, cb));
            v = __fadd_rn(v, __fmul_rn(gd, zc));
            if (g_w) v = __fadd_rn(v, g_w[i]);
            if constexpr (EXT) v = __fadd_rn(v, __fmul_rn(gw_scale, w));
            if constexpr (REG) v = __fadd_rn(v, g_dist);
            v = __fsub_rn(v, bg);
        }
        const float wv_ = valid ? __fmul_rn(w, v) : 0.0f;
        const float incl_rev = wave_incl_sum_rev(wv_, lane);
        float suffix;                                    // strictly later samples
        if constexpr (FINE) {
            float later = __shfl_down(incl_rev, 1, 64);
            if (lane == 63) later = 0.0f;
            suffix = __fadd_rn(later, carry);
        } else {
            suffix = __fadd_rn(__fsub_rn(incl_rev, wv_), carry);
        }
        carry = __fadd_rn(carry, __shfl(incl_rev, 0, 64));
        if (IDX ? (valid && row >= 0) : valid) {
            const int64_t o = IDX ? row : i;
            const float d_alpha = __fsub_rn(__fmul_rn(T, v), suffix / f);
            if constexpr (REG) {
                float ds = __fmul_rn(__fmul_rn(d_alpha, dist), e);
                if (64 * k + lane < rr.occ_m) {          // (occ_m = 0 without the occlusion term)
                    ds = __fadd_rn(ds, rr.occ_scale);
                    acc_O = __fadd_rn(acc_O, fmaxf(sg, 0.0f));
                }
                d_sigma[o * d_sigma_stride] = sg > 0.0f ? ds : 0.0f;
            } else {
                d_sigma[o * d_sigma_stride] = sg > 0.0f ? __fmul_rn(__fmul_rn(d_alpha, dist), e) : 0.0f;
            }
            d_rgb[o * d_rgb_stride] = __fmul_rn(w, gr);
            d_rgb[o * d_rgb_stride + 1] = __fmul_rn(w, gg);
            d_rgb[o * d_rgb_stride + 2] = __fmul_rn(w, gb);
        }
        if constexpr (GEOM) {
            float dd = 0.0f;                             // dL/d dist_i
            if (valid) {
                const float d_alpha = __fsub_rn(__fmul_rn(T, v), suffix / f);
                dd = __fmul_rn(__fmul_rn(d_alpha, fmaxf(sg, 0.0f)), e);
            }
            const bool last = (64 * k + lane + 1 == S);
            // (z_{i+1} - z_i) again, as `sample` formed it: dist / |d| would divide by zero on a zero direction
            float zn = __shfl_down(zc, 1, 64);
            if (lane == 63 && 64 * k + lane + 1 < S) zn = z[i + 1];
            s_norm = __fadd_rn(s_norm, __fmul_rn(dd, last ? 1e10f : __fsub_rn(zn, zc)));
            float up = __shfl_up(dd, 1, 64);
            if (lane == 0) up = 0.0f;
            const float own = last ? 0.0f : dd;
            const float dz = __fadd_rn(__fmul_rn(gd, w), __fmul_rn(norm, __fsub_rn(up, own)));
            if (valid && (lane > 0 || k == 0)) d_z[i] = dz;
            const float dd_end = __shfl(dd, 63, 64);
            if (k + 1 < n_seg && lane == 0)              // the first sample of segment k + 1: its neighbour is this segment's lane 63
                d_z[r * S + 64 * (k + 1)] = __fadd_rn(pend_z, __fmul_rn(norm, dd_end));
            pend_z = __shfl(dz, 0, 64);
        }
    }
    if constexpr (REG) {
        reg_out[0] = wave_sum(acc_D);
        reg_out[1] = __fmul_rn(wave_sum(acc_O), rr.occ_inv);
    }
    if constexpr (GEOM) {
        const float dn = wave_sum(s_norm);
        const float dk = lane == 0 ? d[0] : (lane == 1 ? d[1] : d[2]);
        if (lane < 3) d_rays_d[r * 3 + lane] = norm > 0.0f ? __fmul_rn(dn, dk / norm) : 0.0f;
    }
}

struct LossExt {
    NoiseSrc noise;
    const float* target_depth;        // (R) or NULL
    float gd_scale;                   // depth_weight / R
    float gw_scale;                   // 2 reg_weight / (R S)
};
inline LossExt loss_ext_of(const LossTerms& lt, int64_t n_rays, int S) {
    LossExt ext{};
    ext.noise.std = lt.noise_std; ext.noise.n = lt.noise; ext.noise.seed = lt.rng_seed;
    ext.target_depth = lt.target_depth;
    ext.gd_scale = lt.target_depth ? lt.depth_weight / (float)n_rays : 0.0f;
    ext.gw_scale = 2.0f * lt.reg_weight / ((float)n_rays * (float)S);
    return ext;
}

}  // namespace

}  // namespace nrf
