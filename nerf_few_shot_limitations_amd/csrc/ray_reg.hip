// ray_reg.hip -- the fused training step's loss launch with the two few-shot ray regularisers (nerfhip.h:
// nrf_composite_reg_loss_backward, nrf_ray_terms_finish):
//
//   reg_loss_backward_kernel<false> : composite_loss_backward_kernel<true> (staged_kernels.hip) with composite_backward_ray's REG
//                                     work (composite_core.hpp): the distortion loss of mip-NeRF 360 and the near-camera density
//                                     penalty of FreeNeRF, both formed from what the compositor backward holds in registers.
//   reg_loss_backward_kernel<true>  : the same on the compacted rows of a step under an occupancy grid (indexed_loss_backward_kernel).
//   ray_terms_finish_kernel         : one workgroup adds the rays' two new terms up in a fixed order and appends them to the four
//                                     loss values the optimiser launch left.
//
// One WAVE per ray, LANE <-> sample, as in the two parents; per-ray arithmetic outside the REG work is theirs, so with both new
// weights 0 the outputs are their bits.  No atomics: two runs give the same bits.  Both loss kernels carry the four pointers that
// are touched once per ray in vector registers (as indexed_loss_backward_kernel does), and with them the regularisers' five
// values, the noise source and the two scales of the multi-term loss: the scalar file has no room for them next to the scans'
// masks (without it: 12 - 15 spilled SGPRs).
#include "loss_walk.hpp"          // kBlock, grid_for, ray_reg_of

namespace nrf {

namespace {

// ray_loss (5,R): squared rgb error | sum of w^2 | |depth - target_depth| | D_r | O_r
template <bool IDX>
__global__ void __launch_bounds__(kBlock) reg_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                   int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                   int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                   float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                   int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                   float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                   const LossExt ext, const RayReg reg, const int32_t* __restrict__ slot) {
    __shared__ float seg[kBlock / 64][3 * kMaxSegments];          // per wave: seg_T | the two prefix carries of the distortion scans
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t gtid = blockIdx.x * (int64_t)kBlock + threadIdx.x, n_threads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = gtid; i < zero_n; i += n_threads) zero_buf[i] = 0.0f;
    const float* tdepth = ext.target_depth;
    asm volatile("" : "+v"(target), "+v"(pred), "+v"(ray_loss), "+v"(tdepth));
    RayReg rr = reg;                                     // (so do the regularisers' five values and the depth term's scale)
    float gd_scale = ext.gd_scale;
    asm volatile("" : "+v"(rr.dist_scale), "+v"(rr.kappa), "+v"(rr.occ_scale), "+v"(rr.occ_inv), "+v"(rr.occ_m), "+v"(gd_scale));
    NoiseSrc ns = ext.noise;
    float gw_scale = ext.gw_scale;
    asm volatile("" : "+v"(ns.std), "+v"(ns.n), "+v"(ns.seed), "+v"(gw_scale));
    const float count = 3.0f * (float)n_rays;
    const float scale = 2.0f * weight / count;
    for (int64_t r = gtid >> 6; r < n_rays; r += n_threads >> 6) {
        RaySums o = composite_ray<true, IDX>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, nullptr, ns, slot);
        if (white_bkgd) {
            const float bg = __fsub_rn(1.0f, o.acc);
            o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
        }
        const float dr = o.r - target[r * 3], dg = o.g - target[r * 3 + 1], db = o.b - target[r * 3 + 2];
        const float dd = tdepth ? __fsub_rn(o.depth, tdepth[r]) : 0.0f;
        const float gd = dd > 0.0f ? gd_scale : (dd < 0.0f ? -gd_scale : 0.0f);          // l1_loss: sign(0) = 0
        if (lane == 0) {
            ray_loss[n_rays + r] = o.w2; ray_loss[2 * n_rays + r] = fabsf(dd);
            if (pred) { pred[r * 3] = o.r; pred[r * 3 + 1] = o.g; pred[r * 3 + 2] = o.b; }
            ray_loss[r] = dr * dr + dg * dg + db * db;
        }
        float terms[2];                                  // D_r, O_r
        composite_backward_ray<true, false, IDX, true>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, white_bkgd, scale * dr,
                                                       scale * dg, scale * db, gd, nullptr, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, seg[wv],
                                                       ns, gw_scale, nullptr, nullptr, slot, rr, terms);
        if (lane == 0) { ray_loss[3 * n_rays + r] = terms[0]; ray_loss[4 * n_rays + r] = terms[1]; }
    }
}

// losses6 = [total + dist_weight mean D + occ_weight mean O, rgb, depth, reg, mean D, mean O] from rows 3 and 4 of ray_terms and the
// four values of the optimiser launch.  One workgroup, every partial sum in a fixed order.
__global__ void __launch_bounds__(1024) ray_terms_finish_kernel(const float* __restrict__ ray_terms, int64_t n_rays, float dist_weight,
                                                                float occ_weight, const float* __restrict__ losses4, float* __restrict__ losses6) {
    __shared__ float part[2][16];
    float sd = 0.0f, so = 0.0f;
    for (int64_t i = threadIdx.x; i < n_rays; i += 1024) {
        sd = __fadd_rn(sd, ray_terms[3 * n_rays + i]);
        so = __fadd_rn(so, ray_terms[4 * n_rays + i]);
    }
    sd = wave_sum(sd); so = wave_sum(so);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = sd; part[1][threadIdx.x >> 6] = so; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float td = 0.0f, to = 0.0f;
        for (int k = 0; k < 16; ++k) { td = __fadd_rn(td, part[0][k]); to = __fadd_rn(to, part[1][k]); }
        const float md = td / (float)n_rays, mo = to / (float)n_rays;
        losses6[0] = __fadd_rn(__fadd_rn(losses4[0], __fmul_rn(dist_weight, md)), __fmul_rn(occ_weight, mo));
        losses6[1] = losses4[1]; losses6[2] = losses4[2]; losses6[3] = losses4[3];
        losses6[4] = md; losses6[5] = mo;
    }
}

}  // namespace

int launch_composite_reg_loss_backward(const LossLaunch& a, const RayRegTerms& rt) {
    if (a.n_rays <= 0 || a.S < 1 || a.S > 64 * kMaxSegments) return NRF_EINVAL;
    const LossExt ext = loss_ext_of(a.lt, a.n_rays, a.S);
    const RayReg reg = ray_reg_of(rt, a.n_rays, a.S);
    const int64_t work = std::max(a.n_rays * 64, (a.zero_n + 3) / 4);
    const dim3 grid(grid_for(work, kBlock, 16384)), block(kBlock);
    if (a.slot)
        hipLaunchKernelGGL(reg_loss_backward_kernel<true>, grid, block, 0, a.s, a.rgb, a.rgb_stride, a.sigma, a.sigma_stride, a.z, a.rays_d, a.n_rays,
                           a.S, a.white_bkgd, a.target, a.lt.rgb_weight, a.pred, a.d_rgb, a.d_rgb_stride, a.d_sigma, a.d_sigma_stride, a.ray_terms,
                           a.zero_buf, a.zero_n, ext, reg, a.slot);
    else
        hipLaunchKernelGGL(reg_loss_backward_kernel<false>, grid, block, 0, a.s, a.rgb, a.rgb_stride, a.sigma, a.sigma_stride, a.z, a.rays_d, a.n_rays,
                           a.S, a.white_bkgd, a.target, a.lt.rgb_weight, a.pred, a.d_rgb, a.d_rgb_stride, a.d_sigma, a.d_sigma_stride, a.ray_terms,
                           a.zero_buf, a.zero_n, ext, reg, (const int32_t*)nullptr);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_ray_terms_finish(const float* ray_terms, int64_t n_rays, float dist_weight, float occ_weight, const float* losses4, float* losses6,
                            hipStream_t s) {
    if (n_rays <= 0) return NRF_EINVAL;
    hipLaunchKernelGGL(ray_terms_finish_kernel, dim3(1), dim3(1024), 0, s, ray_terms, n_rays, dist_weight, occ_weight, losses4, losses6);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
