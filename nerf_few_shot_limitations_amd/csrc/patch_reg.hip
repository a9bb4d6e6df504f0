// patch_reg.hip -- the fused training step's loss launch with RegNeRF's depth-smoothness term on patches of unseen views (nerfhip.h:
// nrf_composite_patch_loss_backward, nrf_patch_terms_finish).  The batch layout, the walk over it and the finish body are
// loss_walk.hpp's.
//
//   patch_loss_backward_kernel<false, *> : the walk on dense rows.
//   patch_loss_backward_kernel<true, *>  : the same on the compacted rows of a step under an occupancy grid.
//   <*, true> is launched with N_p > 0: the compositor bodies with composite_core.hpp's FINE; <*, false> with N_p = 0:
//   reg_loss_backward_kernel's (ray_reg.hip) instantiations, for its bits.
//   patch_terms_finish_kernel            : one workgroup forms the step's seven loss values from ray_terms and patch_terms.
#include "loss_walk.hpp"

namespace nrf {

namespace {

template <bool IDX, bool FINE>
__global__ void __launch_bounds__(kBlock) patch_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                     int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                     int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                     float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                     int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                     float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                     const LossExt ext, const RayReg reg, const int32_t* __restrict__ slot,
                                                                     const PatchArgs pa) {
    __shared__ float seg[kWaves][3 * kMaxSegments];
    __shared__ float dep[kMaxPatch * kMaxPatch];
    LossWalk w;
    loss_walk_prologue(w, rgb, rgb_stride, sigma, sigma_stride, z, rays_d, n_rays, S, white_bkgd, target, weight, pred, d_rgb, d_rgb_stride, d_sigma,
                       d_sigma_stride, ray_loss, zero_buf, zero_n, ext, reg, slot, pa);
    loss_walk<IDX, FINE, false>(w, seg, dep);
}

// losses7 = [total, rgb, depth, reg, dist, occ, smooth]
__global__ void __launch_bounds__(1024) patch_terms_finish_kernel(const float* __restrict__ ray_terms, const float* __restrict__ patch_terms,
                                                                  const FinishArgs a, float* __restrict__ losses7) {
    terms_finish<6, 1024>(ray_terms, patch_terms, nullptr, nullptr, a, losses7);
}

}  // namespace

int launch_composite_patch_loss_backward(const LossLaunch& a, const RayRegTerms& rt, const PatchRegTerms& pt, float* patch_terms, float* patch_depth) {
    const int64_t n_sup = batch_n_sup(pt, a.n_rays, a.S);
    if (n_sup < 0) return NRF_EINVAL;
    if (pt.n_patches > 0 && !patch_terms) return NRF_EINVAL;
    // a wave per supervised ray, the zero fill's share, a workgroup per patch until the cap
    const int64_t work = std::max(std::max(n_sup * 64, (a.zero_n + 3) / 4), pt.n_patches * kBlock);
    const dim3 grid(grid_for(work, kBlock, 16384)), block(kBlock);
    // with patches the compositor bodies of better conditioning; without, reg_loss_backward_kernel's, for its bits
    auto* kernel = a.slot ? (pt.n_patches > 0 ? patch_loss_backward_kernel<true, true> : patch_loss_backward_kernel<true, false>)
                          : (pt.n_patches > 0 ? patch_loss_backward_kernel<false, true> : patch_loss_backward_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, a.s, a.rgb, a.rgb_stride, a.sigma, a.sigma_stride, a.z, a.rays_d, a.n_rays, a.S, a.white_bkgd, a.target,
                       a.lt.rgb_weight, a.pred, a.d_rgb, a.d_rgb_stride, a.d_sigma, a.d_sigma_stride, a.ray_terms, a.zero_buf, a.zero_n,
                       patch_loss_ext_of(a.lt, a.n_rays, n_sup, a.S), ray_reg_of(rt, a.n_rays, a.S), a.slot,
                       patch_args_of(pt, n_sup, patch_terms, patch_depth));
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_patch_terms_finish(const float* ray_terms, int64_t n_rays, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                              const float* patch_terms, float* losses7, hipStream_t s) {
    const int64_t n_sup = batch_n_sup(pt, n_rays, S);
    if (n_sup < 0) return NRF_EINVAL;
    hipLaunchKernelGGL(patch_terms_finish_kernel, dim3(1), dim3(1024), 0, s, ray_terms, patch_terms, finish_args_of(n_rays, n_sup, S, lt, rt, pt, nullptr),
                       losses7);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
