// staged_kernels.hip -- one small gfx950 kernel per reference leaf (rays, samples, encoding,
// compositor, inverse-cdf resampling, feature fetch).  They back the drop-in Python surface
// (get_rays, sample_points_along_rays, PositionalEncoding, VolumeRenderer, ...) and the
// stage-wise parity tests.  All of them are HBM-bound elementwise / per-ray kernels: the
// layouts are the reference's own row-major tensors, reads and writes are coalesced along the
// innermost axis wherever the reference layout allows it.
#include <algorithm>

#include "kernels.hpp"
#include "composite_core.hpp"
#include "sample_pdf_impl.hpp"

namespace nrf {

namespace {

constexpr int kBlock = 256;

inline unsigned grid_for(int64_t n, int block, int64_t cap = 1 << 20) {
    int64_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// ---- a1: ray_sampler.py:4-30 ---------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) get_rays_kernel(Camera cam, int64_t ray_begin, int64_t n, float* __restrict__ rays_o,
                                                          float* __restrict__ rays_d) {
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        float o[3], d[3];
        camera_ray(cam, ray_begin + i, o, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) { rays_o[i * 3 + k] = o[k]; rays_d[i * 3 + k] = d[k]; }
    }
}

// ---- a2: ray_utils.py:39-84 ----------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) sample_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays,
                                                        DepthLadder lad, int perturb, const float* __restrict__ t_rand, uint64_t seed,
                                                        float* __restrict__ pts, float* __restrict__ z_vals) {
    const int64_t total = n_rays * lad.S;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / lad.S;
        const int s = (int)(i - r * lad.S);
        float z;
        if (perturb) {
            const float u = t_rand ? t_rand[i] : counter_uniform(seed, (uint64_t)r, (uint32_t)s);
            z = ladder_z_jitter(lad, s, u);
        } else {
            z = ladder_z(lad, s);
        }
        if (z_vals) z_vals[i] = z;
        if (pts) {
#pragma unroll
            for (int k = 0; k < 3; ++k) pts[i * 3 + k] = point_on_ray(rays_o[r * 3 + k], rays_d[r * 3 + k], z);
        }
    }
}

// ---- a4: positional_encoding.py:20-33 ------------------------------------------------------
__global__ void __launch_bounds__(kBlock) encode_kernel(const float* __restrict__ x, int64_t n, int dim, int L, int include_input,
                                                        const float* __restrict__ freq_bands, float* __restrict__ out) {
    const int d_out = dim * (2 * L + (include_input ? 1 : 0));
    const int64_t total = n * d_out;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t row = i / d_out;
        int f = (int)(i - row * d_out);
        float v;
        if (include_input && f < dim) {
            v = x[row * dim + f];
        } else {
            if (include_input) f -= dim;
            const int band = f / (2 * dim);
            const int rem = f - band * 2 * dim;
            const int j = rem >= dim ? rem - dim : rem;
            // log_sampling (every caller of the reference): 2^band, an exact scale; otherwise the caller's table
            // (positional_encoding.py:18: torch.linspace(1, 2^(L-1), L))
            const float arg = __fmul_rn(x[row * dim + j], freq_bands ? freq_bands[band] : (float)(1u << band));
            v = rem >= dim ? cosf(arg) : sinf(arg);
        }
        out[i] = v;
    }
}

// ---- a9/a10: nerf_mlp.py:165-215, volume_renderer.py:4-43 ------------------------------------
// HBM-bound: 20 B read (+4 B written when weights are requested) per ray-sample.  One WAVE per ray, LANE <-> sample, so
// every load/store of z, sigma, rgb and weights is a contiguous 64-element segment of the reference's (R,S,*) rows; the
// exclusive transmittance product (cumprod, :196-199) is a wave prefix product, the four sums are wave reductions.  The per-ray bodies
// (composite_ray, composite_backward_ray) live in composite_core.hpp.
__global__ void __launch_bounds__(kBlock) composite_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                           int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                           int64_t n_rays, int S, int white_bkgd, float* __restrict__ out_rgb,
                                                           float* __restrict__ out_depth, float* __restrict__ out_w) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        RaySums o = composite_ray(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, out_w);
        if (lane == 0) {
            if (white_bkgd) {
                const float bg = __fsub_rn(1.0f, o.acc);
                o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
            }
            out_rgb[r * 3] = o.r; out_rgb[r * 3 + 1] = o.g; out_rgb[r * 3 + 2] = o.b;
            if (out_depth) out_depth[r] = o.depth;
        }
    }
}

__global__ void __launch_bounds__(kBlock) composite_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                    int sigma_stride, const float* __restrict__ z,
                                                                    const float* __restrict__ rays_d, int64_t n_rays, int S, int white_bkgd,
                                                                    const float* __restrict__ g_rgb, const float* __restrict__ g_depth,
                                                                    const float* __restrict__ g_w, float* __restrict__ d_rgb,
                                                                    int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride) {
    __shared__ float seg_T[kBlock / 64][kMaxSegments];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        const float gr = g_rgb ? g_rgb[r * 3] : 0.0f, gg = g_rgb ? g_rgb[r * 3 + 1] : 0.0f, gb = g_rgb ? g_rgb[r * 3 + 2] : 0.0f;
        const float gd = g_depth ? g_depth[r] : 0.0f;
        composite_backward_ray(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, white_bkgd, gr, gg, gb, gd, g_w, d_rgb, d_rgb_stride,
                               d_sigma, d_sigma_stride, seg_T[wv]);
    }
}

// The three launches between the network's forward and its backward in a FusedStep -- compositor, loss with its gradient,
// compositor backward -- as ONE: the loss gradient of a ray needs nothing but the ray's own outputs and targets.  Same per-ray
// arithmetic as the three kernels (the two bodies of composite_core.hpp), so d_rgb / d_sigma are bit-equal to the staged sequence.  The loss VALUE
// needs all rays: every ray leaves its terms in `ray_loss` and a later launch adds them up in a fixed order (adam_kernel's side
// job, train_shared.hip) -- a device-wide "last workgroup sums" inside this kernel costs a release fence (an L2 write-back on this
// chip) per workgroup: measured 53 us against 16 us for the three separate launches.  Side job: `zero_buf` (the caller's flat
// gradient vector, which the weight-gradient reduction adds into) is cleared by the same launch.
//   EXT = false: `rgb_weight * nn.MSELoss()` (train.py:236,36-44,285), d loss / d pred = 2 w (pred - target) / (3 R); ray_loss
//                (R) = the rays' squared errors.  nrf_composite_mse_backward.
//   EXT = true:  nerf_mlp.NeRFLoss on a VolumeRenderer in train() mode (nerf_mlp.py:188-190,217-258; train_multiscale.py:207-211):
//                density noise in front of the compositor's ReLU, + depth_weight * l1(depth, target_depth) + reg_weight *
//                mean(weights^2); ray_loss (3,R) = squared rgb error | sum of w^2 | |depth - target_depth|.  With every option off
//                its d_rgb / d_sigma / pred / ray_loss[0:R] are the EXT = false kernel's bits.
template <bool EXT>
__global__ void __launch_bounds__(kBlock) composite_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride,
                                                                         const float* __restrict__ sigma, int sigma_stride,
                                                                         const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                         int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                         float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                         int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                         float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                         const LossExt ext) {
    __shared__ float seg_T[kBlock / 64][kMaxSegments];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t gtid = blockIdx.x * (int64_t)kBlock + threadIdx.x, n_threads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = gtid; i < zero_n; i += n_threads) zero_buf[i] = 0.0f;
    const float count = 3.0f * (float)n_rays;
    const float scale = 2.0f * weight / count;
    for (int64_t r = gtid >> 6; r < n_rays; r += n_threads >> 6) {
        RaySums o = composite_ray<EXT>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, nullptr, ext.noise);
        if (white_bkgd) {
            const float bg = __fsub_rn(1.0f, o.acc);
            o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
        }
        const float dr = o.r - target[r * 3], dg = o.g - target[r * 3 + 1], db = o.b - target[r * 3 + 2];
        float gd = 0.0f;
        if constexpr (EXT) {
            const float dd = ext.target_depth ? __fsub_rn(o.depth, ext.target_depth[r]) : 0.0f;
            gd = dd > 0.0f ? ext.gd_scale : (dd < 0.0f ? -ext.gd_scale : 0.0f);          // l1_loss: sign(0) = 0
            if (lane == 0) { ray_loss[n_rays + r] = o.w2; ray_loss[2 * n_rays + r] = fabsf(dd); }
        }
        if (lane == 0) {
            if (pred) { pred[r * 3] = o.r; pred[r * 3 + 1] = o.g; pred[r * 3 + 2] = o.b; }
            ray_loss[r] = dr * dr + dg * dg + db * db;
        }
        composite_backward_ray<EXT>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, white_bkgd, scale * dr, scale * dg, scale * db, gd,
                                    nullptr, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, seg_T[wv], ext.noise, ext.gw_scale);
    }
}

// The step under an occupancy grid (nrf_composite_loss_backward_indexed): the EXT = true kernel above on compacted rows -- rgb / sigma /
// d_rgb / d_sigma hold the evaluated samples alone, `slot` (R,S) names each ladder sample's row or -1 (composite_ray: IDX).  A kernel of
// its own, so that the two above stay the code they were.  It holds one more pointer than the scalar register file has room for next
// to the others: the four that are touched once per ray (and live across both passes over its samples) travel in vector registers
// instead of being spilled.
__global__ void __launch_bounds__(kBlock) indexed_loss_backward_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                       int sigma_stride, const float* __restrict__ z, const float* __restrict__ rays_d,
                                                                       int64_t n_rays, int S, int white_bkgd, const float* __restrict__ target,
                                                                       float weight, float* __restrict__ pred, float* __restrict__ d_rgb,
                                                                       int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                       float* __restrict__ ray_loss, float* __restrict__ zero_buf, int64_t zero_n,
                                                                       const LossExt ext, const int32_t* __restrict__ slot) {
    __shared__ float seg_T[kBlock / 64][kMaxSegments];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t gtid = blockIdx.x * (int64_t)kBlock + threadIdx.x, n_threads = (int64_t)gridDim.x * kBlock;
    for (int64_t i = gtid; i < zero_n; i += n_threads) zero_buf[i] = 0.0f;
    const float* tdepth = ext.target_depth;
    asm volatile("" : "+v"(target), "+v"(pred), "+v"(ray_loss), "+v"(tdepth));
    const float count = 3.0f * (float)n_rays;
    const float scale = 2.0f * weight / count;
    for (int64_t r = gtid >> 6; r < n_rays; r += n_threads >> 6) {
        RaySums o = composite_ray<true, true>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, nullptr, ext.noise, slot);
        if (white_bkgd) {
            const float bg = __fsub_rn(1.0f, o.acc);
            o.r = __fadd_rn(o.r, bg); o.g = __fadd_rn(o.g, bg); o.b = __fadd_rn(o.b, bg);
        }
        const float dr = o.r - target[r * 3], dg = o.g - target[r * 3 + 1], db = o.b - target[r * 3 + 2];
        const float dd = tdepth ? __fsub_rn(o.depth, tdepth[r]) : 0.0f;
        const float gd = dd > 0.0f ? ext.gd_scale : (dd < 0.0f ? -ext.gd_scale : 0.0f);          // l1_loss: sign(0) = 0
        if (lane == 0) {
            ray_loss[n_rays + r] = o.w2; ray_loss[2 * n_rays + r] = fabsf(dd);
            if (pred) { pred[r * 3] = o.r; pred[r * 3 + 1] = o.g; pred[r * 3 + 2] = o.b; }
            ray_loss[r] = dr * dr + dg * dg + db * db;
        }
        composite_backward_ray<true, false, true>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, white_bkgd, scale * dr, scale * dg,
                                                  scale * db, gd, nullptr, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, seg_T[wv], ext.noise,
                                                  ext.gw_scale, nullptr, nullptr, slot);
    }
}


// ---- a3: ray_utils.py:86-143 (intent): sample_pdf_impl.hpp (the body shared with hier_kernels.hip) ----------------
__global__ void sample_pdf_kernel(const float* __restrict__ z, const float* __restrict__ w, int64_t n_rays, int S, int Ni,
                                  const float* __restrict__ u_in, int64_t u_ray_stride, float* __restrict__ samples, float* __restrict__ z_union) {
    sample_pdf_rows(z, w, n_rays, S, Ni, u_in, u_ray_stride, samples, z_union, nullptr);
}
// ---- a8: ray_utils.py:176-210 + dino_feature_model.py:114-148 ---------------------------------
__device__ __forceinline__ void project_point(const DinoDev& d, const float p[3], float& xn, float& yn) {
    float pc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        pc[i] = d.inv_pose[4 * i + 0] * p[0] + d.inv_pose[4 * i + 1] * p[1] + d.inv_pose[4 * i + 2] * p[2] + d.inv_pose[4 * i + 3];
    const float zi = pc[2] + 1e-8f;
    const float x = pc[0] / zi * d.focal + (float)d.W / 2.0f;
    const float y = pc[1] / zi * d.focal + (float)d.H / 2.0f;
    xn = x / (float)d.W * 2.0f - 1.0f;
    yn = y / (float)d.H * 2.0f - 1.0f;
}

// points2d: `points` already are normalised image coordinates (n,2) (sample_features_at_points on its own,
// dino_feature_model.py:114-148); otherwise world points (n,3) projected into the source view first
__global__ void __launch_bounds__(kBlock) project_fetch_kernel(DinoDev d, const float* __restrict__ points, int64_t n, float* __restrict__ feats,
                                                               float* __restrict__ xy, int points2d) {
    const int64_t total = n * d.C;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t pi = i / d.C;
        const int ch = (int)(i - pi * d.C);
        float xn, yn;
        if (points2d) {
            xn = points[pi * 2]; yn = points[pi * 2 + 1];
        } else {
            const float p[3] = {points[pi * 3], points[pi * 3 + 1], points[pi * 3 + 2]};
            project_point(d, p, xn, yn);
        }
        if (xy && ch == 0) { xy[pi * 2] = xn; xy[pi * 2 + 1] = yn; }
        // grid_sample, bilinear, zeros padding, align_corners=False
        const float gx = ((xn + 1.0f) * (float)d.Wp - 1.0f) * 0.5f;
        const float gy = ((yn + 1.0f) * (float)d.Hp - 1.0f) * 0.5f;
        const float x0 = floorf(gx), y0 = floorf(gy);
        float acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float xi = x0 + dx, yi = y0 + dy;
                const float wx = dx ? gx - x0 : x0 + 1.0f - gx;
                const float wy = dy ? gy - y0 : y0 + 1.0f - gy;
                if (xi >= 0.0f && xi <= (float)(d.Wp - 1) && yi >= 0.0f && yi <= (float)(d.Hp - 1))
                    acc += d.features[((int64_t)yi * d.Wp + (int64_t)xi) * d.C + ch] * (wx * wy);
            }
        feats[i] = acc;
    }
}

// Adjoint of project_fetch_kernel with respect to the map: d_map[tap] += w_tap * d_feats[sample] over the <= 4 on-map taps
// (the same gx, gy, floorf, wx * wy and on-map test as above).  No atomics: 81 texel rows taking 4 taps from each of 10^4..10^5
// samples is the worst contention shape there is, and the parameter gradients of this library are bit-reproducible on
// purpose.  Slab form instead: workgroup (chunk, slab) walks ITS samples in order and adds into a private copy of ITS chunk of
// the map in LDS -- thread <-> channel, so no two threads ever touch one address of it and the order of the
// additions is fixed -- then leaves the copy in the workspace with plain stores; fetch_backward_reduce_kernel adds the
// slabs' copies per element in slab order.  A chunk = kFetchLdsFloats / cw texels x cw = min(C, kFetchLdsFloats) channels: one
// chunk for the 9 x 9 maps of the reference, 22 for a 37 x 37 x 128 one.
constexpr int kFetchLdsFloats = 8192;        // 32 KiB
constexpr int kFetchBatch = 8;               // samples whose gradient rows are in flight together
constexpr int kFetchTaps = 64;               // samples whose taps are worked out together (one per thread of the first wave)

struct FetchBwdGeo {
    int cw, n_cchunks, tpc, n_tchunks, threads;
    int64_t slabs, per_slab;
};

inline FetchBwdGeo fetch_bwd_geo(int Hp, int Wp, int C, int64_t n) {
    FetchBwdGeo g;
    g.cw = C < kFetchLdsFloats ? C : kFetchLdsFloats;
    g.n_cchunks = (C + g.cw - 1) / g.cw;
    g.tpc = kFetchLdsFloats / g.cw;
    const int64_t texels = (int64_t)Hp * Wp;
    if (g.tpc > texels) g.tpc = (int)texels;
    g.n_tchunks = (int)((texels + g.tpc - 1) / g.tpc);
    g.threads = g.cw <= 64 ? 64 : (g.cw <= 128 ? 128 : 256);
    // ~64 samples per slab, at most ~1024 workgroups in all (a function of the sizes only: the workspace is sized without a device)
    const int64_t chunks = (int64_t)g.n_tchunks * g.n_cchunks;
    int64_t max_slabs = 1024 / chunks;
    if (max_slabs < 1) max_slabs = 1;
    int64_t slabs = (n + 63) / 64;
    if (slabs > max_slabs) slabs = max_slabs;
    if (slabs < 1) slabs = 1;
    g.per_slab = (n + slabs - 1) / slabs;
    if (g.per_slab < 1) g.per_slab = 1;
    g.slabs = (n + g.per_slab - 1) / g.per_slab;
    if (g.slabs < 1) g.slabs = 1;
    return g;
}

__global__ void __launch_bounds__(256) project_fetch_backward_kernel(DinoDev d, const float* __restrict__ points, int64_t n,
                                                                     const float* __restrict__ d_feats, float* __restrict__ ws, int points2d,
                                                                     int cw, int n_cchunks, int tpc, int64_t per_slab) {
    __shared__ float acc[kFetchLdsFloats];
    __shared__ int4 s_tap[kFetchTaps];
    __shared__ float4 s_wt[kFetchTaps];
    const int chunk = blockIdx.x, slab = blockIdx.y;
    const int tchunk = chunk / n_cchunks, c0 = (chunk - tchunk * n_cchunks) * cw;
    const int64_t texels = (int64_t)d.Hp * d.Wp;
    const int64_t t0 = (int64_t)tchunk * tpc, t1 = t0 + tpc < texels ? t0 + tpc : texels;
    const int nt = (int)(t1 - t0);
    const int cn = c0 + cw <= d.C ? cw : d.C - c0;          // channels of this chunk
    for (int t = 0; t < nt; ++t)
        for (int c = threadIdx.x; c < cn; c += blockDim.x) acc[t * cw + c] = 0.0f;
    const int64_t s0 = slab * per_slab, s1 = s0 + per_slab < n ? s0 + per_slab : n;
    for (int64_t sb = s0; sb < s1; sb += kFetchTaps) {
        // the taps of the next kFetchTaps samples, one sample per thread of the first wave: texel inside the chunk (-1: off the
        // map or in another chunk) and weight
        __syncthreads();
        if (threadIdx.x < kFetchTaps) {
            const int64_t pi = sb + threadIdx.x;
            int tp[4] = {-1, -1, -1, -1};
            float wt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (pi < s1) {
                float xn, yn;
                if (points2d) {
                    xn = points[pi * 2]; yn = points[pi * 2 + 1];
                } else {
                    const float p[3] = {points[pi * 3], points[pi * 3 + 1], points[pi * 3 + 2]};
                    project_point(d, p, xn, yn);
                }
                const float gx = ((xn + 1.0f) * (float)d.Wp - 1.0f) * 0.5f;
                const float gy = ((yn + 1.0f) * (float)d.Hp - 1.0f) * 0.5f;
                const float x0 = floorf(gx), y0 = floorf(gy);
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const float xi = x0 + dx, yi = y0 + dy;
                        const float wx = dx ? gx - x0 : x0 + 1.0f - gx;
                        const float wy = dy ? gy - y0 : y0 + 1.0f - gy;
                        if (xi >= 0.0f && xi <= (float)(d.Wp - 1) && yi >= 0.0f && yi <= (float)(d.Hp - 1)) {
                            const int64_t texel = (int64_t)yi * d.Wp + (int64_t)xi;
                            if (texel >= t0 && texel < t1) {
                                tp[2 * dy + dx] = (int)(texel - t0);
                                wt[2 * dy + dx] = wx * wy;
                            }
                        }
                    }
            }
            s_tap[threadIdx.x] = make_int4(tp[0], tp[1], tp[2], tp[3]);
            s_wt[threadIdx.x] = make_float4(wt[0], wt[1], wt[2], wt[3]);
        }
        __syncthreads();
        const int cnt = (int)(s1 - sb < kFetchTaps ? s1 - sb : kFetchTaps);
        for (int c = threadIdx.x; c < cn; c += blockDim.x) {
            const float* gp = d_feats + sb * d.C + c0 + c;
            for (int u0 = 0; u0 < cnt; u0 += kFetchBatch) {      // kFetchBatch gradient rows in flight, applied in sample order
                int4 tp[kFetchBatch];
                float g[kFetchBatch];
#pragma unroll
                for (int u = 0; u < kFetchBatch; ++u) {
                    tp[u] = u0 + u < cnt ? s_tap[u0 + u] : make_int4(-1, -1, -1, -1);
                    const bool any = (tp[u].x & tp[u].y & tp[u].z & tp[u].w) >= 0;       // -1 = all bits set
                    g[u] = any ? gp[(int64_t)(u0 + u) * d.C] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < kFetchBatch; ++u) {
                    if ((tp[u].x & tp[u].y & tp[u].z & tp[u].w) < 0) continue;
                    const float4 w = s_wt[u0 + u];
                    if (tp[u].x >= 0) acc[tp[u].x * cw + c] += g[u] * w.x;
                    if (tp[u].y >= 0) acc[tp[u].y * cw + c] += g[u] * w.y;
                    if (tp[u].z >= 0) acc[tp[u].z * cw + c] += g[u] * w.z;
                    if (tp[u].w >= 0) acc[tp[u].w * cw + c] += g[u] * w.w;
                }
            }
        }
    }
    float* out = ws + (int64_t)slab * texels * d.C;
    for (int t = 0; t < nt; ++t)
        for (int c = threadIdx.x; c < cn; c += blockDim.x) out[(t0 + t) * d.C + c0 + c] = acc[t * cw + c];
}

// d_map[e] = (accumulate ? d_map[e] : 0) + sum over the slabs, in slab order, of their copies' element e
__global__ void __launch_bounds__(kBlock) fetch_backward_reduce_kernel(const float* __restrict__ ws, int64_t elems, int64_t slabs,
                                                                       float* __restrict__ d_map, int accumulate) {
    for (int64_t e = blockIdx.x * (int64_t)kBlock + threadIdx.x; e < elems; e += (int64_t)gridDim.x * kBlock) {
        float s = 0.0f;
        int64_t k = 0;
        for (; k + 8 <= slabs; k += 8) {                     // eight loads in flight, added in order
            float q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = ws[(k + j) * elems + e];
#pragma unroll
            for (int j = 0; j < 8; ++j) s += q[j];
        }
        for (; k < slabs; ++k) s += ws[k * elems + e];
        d_map[e] = accumulate ? d_map[e] + s : s;
    }
}

int fetch_backward_impl(const DinoDev& d, const float* points, int points2d, int64_t n, const float* d_feats, float* d_map, int accumulate,
                          float* ws, hipStream_t s) {
    const FetchBwdGeo g = fetch_bwd_geo(d.Hp, d.Wp, d.C, n);
    const int64_t elems = (int64_t)d.Hp * d.Wp * d.C;
    hipLaunchKernelGGL(project_fetch_backward_kernel, dim3((unsigned)(g.n_tchunks * g.n_cchunks), (unsigned)g.slabs), dim3(g.threads), 0, s, d,
                       points, n, d_feats, ws, points2d, g.cw, g.n_cchunks, g.tpc, g.per_slab);
    if (hipGetLastError() != hipSuccess) return NRF_EHIP;
    hipLaunchKernelGGL(fetch_backward_reduce_kernel, dim3(grid_for(elems, kBlock, 4096)), dim3(kBlock), 0, s, ws, elems, g.slabs, d_map, accumulate);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

// Adjoint of project_fetch_kernel with respect to the point: the bilinear fetch's derivative along x and y (the same gx, gy,
// floorf and on-map test as the forward; piecewise constant in the sample, with a kink at every texel edge), the normalisation,
// the pinhole projection with Zi = Z + 1e-8, and inv_pose's rotation.  With m_ab the texel row at (x0 + a, y0 + b), or 0 where
// that tap is off the map, and (tx, ty) = (gx - x0, gy - y0):
//     G_x = sum_c g_c [(1 - ty)(m_10 - m_00) + ty (m_11 - m_01)]        G_y = sum_c g_c [(1 - tx)(m_01 - m_00) + tx (m_11 - m_10)]
//     d_xn = G_x Wp / 2,  d_yn = G_y Hp / 2                              (points2d: these two are the result)
//     d_pc = (d_xn 2f / (W Zi),  d_yn 2f / (H Zi),  -(d_xn 2f X / W + d_yn 2f Y / H) / Zi^2),      d_p_j = sum_i inv_pose[i][j] d_pc_i
// An off-map tap is selected out, not multiplied by 0: a NaN / Inf texel reaches only the samples that have it among their
// on-map taps, and a sample with no tap on the map gets +0.  kFetchPtLanes lanes per sample: each takes every kFetchPtLanes-th
// group of 4 channels of the d_feats row and of the four tap rows (16-byte loads; the map is L2-resident) in ascending
// order, then a fixed xor-shuffle tree adds the lanes' sums -- no atomics, so a sample's result is bit-reproducible and does
// not depend on the batch around it -- and lane 0 writes.  Per sample 4 C bytes of d_feats read, 12 (8) B written, + 12 B read
// when accumulating.
constexpr int kFetchPtLanes = 16;

struct FetchVec { float v[4]; };

// channels c0 .. c0 + 3 of a row: one 16-byte load, or (VEC == false: C no multiple of 4, or a misaligned base) the ones below C
template <bool VEC>
__device__ __forceinline__ FetchVec fetch_vec_load(const float* row, int c0, int C) {
    FetchVec r;
    if constexpr (VEC) {
        const float4 q = *(const float4*)(row + c0);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.v[k] = c0 + k < C ? row[c0 + k] : 0.0f;
    }
    return r;
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock) fetch_points_backward_kernel(DinoDev d, const float* __restrict__ points, int64_t n,
                                                                       const float* __restrict__ d_feats, float* __restrict__ out, int points2d,
                                                                       int accumulate) {
    constexpr int kGroups = kBlock / kFetchPtLanes;
    const int sub = threadIdx.x % kFetchPtLanes, grp = threadIdx.x / kFetchPtLanes;
    for (int64_t base = blockIdx.x * (int64_t)kGroups; base < n; base += (int64_t)gridDim.x * kGroups) {
        const bool live = base + grp < n;
        const int64_t pi = live ? base + grp : n - 1;            // groups past the end keep their lanes in the shuffles and write nothing
        float xn, yn, pc[3] = {0.0f, 0.0f, 0.0f};
        if (points2d) {
            xn = points[pi * 2]; yn = points[pi * 2 + 1];
        } else {
            const float p[3] = {points[pi * 3], points[pi * 3 + 1], points[pi * 3 + 2]};
#pragma unroll
            for (int i = 0; i < 3; ++i)
                pc[i] = d.inv_pose[4 * i + 0] * p[0] + d.inv_pose[4 * i + 1] * p[1] + d.inv_pose[4 * i + 2] * p[2] + d.inv_pose[4 * i + 3];
            project_point(d, p, xn, yn);
        }
        const float gx = ((xn + 1.0f) * (float)d.Wp - 1.0f) * 0.5f;
        const float gy = ((yn + 1.0f) * (float)d.Hp - 1.0f) * 0.5f;
        const float x0 = floorf(gx), y0 = floorf(gy);
        const float tx = gx - x0, ty = gy - y0;
        bool on[4];
        const float* row[4];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float xi = x0 + dx, yi = y0 + dy;
                const bool ok = xi >= 0.0f && xi <= (float)(d.Wp - 1) && yi >= 0.0f && yi <= (float)(d.Hp - 1);
                on[2 * dy + dx] = ok;
                row[2 * dy + dx] = d.features + (ok ? ((int64_t)yi * d.Wp + (int64_t)xi) * d.C : 0);
            }
        const bool any = on[0] || on[1] || on[2] || on[3];
        float Gx = 0.0f, Gy = 0.0f;
        if (any) {
            const float* g_row = d_feats + pi * d.C;
            for (int c0 = sub * 4; c0 < d.C; c0 += kFetchPtLanes * 4) {
                const FetchVec g = fetch_vec_load<VEC>(g_row, c0, d.C);
                FetchVec m[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (on[k]) m[k] = fetch_vec_load<VEC>(row[k], c0, d.C);
                    else m[k] = FetchVec{{0.0f, 0.0f, 0.0f, 0.0f}};
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!VEC && c0 + q >= d.C) continue;
                    const float m00 = m[0].v[q], m10 = m[1].v[q], m01 = m[2].v[q], m11 = m[3].v[q];
                    Gx += g.v[q] * ((1.0f - ty) * (m10 - m00) + ty * (m11 - m01));
                    Gy += g.v[q] * ((1.0f - tx) * (m01 - m00) + tx * (m11 - m10));
                }
            }
        }
#pragma unroll
        for (int m = kFetchPtLanes / 2; m >= 1; m >>= 1) {
            Gx += __shfl_xor(Gx, m, kFetchPtLanes);
            Gy += __shfl_xor(Gy, m, kFetchPtLanes);
        }
        if (!live || sub != 0) continue;
        const float dxn = Gx * ((float)d.Wp * 0.5f), dyn = Gy * ((float)d.Hp * 0.5f);
        if (points2d) {
            out[pi * 2] = any ? dxn : 0.0f;
            out[pi * 2 + 1] = any ? dyn : 0.0f;
            continue;
        }
        const float zi = pc[2] + 1e-8f;
        const float ax = dxn * (2.0f * d.focal / (float)d.W), ay = dyn * (2.0f * d.focal / (float)d.H);
        const float dpc[3] = {ax / zi, ay / zi, -(ax * pc[0] + ay * pc[1]) / (zi * zi)};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float v = d.inv_pose[j] * dpc[0] + d.inv_pose[4 + j] * dpc[1] + d.inv_pose[8 + j] * dpc[2];
            const float r = any ? v : 0.0f;
            out[pi * 3 + j] = accumulate ? out[pi * 3 + j] + r : r;
        }
    }
}

int fetch_points_backward_impl(const DinoDev& d, const float* points, int points2d, int64_t n, const float* d_feats, float* out, int accumulate,
                               hipStream_t s) {
    if (n <= 0) return NRF_OK;
    const unsigned grid = grid_for(n * kFetchPtLanes, kBlock, 8192);
    const bool vec = d.C % 4 == 0 && ((reinterpret_cast<uintptr_t>(d.features) | reinterpret_cast<uintptr_t>(d_feats)) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(fetch_points_backward_kernel<true>, dim3(grid), dim3(kBlock), 0, s, d, points, n, d_feats, out, points2d, accumulate);
    else hipLaunchKernelGGL(fetch_points_backward_kernel<false>, dim3(grid), dim3(kBlock), 0, s, d, points, n, d_feats, out, points2d, accumulate);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

// ---- occupancy bit grids (nerfhip.h: nrf_occupancy) ----------------------------------------------
// Cell c is occupied iff one of its k consecutive densities is > threshold or NaN; a wave packs 64 cells into two words with one
// ballot, lanes 0 and 32 store them.  The loop bound is wave-uniform (whole waves step together), so the ballot sees every lane.
__global__ void __launch_bounds__(kBlock) occupancy_pack_kernel(const float* __restrict__ density, int64_t n_cells, int k, float threshold,
                                                                uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    for (int64_t first = blockIdx.x * (int64_t)kBlock + (threadIdx.x - lane); first < n_cells; first += (int64_t)gridDim.x * kBlock) {
        const int64_t c = first + lane;
        bool occ = false;
        if (c < n_cells) {
            const float* d = density + c * k;
            for (int j = 0; j < k; ++j) occ |= !(d[j] <= threshold);
        }
        const unsigned long long m = __ballot(occ);
        if (lane == 0) bits[first >> 5] = (uint32_t)m;
        if (lane == 32 && first + 32 < n_cells) bits[(first >> 5) + 1] = (uint32_t)(m >> 32);
    }
}

// One thread per word (32 cells along x): the OR of the nine rows around it, each spread by one cell to either side
__global__ void __launch_bounds__(kBlock) occupancy_dilate_kernel(const uint32_t* __restrict__ in, int wx, int ry, int rz, uint32_t* __restrict__ out) {
    const int64_t n_words = (int64_t)wx * ry * rz;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * kBlock) {
        const int x = (int)(i % wx), y = (int)((i / wx) % ry), z = (int)(i / ((int64_t)wx * ry));
        uint32_t acc = 0;
        for (int dz = -1; dz <= 1; ++dz) {
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy, zz = z + dz;
                if (yy < 0 || yy >= ry || zz < 0 || zz >= rz) continue;
                const uint32_t* row = in + ((int64_t)zz * ry + yy) * wx;
                const uint32_t w = row[x];
                acc |= w | (w << 1) | (w >> 1);
                if (x > 0) acc |= row[x - 1] >> 31;
                if (x + 1 < wx) acc |= row[x + 1] << 31;
            }
        }
        out[i] = acc;
    }
}

// Marking a grid from rendered weights (nerfhip.h: nrf_occupancy_mark_rays).  One WAVE per ray, LANE <-> sample, 64-sample segments
// front to back like composite_ray: the rows of weights and z_vals are read as contiguous segments (8 B per sample), the
// transmittance in front of a sample is 1 - (the wave's exclusive prefix sum of the weights + the carry of the earlier segments).
// The cell rule is that of fused_impl.hpp:occ_skips, restated here in the same single fp32 operations (sharing it would put this
// translation unit's needs into the ray-queue kernels' register allocation).  Marks are word-wide atomic ORs, issued only where a
// plain load of the word shows the bit clear and the lane in front does not set the same bit: OR is order-independent, so the arrays
// are the same bits from run to run and for any cut of the rays into calls.
struct MarkGrid { int res[3]; float lo[3], scale[3]; float weight_threshold, seen_eps; };

__device__ __forceinline__ void mark_bit(uint32_t* bits, int idx, bool mark, int lane) {
    // the lane in front often sits in the same cell (adjacent samples of one ray): one of the two is enough
    const int idx_up = __shfl_up(mark ? idx : -1, 1, 64);
    if (mark && !(lane > 0 && idx_up == idx)) {
        uint32_t* word = bits + (idx >> 5);
        const uint32_t bit = 1u << (idx & 31);
        if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0u) atomicOr(word, bit);       // (read where the atomics land)
    }
}

template <bool CAMERA>
__global__ void __launch_bounds__(kBlock) occupancy_mark_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, const Camera cam,
                                                                int64_t ray_begin, int64_t n_rays, int S, const float* __restrict__ z_vals,
                                                                const float* __restrict__ weights, const MarkGrid g, uint32_t* hit_bits,
                                                                uint32_t* seen_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        float o[3], d[3];
        if constexpr (CAMERA) {
            camera_ray(cam, ray_begin + r, o, d);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { o[k] = rays_o[r * 3 + k]; d[k] = rays_d[r * 3 + k]; }
        }
        float carry = 0.0f;                                  // sum of the weights of the earlier segments
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const bool valid = s < S;
            const int64_t i = r * S + (valid ? s : S - 1);
            const float w = valid ? weights[i] : 0.0f;
            const float z = z_vals[i];
            const float incl = wave_incl_sum(w, lane);
            float excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 0.0f;
            const float T = __fsub_rn(1.0f, __fadd_rn(carry, excl));           // a NaN in the prefix: no later sample is seen
            carry = __fadd_rn(carry, __shfl(incl, 63, 64));
            float t[3];
            bool inside = valid;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                t[k] = __fmul_rn(__fsub_rn(point_on_ray(o[k], d[k], z), g.lo[k]), g.scale[k]);
                inside = inside && t[k] >= 0.0f && t[k] < (float)g.res[k];      // (a NaN or an infinity fails one of the comparisons)
            }
            const int idx = inside ? ((int)floorf(t[2]) * g.res[1] + (int)floorf(t[1])) * g.res[0] + (int)floorf(t[0]) : 0;   // < 512^3 = 2^27
            if (hit_bits) mark_bit(hit_bits, idx, inside && !(w <= g.weight_threshold), lane);
            if (seen_bits) mark_bit(seen_bits, idx, inside && T > g.seen_eps, lane);
        }
    }
}

// ---- compaction in front of a training step under a grid (nerfhip.h: nrf_occupancy_compact_rays) ----------------------------------
// Chooses the samples of a ray batch that lie in occupied cells and leaves their points, directions and flat ids as dense rows, in
// ascending order of the flat id r * S + s.  One WAVE per ray, LANE <-> sample, 64-sample segments front to back like the marker;
// three launches, none of which waits for another workgroup:
//   count : a ray's kept samples (ballot + popcount per segment) -> counts[r]; z_vals and (pixel mode) rays_d_out on the way
//   scan  : ONE workgroup turns counts[] into exclusive offsets in place, 1024 rays per round with a running carry, and leaves M
//   write : lane ranks (mbcnt of the segment's ballot) below the ray's offset -> index / slot / positions / directions
// Depths, rays and points are formed with sample_kernel's / get_rays_kernel's operations in their order (RaySample of train_impl.hpp
// does the same): z_vals, rays_d_out and positions are theirs to the bit.  The cell rule is that of fused_impl.hpp:occ_skips,
// restated here as the marker restates it.  Both passes evaluate the same pure function of (ray, depth, grid): the write pass reads
// the depths the count pass stored.  A row index is still checked against the capacity in front of every store.
struct CompactDev {
    const float* rays_o;        // (R,3), or NULL: pixel mode
    const float* rays_d;
    const int64_t* pixels;      // pixel mode: (R) ray ids of `cam`
    Camera cam;
    DepthLadder lad;
    int perturb;
    const float* t_rand;        // (R,S) or NULL: counter_uniform(seed, row, sample)
    const float* z_in;          // (R,S) explicit depths or NULL
    uint64_t seed;
    float* z_vals;              // out (R,S)
    float* rays_d_out;          // out (R,3) or NULL
    const uint32_t* bits;
    int res[3];
    float lo[3], scale[3];
    int outside;
};

__device__ __forceinline__ void compact_ray(const CompactDev& P, int64_t r, float (&o)[3], float (&d)[3]) {
    if (P.pixels) {
        camera_ray(P.cam, P.pixels[r], o, d);
        // (the origin is a load from the kernel arguments: left as one, the compiler merges it with the other branch's load into ONE
        // load through a selected pointer and parks the selection in scratch -- train_impl.hpp:RaySample::origin_dir)
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = uniform_f(o[k]);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { o[k] = P.rays_o[r * 3 + k]; d[k] = P.rays_d[r * 3 + k]; }
    }
}

// true: the sample at p is evaluated (occ_skips negated: an empty cell skips; outside the box `outside` decides, except that a
// non-finite position is always evaluated)
__device__ __forceinline__ bool compact_keeps(const CompactDev& P, const float (&p)[3]) {
    float t[3];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t[k] = __fmul_rn(__fsub_rn(p[k], P.lo[k]), P.scale[k]);
        inside = inside && t[k] >= 0.0f && t[k] < (float)P.res[k];              // (a NaN fails both comparisons)
    }
    if (!inside) {
        const float big = __builtin_huge_valf();
        return !(P.outside && fabsf(p[0]) < big && fabsf(p[1]) < big && fabsf(p[2]) < big);
    }
    const int idx = ((int)floorf(t[2]) * P.res[1] + (int)floorf(t[1])) * P.res[0] + (int)floorf(t[0]);       // < 512^3 = 2^27
    return ((P.bits[idx >> 5] >> (idx & 31)) & 1u) != 0u;
}

__global__ void __launch_bounds__(kBlock) occupancy_compact_count_kernel(const CompactDev P, int64_t n_rays, int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int S = P.lad.S;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        float o[3], d[3];
        compact_ray(P, r, o, d);
        if (P.rays_d_out && lane < 3) P.rays_d_out[r * 3 + lane] = lane == 0 ? d[0] : (lane == 1 ? d[1] : d[2]);
        int count = 0;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const bool valid = s < S;
            bool keep = false;
            if (valid) {
                const int64_t i = r * S + s;
                float z;
                if (P.z_in) {
                    z = P.z_in[i];
                } else if (!P.perturb) {
                    z = ladder_z(P.lad, s);
                } else {
                    const float u = P.t_rand ? P.t_rand[i] : counter_uniform(P.seed, (uint64_t)r, (uint32_t)s);
                    z = ladder_z_jitter(P.lad, s, u);
                }
                P.z_vals[i] = z;
                const float p[3] = {point_on_ray(o[0], d[0], z), point_on_ray(o[1], d[1], z), point_on_ray(o[2], d[2], z)};
                keep = compact_keeps(P, p);
            }
            count += __popcll(__ballot(keep));
        }
        if (lane == 0) counts[r] = count;
    }
}

// counts[0..n) -> exclusive prefix sums in place, total[0] = their sum.  One workgroup of 1024 threads; n_rays * S < 2^31 bounds every sum.
__global__ void __launch_bounds__(1024) occupancy_compact_scan_kernel(int32_t* __restrict__ counts, int64_t n, int64_t* __restrict__ total) {
    __shared__ int wave_sums[16];
    __shared__ int round_sum;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const int c = i < n ? counts[i] : 0;
        int incl = c;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const int u = __shfl_up(incl, k, 64);
            if (lane >= k) incl += u;
        }
        if (lane == 63) wave_sums[wv] = incl;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wv; ++w) before += wave_sums[w];
        if (i < n) counts[i] = carry + before + incl - c;
        if (threadIdx.x == 1023) round_sum = before + incl;
        __syncthreads();
        carry += round_sum;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ void __launch_bounds__(kBlock) occupancy_compact_write_kernel(const CompactDev P, int64_t n_rays, const int32_t* __restrict__ offsets,
                                                                         int64_t capacity, int32_t* __restrict__ index, int32_t* __restrict__ slot,
                                                                         float* __restrict__ positions, float* __restrict__ directions) {
    const int lane = threadIdx.x & 63;
    const int S = P.lad.S;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        float o[3], d[3];
        compact_ray(P, r, o, d);
        int64_t base = offsets[r];
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            const bool valid = s < S;
            const int64_t i = r * S + s;
            bool keep = false;
            float p[3] = {0.0f, 0.0f, 0.0f};
            if (valid) {
                const float z = P.z_vals[i];
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = point_on_ray(o[k], d[k], z);
                keep = compact_keeps(P, p);
            }
            const unsigned long long m = __ballot(keep);
            const int64_t j = base + (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const bool store = keep && j < capacity;
            if (valid) slot[i] = store ? (int32_t)j : -1;
            if (store) {
                index[j] = (int32_t)i;
#pragma unroll
                for (int k = 0; k < 3; ++k) positions[j * 3 + k] = p[k];
                if (directions) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) directions[j * 3 + k] = d[k];
                }
            }
            base += __popcll(m);
        }
    }
}

}  // namespace

int64_t occupancy_compact_ws_bytes(int64_t n_rays) { return ((n_rays < 1 ? 1 : n_rays) * 4 + 15) / 16 * 16; }

int launch_occupancy_compact(const TrainRaysDev& r, int64_t n_rays, const OccDev& g, int64_t capacity, int32_t* index, int32_t* slot,
                             float* positions, float* directions, int64_t* count, void* workspace, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    CompactDev P{};
    P.rays_o = r.rays_o; P.rays_d = r.rays_d; P.pixels = r.pixels; P.cam = r.cam; P.lad = r.lad; P.perturb = r.perturb; P.t_rand = r.t_rand;
    P.z_in = r.z_in; P.seed = r.seed; P.z_vals = r.z_vals; P.rays_d_out = r.rays_d_out;
    P.bits = g.bits; P.outside = g.outside;
    for (int k = 0; k < 3; ++k) { P.res[k] = g.res[k]; P.lo[k] = g.lo[k]; P.scale[k] = g.scale[k]; }
    int32_t* counts = static_cast<int32_t*>(workspace);
    const dim3 grid(grid_for(n_rays * 64, kBlock, 16384)), block(kBlock);
    hipLaunchKernelGGL(occupancy_compact_count_kernel, grid, block, 0, s, P, n_rays, counts);
    hipLaunchKernelGGL(occupancy_compact_scan_kernel, dim3(1), dim3(1024), 0, s, counts, n_rays, count);
    hipLaunchKernelGGL(occupancy_compact_write_kernel, grid, block, 0, s, P, n_rays, counts, capacity, index, slot, positions, directions);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_occupancy_mark(const float* rays_o, const float* rays_d, const Camera* cam, int64_t ray_begin, int64_t n_rays, int S, const float* z_vals,
                          const float* weights, const int res[3], const float lo[3], const float scale[3], float weight_threshold, float seen_eps,
                          uint32_t* hit_bits, uint32_t* seen_bits, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    MarkGrid g;
    for (int k = 0; k < 3; ++k) { g.res[k] = res[k]; g.lo[k] = lo[k]; g.scale[k] = scale[k]; }
    g.weight_threshold = weight_threshold; g.seen_eps = seen_eps;
    const dim3 grid(grid_for(n_rays * 64, kBlock, 16384)), block(kBlock);
    if (cam)
        hipLaunchKernelGGL(occupancy_mark_kernel<true>, grid, block, 0, s, nullptr, nullptr, *cam, ray_begin, n_rays, S, z_vals, weights, g, hit_bits,
                           seen_bits);
    else
        hipLaunchKernelGGL(occupancy_mark_kernel<false>, grid, block, 0, s, rays_o, rays_d, Camera{}, (int64_t)0, n_rays, S, z_vals, weights, g, hit_bits,
                           seen_bits);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_occupancy_pack(const float* density, int64_t n_cells, int k, float threshold, uint32_t* bits, hipStream_t s) {
    if (n_cells <= 0) return NRF_OK;
    hipLaunchKernelGGL(occupancy_pack_kernel, dim3(grid_for(n_cells, kBlock, 8192)), dim3(kBlock), 0, s, density, n_cells, k, threshold, bits);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_occupancy_dilate(const uint32_t* bits_in, const int res[3], uint32_t* bits_out, hipStream_t s) {
    const int wx = res[0] / 32;
    hipLaunchKernelGGL(occupancy_dilate_kernel, dim3(grid_for((int64_t)wx * res[1] * res[2], kBlock, 8192)), dim3(kBlock), 0, s, bits_in, wx, res[1],
                       res[2], bits_out);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_get_rays(const Camera& cam, int64_t ray_begin, int64_t n, float* rays_o, float* rays_d, hipStream_t s) {
    if (n <= 0) return NRF_OK;
    hipLaunchKernelGGL(get_rays_kernel, dim3(grid_for(n, kBlock, 4096)), dim3(kBlock), 0, s, cam, ray_begin, n, rays_o, rays_d);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_sample(const float* rays_o, const float* rays_d, int64_t n_rays, float near, float far, int S, int lindisp, int perturb,
                  const float* t_rand, const float* z_ladder, uint64_t seed, float* pts, float* z_vals, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    const DepthLadder lad = make_ladder(near, far, S, lindisp, z_ladder);
    hipLaunchKernelGGL(sample_kernel, dim3(grid_for(n_rays * S, kBlock, 8192)), dim3(kBlock), 0, s, rays_o, rays_d, n_rays, lad, perturb,
                       t_rand, seed, pts, z_vals);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_encode(const float* x, int64_t n, int dim, int L, int include_input, const float* freq_bands, float* out, hipStream_t s) {
    if (n <= 0) return NRF_OK;
    const int64_t total = n * dim * (2 * L + (include_input ? 1 : 0));
    hipLaunchKernelGGL(encode_kernel, dim3(grid_for(total, kBlock, 8192)), dim3(kBlock), 0, s, x, n, dim, L, include_input, freq_bands, out);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_composite(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                     int64_t n_rays, int S, int white_bkgd, float* out_rgb, float* out_depth, float* out_w, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    hipLaunchKernelGGL(composite_kernel, dim3(grid_for(n_rays * 64, kBlock, 16384)), dim3(kBlock), 0, s, rgb, rgb_stride, sigma, sigma_stride, z,
                       rays_d, n_rays, S, white_bkgd, out_rgb, out_depth, out_w);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

// composite_backward_kernel with the geometric terms (composite_backward_ray<false, true>): a kernel of its own, so that the one
// above stays what it is
__global__ void __launch_bounds__(kBlock) composite_backward_geom_kernel(const float* __restrict__ rgb, int rgb_stride, const float* __restrict__ sigma,
                                                                         int sigma_stride, const float* __restrict__ z,
                                                                         const float* __restrict__ rays_d, int64_t n_rays, int S, int white_bkgd,
                                                                         const float* __restrict__ g_rgb, const float* __restrict__ g_depth,
                                                                         const float* __restrict__ g_w, float* __restrict__ d_rgb,
                                                                         int d_rgb_stride, float* __restrict__ d_sigma, int d_sigma_stride,
                                                                         float* __restrict__ d_z, float* __restrict__ d_rays_d) {
    __shared__ float seg_T[kBlock / 64][kMaxSegments];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        const float gr = g_rgb ? g_rgb[r * 3] : 0.0f, gg = g_rgb ? g_rgb[r * 3 + 1] : 0.0f, gb = g_rgb ? g_rgb[r * 3 + 2] : 0.0f;
        const float gd = g_depth ? g_depth[r] : 0.0f;
        composite_backward_ray<false, true>(rgb, rgb_stride, sigma, sigma_stride, z, rays_d, r, S, lane, white_bkgd, gr, gg, gb, gd, g_w, d_rgb,
                                            d_rgb_stride, d_sigma, d_sigma_stride, seg_T[wv], NoiseSrc{}, 0.0f, d_z, d_rays_d);
    }
}

// Adjoint of point_on_ray (p = o + d z) and of the expansion of a ray's direction over its samples.  One WAVE per ray, LANE <->
// sample, 64-sample segments, wave_sum in a fixed order, no atomics:
//   d_rays_o = sum_s d_p,   d_rays_d = sum_s (z_s d_p + d_dirs) + d_rays_d_in,   d_z_out[s] = d . d_p_s + d_z_in[s]
// HBM-bound: 16 (+ 12 + 4) B read and 4 B written per ray-sample.
__global__ void __launch_bounds__(kBlock) ray_grad_kernel(const float* __restrict__ d_points, const float* __restrict__ d_dirs,
                                                          const float* __restrict__ z, const float* __restrict__ rays_d,
                                                          const float* __restrict__ d_z_in, const float* __restrict__ d_rays_d_in,
                                                          int64_t n_rays, int S, float* __restrict__ d_rays_o, float* __restrict__ d_rays_d,
                                                          float* __restrict__ d_z_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (blockIdx.x * (int64_t)kBlock + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * kBlock) >> 6;
    for (int64_t r = wave0; r < n_rays; r += n_waves) {
        const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
        float so[3] = {0.0f, 0.0f, 0.0f}, sd[3] = {0.0f, 0.0f, 0.0f};
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int s = s0 + lane;
            if (s < S) {
                const int64_t i = r * S + s;
                const float zc = z[i];
                float dot = 0.0f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float dp = d_points[i * 3 + k];
                    so[k] = __fadd_rn(so[k], dp);
                    float t = __fmul_rn(zc, dp);
                    if (d_dirs) t = __fadd_rn(t, d_dirs[i * 3 + k]);
                    sd[k] = __fadd_rn(sd[k], t);
                    dot = __fadd_rn(dot, __fmul_rn(d[k], dp));
                }
                if (d_z_out) d_z_out[i] = d_z_in ? __fadd_rn(dot, d_z_in[i]) : dot;
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { so[k] = wave_sum(so[k]); sd[k] = wave_sum(sd[k]); }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (d_rays_o) d_rays_o[r * 3 + k] = so[k];
                if (d_rays_d) d_rays_d[r * 3 + k] = d_rays_d_in ? __fadd_rn(sd[k], d_rays_d_in[r * 3 + k]) : sd[k];
            }
        }
    }
}

int launch_composite_backward_geom(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                                   int64_t n_rays, int S, int white_bkgd, const float* g_rgb, const float* g_depth, const float* g_w,
                                   float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* d_z, float* d_rays_d, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    if (S > 64 * kMaxSegments) return NRF_EINVAL;
    hipLaunchKernelGGL(composite_backward_geom_kernel, dim3(grid_for(n_rays * 64, kBlock, 16384)), dim3(kBlock), 0, s, rgb, rgb_stride, sigma,
                       sigma_stride, z, rays_d, n_rays, S, white_bkgd, g_rgb, g_depth, g_w, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, d_z,
                       d_rays_d);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_ray_grad(const float* d_points, const float* d_dirs, const float* z, const float* rays_d, const float* d_z_in, const float* d_rays_d_in,
                    int64_t n_rays, int S, float* d_rays_o, float* d_rays_d, float* d_z_out, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    hipLaunchKernelGGL(ray_grad_kernel, dim3(grid_for(n_rays * 64, kBlock, 16384)), dim3(kBlock), 0, s, d_points, d_dirs, z, rays_d, d_z_in,
                       d_rays_d_in, n_rays, S, d_rays_o, d_rays_d, d_z_out);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_composite_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                              int64_t n_rays, int S, int white_bkgd, const float* g_rgb, const float* g_depth, const float* g_w,
                              float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    if (S > 64 * kMaxSegments) return NRF_EINVAL;
    hipLaunchKernelGGL(composite_backward_kernel, dim3(grid_for(n_rays * 64, kBlock, 16384)), dim3(kBlock), 0, s, rgb, rgb_stride, sigma,
                       sigma_stride, z, rays_d, n_rays, S, white_bkgd, g_rgb, g_depth, g_w, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

// loss = w * mean((pred - target)^2) and d loss / d pred in one launch (train.py:36-44: rgb_weight * nn.MSELoss()).
// One block: the reference's ray batches are a few thousand values; fixed summation order.
__global__ void __launch_bounds__(1024) mse_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target, int n, float weight,
                                                        float* __restrict__ g_pred, float* __restrict__ loss) {
    __shared__ float part[16];
    const float scale = 2.0f * weight / (float)n;
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float d = pred[i] - target[i];
        g_pred[i] = scale * d;
        s += d * d;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int k = 0; k < 16; ++k) t += part[k];
        *loss = weight * t / (float)n;
    }
}

int launch_composite_mse_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                                  int64_t n_rays, int S, int white_bkgd, const float* target, float weight, float* pred, float* d_rgb,
                                  int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_loss, float* zero_buf,
                                  int64_t zero_n, hipStream_t s) {
    if (n_rays <= 0 || S > 64 * kMaxSegments) return NRF_EINVAL;
    const int64_t work = std::max(n_rays * 64, (zero_n + 3) / 4);
    hipLaunchKernelGGL(composite_loss_backward_kernel<false>, dim3(grid_for(work, kBlock, 16384)), dim3(kBlock), 0, s, rgb, rgb_stride, sigma,
                       sigma_stride, z, rays_d, n_rays, S, white_bkgd, target, weight, pred, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_loss,
                       zero_buf, zero_n, LossExt{});
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_composite_loss_backward(const LossLaunch& a) {
    if (a.n_rays <= 0 || a.S > 64 * kMaxSegments) return NRF_EINVAL;
    const LossExt ext = loss_ext_of(a.lt, a.n_rays, a.S);
    const int64_t work = std::max(a.n_rays * 64, (a.zero_n + 3) / 4);
    if (a.slot)
        hipLaunchKernelGGL(indexed_loss_backward_kernel, dim3(grid_for(work, kBlock, 16384)), dim3(kBlock), 0, a.s, a.rgb, a.rgb_stride, a.sigma,
                           a.sigma_stride, a.z, a.rays_d, a.n_rays, a.S, a.white_bkgd, a.target, a.lt.rgb_weight, a.pred, a.d_rgb, a.d_rgb_stride,
                           a.d_sigma, a.d_sigma_stride, a.ray_terms, a.zero_buf, a.zero_n, ext, a.slot);
    else
        hipLaunchKernelGGL(composite_loss_backward_kernel<true>, dim3(grid_for(work, kBlock, 16384)), dim3(kBlock), 0, a.s, a.rgb, a.rgb_stride,
                           a.sigma, a.sigma_stride, a.z, a.rays_d, a.n_rays, a.S, a.white_bkgd, a.target, a.lt.rgb_weight, a.pred, a.d_rgb,
                           a.d_rgb_stride, a.d_sigma, a.d_sigma_stride, a.ray_terms, a.zero_buf, a.zero_n, ext);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_mse_grad(const float* pred, const float* target, int64_t n, float weight, float* g_pred, float* loss, hipStream_t s) {
    if (n <= 0 || n > (1 << 22)) return NRF_EINVAL;
    hipLaunchKernelGGL(mse_grad_kernel, dim3(1), dim3(1024), 0, s, pred, target, (int)n, weight, g_pred, loss);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_sample_pdf(const float* z, const float* w, int64_t n_rays, int S, int Ni, const float* u, int64_t u_ray_stride, float* samples,
                      float* z_union, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    SamplePdfGrid g;
    if (!sample_pdf_grid(n_rays, S, Ni, g)) return NRF_EINVAL;
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)g.blocks), dim3(g.waves * 64), g.lds_bytes, s, z, w, n_rays, S, Ni, u, u_ray_stride,
                       samples, z_union);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_project_fetch(const DinoDev& d, const float* points, int64_t n, float* feats, float* xy, hipStream_t s) {
    if (n <= 0) return NRF_OK;
    hipLaunchKernelGGL(project_fetch_kernel, dim3(grid_for(n * d.C, kBlock, 8192)), dim3(kBlock), 0, s, d, points, n, feats, xy, 0);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_sample_features(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, float* feats, hipStream_t s) {
    if (n <= 0) return NRF_OK;
    DinoDev d{};
    d.features = features; d.Hp = Hp; d.Wp = Wp; d.C = C;
    hipLaunchKernelGGL(project_fetch_kernel, dim3(grid_for(n * C, kBlock, 8192)), dim3(kBlock), 0, s, d, points_2d, n, feats, (float*)nullptr, 1);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int64_t fetch_backward_ws_floats(int Hp, int Wp, int C, int64_t n) { return fetch_bwd_geo(Hp, Wp, C, n).slabs * (int64_t)Hp * Wp * C; }

int launch_project_fetch_backward(const DinoDev& d, const float* points, int64_t n, const float* d_feats, float* d_map, int accumulate, float* ws,
                                  hipStream_t s) {
    return fetch_backward_impl(d, points, 0, n, d_feats, d_map, accumulate, ws, s);
}

int launch_sample_features_backward(int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats, float* d_map, int accumulate,
                                    float* ws, hipStream_t s) {
    DinoDev d{};
    d.Hp = Hp; d.Wp = Wp; d.C = C;
    return fetch_backward_impl(d, points_2d, 1, n, d_feats, d_map, accumulate, ws, s);
}

int launch_project_fetch_backward_points(const DinoDev& d, const float* points, int64_t n, const float* d_feats, float* d_points, int accumulate,
                                         hipStream_t s) {
    return fetch_points_backward_impl(d, points, 0, n, d_feats, d_points, accumulate, s);
}

int launch_sample_features_backward_points(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats,
                                           float* d_xy, hipStream_t s) {
    DinoDev d{};
    d.features = features; d.Hp = Hp; d.Wp = Wp; d.C = C;
    return fetch_points_backward_impl(d, points_2d, 1, n, d_feats, d_xy, 0, s);
}

}  // namespace nrf
