/* nerfhip.h -- C ABI of libnerfhip.so, the MI355X (gfx950) renderer for the
 * ray-marching hot path of ANKITSANJYAL/nerf-few-shot-limitations.
 *
 * The reference has no FFI of its own (it is 100 % Python, SURVEY.md section
 * 8b): the "interface each entry point replaces" is therefore the Python
 * callable named next to it (paths relative to the reference root).  The
 * Python package nerf_few_shot_limitations_amd binds this header with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative NRF_E* code; the
 *     message is kept per thread and read with nrf_last_error();
 *   - no C++ exception crosses the boundary;
 *   - the CALLER owns every buffer (device pointers unless stated "host");
 *     the library owns only the packed weight copies inside a nrf_model;
 *   - all work is enqueued on the caller's stream (void* = hipStream_t,
 *     NULL = the default stream); nothing synchronises, nothing allocates on
 *     a render / staged call;
 *   - all tensors are contiguous fp32, row-major, in the reference's layouts;
 *     ray id r = y*W + x (row-major pixel order) is the integer contract.
 */
#ifndef NERFHIP_H
#define NERFHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRF_ABI_VERSION 5

/* error codes */
#define NRF_OK            0
#define NRF_EINVAL       -1   /* bad argument (shape, null pointer, unsupported size) */
#define NRF_EUNSUPPORTED -2   /* architecture / mode not built into this library */
#define NRF_EHIP         -3   /* a HIP runtime call failed */
#define NRF_ENOMEM       -4

/* network families on the path */
#define NRF_NET_V1 1  /* src/models/nerf_model.py:5-24  NeRFMLP(pos_dim=63,hidden,n_layers): PE(10) -> 8x(Linear+ReLU) -> sigma | sigmoid rgb */
#define NRF_NET_V2 2  /* src/models/nerf_mlp.py:41-84   PE(pos) -> DensityMLP -> ColorMLP(feature, PE(dir)): train.py:82-89 with use_dino=False */
#define NRF_NET_V3 3  /* src/models/nerf_mlp.py:86-158  NeRFWithDINO: + lora_dino.py:146-193 NeRFDINOFusion */

/* arithmetic of the MLP contraction (accumulation is always fp32) */
#define NRF_MMA_BF16 0  /* v_mfma_f32_32x32x16_bf16: weights + activations rounded to bf16 (8 mantissa bits: misses the 0.01 dB PSNR bar) */
#define NRF_MMA_F16  1  /* v_mfma_f32_32x32x16_f16 : same rate, 3 more mantissa bits: the throughput mode whose PSNR stays within 0.01 dB of
                           the fp32 render (bench.py's default).  f16-typed weight streams (this mode and NRF_MMA_F16X3) saturate at
                           +-65504 instead of overflowing to inf                                                                     */
#define NRF_MMA_F32  2  /* v_mfma_f32_32x32x2_f32  : exact fp32 fma chain (parity mode, 1/16 rate)           */
#define NRF_MMA_F16X3 3 /* split f16: x = hi + lo (22 bits), W_hi X_hi + W_hi X_lo + W_lo X_hi as three 32x32x16 MFMAs: fp32-class
                           results (meets the 1e-4 bar of the fp32 mode) at up to 1/3 of the 16-bit rate.  Inference entry
                           points only (render / mlp_forward); operands must lie within the f16 range (|x| <= 65504)       */

typedef struct nrf_model nrf_model;

typedef struct nrf_arch {
    int32_t net;        /* NRF_NET_* */
    int32_t pos_freq;   /* L of the position encoding (10 -> 63 features, 12 -> 75) */
    int32_t dir_freq;   /* L of the direction encoding (V2/V3; 4 -> 27 features)   */
    int32_t hidden;     /* hidden width (256)                                       */
    int32_t n_layers;   /* number of Linear+ReLU layers of the trunk (8)            */
    int32_t dino_dim;   /* feature-map channels (V3; 64)                            */
} nrf_arch;

/* One nn.Linear, HOST pointers, weight (out_f,in_f) row-major and bias (out_f),
 * in the order of the module's state_dict:
 *   V1: layers.0 .. layers.{n-1}, sigma_out, rgb_out                        (nerf_model.py:8-14)
 *   V2: density_mlp.density_layers.{0,2,..}, density_head, feature_head,
 *       color_mlp.color_layers.{0,2,4}                                      (nerf_mlp.py:46-57,72-79)
 *   V3: dino_fusion.fusion.{0,2}, dino_fusion.attention.{0,2},
 *       dino_fusion.output_proj, then the V2 list                           (lora_dino.py:153-169) */
typedef struct nrf_linear {
    const float* weight;
    const float* bias;
    int32_t out_f;
    int32_t in_f;
} nrf_linear;

/* DINO side channel of V3 (train.py:203-214): the feature map of ONE source
 * view, its camera and intrinsics. */
typedef struct nrf_dino {
    const float* features;   /* device, (1,Hp,Wp,C) fp32, channel-last (dino_feature_model.py:114-148) */
    int32_t Hp, Wp, C;
    float   inv_pose[16];    /* inverse of the source view's 4x4 camera-to-world, row-major (ray_utils.py:191) */
    float   focal;
    int32_t H, W;            /* image size the projection normalises by (ray_utils.py:199-204) */
} nrf_dino;

typedef struct nrf_render_opts {
    float    near, far;      /* train.py:192-193                                                      */
    int32_t  n_samples;      /* S                                                                     */
    int32_t  lindisp;        /* ray_utils.py:59-62                                                    */
    int32_t  perturb;        /* 1: stratified jitter (ray_utils.py:71-79)                             */
    const float* t_rand;     /* device (R,S) U[0,1) jitter, or NULL -> in-kernel counter RNG(rng_seed) */
    const float* z_ladder;   /* device (S) un-jittered depths z_0..z_{S-1}, or NULL -> computed in-kernel from near/far
                                (scalar torch.linspace formula).  torch's CPU linspace is vectorised and its last ulp
                                depends on the host: a caller that must match the reference bit for bit passes the
                                ladder the reference computes (ray_utils.py:58-66) */
    const float* z_in;       /* device (R,S) explicit, ascending per-ray depths (e.g. the sorted union of the coarse and the
                                importance samples, ray_utils.py:136-139): overrides near/far/perturb/lindisp sampling */
    uint64_t rng_seed;
    float    ert_eps;        /* early ray termination: stop a wave once every live ray has T < eps; 0 = off (reference behaviour) */
    int32_t  white_bkgd;     /* nerf_mlp.py:209-212                                                   */
    int32_t  mma_mode;       /* NRF_MMA_*                                                             */
    const nrf_dino* dino;    /* V3 only (host struct, copied at launch)                               */
    int32_t  out_rgbd;       /* 1: `rgb` points at (R,4) rows [r,g,b,depth] written with one 16-byte store per ray and `depth` is ignored
                                (may be NULL) -- the layout of the multi-GPU gather buffer; `rgb` must be 16-byte aligned, a
                                misaligned pointer is refused with NRF_EINVAL; 0: (R,3) + (R) */
} nrf_render_opts;

/* ---- model handle -------------------------------------------------------- */

/* Build the device-side packed weight streams (all NRF_MMA_* modes) for
 * `arch` from `n_linear` host Linear layers.  Replaces: module construction +
 * .to(device), train.py:82-89 / nerf_model.py:6-14. */
int nrf_model_create(nrf_model** out, int device, const nrf_arch* arch,
                     const nrf_linear* linears, int n_linear);
/* Re-pack after the weights changed (optimizer.step / load_state_dict). */
int nrf_model_update(nrf_model* m, const nrf_linear* linears, int n_linear, void* stream);
void nrf_model_destroy(nrf_model* m);
/* 2*MAC of the Linear layers per ray-sample. */
int64_t nrf_model_flops_per_sample(const nrf_model* m);

/* ---- the fused path -------------------------------------------------------- */

/* sample -> encode -> MLP -> composite for explicit rays.
 * Replaces NeRFDINOTrainer.render_rays, train.py:188-242.
 * rays_o, rays_d: (R,3).  Outputs: rgb (R,3), depth (R); weights (R,S) and
 * z_vals (R,S) may be NULL. */
int nrf_render_rays(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays,
                    const nrf_render_opts* opts,
                    float* rgb, float* depth, float* weights, float* z_vals, void* stream);

/* Same, with the rays generated in-kernel from a pinhole camera
 * (ray_sampler.py:4-30) for the ray-id range [ray_begin, ray_end) of an HxW
 * image; output row i holds ray ray_begin+i.  c2w = first 3 rows of the pose,
 * row-major, host.  Replaces get_rays + the eval chunk loop, train.py:305-319 /
 * evaluate.py:65-81. */
int nrf_render_camera(const nrf_model* m, int H, int W, float focal, const float c2w[12],
                      int64_t ray_begin, int64_t ray_end, const nrf_render_opts* opts,
                      float* rgb, float* depth, float* weights, float* z_vals, void* stream);

/* Pixel-tile sharded, multi-view form (no reference counterpart; the batch
 * of views is the reference's loop over test views, train.py:304).  The image's rays are cut into
 * tiles of tile_rays consecutive ray ids; ONE launch renders, for each of the n_cams (<= 8) poses
 * c2w[c*12 .. c*12+11] of the same HxW/focal sensor, tiles first_tile, first_tile+tile_step, ...
 * (n_tiles of them, e.g. first_tile=rank, tile_step=world).  Output row
 * (c*n_tiles + k)*tile_rays + j holds ray (first_tile + k*tile_step)*tile_rays + j of view c; rows
 * whose ray id falls beyond H*W repeat the last ray (padding, so every rank's buffer has the same
 * shape for the gather).  Per-ray arithmetic is identical to nrf_render_camera: shards reassemble
 * bit-exactly. */
int nrf_render_cameras_tiles(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams,
                             int64_t tile_rays, int64_t first_tile, int64_t tile_step, int64_t n_tiles,
                             const nrf_render_opts* opts,
                             float* rgb, float* depth, float* weights, float* z_vals, void* stream);

/* ---- tail mode: a 16-bit render whose last sample is evaluated in split-f16 -------------
 *
 * The reference composites a ray's last sample with dists[-1] = 1e10 (nerf_mlp.py:182): its
 * opacity is 1 if sigma_last > 0 and 0 otherwise, so on a ray whose last density is ~ 0 any
 * rounding of the network flips a weight of size T_last.  That one rule is the source of every
 * large single-pixel error of NRF_MMA_BF16 / NRF_MMA_F16.  The *_tail entry points march samples
 * 0 .. S-2 exactly as the plain call in opts->mma_mode (bf16 or f16) does -- weights[:, :S-1] and
 * z_vals are its bits -- and evaluate sample S-1 (encoding, network, sigmoid / exp of the
 * compositor step) with the arithmetic of NRF_MMA_F16X3, then run the plain epilogue.  With
 * n_samples == 1 the result is the NRF_MMA_F16X3 render's, bit for bit.
 *
 * Two launches on the caller's stream (one when n_samples == 1); between them the six compositor
 * floats of every ray (T, r, g, b, depth, acc) rest in the caller's `workspace`.  The library
 * still allocates nothing.  A tail render READS TWO WEIGHT STREAMS of the model: the one of
 * opts->mma_mode and the one of NRF_MMA_F16X3 -- after nrf_model_update_device both bits must
 * have been in a mode_mask since the parameters last changed.
 *
 * Refused with NRF_EINVAL: tail == NULL, a tail mode other than NRF_MMA_F16X3, a base mode other
 * than NRF_MMA_BF16 / NRF_MMA_F16, a workspace that is NULL, smaller than nrf_render_tail_bytes
 * or not 16-byte aligned, and ert_eps > 0: the ray-queue kernel is deliberately not part of this
 * mode (a ray that terminated early has, by construction, a tail worth less than eps). */
typedef struct nrf_tail {
    int32_t mode;             /* arithmetic of the last sample: NRF_MMA_F16X3 */
    void*   workspace;        /* device, 16-byte aligned, written and read by the call */
    int64_t workspace_bytes;  /* >= nrf_render_tail_bytes of the call's ray count */
} nrf_tail;

/* Bytes of workspace a tail render of n_rays rays needs (24 per ray, rounded up to 16); -1 if n_rays < 0.
 * For nrf_render_cameras_tiles_tail n_rays = n_cams * n_tiles * tile_rays. */
int64_t nrf_render_tail_bytes(int64_t n_rays);

/* nrf_render_rays / nrf_render_camera / nrf_render_cameras_tiles with a tail: same arguments, same outputs. */
int nrf_render_rays_tail(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays,
                         const nrf_render_opts* opts, const nrf_tail* tail,
                         float* rgb, float* depth, float* weights, float* z_vals, void* stream);
int nrf_render_camera_tail(const nrf_model* m, int H, int W, float focal, const float c2w[12],
                           int64_t ray_begin, int64_t ray_end, const nrf_render_opts* opts, const nrf_tail* tail,
                           float* rgb, float* depth, float* weights, float* z_vals, void* stream);
int nrf_render_cameras_tiles_tail(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams,
                                  int64_t tile_rays, int64_t first_tile, int64_t tile_step, int64_t n_tiles,
                                  const nrf_render_opts* opts, const nrf_tail* tail,
                                  float* rgb, float* depth, float* weights, float* z_vals, void* stream);

/* ---- empty-space skipping: an occupancy bit grid over the scene's box ----------------------
 *
 * The *_occ entry points render on the ray-queue kernel (the one behind ert_eps > 0) and let a
 * column step over every sample whose cell of the grid is empty.  A skipped sample is composited
 * as if the network had returned density 0: alpha = 0, weight 0, T unchanged, +0 on the colour,
 * depth and acc sums -- so the result is, bit for bit, the plain render in which the density of
 * every sample in an empty cell is replaced by 0, and with an all-ones grid the plain render.  A
 * ray none of whose samples lies in an occupied cell costs no network pass.
 *
 * The cell of a sample at position p (the position the network is given), in fp32 with a rounding
 * after every operation:  t_k = (p_k - lo_k) * scale_k;  inside iff 0 <= t_k < res_k for all k (a
 * NaN is not inside);  i_k = (int)floor(t_k).  A sample that is not inside follows `outside`,
 * except that a non-finite position is always evaluated.
 *
 * ert_eps >= 0 (0: skipping alone; > 0: skipping and early termination); everything else of opts
 * keeps its meaning; weights / z_vals of a skipped sample are 0 and its depth.  Not combined with
 * the *_tail family.  Refused with NRF_EINVAL before any launch: occ == NULL, a wrong
 * struct_bytes, `outside` not 0 or 1, bits NULL or not 4-byte aligned, a res outside 1..512 or a
 * res[0] that is no multiple of 32, a non-finite lo, a scale that is not finite and > 0, and
 * 2^31 or more rays. */
typedef struct nrf_occupancy {
    int32_t  struct_bytes;   /* sizeof(nrf_occupancy), checked */
    int32_t  outside;        /* sample outside the box: 0 = evaluate it (default), 1 = skip it */
    const uint32_t* bits;    /* device, 4-byte aligned; bit index ((iz*res[1] + iy)*res[0] + ix), word = index >> 5, bit = index & 31; 1 = occupied */
    int32_t  res[3];         /* cells along x, y, z: each 1..512, res[0] a multiple of 32 */
    float    lo[3];          /* lower corner of the box */
    float    scale[3];       /* cells per unit length, computed by the caller: res[k] / (hi[k] - lo[k]); finite, > 0 */
    unsigned long long* stats; /* optional device [2], the call ADDS to it: [0] network-evaluated (ray, sample) pairs,
                                  [1] MLP passes run by a wave that held at least one live ray: [0] / ([1] * columns per wave)
                                  (64 in the 16-bit modes, 32 otherwise) is the column utilisation */
} nrf_occupancy;

/* nrf_render_rays / nrf_render_camera / nrf_render_cameras_tiles with a grid: same arguments, same outputs. */
int nrf_render_rays_occ(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays,
                        const nrf_render_opts* opts, const nrf_occupancy* occ,
                        float* rgb, float* depth, float* weights, float* z_vals, void* stream);
int nrf_render_camera_occ(const nrf_model* m, int H, int W, float focal, const float c2w[12],
                          int64_t ray_begin, int64_t ray_end, const nrf_render_opts* opts, const nrf_occupancy* occ,
                          float* rgb, float* depth, float* weights, float* z_vals, void* stream);
int nrf_render_cameras_tiles_occ(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams,
                                 int64_t tile_rays, int64_t first_tile, int64_t tile_step, int64_t n_tiles,
                                 const nrf_render_opts* opts, const nrf_occupancy* occ,
                                 float* rgb, float* depth, float* weights, float* z_vals, void* stream);

/* Building a grid.  Cell c of n_cells (a multiple of 32) is occupied iff the maximum of its k consecutive
 * densities density[c*k .. c*k + k-1] is > threshold; a NaN density makes the cell occupied.  bits: n_cells / 32 words. */
int nrf_occupancy_pack(const float* density, int64_t n_cells, int k, float threshold, uint32_t* bits, void* stream);
/* bits_out (res[0]*res[1]*res[2] / 32 words, not bits_in) = bits_in with every cell occupied whose 3x3x3 neighbourhood
 * holds an occupied cell; cells beyond the box count as empty.  res as in nrf_occupancy. */
int nrf_occupancy_dilate(const uint32_t* bits_in, const int32_t res[3], uint32_t* bits_out, void* stream);

/* Marking a grid from what the renderer itself produced: weights (R,S) and z_vals (R,S) of a batch of rays, as the render entry
 * points write them, and the rays -- explicit (R,3) origins and directions, or rays [ray_begin, ray_end) of a pinhole camera,
 * generated exactly as nrf_render_camera generates them.  hit_bits / seen_bits are two bit arrays in the layout of
 * nrf_occupancy.bits (res[0]*res[1]*res[2] / 32 words, device, 4-byte aligned); the call ORs into them, the caller zeroes them
 * first; either may be NULL, not both.  Per sample i of a ray (origin o, direction d):
 *   position  p = o + d * z_i (one rounded product, one rounded sum per axis: the renderer's own points);
 *   cell      t = (p - lo) * scale per axis, each one rounded fp32 operation; the sample is inside iff 0 <= t < res on every axis,
 *             its cell index is (floor(t_z)*res[1] + floor(t_y))*res[0] + floor(t_x): the rule the *_occ entry points skip by;
 *             a sample outside the box or at a non-finite position marks nothing;
 *   hit       bit set iff !(w_i <= weight_threshold): a NaN weight marks, as a NaN density does in nrf_occupancy_pack;
 *   seen      bit set iff 1 - sum_{j<i} w_j > seen_eps, the sum in fp32 over the ray's earlier samples (the order of the additions is
 *             not specified); a NaN in that sum makes every later sample of the ray unseen.
 * OR is order-independent: the arrays are the same bits from run to run and for every cut of the rays into calls.
 * res, lo, scale as in nrf_occupancy; n_samples >= 1; fewer than 2^31 rays; weight_threshold finite and >= 0; seen_eps in [0,1).
 * n_rays == 0 is NRF_OK.  Runs on the current device. */
int nrf_occupancy_mark_rays(const float* rays_o, const float* rays_d, int64_t n_rays, int n_samples,
                            const float* z_vals, const float* weights,
                            const int32_t res[3], const float lo[3], const float scale[3],
                            float weight_threshold, float seen_eps,
                            uint32_t* hit_bits, uint32_t* seen_bits, void* stream);
int nrf_occupancy_mark_camera(int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                              int n_samples, const float* z_vals, const float* weights,
                              const int32_t res[3], const float lo[3], const float scale[3],
                              float weight_threshold, float seen_eps,
                              uint32_t* hit_bits, uint32_t* seen_bits, void* stream);

/* ---- staged entry points (one reference leaf each; used by the drop-in
 *      Python surface and by the stage-wise parity tests) ------------------- */

/* ray_sampler.py:4-30 == ray_utils.py:4-37.  Rays [ray_begin,ray_end) -> (n,3),(n,3). */
int nrf_get_rays(int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                 float* rays_o, float* rays_d, void* stream);
/* ray_utils.py:39-84 == ray_sampler.py:32-61.  pts (R,S,3) and/or z_vals (R,S) (either may be NULL). */
int nrf_sample_along_rays(const float* rays_o, const float* rays_d, int64_t n_rays,
                          float near, float far, int n_samples, int lindisp, int perturb,
                          const float* t_rand, const float* z_ladder, uint64_t rng_seed,
                          float* pts, float* z_vals, void* stream);
/* positional_encoding.py:20-33 == nerf_mlp.py:17-33.  x (n,dim) -> out (n, dim*(2L+include_input)).
 * freq_bands: NULL = 2^k, k = 0..L-1 (log_sampling=True, every caller of the reference), or a device table of L
 * frequencies (log_sampling=False, positional_encoding.py:18: torch.linspace(1, 2^(L-1), L) as the caller computed it). */
int nrf_encode(const float* x, int64_t n, int dim, int num_freqs, int include_input, const float* freq_bands, float* out, void* stream);
/* V1: nerf_model.py:16-24, x_enc (P, 3*(2*pos_freq+1)) -> out4 (P,4) = [rgb, sigma]. */
int nrf_mlp_forward_v1(const nrf_model* m, int mma_mode, const float* x_enc, int64_t n, float* out4, void* stream);
/* V2/V3: NeRFMLP.forward(positions, directions, dino_features), train.py:229 / nerf_mlp.py:134-158:
 * positions (P,3), directions (P,3), dino (P,dino_dim) or NULL (V2) -> rgb (P,3), density (P,1). */
int nrf_mlp_forward(const nrf_model* m, int mma_mode, const float* positions, const float* directions,
                    const float* dino, int64_t n, float* rgb, float* density, void* stream);
/* nerf_mlp.py:165-215 (VolumeRenderer.forward, eval path) and volume_renderer.py:4-43:
 * rgb (R,S,*) with element stride rgb_stride (3, or 4 for the [r,g,b,sigma] layout),
 * sigma (R,S,*) with stride sigma_stride (1 or 4).  out_depth / out_weights may be NULL. */
int nrf_composite(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                  const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                  float* out_rgb, float* out_depth, float* out_weights, void* stream);
/* ray_utils.py:86-143 (intent; the reference function raises):
 * z_vals, weights (R,S) -> samples (R,Ni) and sorted union (R,S+Ni); u: ray r reads u[r * u_ray_stride + j] -- (R,Ni) rows with
 * u_ray_stride = Ni, or ONE row shared by all rays with u_ray_stride = 0 (the caller's torch.linspace(0,1,Ni): its last ulp
 * is host dependent and a nearly empty bin amplifies one ulp of u to 2e-4 of depth) -- or NULL -> linspace(0,1,Ni) in-kernel.
 * The two reductions (:107-109) follow PyTorch's CPU kernels -- weights.sum in ATen's cascade order (8-float vectors),
 * torch.cumsum accumulated in double and rounded per knot -- so the `denom < 1e-5` guard (:131) takes the same branch as the
 * reference's fp32 CPU run would. */
int nrf_sample_pdf(const float* z_vals, const float* weights, int64_t n_rays, int n_samples, int n_importance,
                   const float* u, int64_t u_ray_stride, float* samples, float* z_union, void* stream);
/* nrf_sample_pdf with a third optional output: samples_sorted (R,Ni), the new samples in ascending order (equal values keep the
 * order of u) -- the row the kernel merges into the union.  At least one of the three outputs is given. */
int nrf_sample_pdf_sorted(const float* z_vals, const float* weights, int64_t n_rays, int n_samples, int n_importance,
                          const float* u, int64_t u_ray_stride, float* samples, float* samples_sorted, float* z_union, void* stream);

/* ---- hierarchical render that evaluates only the new samples in its fine pass -------------------------------------------
 * A sample's network output depends on its ray and its depth alone, and the fine pass' sorted union holds the S coarse depths
 * bit for bit: S of its S + Ni evaluations repeat the coarse pass.  The route below keeps them instead:
 *   1. nrf_render_rays_emit / nrf_render_camera_emit: the plain render (same rgb, depth, weights, z_vals bits) that also stores,
 *      for every (ray, sample), the four head outputs its compositor consumes -- r, g, b before the sigmoid, density before the
 *      ReLU -- as the 16-byte row raw4[(ray * n_samples + s) * 4 ..]; raw4 (R, n_samples, 4), 16-byte aligned.
 *   2. nrf_sample_pdf_sorted on the coarse weights: the Ni new depths, ascending.
 *   3. the emitting render again with opts->z_in = the new depths, opts->n_samples = Ni and raw_only = 1: rgb, depth, weights
 *      and z_vals are ignored (may be NULL), only raw4 (R, Ni, 4) is stored.
 *   4. nrf_composite_merge / nrf_composite_merge_camera: one lane per ray merges the two ascending depth lists -- the coarse
 *      sample first among equals, the rule of the sorted union -- and composites the merged order front to back with the fused
 *      renderer's operations in its order (dist to the next merged depth, 1e10 |d| for the last).  mma_mode: the mode that
 *      emitted the rows (it selects the compositor's exp / sigmoid as in the renderer).  n_importance = 0 composites the coarse
 *      rows alone (z_new, raw_new unused).  out_rgbd: rgb is (R,4) rows [r,g,b,depth], 16-byte aligned, depth unused.
 *      weights, z_union (R, S+Ni): optional.
 * The result equals, bit for bit, the fine pass rendered on the sorted union through opts->z_in.  The emitting entries take
 * ert_eps == 0 only (NRF_EINVAL otherwise) and have no tail or occupancy form.
 * nrf_hier_workspace_bytes: n_rays * (S * (4 + 4 + 16) + Ni * (4 + 16)) -- coarse depths, weights and rows, new depths and rows:
 * what a caller marching a frame in ray ranges holds per range. */
int nrf_render_rays_emit(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays,
                         const nrf_render_opts* opts, float* rgb, float* depth, float* weights, float* z_vals,
                         float* raw4, int raw_only, void* stream);
int nrf_render_camera_emit(const nrf_model* m, int H, int W, float focal, const float c2w[12],
                           int64_t ray_begin, int64_t ray_end, const nrf_render_opts* opts,
                           float* rgb, float* depth, float* weights, float* z_vals, float* raw4, int raw_only, void* stream);
int nrf_composite_merge(const float* z_coarse, const float* raw_coarse, const float* z_new, const float* raw_new,
                        const float* rays_d, int64_t n_rays, int n_samples, int n_importance, int mma_mode, int white_bkgd,
                        int out_rgbd, float* rgb, float* depth, float* weights, float* z_union, void* stream);
int nrf_composite_merge_camera(const float* z_coarse, const float* raw_coarse, const float* z_new, const float* raw_new,
                               int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                               int n_samples, int n_importance, int mma_mode, int white_bkgd, int out_rgbd,
                               float* rgb, float* depth, float* weights, float* z_union, void* stream);
int64_t nrf_hier_workspace_bytes(int64_t n_rays, int n_samples, int n_importance);

/* ray_utils.py:176-210 + dino_feature_model.py:114-148: points (N,3) -> features (N,C); xy (N,2) may be NULL. */
int nrf_project_fetch(const nrf_dino* dino, const float* points, int64_t n, float* feats, float* xy, void* stream);

/* dino_feature_model.py:114-148 on its own (== lora_dino.py:110-144, multi_scale_dino.py:156-183): bilinear grid_sample
 * (zeros padding, align_corners=False) of a (1,Hp,Wp,C) channel-last map at n normalised image points (n,2) -> (n,C). */
int nrf_sample_features(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, float* feats, void* stream);

/* The adjoints of the two fetches with respect to the map -- what autograd through F.grid_sample (dino_feature_model.py:137-143)
 * hands to the feature extractor when its map requires grad (the LoRA matrices of lora_dino.py are in train.py:105-110's
 * optimizer): d_map (Hp,Wp,C) = [accumulate ? d_map : 0] + sum over samples and their <= 4 on-map taps of weight * d_feats (n,C).
 * The same tap arithmetic as the forward; no gradient with respect to the points.  No atomics: workgroups add their slab of
 * samples, in order, into private copies of the map in `ws` (device, nrf_fetch_backward_workspace_bytes(Hp, Wp, C, n) bytes --
 * a function of the sizes alone), which a second launch adds up in a fixed order, so d_map is bit-identical from run to run.
 * dino->features is not read (may be NULL).  n == 0 with accumulate == 0 clears d_map. */
int64_t nrf_fetch_backward_workspace_bytes(int Hp, int Wp, int C, int64_t n);
int nrf_project_fetch_backward(const nrf_dino* dino, const float* points, int64_t n, const float* d_feats,
                               float* d_map, int accumulate, void* ws, int64_t ws_bytes, void* stream);
int nrf_sample_features_backward(int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats,
                                 float* d_map, int accumulate, void* ws, int64_t ws_bytes, void* stream);

/* The adjoints of the two fetches with respect to the points -- what autograd through ray_utils.py:176-210 and F.grid_sample hands
 * to points (or rays, or a pose) that require grad: with m_ab the texel row at (x0+a, y0+b), or 0 where that tap is off the map
 * (selected out, not multiplied by 0: a NaN / Inf texel reaches only the samples that have it among their on-map taps), and
 * (tx, ty) the fractional texel coordinates,
 *   G_x = sum_c g_c [(1-ty)(m_10 - m_00) + ty (m_11 - m_01)],   G_y = sum_c g_c [(1-tx)(m_01 - m_00) + tx (m_11 - m_10)],
 *   d_xy = (G_x Wp/2, G_y Hp/2)                                                   (nrf_sample_features_backward_points, (n,2))
 *   d_points = inv_pose[:3,:3]^T (d_x 2f/(W Zi), d_y 2f/(H Zi), -(d_x 2f X/W + d_y 2f Y/H)/Zi^2),  Zi = Z + 1e-8  ((n,3))
 * the same gx, gy, floor and on-map test as the forward.  The fetch is piecewise bilinear: on a texel edge the derivative is the
 * one of the cell floor() selects.  A sample with no tap on the map gets +0.  accumulate != 0 adds onto d_points (the V3 input
 * gradient: onto nrf_mlp_backward_inputs_v3's d_positions); otherwise the output is overwritten.  No atomics: a sample's result
 * is bit-identical from run to run and does not depend on the batch around it.  No gradient with respect to the source view's
 * pose or intrinsics. */
int nrf_project_fetch_backward_points(const nrf_dino* dino, const float* points, int64_t n, const float* d_feats,
                                      float* d_points, int accumulate, void* stream);
int nrf_sample_features_backward_points(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n,
                                        const float* d_feats, float* d_xy, void* stream);

/* ---- host-only introspection (no GPU needed; used by the CPU test-suite to replay the
 *      kernel's MFMA walk over the packed stream) -------------------------------- */
/* Packs `linears` exactly as nrf_model_create would for `mma_mode`.  stream_out / bias_out may be
 * NULL to query the sizes (bytes of the fragment stream, floats of the bias table). */
int nrf_debug_pack(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode,
                   uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes,
                   float* bias_out, int64_t bias_cap, int64_t* n_bias);

/* Host-only, like nrf_debug_pack, for the training path: the transposed (backward-chain) fragment stream, and the
 * saved-tensor / weight-gradient plan serialised as int32:
 *   n_slots, slot_tiles[n_slots], n_jobs, then per job: x_slot, dz_slot, KT, MT, x_first,
 *   row_w[32*MT], row_b[32*MT] (flat-parameter offsets of the weight row / of the bias, -1 = none), col[32*KT];
 *   finally n_mask_planes (ReLU-mask bit planes of 1 KiB per 32 samples appended to the context).
 * Used by the CPU tests to replay the backward pass through a numpy model of the MFMA lane maps. */
int nrf_debug_pack_backward(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode,
                            uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes);
int nrf_debug_train_plan(const nrf_arch* arch, const nrf_linear* linears, int n_linear,
                         int32_t* out, int64_t cap, int64_t* n_ints);
/* NRF_NET_V3, host-only: the fragment stream of nrf_mlp_backward_dino's A operand -- W0d^T, the dino_dim columns of
 * dino_fusion.fusion.0 (lora_dino.py:156) transposed: dino_dim/32 output tiles x 8 K tiles, fragment order (m, t, s). */
int nrf_debug_pack_dino_grad(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode,
                             uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes);
/* NRF_NET_V1 / V2, host-only: the fragment stream of nrf_mlp_backward_inputs' A operands, every layer from a 16-fragment boundary.
 * Layer 0: W0^T of the first Linear restricted to the positional-encoding tiles, pe_tiles(pos_freq) output tiles x 8 K tiles in
 * (m, t, s) order; accumulator register r of lane half h in output tile m belongs to feature (slot 16m + r, half h) of the kernel
 * order (slot u < 3L: sin | cos of (f = u/3, c = u%3); u = 3L: x | z; u = 3L+1: y | unused).  Layer 1 (V2): color_layers.0^T
 * restricted to the direction-encoding tile, 1 output tile x 4 K tiles. */
int nrf_debug_pack_input_grad(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode,
                              uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes);

/* NRF_NET_V3, host-only: the fragment stream of nrf_mlp_backward_inputs_v3's A operands, every layer from a 16-fragment boundary.
 * Layer 0: W0p^T, the positional-encoding columns of dino_fusion.fusion.0 transposed, pe_tiles(pos_freq) output tiles x 8 K tiles
 * in (m, t, s) order and the slot order of nrf_debug_pack_input_grad.  Layer 1: color_layers.0^T restricted to the
 * direction-encoding tile, 1 output tile x 4 K tiles. */
int nrf_debug_pack_input_grad_v3(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode,
                                 uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes);

/* Host-only: the frequency mask's scale id of every flat parameter (nrf_model_set_freq_mask): position column c is id c, direction
 * column c is id 3*(2*pos_freq+1) + c, -1 = the parameter is not scaled.  out (may be NULL to query n_ids): nrf_param_count values. */
int nrf_debug_freq_mask_ids(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int8_t* out, int64_t cap, int64_t* n_ids);

/* Host-only: how render_kernel / render_hold_kernel deal a launch of n_rays rays x n_samples samples to the workgroups of a device
 * with n_cu compute units, for a geometry of cols_per_wave sample columns per wave (64: NRF_MMA_BF16 / F16, 32: the fp32-class modes).
 * head[4] = { 1: the even deal / 0: equal tiles round-robin, log2 of the uniform deal's samples per ray and pass, workgroups,
 * MLP passes of the longest workgroup }.  items (may be NULL to query n_items) receives, per work item in the order the
 * workgroups march them, 4 values: workgroup, first ray, rays (the launch's last item may reach past n_rays), log2 of its
 * samples per ray and pass.  Honours NRF_SPW like the launchers. */
int nrf_debug_ray_deal(int64_t n_rays, int n_samples, int cols_per_wave, int n_cu, int64_t* head,
                       int64_t* items, int64_t cap, int64_t* n_items);

/* ---- misc ------------------------------------------------------------------ */
const char* nrf_last_error(void);
int nrf_abi_version(void);
/* sizeof() of the ABI structs as this library was compiled (0: nrf_arch, 1: nrf_linear, 2: nrf_dino,
 * 3: nrf_render_opts, 4: nrf_tail; -1 otherwise): lets a binding check its struct declarations before the first call. */
int nrf_abi_sizeof(int which);
/* name / average duration bookkeeping is the caller's business: the library never times anything. */

/* ------------------------------------------------------------------------
 * Training path: what loss.backward() and
 * optimizer.step() of src/training/train.py:282-288 run through.  Built for
 * NRF_NET_V1 (nerf_model.NeRFMLP, the network of train_minimal.py:28),
 * NRF_NET_V2 (train.py's model with use_dino=False) and NRF_NET_V3 (use_dino=True).
 *
 * Parameters and gradients travel as ONE flat fp32 device vector: the Linears
 * in state_dict order, each weight (out_f*in_f, row-major) followed by its
 * bias (out_f) -- nrf_param_count() floats.  The Python module keeps its
 * nn.Parameters as views into such a vector, so torch.optim.Adam (or
 * nrf_adam_step) updates it in place and nrf_model_update_device re-packs
 * the MFMA operand streams from it without leaving the device.
 * ------------------------------------------------------------------------ */
int64_t nrf_param_count(const nrf_model* m);

/* Replaces nrf_model_update for device-resident parameters: re-packs the
 * forward (and, once training has been used, backward) streams of the modes in
 * mode_mask (bit NRF_MMA_*) from flat_params, plus the bias table.  Enqueued on
 * `stream`; a single mode is one kernel launch.  The streams of the modes NOT in the
 * mask keep the previous parameters (a later render / backward in such a mode needs
 * its own update; nrf_mlp_backward* refuses stale backward weights).  A tail render
 * (nrf_render_*_tail) reads two streams: put the base mode's bit and NRF_MMA_F16X3's into
 * ONE mask -- a second call for the other mode would mark the first one's backward weights
 * stale. */
int nrf_model_update_device(nrf_model* m, const float* flat_params, int mode_mask, void* stream);

/* Per-column scale of the positional encodings (FreeNeRF's frequency mask, general form).
 * pos_scale: HOST, 3*(2*pos_freq+1) floats in the encoder's column order [x | sin f0 | cos f0 | sin f1 | ...], or NULL = all ones.
 * dir_scale: HOST, 3*(2*dir_freq+1) floats, or NULL; must be NULL for NRF_NET_V1.
 * Values finite and in [0,1], otherwise NRF_EINVAL.  A mask that is all ones (or both NULL) clears the mask.
 *
 * A mask m on an encoding is a column scale of the Linears that read it, W (m . enc) = (W diag m) enc: layers.0 (V1),
 * density_layers.0 and the direction columns of color_layers.0 (V2), the position columns of dino_fusion.fusion.0 and the same
 * columns of color_layers.0 (V3).  The setter only RECORDS the mask in the handle: no GPU call, no copy, no synchronisation.
 * It takes effect at the next pack -- nrf_model_update_device (the modes in its mask), nrf_model_update or nrf_model_create
 * (every mode) -- which writes the streams a pack of parameters holding the fp32 products weight * scale would write; every render,
 * forward and backward entry reads those streams.  Each mode remembers the mask its streams were last packed with and scales the
 * weight gradients of nrf_mlp_backward* with that one (dW = (dZ enc^T) diag m; biases are never scaled), so a forward, its backward
 * and its weight gradients agree; a hidden column (scale 0) receives gradient exactly 0.  Setting a mask that differs from the
 * recorded one marks the backward weights of all modes stale: nrf_mlp_backward* refuses a mode until it has been re-packed.
 * The getter returns the recorded mask (either pointer may be NULL) and active = 1 unless it is all ones. */
int nrf_model_set_freq_mask(nrf_model* m, const float* pos_scale, const float* dir_scale);
int nrf_model_get_freq_mask(const nrf_model* m, float* pos_scale, float* dir_scale, int* active);

/* Bytes of saved tensors ("context") a forward_train/backward pair needs for n
 * samples; the caller allocates it (device) and keeps it until backward ran.  It holds
 * the saved operand tiles of every layer, the ReLU bit planes, (V3) the softmax gate and
 * the weight-gradient partial sums: about 9 KiB per sample for the 8x256 network in the
 * 16-bit modes plus ~64 MiB of partial sums. */
int64_t nrf_train_context_bytes(nrf_model* m, int mma_mode, int64_t n);

/* nerf_model.py:16-24 forward with grad enabled: out4 as nrf_mlp_forward_v1,
 * and every layer's activations saved into ctx. */
int nrf_mlp_forward_train_v1(nrf_model* m, int mma_mode, const float* x_enc, int64_t n, float* out4,
                             void* ctx, int64_t ctx_bytes, void* stream);

/* Its backward: g_out4 = dL/d out4 (n,4); flat_grad (nrf_param_count floats)
 * += dL/d parameters.  out4 is the tensor forward_train wrote.  No gradient
 * with respect to x_enc is produced (the reference never needs one). */
int nrf_mlp_backward_v1(nrf_model* m, int mma_mode, const float* out4, const float* g_out4, int64_t n,
                        void* ctx, int64_t ctx_bytes, float* flat_grad, void* stream);

/* The same pair for NRF_NET_V2 (train.py:229 `rgb, density = self.nerf_model(positions, directions, None)` with grad
 * enabled; nerf_mlp.py:134-158 without the DINO branch).  rgb (n,3) / density (n,1) are written by the forward and
 * read again by the backward (sigmoid', relu'); g_rgb / g_density are dL/d of them.  These calls produce no gradient with respect to
 * positions, directions or the DINO features (one more launch does: nrf_mlp_backward_inputs, nrf_mlp_backward_dino).  NRF_NET_V3 (nerf_mlp.py:134-158 with lora_dino.py:171-193: the fusion
 * block runs twice on the same weights, gated by a 2-way softmax) takes the per-sample features as `dino`; up to 8 trunk
 * layers. */
int nrf_mlp_forward_train(nrf_model* m, int mma_mode, const float* positions, const float* directions,
                          const float* dino /* NRF_NET_V3: (n, dino_dim) per-sample features, else NULL */, int64_t n,
                          float* rgb, float* density, void* ctx, int64_t ctx_bytes, void* stream);
int nrf_mlp_backward(nrf_model* m, int mma_mode, const float* rgb, const float* density,
                     const float* g_rgb, const float* g_density, int64_t n,
                     void* ctx, int64_t ctx_bytes, float* flat_grad, void* stream);

/* NRF_NET_V3, after nrf_mlp_backward on the same ctx (same n and mode): d_dino (n, dino_dim) = dL/d dino, the gradient with
 * respect to the per-sample features nrf_mlp_forward_train read (lora_dino.py:181,187-191: through both fusion passes and the
 * gate).  One more launch over what the backward saved; nrf_train_context_bytes does not change.  d_dino is overwritten
 * (16-byte aligned).  NRF_EINVAL for another network family, a context that is too small or stale backward weights. */
int nrf_mlp_backward_dino(nrf_model* m, int mma_mode, int64_t n, void* ctx, int64_t ctx_bytes, float* d_dino, void* stream);

/* NRF_NET_V1 / V2, after nrf_mlp_backward_v1 / nrf_mlp_backward on the same ctx (same n and mode): the gradient with respect to
 * the inputs of the field, from the dZ tiles of the first Linear (and, V2, of color_layers.0) that the backward saved.  One more
 * launch; nrf_train_context_bytes does not change.  Any output may be NULL (not computed), not all of them:
 *   d_x_enc      (n, pe_dim)  V1 only: dL/d x_enc in the reference's column order (positional_encoding.py:27-33);
 *   d_positions  (n,3)        dL/d positions through the adjoint of the encoding; reads `positions` (n,3), the points the forward
 *                             encoded (V1: the points x_enc was computed from);
 *   d_directions (n,3)        V2 only: the same for the view directions; reads `directions` (n,3).
 * Rows >= n are not written; the outputs are overwritten.  A sample's result does not depend on the batch around it and two runs
 * give the same bits.  NRF_EINVAL before any launch for NRF_NET_V3 (it also needs the adjoint of the projection and bilinear
 * fetch with respect to the points: nrf_mlp_backward_inputs_v3 and nrf_project_fetch_backward_points), d_x_enc on another family than V1, d_directions on V1, a missing positions / directions
 * where its derivative is asked for, no output at all, a pointer that is not 4-byte aligned, a context that is too small, or
 * stale backward weights (nrf_model_update_device).  n == 0 is NRF_OK and launches nothing. */
int nrf_mlp_backward_inputs(nrf_model* m, int mma_mode, int64_t n, void* ctx, int64_t ctx_bytes,
                            const float* positions, const float* directions,
                            float* d_x_enc, float* d_positions, float* d_directions, void* stream);

/* NRF_NET_V3, after nrf_mlp_backward on the same ctx (same n and mode): the gradient with respect to positions and directions
 * through the positional encodings, from the two dZ tiles of dino_fusion.fusion.0, the gate and the dZ tiles of color_layers.0 that
 * the backward saved: dL/d PE(pos) = W0p^T d1 + w0 (W0p^T d2) (joined in fp32), dL/d PE(dir) as for V2, then the adjoint of the
 * encodings.  One more launch; nrf_train_context_bytes does not change.  This is NOT all of dL/d positions: the features the
 * forward read were fetched at the projections of the same points.  That share is nrf_mlp_backward_dino's d_dino handed to
 * nrf_project_fetch_backward_points with accumulate = 1 on this call's d_positions.  (On fields of the reference's initialisation
 * it is 100 to 3000 times smaller than the share through the encoding: test it on its own.)
 * Either output may be NULL (not computed), not both; rows >= n are not written; the outputs are overwritten.  A sample's result
 * does not depend on the batch around it and two runs give the same bits.  NRF_EINVAL before any launch for another network
 * family, a missing positions / directions where its derivative is asked for, a pointer that is not 4-byte aligned, a context
 * that is too small, or stale backward weights.  n == 0 is NRF_OK and launches nothing. */
int nrf_mlp_backward_inputs_v3(nrf_model* m, int mma_mode, int64_t n, void* ctx, int64_t ctx_bytes,
                               const float* positions, const float* directions,
                               float* d_positions, float* d_directions, void* stream);

/* Backward of nrf_composite (autograd through nerf_mlp.py:181-212): given
 * dL/d rgb_map (n_rays,3), optionally dL/d depth (n_rays) and dL/d weights
 * (n_rays,S), writes dL/d rgb (strided like the inputs) and dL/d sigma. */
int nrf_composite_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                           const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                           const float* g_rgb, const float* g_depth, const float* g_weights,
                           float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, void* stream);
/* The same, and the geometric terms of that autograd: d_z (n_rays,S) = dL/d z_vals (through the interval lengths and the depth
 * map) and d_rays_d (n_rays,3) = dL/d rays_d through |rays_d| (nerf_mlp.py:185).  Both required.  d_rgb / d_sigma are
 * nrf_composite_backward's bits. */
int nrf_composite_backward_geom(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                                const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                                const float* g_rgb, const float* g_depth, const float* g_weights,
                                float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                                float* d_z, float* d_rays_d, void* stream);
/* Adjoint of pts = rays_o + rays_d * z (nrf_sample_along_rays) and of the expansion of rays_d over a ray's samples:
 *   d_rays_o (R,3) = sum_s d_points;   d_rays_d (R,3) = sum_s (z_s d_points + d_dirs) + d_rays_d_in;
 *   d_z_out (R,S)  = rays_d . d_points + d_z_in.
 * d_points (R*S,3), z_vals (R,S), rays_d (R,3) are required; d_dirs (R*S,3), d_z_in (R,S), d_rays_d_in (R,3) may be NULL (zero);
 * any output may be NULL, not all.  Sums in a fixed order, no atomics: two runs give the same bits.  n_rays == 0 is NRF_OK. */
int nrf_ray_grad(const float* d_points, const float* d_dirs, const float* z_vals, const float* rays_d,
                 const float* d_z_in, const float* d_rays_d_in, int64_t n_rays, int n_samples,
                 float* d_rays_o, float* d_rays_d, float* d_z_out, void* stream);

/* `rgb_weight * nn.MSELoss()(pred, target)` (train.py:36-44) and its gradient in one launch: loss[0] = weight * mean((pred -
 * target)^2) over n values, g_pred = d loss / d pred.  n <= 2^22 (ray batches). */
int nrf_mse_grad(const float* pred, const float* target, int64_t n, float weight, float* g_pred, float* loss, void* stream);

/* nrf_composite + nrf_mse_grad + nrf_composite_backward in ONE launch (the three steps between the network's forward and its
 * backward in the reference's train_step, train.py:236,36-44,285): a ray's loss gradient needs only its own prediction and
 * target -- d loss / d pred = 2 weight (pred - target) / (3 n_rays).  d_rgb / d_sigma are bit-equal to the three-call sequence;
 * pred (n_rays,3) may be NULL.
 *   ray_loss : n_rays floats, receives each ray's squared error; the loss is weight * sum(ray_loss) / (3 n_rays)
 *              (nrf_adam_step_loss adds them up in a fixed order as a side job of its launch);
 *   zero_buf : optional, zero_n floats cleared by the same launch (the flat gradient vector nrf_mlp_backward* adds into). */
int nrf_composite_mse_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                               const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                               const float* target, float weight, float* pred,
                               float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                               float* ray_loss, float* zero_buf, int64_t zero_n, void* stream);

/* torch.optim.Adam's update (train.py:113-118; no amsgrad) on flat vectors;
 * step counts from 1. */
int nrf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* The same update, and as a side job of the launch loss[0] = loss_weight * sum(ray_loss[0..n_rays)) / (3 n_rays), summed in a
 * fixed order (ray_loss: nrf_composite_mse_backward's per-ray squared errors). */
int nrf_adam_step_loss(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                       const float* ray_loss, int64_t n_rays, float loss_weight, float* loss, void* stream);

/* ------------------------------------------------------------------------
 * The multiscale trainer's step (src/training/train_multiscale.py:207-211,249-266):
 * nerf_mlp.NeRFLoss on a VolumeRenderer in train() mode, clip_grad_norm_, optim.AdamW.  Additive to ABI 5: the
 * struct carries its own size, nrf_abi_sizeof knows nothing of it.
 * ------------------------------------------------------------------------ */
typedef struct nrf_loss_opts {
    int32_t      struct_bytes;  /* sizeof(nrf_loss_opts): checked by the library */
    float        rgb_weight;    /* nerf_mlp.py:219-223; all three >= 0 */
    float        reg_weight;    /* * mean(weights^2) */
    float        depth_weight;  /* * l1(depth, target_depth); inert without target_depth */
    const float* target_depth;  /* device, (n_rays), or NULL: no depth term */
    float        noise_std;     /* >= 0; nerf_mlp.py:188-190: density + noise * noise_std in front of the compositor's ReLU */
    const float* noise;         /* device, (n_rays, n_samples) standard normals (the parity route), or NULL: the in-kernel
                                   counter RNG (two uniforms -> Box-Muller) keyed by (rng_seed, ray index in the call, sample) */
    uint64_t     rng_seed;
} nrf_loss_opts;

/* nrf_composite_mse_backward generalised to the three-term loss, still ONE launch: composites sigma + noise_std * n, forms
 *   g_rgb = 2 rgb_weight (pred - target) / (3 R),  g_depth = depth_weight sign(depth - target_depth) / R,
 *   g_w[i] = 2 reg_weight w_i / (R S)   (in registers)
 * and runs the compositor backward with them; the ReLU mask of d_sigma is [sigma + noise_std * n > 0].  With
 * noise_std == 0, reg_weight == 0 and no target_depth, d_rgb / d_sigma / pred / ray_terms[0..n_rays) are
 * nrf_composite_mse_backward's bits.
 *   ray_terms : 3 * n_rays floats: every ray's squared rgb error | sum of w^2 | |depth - target_depth|
 *               (nrf_adamw_step_loss adds them up in a fixed order as a side job of its launch). */
int nrf_composite_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                                const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                                const float* target, const nrf_loss_opts* loss, float* pred,
                                float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                                float* ray_terms, float* zero_buf, int64_t zero_n, void* stream);

/* Global L2 norm of a flat gradient vector for clip_grad_norm_, without a read-back: this launch leaves at most 1024 partial
 * sums of squares in `workspace` (nrf_grad_sqnorm_workspace_bytes(n) bytes, device, 4-byte aligned); nrf_adamw_step_loss adds
 * them up.  Fixed summation order, no atomics: bit-reproducible.  Data parallel: call after the gradient all-reduce. */
int64_t nrf_grad_sqnorm_workspace_bytes(int64_t n);
int nrf_grad_sqnorm_partials(const float* grads, int64_t n, void* workspace, int64_t workspace_bytes, void* stream);

/* nrf_adam_step_loss with clipping and the choice of decay:
 *   max_norm > 0 : g is scaled on load by min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), norm from
 *                  `sqnorm_partials` (the workspace nrf_grad_sqnorm_partials filled for the same n); <= 0: no clipping;
 *   decoupled    : 0 = torch.optim.Adam (weight_decay * p added to the gradient), 1 = torch.optim.AdamW
 *                  (p *= 1 - lr * weight_decay in front of the moment update);
 *   grad_norm    : optional device float, receives the pre-clip norm (needs sqnorm_partials);
 *   ray_terms / losses : both or neither; losses[4] = total, rgb (mse), depth (l1), reg (mean w^2) with
 *                  total = rgb_weight rgb + depth_weight depth + reg_weight reg (nerf_mlp.py:249-257). */
int nrf_adamw_step_loss(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                        int decoupled, float max_norm, const float* sqnorm_partials, float* grad_norm,
                        const float* ray_terms, int64_t n_rays, int n_samples,
                        float rgb_weight, float depth_weight, float reg_weight, float* losses, void* stream);

/* ------------------------------------------------------------------------
 * Training from rays: what src/training/train.py:188-229 (`render_rays`: sample_points_along_rays, the directions expanded
 * per sample, project_points_to_image + sample_features_at_points, the positional encodings) builds in front of the network
 * happens inside the saving forward kernel instead.  A lane pair derives its sample's ray, depth and position with the same
 * explicitly rounded functions the staged kernels use (nrf_get_rays, nrf_sample_along_rays), encodes it, and (NRF_NET_V3)
 * gathers its feature-map channels with the renderer's taps in both fusion passes: no (n,3) positions, (n,3) directions,
 * (n, dino_dim) features or (n,63) encodings in memory.  Additive to ABI 5: the struct carries its own size, nrf_abi_sizeof
 * knows nothing of it.
 * ------------------------------------------------------------------------ */
typedef struct nrf_train_rays {
    int32_t        struct_bytes;   /* sizeof(nrf_train_rays): checked by the library */
    int32_t        reserved;       /* 0 */
    const float*   rays_o;         /* device (R,3); NULL in pixel mode */
    const float*   rays_d;         /* device (R,3); NULL in pixel mode */
    const int64_t* pixels;         /* pixel mode: device (R) ray ids y*W+x of the camera below; else NULL */
    int32_t        H;              /* pixel mode: the pinhole camera (ray_sampler.py:4-30) */
    int32_t        W;
    float          focal;
    float          c2w[12];        /* first 3 rows of the camera-to-world matrix */
    float*         z_vals;         /* out (R,S), required: the compositor and its backward read it */
    float*         rays_d_out;     /* out (R,3), required in pixel mode (the compositor needs |d|); else may be NULL */
    float*         points_out;     /* out (R*S,3), optional: what nrf_project_fetch_backward needs for dL/d map */
} nrf_train_rays;

/* The saving forward of all three families on n = n_rays * opts->n_samples samples, in sample order (ray-major), with the context
 * of nrf_train_context_bytes(m, mode, n); its backward is nrf_mlp_backward_v1 / nrf_mlp_backward / nrf_mlp_backward_dino on the
 * same context.
 *   NRF_NET_V1      : out_a = the (n,4) tensor of nrf_mlp_forward_train_v1, out_b must be NULL;
 *   NRF_NET_V2 / V3 : out_a = rgb (n,3), out_b = density (n,1), as nrf_mlp_forward_train.
 * Of `opts` the call reads near, far, n_samples, lindisp, perturb, t_rand, z_ladder, z_in, rng_seed (the renderer's meaning),
 * mma_mode (bf16, f16, f32; f16x3 trains in fp32) and dino (NRF_NET_V3: the source view's map, required).  The jitter of row r,
 * sample s of the call is counter_uniform(rng_seed, r, s): nrf_sample_along_rays' key -- the row in the call, not the pixel id
 * -- so that ray mode, pixel mode and the staged route produce the same depths.
 * z_vals, points_out and rays_d_out receive what nrf_sample_along_rays / nrf_get_rays would have written, to the bit.
 * NRF_EINVAL, before any launch: ert_eps > 0, a wrong struct_bytes, both or neither of rays and pixels, a missing required
 * output, NRF_NET_V3 without dino or with dino->C != dino_dim, n_samples < 1, n_rays < 0, n > 2^31 - 1, a context that is too
 * small.  n_rays == 0 succeeds and launches nothing. */
int nrf_mlp_forward_train_rays(nrf_model* m, const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts,
                               float* out_a, float* out_b, void* ctx, int64_t ctx_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Training under an occupancy grid.  A step under a grid G is the plain step with every sample in an empty cell of G replaced by
 * a constant: it composites as colour (0,0,0) and EFFECTIVE density -inf -- effective means behind the density noise, so that
 * noise_std > 0 cannot bring it back.  In the compositor that gives relu(-inf) = 0, exp(-0) = 1, alpha = 0, weight 0 and the
 * factor 1 + 1e-10 on the transmittance; in its backward the mask [sigma > 0] is false, so d_sigma = 0, and d_rgb = w g = 0.
 * Without noise these are the bits of density 0, which is how the *_occ renderers skip.  The network -- forward, dZ chain, weight
 * gradients -- runs on the M occupied samples alone, as dense rows: the staged entry points (nrf_encode, nrf_project_fetch,
 * nrf_mlp_forward_train[_v1], nrf_mlp_backward[_v1]) take any n and treat every sample independently of its neighbours.  A skipped
 * sample passes no gradient to the parameters; the regulariser and the depth term see its weight 0.  z_vals is always the full
 * (R,S) ladder: the interval of an evaluated sample still runs to the next ladder sample, as in the renderers.
 * Additive to ABI 5: the struct carries its own size, nrf_abi_sizeof knows nothing of it.
 * ------------------------------------------------------------------------ */
typedef struct nrf_compact {
    int32_t  struct_bytes;   /* sizeof(nrf_compact): checked by the library */
    int32_t  reserved;       /* 0 */
    int64_t  capacity;       /* rows the compacted outputs hold; R*S always suffices (and is required: M is not known before the call) */
    int32_t* index;          /* out (capacity): flat sample id r*S+s of compacted row j < M, strictly ascending */
    int32_t* slot;           /* out (R*S): compacted row of sample i, or -1 */
    float*   positions;      /* out (capacity,3): the renderer's points, o + d*z, bit for bit */
    float*   directions;     /* out (capacity,3): the ray's direction per row; may be NULL (V1) */
    int64_t* count;          /* out, device [1], 8-byte aligned: M */
    void*    workspace;      /* device, 4-byte aligned, written and read by the call */
    int64_t  workspace_bytes; /* >= nrf_occupancy_compact_workspace_bytes(n_rays) */
} nrf_compact;

/* Bytes of workspace a compaction of n_rays rays needs (4 per ray, rounded up to 16; 16 for no ray); -1 if n_rays < 0. */
int64_t nrf_occupancy_compact_workspace_bytes(int64_t n_rays);

/* Chooses the samples of a ray batch that the grid `occ` keeps and leaves them as dense rows in ascending order of the flat id:
 * row j of index / positions / directions belongs to sample index[j] = r*S+s, slot is the inverse map with -1 for a skipped sample.
 * The cell of a sample is decided by the rule of nrf_occupancy above, in the same single fp32 operations on p = o + d*z, the
 * point the network would be given (a sample outside the box follows occ->outside; a non-finite position is always kept).
 * `rays` is the ray source of nrf_mlp_forward_train_rays -- explicit rays, or pixel ids and a camera; of `opts` the call reads the
 * fields that entry point reads (near, far, n_samples, lindisp, perturb, t_rand, z_ladder, z_in, rng_seed), the jitter of row r,
 * sample s of the call is counter_uniform(rng_seed, r, s).  rays->z_vals (required) and rays->rays_d_out (required in pixel mode)
 * receive what nrf_sample_along_rays / nrf_get_rays would have written, to the bit; rays->points_out is not used.  occ->stats is
 * not touched.  Rows >= M of the outputs are not written.
 * Three launches on `stream` (per-ray counts, an exclusive scan of them by one workgroup, the write pass): no workgroup waits for
 * another, no atomics; the outputs are the same bits from run to run.  Nothing synchronises: the caller reads `count` back when it
 * needs M on the host.
 * NRF_EINVAL, before any launch: rays, opts, occ or out NULL, a wrong struct_bytes in any of them, both or neither of rays and
 * pixels, a missing required output (z_vals, rays_d_out in pixel mode, index, slot, positions, count), capacity < R*S,
 * R*S > 2^31 - 1, index / slot / positions / directions / z_vals / workspace not 4-byte aligned or count not 8-byte aligned, a
 * workspace that is NULL or too small, ert_eps > 0, and every condition nrf_occupancy refuses.  n_rays == 0 is NRF_OK and launches
 * nothing (count is not written). */
int nrf_occupancy_compact_rays(const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts,
                               const nrf_occupancy* occ, const nrf_compact* out, void* stream);

/* nrf_composite_loss_backward on compacted rows: `slot` (n_rays, n_samples) is nrf_compact.slot, and rgb / sigma / d_rgb / d_sigma
 * address compacted rows (row slot[i] of sample i, with their strides).  A sample with slot[i] < 0 is composited as colour (0,0,0)
 * and effective density -inf and stores nothing; z_vals, loss->noise and loss->target_depth keep their (n_rays, n_samples) /
 * (n_rays) layouts, the counter RNG its key (ray index in the call, sample).  With every slot[i] == i the results are
 * nrf_composite_loss_backward's bits -- and so, with noise_std == 0, reg_weight == 0 and no target_depth, those of
 * nrf_composite_mse_backward: the one entry serves both steps.  slot must be 4-byte aligned; everything else as
 * nrf_composite_loss_backward. */
int nrf_composite_loss_backward_indexed(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                                        const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                                        const float* target, const nrf_loss_opts* loss, const int32_t* slot, float* pred,
                                        float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                                        float* ray_terms, float* zero_buf, int64_t zero_n, void* stream);

/* nrf_mlp_forward_train_rays on a compacted sample list: the ray route's front end under a grid.  Row j < n_rows of out_a / out_b
 * and of the saved context is sample index[j] = r*S + s of the ray batch (nrf_compact.index), derived exactly as
 * nrf_mlp_forward_train_rays derives its row r*S + s: the ray from rays_o / rays_d or from the pixel id and the camera, the position
 * o + d*z by the same single fp32 operations, the V1 encoding in the kernel, the NRF_NET_V3 feature map gathered in both fusion
 * passes -- except that the depth is READ from rays->z_vals (R,S), where nrf_occupancy_compact_rays has left the ladder, and is not
 * drawn again.  The call writes none of the nrf_train_rays outputs (z_vals, rays_d_out, points_out); no encodings, positions,
 * directions or per-sample features pass through memory.  The context is the ordinary one of
 * nrf_train_context_bytes(m, mode, n_rows) or larger; nrf_mlp_backward_v1 / nrf_mlp_backward / nrf_mlp_backward_dino run on it with
 * n = n_rows.  Of `opts` the call reads n_samples, mma_mode and dino (NRF_NET_V3); the sampling fields are checked as
 * nrf_mlp_forward_train_rays checks them and otherwise unused.
 * An index entry outside [0, n_rays * n_samples) is the caller's error: the behaviour is undefined (the kernel reads z_vals and the
 * ray arrays at it unchecked).
 * NRF_EINVAL, before any launch: index NULL or not 4-byte aligned, n_rows < 0 or n_rows > n_rays * n_samples, a missing
 * rays->z_vals, a context too small for n_rows, and everything nrf_mlp_forward_train_rays refuses.  n_rows == 0 succeeds and
 * launches nothing.  Additive to ABI 5. */
int nrf_mlp_forward_train_rays_indexed(nrf_model* m, const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts,
                                       const int32_t* index, int64_t n_rows, float* out_a, float* out_b, void* ctx,
                                       int64_t ctx_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The hierarchical training step: one network, a coarse and a fine image (NeRF's coarse-to-fine sampling; the render side is
 * nrf_sample_pdf_sorted / nrf_composite_merge above).  Additive to ABI 5: the struct carries its own size.
 *   loss = w_coarse * mse(pred_coarse, target) + w_fine * mse(pred_fine, target)
 * pred_coarse composites the S coarse rows on z_coarse; pred_fine composites the S + Ni rows of both sets in the merged order on
 * the merged depths.  The merge rule is nrf_sample_pdf's: a coarse depth goes in front of an equal new one, equal new depths keep
 * their order -- the order of a stable sort of [z_coarse | z_new] -- the interval of a sample runs to the next merged depth, the
 * last one is 1e10 |d|.  No gradient reaches the depths: the resampling is a constant, as in NeRF.
 * The sequence between the step's two saving forwards and its two backwards:
 *   nrf_mlp_forward_train_rays on the S ladder samples -> nrf_composite (the coarse weights) -> nrf_sample_pdf_sorted (Ni new
 *   depths, ascending) -> nrf_mlp_forward_train_rays with opts->z_in = the new depths, n_samples = Ni, a context of its own
 *   -> THIS ENTRY -> nrf_mlp_backward* on the coarse context -> nrf_mlp_backward* on the new one (both add into zero_buf)
 * Each sample is evaluated once forward and once backward: S + Ni network rows per ray.
 * ------------------------------------------------------------------------ */
typedef struct nrf_hier_loss {
    int32_t      struct_bytes;    /* sizeof(nrf_hier_loss): checked by the library */
    int32_t      white_bkgd;
    int32_t      rgb_stride;      /* of rgb_* and d_rgb_*: 3, or 4 for [r,g,b,sigma] rows */
    int32_t      sigma_stride;    /* of sigma_* and d_sigma_*: 1 or 4 */
    const float* rgb_coarse;      /* the network rows of the coarse samples, (n_rays * S) rows */
    const float* sigma_coarse;
    const float* rgb_new;         /* the network rows of the new samples, (n_rays * Ni) rows, laid out the same way */
    const float* sigma_new;
    const float* z_coarse;        /* (n_rays, S), ascending */
    const float* z_new;           /* (n_rays, Ni), ascending (nrf_sample_pdf_sorted: samples_sorted) */
    const float* rays_d;          /* (n_rays, 3) */
    const float* target;          /* (n_rays, 3) */
    float        w_coarse;        /* both >= 0 */
    float        w_fine;
    float*       d_rgb_coarse;    /* out: d loss / d rows, the strides of the rows.  Coarse rows receive the coarse term's */
    float*       d_sigma_coarse;  /*      gradient plus the fine term's (one fp32 addition), new rows the fine term's */
    float*       d_rgb_new;
    float*       d_sigma_new;
    float*       pred_coarse;     /* out, (n_rays, 3), may be NULL */
    float*       pred_fine;       /* out, (n_rays, 3), may be NULL */
    float*       ray_loss;        /* out, (n_rays): w_coarse * se_c + w_fine * se_f, se = a ray's squared rgb error; the loss is
                                     sum(ray_loss) / (3 n_rays): nrf_adam_step_loss with loss_weight = 1 */
    float*       ray_parts;       /* out, (2, n_rays): se_c | se_f, may be NULL */
    float*       z_union;         /* out, (n_rays, S + Ni): the merged depths, may be NULL */
    float*       weights_fine;    /* out, (n_rays, S + Ni): the fine image's weights, may be NULL (costs one more launch) */
    float*       zero_buf;        /* optional, zero_n floats cleared by the first launch, as in nrf_composite_mse_backward */
    int64_t      zero_n;
    void*        workspace;       /* nrf_hier_train_workspace_bytes(n_rays, S, Ni) bytes, 16-byte aligned */
    int64_t      workspace_bytes;
} nrf_hier_loss;

/* Bytes of nrf_hier_loss.workspace: the gathered union's rows, their d rows, depths and merge ranks (40 B per sample) and 20 B per
 * ray, rounded up to 16; -1 for n_rays < 0, n_samples < 1, n_importance < 1 or n_samples + n_importance > 4096. */
int64_t nrf_hier_train_workspace_bytes(int64_t n_rays, int n_samples, int n_importance);

/* The stage itself.  Four launches on `stream`, five with weights_fine: nrf_composite_mse_backward's kernel on the coarse rows
 * at weight w_coarse (it clears zero_buf) -> every sample finds its merge rank (coarse a: a + #{new < z_a}, new k: k + #{coarse <= z_k})
 * by a binary search of the other list and leaves its depth and its row at that place of the workspace -> the same compositor kernel
 * on the gathered union at weight w_fine -> every sample fetches the fine term's d row from its rank, a new sample stores it, a
 * coarse sample adds it to the coarse term's.  pred_*, ray_parts, d rows, z_union and weights_fine are therefore the bits of
 * nrf_composite_mse_backward / nrf_composite on the coarse rows and on the union gathered by a stable sort.  Every element is
 * written by one thread: no atomics, two runs give the same bits.  Nothing synchronises or allocates.
 * NRF_EINVAL, before any launch: a NULL, a wrong struct_bytes, n_rays < 0, n_samples < 1, n_importance < 1, n_samples +
 * n_importance > 4096, strides below 3 / 1, a negative or non-finite weight, a required pointer (rows, depths, rays_d, target, d
 * rows, ray_loss) that is NULL, any float pointer not 4-byte aligned, zero_n < 0 or zero_n > 0 without zero_buf, a workspace that
 * is NULL, not 16-byte aligned or too small.  n_rays == 0 is NRF_OK and launches nothing (zero_buf is not cleared: the plain
 * entry refuses an empty batch, there is no clearing launch to follow). */
int nrf_composite_hier_loss_backward(const nrf_hier_loss* a, int64_t n_rays, int n_samples, int n_importance, void* stream);

/* ------------------------------------------------------------------------
 * Few-shot ray regularisers in the fused training step: the distortion loss of mip-NeRF 360 and the occlusion (near-camera
 * density) penalty of FreeNeRF, both per-ray functions of what the compositor backward holds in registers.  Per ray, with w_i the
 * compositor's weights (behind the density noise), z_i the depths (non-decreasing), s_i the density the compositor's ReLU sees
 * (sigma_i + noise_std n_i; -inf for a sample the slot map skips), kappa = dist_inv_span and S = n_samples:
 *   m_i = kappa (z_i + z_{i+1}) / 2,  delta_i = kappa (z_{i+1} - z_i)   for i < S-1
 *   m_{S-1} = kappa z_{S-1},          delta_{S-1} = 0                   (the compositor's last interval is 1e10: no width here)
 *   D = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i
 *   O = (1/M') sum_{i<M'} relu(s_i),   M' = min(occ_samples, S)
 *   loss = nrf_composite_loss_backward's + dist_weight mean_r D_r + occ_weight mean_r O_r
 * Depths carry no gradient.  Additive to ABI 5: the struct carries its own size, nrf_abi_sizeof knows nothing of it.
 * ------------------------------------------------------------------------ */
typedef struct nrf_ray_reg {
    int32_t struct_bytes;   /* sizeof(nrf_ray_reg): checked by the library */
    float   dist_weight;    /* >= 0; 0: the distortion term is not computed, its row of ray_terms is 0 */
    float   dist_inv_span;  /* kappa, 1 / (far - near) for depths in [near, far]; finite and > 0 when dist_weight > 0 */
    float   occ_weight;     /* >= 0; 0: the occlusion term is not computed, its row of ray_terms is 0 */
    int32_t occ_samples;    /* >= 1 when occ_weight > 0; clamped to n_samples */
} nrf_ray_reg;

/* nrf_composite_loss_backward (slot == NULL) or nrf_composite_loss_backward_indexed (slot = nrf_compact.slot) with the two terms,
 * still ONE launch: dL/dw_i gains dist_weight / R (2 sum_j w_j |m_i - m_j| + (2/3) w_i delta_i) where the regulariser's
 * 2 reg_weight w_i / (R S) enters, d_sigma_i gains occ_weight / (R M') [s_i > 0] for i < M'.  The double sum costs O(S) per ray:
 * prefix and suffix scans of w and w m over the ray's 64-sample segments.  With both weights 0 pred, d_rgb, d_sigma and the first
 * three rows of ray_terms are the bits of the entry without the terms.
 *   ray_terms : 5 * n_rays floats: the three rows of nrf_composite_loss_backward | D_r | O_r
 * NRF_EINVAL, before any launch: what nrf_composite_loss_backward refuses (n_samples > 4096 among it), reg NULL or of a wrong
 * struct_bytes, a negative or non-finite weight, dist_weight > 0 with a dist_inv_span that is not finite and > 0, occ_weight > 0
 * with occ_samples < 1, a slot that is not 4-byte aligned. */
int nrf_composite_reg_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                                    const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                                    const float* target, const nrf_loss_opts* loss, const nrf_ray_reg* reg, const int32_t* slot,
                                    float* pred, float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                                    float* ray_terms, float* zero_buf, int64_t zero_n, void* stream);

/* One small launch behind nrf_adamw_step_loss (which was handed the same ray_terms and left losses4 = total, rgb, depth, reg):
 *   losses6 = [total + dist_weight mean D + occ_weight mean O, rgb, depth, reg, mean D, mean O]
 * Rows 3 and 4 of ray_terms are added up by one workgroup in a fixed order: no atomics, two runs give the same bits.  losses4 and
 * losses6 are device pointers and may not overlap.  NRF_EINVAL: a NULL, n_rays < 1, and what the entry above refuses of reg. */
int nrf_ray_terms_finish(const float* ray_terms, int64_t n_rays, const nrf_ray_reg* reg, const float* losses4, float* losses6,
                         void* stream);

/* ------------------------------------------------------------------------
 * Patch regulariser: RegNeRF's depth-smoothness loss on small patches rendered from poses nobody observed.  A batch of R = n_rays
 * rays is R_s supervised rays followed by N_p = n_patches patches of P x P rays (P = patch_size), R = R_s + N_p P^2, patch-major and
 * row-major inside a patch: ray (i, j) of patch p is row R_s + p P^2 + i P + j.  target and loss->target_depth hold R_s rows.
 * With d(p,i,j) the compositor's depth sum_k w_k z_k of a patch ray (behind the density noise):
 *   DS_p   = sum_{i<P-1, j<P-1} (d(i,j) - d(i,j+1))^2 + (d(i,j) - d(i+1,j))^2
 *   smooth = sum_p DS_p / (N_p (P-1)^2)                                       (RegNeRF's compute_tv_norm(...).mean())
 *   loss   = rgb_weight mse (R_s rays, divisor 3 R_s) + depth_weight l1 (R_s rays, divisor R_s) + reg_weight mean w^2 (R rays)
 *            + dist_weight mean D + occ_weight mean O (R rays) + depth_smooth_weight smooth
 * A patch ray has no target: its colour gradient is 0, it takes the three target-free terms like any ray, and its dL/d depth is
 *   (2 depth_smooth_weight / (N_p (P-1)^2)) ([i<P-1, j<P-1] ((d(i,j) - d(i,j+1)) + (d(i,j) - d(i+1,j)))
 *                                            - [i<P-1, j>0] (d(i,j-1) - d(i,j)) - [i>0, j<P-1] (d(i-1,j) - d(i,j)))
 * formed in single fp32 operations in this order.  Depths and poses carry no gradient.  Additive to ABI 5, as nrf_ray_reg is.
 * ------------------------------------------------------------------------ */
typedef struct nrf_patch_reg {
    int32_t struct_bytes;          /* sizeof(nrf_patch_reg): checked by the library */
    float   depth_smooth_weight;   /* >= 0 */
    int32_t patch_size;            /* P, 2 ... 16 */
    int32_t n_patches;             /* N_p >= 0, N_p P^2 < n_rays: a batch keeps at least one supervised ray */
} nrf_patch_reg;

/* nrf_composite_reg_loss_backward with the patch term, still ONE launch: the supervised rays are that entry's code, one wave per
 * ray; a workgroup owns a patch, composites its rays, exchanges their depths through LDS, and runs the compositor backward of every
 * patch ray with the dL/d depth above.  No atomics: two runs give the same bits.  With n_patches = 0 every output is
 * nrf_composite_reg_loss_backward's, bit for bit.  With n_patches > 0 every ray's compositor forms a sample's transmittance factor
 * as e + 1e-10 from e = exp(-relu(s) dist) itself and its suffix sums without a subtraction -- the same values in exact arithmetic,
 * better conditioned behind a nearly opaque sample -- so pred and d rows differ from the other loss entries' in the last digits.
 *   ray_terms   : 5 * n_rays floats, as there; rows 0 and 2 of a patch ray are 0
 *   patch_terms : n_patches floats: DS_p
 *   patch_depth : n_patches * P * P floats: d(p,i,j), or NULL
 *   pred        : n_rays * 3 floats (or NULL): the patch rays' colours too
 * NRF_EINVAL, before any launch: what nrf_composite_reg_loss_backward refuses, patch NULL or of a wrong struct_bytes, a negative or
 * non-finite depth_smooth_weight, patch_size outside 2 ... 16, n_patches < 0, n_patches * patch_size^2 >= n_rays, patch_terms NULL
 * with n_patches > 0. */
int nrf_composite_patch_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                                      const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                                      const float* target, const nrf_loss_opts* loss, const nrf_ray_reg* reg, const int32_t* slot,
                                      float* pred, float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                                      float* ray_terms, float* zero_buf, int64_t zero_n, void* stream, const nrf_patch_reg* patch,
                                      float* patch_terms, float* patch_depth);

/* One small launch behind the optimiser (whose own four loss values divide every term by R and are not the step's with patches):
 *   losses7 = [total, rgb, depth, reg, mean D, mean O, smooth]
 * formed by one workgroup from the five rows of ray_terms and from patch_terms with the divisors above, in a fixed order; the depth
 * term counts only with loss->target_depth set, as in the loss launch.  NRF_EINVAL: a NULL (patch_terms may be NULL with
 * n_patches = 0), n_rays < 1, n_samples outside 1 ... 4096, and what the entry above refuses of loss, reg and patch. */
int nrf_patch_terms_finish(const float* ray_terms, int64_t n_rays, int n_samples, const nrf_loss_opts* loss, const nrf_ray_reg* reg,
                           const nrf_patch_reg* patch, const float* patch_terms, float* losses7, void* stream);

/* ------------------------------------------------------------------------
 * Information regularisers: InfoNeRF's ray-entropy loss on every ray and its information-gain (KL) loss between neighbouring
 * rays, here the neighbouring rays of the patches of nrf_patch_reg.  Both act on the per-sample distribution of a ray.  For ray r
 * with S samples, s_i the density the ReLU sees (behind the density noise; -inf for a sample skipped under an occupancy grid),
 * dist_i as the compositor forms it, over the S - 1 samples i = 0 ... S-2 with a finite interval (the last sample, whose dist is
 * 1e10 |d|, takes no part), eps = 1e-10, tau = ent_threshold, natural logarithms:
 *   x_i = relu(s_i) dist_i      a_i = -expm1(-x_i)      A = sum_i a_i      p_i = a_i / (A + eps)
 *   H_r = -sum_i p_i ln(p_i + eps)                       m_r = [A > tau]   (a constant: no gradient)
 *   KL(p || q) = sum_i p_i (ln(p_i + eps) - ln(q_i + eps))
 *   entropy = (1/R) sum_r m_r H_r                        over all R rays of the batch, the patch rays included
 *   K_p     = sum_{i<P-1, j<P-1} m(i,j) m(i,j+1) KL(p(i,j) || p(i,j+1)) + m(i,j) m(i+1,j) KL(p(i,j) || p(i+1,j))
 *   kl      = sum_p K_p / (N_p (P-1)^2)
 *   loss    = nrf_composite_patch_loss_backward's + ent_weight entropy + kl_weight kl
 * The gradient flows into both arguments of every KL, to the densities alone: with G_i = dL/dp_i summed over a ray's roles
 * (entropy: -ln(p_i+eps) - p_i/(p_i+eps); first argument of a KL: ln(p_i+eps) - ln(q_i+eps) + p_i/(p_i+eps); second argument,
 * p' the first: -p'_i/(p_i+eps)), M = sum_i p_i G_i,
 *   dL/ds_j += [s_j > 0] dist_j exp(-x_j) (G_j - M) / (A + eps).
 * a_i comes from expm1, not from the compositor's alpha = 1 - e: next to e = 1 that subtraction keeps three digits of a_i.  The
 * compositor's own alpha is what it was.  A ray with S = 1, a masked ray (A <= tau) and a sample with s_j <= 0 receive exactly
 * nothing from the two terms.  Additive to ABI 5, as nrf_patch_reg is.
 * ------------------------------------------------------------------------ */
typedef struct nrf_info_reg {
    int32_t struct_bytes;          /* sizeof(nrf_info_reg): checked by the library */
    float   ent_weight;            /* >= 0; 0: the entropy term is not computed */
    float   ent_threshold;         /* tau >= 0: rays with A <= tau take part in neither term */
    float   kl_weight;             /* >= 0; 0: the KL term is not computed */
} nrf_info_reg;

/* The KL term keeps a patch's distributions in LDS between the two phases of the loss launch: patch_size^2 * n_samples floats
 * (P^2 rows of S - 1 values and their sums), sized at launch.  A request with kl_weight > 0 and patch_size^2 * n_samples above
 * this is refused; it admits P = 8 at S = 192 and P = 16 at S = 48.  The entropy term alone has no such cap. */
#define NRF_INFO_KL_MAX_LDS_FLOATS 12288

/* nrf_composite_patch_loss_backward with the two terms, still ONE launch and its walk: a wave that has run the compositor
 * backward of a ray forms G and M for it, LANE <-> sample (M a wave reduction per 64-sample segment, the segments added front to
 * back; rays of S - 1 <= 64 keep everything in registers, longer ones walk their segments once more), and adds
 *   fl(fl(dist_j e_j) * fl(fl(G_j - M) / fl(A + eps)))
 * in one rounded addition to the d_sigma entry that the compositor backward has just stored, regularisers included.  With
 * kl_weight > 0 phase 1 of a patch leaves every ray's a_i and A in LDS, and phase 2 reads up to four neighbours' rows.  No atomics:
 * two runs give the same bits.  With ent_weight = kl_weight = 0 every output is nrf_composite_patch_loss_backward's, bit for bit
 * (n_patches = 0 or not), and the launch carries no dynamic LDS.  A term whose weight is 0 is not computed and its output is 0.
 *   info_terms : n_rays floats: m_r H_r       (may be NULL with ent_weight = 0)
 *   patch_kl   : n_patches floats: K_p        (may be NULL with kl_weight = 0)
 * NRF_EINVAL, before any launch: what nrf_composite_patch_loss_backward refuses; info NULL or of a wrong struct_bytes; a negative
 * or non-finite ent_weight, ent_threshold or kl_weight; kl_weight > 0 with n_patches = 0; kl_weight > 0 with
 * patch_size^2 * n_samples > NRF_INFO_KL_MAX_LDS_FLOATS; info_terms NULL with ent_weight > 0; patch_kl NULL with kl_weight > 0. */
int nrf_composite_info_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride,
                                     const float* z_vals, const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd,
                                     const float* target, const nrf_loss_opts* loss, const nrf_ray_reg* reg, const int32_t* slot,
                                     float* pred, float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride,
                                     float* ray_terms, float* zero_buf, int64_t zero_n, void* stream, const nrf_patch_reg* patch,
                                     float* patch_terms, float* patch_depth, const nrf_info_reg* info, float* info_terms,
                                     float* patch_kl);

/* nrf_patch_terms_finish with the two terms:
 *   losses9 = [total, rgb, depth, reg, mean D, mean O, smooth, entropy, kl]
 * unweighted components with the divisors above (entropy: R; kl: N_p (P-1)^2, 0 with n_patches = 0), the total with both weighted
 * terms, one workgroup, a fixed order.  NRF_EINVAL: what nrf_patch_terms_finish refuses, what the entry above refuses of info,
 * info_terms NULL with ent_weight > 0, patch_kl NULL with kl_weight > 0. */
int nrf_info_terms_finish(const float* ray_terms, int64_t n_rays, int n_samples, const nrf_loss_opts* loss, const nrf_ray_reg* reg,
                          const nrf_patch_reg* patch, const float* patch_terms, const nrf_info_reg* info, const float* info_terms,
                          const float* patch_kl, float* losses9, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFHIP_H */
