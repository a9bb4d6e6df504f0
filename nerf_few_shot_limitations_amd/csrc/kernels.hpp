// kernels.hpp -- host-visible launch interface between api.cpp and the .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/nerfhip.h"
#include "device_math.hpp"

namespace nrf {

constexpr int kMaxCams = 8;
constexpr int kModes = 4;           // NRF_MMA_BF16, _F16, _F32, _F16X3 (the training path is built for the first three)

// device-side image of one nrf_model
struct DeviceNet {
    nrf_arch arch;
    const void* stream[kModes];   // packed fragment streams, indexed by NRF_MMA_*
    uint32_t n_chunks[kModes];
    const float* bias;          // bias table (fp32, shared by all modes)
    int n_bias;
    int64_t flops_per_sample;
    int device;
    int cu_count;
    unsigned long long* queues;   // kQueueSlots counters; launches cycle through them
};

constexpr int kQueueSlots = 64;

struct DinoDev {                // V3 side channel, by value in the kernel arguments
    const float* features;
    int Hp, Wp, C;
    float inv_pose[12];         // first 3 rows of inverse(pose)
    float focal;
    int H, W;
};

struct RenderArgs {
    // rays: explicit (rays_o/rays_d) or camera (cam + ray_begin)
    const float* rays_o;
    const float* rays_d;
    int camera_mode;
    int n_cams;             // camera mode: a batch of up to kMaxCams views of one HxW sensor rendered by ONE launch
    int64_t rays_per_cam;   // local rays [c*rays_per_cam, (c+1)*rays_per_cam) belong to cams[c]
    Camera cams[8];
    int64_t ray_begin;
    int64_t n_rays;
    int64_t tile_rays;      // camera mode: local ray i is global ray ray_begin + (i / tile_rays) * tile_stride + i % tile_rays,
    int64_t tile_stride;    // clamped to the image (tile_rays >= n_rays: one contiguous range)
    // sampling
    float near, far;
    int n_samples, lindisp, perturb;
    const float* t_rand;
    const float* z_ladder;
    const float* z_in;
    uint64_t seed;
    // compositing
    float ert_eps;
    int white_bkgd;
    // outputs
    int interleaved;        // 1: rgb points at (R,4) rows [r,g,b,depth] (one 16-B store per ray), depth is unused
    float* rgb;
    float* depth;
    float* weights;
    float* z_vals;
    DinoDev dino;
    unsigned long long* queue;   // ERT (ray-queue) kernel: device counter of rays handed out, zeroed before the launch
    int spw_log2;                // render_kernel: log2 of the samples per ray and MLP pass (set by the launcher)
};

int launch_render(const DeviceNet& net, int mma_mode, const RenderArgs& a, hipStream_t s, std::string& err);
// Tail mode: samples 0 .. S-2 in base_mode (bf16 / f16), compositor state through `carry` (render_tail_floats(n_rays) floats), sample
// S-1 in split-f16; two launches on s (one when n_samples == 1).  Reads the streams of base_mode AND of NRF_MMA_F16X3.
constexpr int kCarryRows = 6;       // T, r, g, b, depth, acc: one row of n_rays floats each
inline int64_t render_tail_floats(int64_t n_rays) { return kCarryRows * n_rays; }
int launch_render_tail(const DeviceNet& net, int base_mode, const RenderArgs& a, float* carry, hipStream_t s, std::string& err);
// Empty-space skipping (nerfhip.h: nrf_occupancy), by value in the arguments of the skipping ray-queue kernels alone
struct OccDev {
    const uint32_t* bits;       // bit ((iz * res[1] + iy) * res[0] + ix): 1 = occupied
    int res[3];
    float lo[3], scale[3];
    int outside;                // 1: a (finite) sample outside the box is skipped
    unsigned long long* stats;  // optional [2]: += evaluated (ray, sample) pairs | MLP passes of waves that held a live ray
};
// the ray-queue kernel with skipping (ert_eps >= 0: 0 = skipping alone)
int launch_render_occ(const DeviceNet& net, int mma_mode, const RenderArgs& a, const OccDev& g, hipStream_t s, std::string& err);
// render_kernel's march (ert_eps == 0) that also stores every real (ray, sample)'s raw head outputs [r, g, b before the sigmoid, density
// before the ReLU] as the 16-byte row raw4[ray * n_samples + s]; a.rgb == NULL: the image is not stored
int launch_render_emit(const DeviceNet& net, int mma_mode, const RenderArgs& a, float* raw4, hipStream_t s, std::string& err);
// The hierarchical fine pass from kept rows (hier_kernels.hip: composite_merge_kernel): per ray the S coarse and the Ni new samples
// (each list ascending) are merged -- the coarse one first among equals, sample_pdf_kernel's rule -- and composited front to back by one
// lane with the operations of render_march's SPW = 1 branch.
struct MergeArgs {
    const float* z_coarse;      // (R,S)
    const float* raw_coarse;    // (R,S,4)
    const float* z_new;         // (R,Ni) ascending; unused with Ni == 0
    const float* raw_new;       // (R,Ni,4)
    const float* rays_d;        // (R,3), or NULL: rays ray_begin .. of `cam`
    Camera cam;
    int64_t ray_begin;
    int64_t n_rays;
    int S, Ni;
    int white_bkgd, interleaved;
    float* rgb;                 // (R,3), or (R,4) rows [r,g,b,depth] with `interleaved`
    float* depth;               // (R), unused with `interleaved`
    float* weights;             // optional (R,S+Ni)
    float* z_union;             // optional (R,S+Ni)
};
int launch_composite_merge(const MergeArgs& m, bool fast_exp, hipStream_t s);
// launch_sample_pdf with the new samples in ascending order as a third optional output (R,Ni)
int launch_sample_pdf_sorted(const float* z, const float* w, int64_t n_rays, int S, int Ni, const float* u, int64_t u_ray_stride, float* samples,
                             float* samples_sorted, float* z_union, hipStream_t s);
int launch_forward_v1(const DeviceNet& net, int mma_mode, const float* x_enc, int64_t n, float* out4, hipStream_t s, std::string& err);
int launch_forward(const DeviceNet& net, int mma_mode, const float* pos, const float* dir, const float* dino, int64_t n,
                   float* rgb, float* density, hipStream_t s, std::string& err);

// ---- training path (train_shared.hip, train_v1.hip ... train_v3.hip) ----------------
constexpr int kMaxSlots = 40;
constexpr int kMaxJobs = 24;
constexpr int kMaxMaskSlots = 20;
constexpr int kMapStride = 3 * 320;      // per weight-gradient job: row_w[320] | row_b[320] | col[320]

struct FreqMaskArgs;             // freq_mask.hpp
struct TrainDev {
    const void* bstream[3];     // backward-chain (transposed) streams by NRF_MMA_*
    uint32_t n_bchunks[3];
    const int32_t* maps;        // device, n_jobs * kMapStride
    int n_slots;
    int slot_tiles[kMaxSlots];  // feature tiles per saved-tensor slot
    int n_mask_slots;           // ReLU-mask bit planes (one per masked layer)
    int aux_floats;             // extra fp32 values saved per sample (V3: the softmax gate)
    int cu_count;               // sizes the weight-gradient partial sums (one block per workgroup)
    int n_jobs;
    int job_x_slot[kMaxJobs], job_dz_slot[kMaxJobs], job_KT[kMaxJobs], job_MT[kMaxJobs], job_x_first[kMaxJobs];
    int64_t n_params;
    const void* gstream[3];     // V3: the W0d^T fragments of dino_grad_kernel (train_dino_grad_impl.hpp), behind the chain's layers in bstream
    const void* istream[3];     // V1, V2: the W0^T (and color_layers.0^T) fragments of input_grad_kernel (train_input_grad_impl.hpp), likewise;
                                // V3: the W0p^T and color_layers.0^T fragments of input_grad_v3_kernel (train_input_grad_v3_impl.hpp), behind gstream's
    const FreqMaskArgs* freq[3];  // HOST: the frequency mask the mode's streams were last packed with, NULL = none: its weight gradients scale with it
};

int64_t train_ctx_bytes(const TrainDev& t, int mma_mode, int64_t n);
int launch_train_forward(const DeviceNet& net, const TrainDev& t, int mma_mode, const float* x_enc, int64_t n, float* out4, void* ctx,
                         hipStream_t s, std::string& err);
// dZ chain + weight gradients: grad (flat, n_params floats) += dL/dparams
int launch_train_backward(const DeviceNet& net, const TrainDev& t, int mma_mode, const float* out4, const float* g_out4, int64_t n,
                          void* ctx, float* grad, hipStream_t s, std::string& err);
int launch_train_forward_v2(const DeviceNet& net, const TrainDev& t, int mma_mode, const float* pos, const float* dir, int64_t n, float* rgb,
                            float* density, void* ctx, hipStream_t s, std::string& err);
int launch_train_backward_v2(const DeviceNet& net, const TrainDev& t, int mma_mode, const float* rgb, const float* density,
                             const float* g_rgb, const float* g_density, int64_t n, void* ctx, float* grad, hipStream_t s, std::string& err);
int launch_train_forward_v3(const DeviceNet& net, const TrainDev& t, int mma_mode, const float* pos, const float* dir, const float* dino, int64_t n,
                            float* rgb, float* density, void* ctx, hipStream_t s, std::string& err);
int launch_train_backward_v3(const DeviceNet& net, const TrainDev& t, int mma_mode, const float* rgb, const float* density,
                             const float* g_rgb, const float* g_density, int64_t n, void* ctx, float* grad, hipStream_t s, std::string& err);
// The ray-input source of the saving forward kernels (train_impl.hpp: RayInputs), by value in their arguments: a sample's ray,
// depth, position, direction and (V3) feature-map taps are derived in the kernel (nerfhip.h: nrf_mlp_forward_train_rays)
struct TrainRaysDev {
    const float* rays_o;        // (R,3), or NULL: pixel mode
    const float* rays_d;
    const int64_t* pixels;      // pixel mode: (R) ray ids of `cam`
    Camera cam;
    DepthLadder lad;            // make_ladder on the host, as launch_sample hands it to sample_kernel
    int perturb;
    const float* t_rand;        // (R,S) or NULL: counter_uniform(seed, row, sample)
    const float* z_in;          // (R,S) explicit depths or NULL
    uint64_t seed;
    float* z_vals;              // out (R,S)
    float* rays_d_out;          // out (R,3) or NULL
    float* points_out;          // out (R*S,3) or NULL
    DinoDev dino;               // V3
};
// n = n_rays * r.lad.S samples; V1: out_a = out4 (n,4); V2 / V3: out_a = rgb (n,3), out_b = density (n,1)
int launch_train_forward_rays_v1(const DeviceNet& net, const TrainDev& t, int mma_mode, const TrainRaysDev& r, int64_t n, float* out4, void* ctx,
                                 hipStream_t s, std::string& err);
int launch_train_forward_rays_v2(const DeviceNet& net, const TrainDev& t, int mma_mode, const TrainRaysDev& r, int64_t n, float* rgb,
                                 float* density, void* ctx, hipStream_t s, std::string& err);
int launch_train_forward_rays_v3(const DeviceNet& net, const TrainDev& t, int mma_mode, const TrainRaysDev& r, int64_t n, float* rgb,
                                 float* density, void* ctx, hipStream_t s, std::string& err);
// the same on a compacted sample list (train_impl.hpp: IndexedRayInputs): row j < n_rows is sample index[j] of the ray batch, its depth is
// read from r.z_vals, and none of r's outputs is written
int launch_train_forward_rays_indexed_v1(const DeviceNet& net, const TrainDev& t, int mma_mode, const TrainRaysDev& r, const int32_t* index,
                                         int64_t n_rows, float* out4, void* ctx, hipStream_t s, std::string& err);
int launch_train_forward_rays_indexed_v2(const DeviceNet& net, const TrainDev& t, int mma_mode, const TrainRaysDev& r, const int32_t* index,
                                         int64_t n_rows, float* rgb, float* density, void* ctx, hipStream_t s, std::string& err);
int launch_train_forward_rays_indexed_v3(const DeviceNet& net, const TrainDev& t, int mma_mode, const TrainRaysDev& r, const int32_t* index,
                                         int64_t n_rows, float* rgb, float* density, void* ctx, hipStream_t s, std::string& err);
// V3, after launch_train_backward_v3 on the same context: d_dino (n, dino_dim) = dL/d per-sample DINO features
int launch_dino_grad(const DeviceNet& net, const TrainDev& t, int mma_mode, int64_t n, void* ctx, float* d_dino, hipStream_t s, std::string& err);
// V1 / V2, after the family's launch_train_backward* on the same context: dL/d encoded inputs (V1), positions, directions (V2); a NULL
// output is not computed
int launch_input_grad(const DeviceNet& net, const TrainDev& t, int mma_mode, int64_t n, void* ctx, const float* positions, const float* directions,
                      float* d_x_enc, float* d_positions, float* d_directions, hipStream_t s, std::string& err);
// V3, after launch_train_backward_v3 on the same context: dL/d positions and directions through the positional encodings alone (the
// share through the fetched features: launch_dino_grad, then launch_project_fetch_backward_points); a NULL output is not computed
int launch_input_grad_v3(const DeviceNet& net, const TrainDev& t, int mma_mode, int64_t n, void* ctx, const float* positions, const float* directions,
                         float* d_positions, float* d_directions, hipStream_t s, std::string& err);
int launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd, int step,
                const float* ray_loss, int64_t n_rays, float loss_weight, float* loss, hipStream_t s);
int launch_mse_grad(const float* pred, const float* target, int64_t n, float weight, float* g_pred, float* loss, hipStream_t s);
int launch_composite_mse_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                                  int64_t n_rays, int S, int white_bkgd, const float* target, float weight, float* pred, float* d_rgb,
                                  int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_loss, float* zero_buf,
                                  int64_t zero_n, hipStream_t s);
// The hierarchical training step's stage between its forwards and its backwards (hier_train.hip; nerfhip.h: nrf_hier_loss, whose
// fields these are): launch_composite_mse_backward on the coarse rows, the union gathered in the merged order, the same launch on
// it, the fine term's d rows scattered back.  workspace: hier_train_ws_bytes, 16-byte aligned.
struct HierTrainArgs {
    int white_bkgd, rgb_stride, sigma_stride;
    const float *rgb_coarse, *sigma_coarse, *rgb_new, *sigma_new, *z_coarse, *z_new, *rays_d, *target;
    float w_coarse, w_fine;
    float *d_rgb_coarse, *d_sigma_coarse, *d_rgb_new, *d_sigma_new;
    float *pred_coarse, *pred_fine, *ray_loss, *ray_parts, *z_union, *weights_fine;      // all but ray_loss may be NULL
    float* zero_buf; int64_t zero_n;
    void* workspace;
};
int64_t hier_train_ws_bytes(int64_t n_rays, int S, int Ni);
int launch_hier_loss_backward(const HierTrainArgs& a, int64_t n_rays, int S, int Ni, hipStream_t s);
// The multiscale trainer's step (train_multiscale.py:207-211,249-266): nerf_mlp.NeRFLoss on a VolumeRenderer in train() mode,
// clip_grad_norm_, AdamW
struct LossTerms {
    float rgb_weight, reg_weight, depth_weight;
    const float* target_depth;      // (R) or NULL
    float noise_std;
    const float* noise;             // (R,S) standard normals, or NULL: in-kernel counter RNG
    uint64_t rng_seed;
};
// What every launch_composite_*loss_backward takes: the two heads (dense rows, or with slot (R,S) the compacted rows of the indexed
// form, as d_rgb / d_sigma then are), the rays, the loss, the outputs and the flat gradient vector to clear
struct LossLaunch {
    const float* rgb; int rgb_stride; const float* sigma; int sigma_stride;
    const float *z, *rays_d; int64_t n_rays; int S; int white_bkgd; const float* target;
    LossTerms lt;
    const int32_t* slot;            // or NULL
    float* pred;                    // or NULL
    float* d_rgb; int d_rgb_stride; float* d_sigma; int d_sigma_stride;
    float* ray_terms;
    float* zero_buf; int64_t zero_n;
    hipStream_t s;
};
// ray_terms (3,R): squared rgb error | sum of w^2 | |depth - target_depth|
int launch_composite_loss_backward(const LossLaunch& a);
// The same launch with the two few-shot ray regularisers (ray_reg.hip; nerfhip.h: nrf_ray_reg, whose fields these are); ray_terms
// (5,R): the three rows above | D_r | O_r.  launch_ray_terms_finish: losses6 from rows 3, 4 and the optimiser launch's four values.
struct RayRegTerms { float dist_weight, dist_inv_span, occ_weight; int occ_samples; };
int launch_composite_reg_loss_backward(const LossLaunch& a, const RayRegTerms& rt);
int launch_ray_terms_finish(const float* ray_terms, int64_t n_rays, float dist_weight, float occ_weight, const float* losses4, float* losses6,
                            hipStream_t s);
// The same launch with RegNeRF's depth-smoothness term on patches as well (patch_reg.hip; nerfhip.h: nrf_patch_reg, whose fields
// these are): the last n_patches patch_size^2 rays are patch rays, target and target_depth hold the other rows.  patch_terms (N_p):
// DS_p; patch_depth (N_p, P, P) or NULL.  launch_patch_terms_finish: losses7 from the five rows of ray_terms and patch_terms.
struct PatchRegTerms { float depth_smooth_weight; int patch_size; int64_t n_patches; };
int launch_composite_patch_loss_backward(const LossLaunch& a, const RayRegTerms& rt, const PatchRegTerms& pt, float* patch_terms, float* patch_depth);
int launch_patch_terms_finish(const float* ray_terms, int64_t n_rays, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                              const float* patch_terms, float* losses7, hipStream_t s);
// The same launch with InfoNeRF's ray entropy and patch KL terms on top (info_reg.hip; nerfhip.h: nrf_info_reg, whose fields these
// are).  info_terms (R): m_r H_r; patch_kl (N_p): K_p.  launch_info_terms_finish: losses9 from ray_terms, patch_terms and those two.
struct InfoRegTerms { float ent_weight, ent_threshold, kl_weight; };
int launch_composite_info_loss_backward(const LossLaunch& a, const RayRegTerms& rt, const PatchRegTerms& pt, const InfoRegTerms& it,
                                        float* patch_terms, float* patch_depth, float* info_terms, float* patch_kl);
int launch_info_terms_finish(const float* ray_terms, int64_t n_rays, int S, const LossTerms& lt, const RayRegTerms& rt, const PatchRegTerms& pt,
                             const InfoRegTerms& it, const float* patch_terms, const float* info_terms, const float* patch_kl, float* losses9,
                             hipStream_t s);
// partial sums of squares of a flat vector (one float per workgroup, fixed order); the optimiser launch adds them up
constexpr int kMaxSqnormPartials = 1024;
inline int sqnorm_partials(int64_t n) {
    const int64_t p = (n + 1023) / 1024;
    return (int)(p < 1 ? 1 : (p > kMaxSqnormPartials ? kMaxSqnormPartials : p));
}
int launch_grad_sqnorm_partials(const float* g, int64_t n, float* partials, hipStream_t s);
struct AdamExt {
    int decoupled;                  // torch.optim.AdamW: p *= 1 - lr wd in front of the moment update, no decay in the gradient
    float max_norm;                 // > 0: clip_grad_norm_(max_norm) applied to g on load
    const float* partials;          // sqnorm_partials(n) floats of launch_grad_sqnorm_partials (max_norm > 0 or grad_norm)
    float* grad_norm;               // optional: receives the (pre-clip) L2 norm
    const float* ray_terms;         // optional (3,R) of launch_composite_loss_backward, with losses[4] = total, rgb, depth, reg
    int64_t n_rays; int n_samples;
    float rgb_weight, depth_weight, reg_weight;
    float* losses;
};
int launch_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, float wd, int step,
                 const AdamExt& ext, hipStream_t s);
// freq: the recorded frequency mask (freq_mask.hpp), or NULL: masked elements are converted from the fp32 product with their scale
int launch_repack3(const float* flat, const int32_t* const src[3], const int64_t n_elems[3], const int modes[3], void* const out[3], hipStream_t s,
                   const FreqMaskArgs* freq = nullptr);
int launch_composite_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                              int64_t n_rays, int S, int white_bkgd, const float* g_rgb, const float* g_depth, const float* g_w,
                              float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, hipStream_t s);
// launch_composite_backward with the geometric terms: d_z (R,S) = dL/d z_vals, d_rays_d (R,3) = dL/d rays_d through the ray norm
int launch_composite_backward_geom(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                                   int64_t n_rays, int S, int white_bkgd, const float* g_rgb, const float* g_depth, const float* g_w,
                                   float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* d_z, float* d_rays_d, hipStream_t s);
// adjoint of point_on_ray and of the expansion of the directions over a ray's samples (nerfhip.h: nrf_ray_grad)
int launch_ray_grad(const float* d_points, const float* d_dirs, const float* z, const float* rays_d, const float* d_z_in, const float* d_rays_d_in,
                    int64_t n_rays, int S, float* d_rays_o, float* d_rays_d, float* d_z_out, hipStream_t s);

// staged kernels (staged_kernels.hip)
int launch_get_rays(const Camera& cam, int64_t ray_begin, int64_t n, float* rays_o, float* rays_d, hipStream_t s);
int launch_sample(const float* rays_o, const float* rays_d, int64_t n_rays, float near, float far, int S, int lindisp,
                  int perturb, const float* t_rand, const float* z_ladder, uint64_t seed, float* pts, float* z_vals, hipStream_t s);
int launch_encode(const float* x, int64_t n, int dim, int L, int include_input, const float* freq_bands, float* out, hipStream_t s);
int launch_composite(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z, const float* rays_d,
                     int64_t n_rays, int S, int white_bkgd, float* out_rgb, float* out_depth, float* out_w, hipStream_t s);
int launch_sample_pdf(const float* z, const float* w, int64_t n_rays, int S, int Ni, const float* u, int64_t u_ray_stride, float* samples,
                      float* z_union, hipStream_t s);
// occupancy bit grids: cell c is occupied iff max(density[c*k .. c*k+k-1]) > threshold (a NaN counts as occupied); n_cells a multiple of 32
int launch_occupancy_pack(const float* density, int64_t n_cells, int k, float threshold, uint32_t* bits, hipStream_t s);
// bits_out = the 3x3x3 dilation of bits_in (cells beyond the box are empty); res[0] a multiple of 32
int launch_occupancy_dilate(const uint32_t* bits_in, const int res[3], uint32_t* bits_out, hipStream_t s);
// marks from rendered weights (nerfhip.h: nrf_occupancy_mark_rays): cam == NULL takes rays_o / rays_d, otherwise rays ray_begin .. of the camera
int launch_occupancy_mark(const float* rays_o, const float* rays_d, const Camera* cam, int64_t ray_begin, int64_t n_rays, int S, const float* z_vals,
                          const float* weights, const int res[3], const float lo[3], const float scale[3], float weight_threshold, float seen_eps,
                          uint32_t* hit_bits, uint32_t* seen_bits, hipStream_t s);
// compaction in front of a training step under a grid (nerfhip.h: nrf_occupancy_compact_rays): of `r` the ray source, the sampling fields,
// z_vals and rays_d_out are used; workspace: occupancy_compact_ws_bytes(n_rays) bytes
int64_t occupancy_compact_ws_bytes(int64_t n_rays);
int launch_occupancy_compact(const TrainRaysDev& r, int64_t n_rays, const OccDev& g, int64_t capacity, int32_t* index, int32_t* slot,
                             float* positions, float* directions, int64_t* count, void* workspace, hipStream_t s);
int launch_project_fetch(const DinoDev& d, const float* points, int64_t n, float* feats, float* xy, hipStream_t s);
int launch_sample_features(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, float* feats, hipStream_t s);
// adjoints of the two fetches with respect to the map (no atomics: per-slab private copies in `ws`, fetch_backward_ws_floats(...)
// floats, added in a fixed order): d_map (Hp,Wp,C) = [d_map +] fetch^T(d_feats (n,C)); d.features is not read
int64_t fetch_backward_ws_floats(int Hp, int Wp, int C, int64_t n);
int launch_project_fetch_backward(const DinoDev& d, const float* points, int64_t n, const float* d_feats, float* d_map, int accumulate, float* ws,
                                  hipStream_t s);
int launch_sample_features_backward(int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats, float* d_map, int accumulate,
                                    float* ws, hipStream_t s);
// adjoints of the two fetches with respect to the points: d_points (n,3) = [d_points +] (projection o fetch)^T d_feats (n,C), or d_xy (n,2)
int launch_project_fetch_backward_points(const DinoDev& d, const float* points, int64_t n, const float* d_feats, float* d_points, int accumulate,
                                         hipStream_t s);
int launch_sample_features_backward_points(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats,
                                           float* d_xy, hipStream_t s);

}  // namespace nrf
