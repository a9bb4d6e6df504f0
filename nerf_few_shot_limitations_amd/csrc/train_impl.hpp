// train_impl.hpp -- the training path of the V1 network (reference loop:
// src/training/train.py:244-292, loss.backward() through nerf_model.py:16-24):
//
//   train_forward_kernel   forward chain of fused_impl.hpp's staged forward, one 32-sample tile per wave, which also
//                          saves every layer's operand tiles (train_core.hpp);
//   train_backward_kernel  dZ chain: head^T, then layers.{n-1..1}^T streamed like the forward weights, ReLU' taken
//                          from the forward's bit planes, every dZ tile saved;
//   weight_grad_kernel     dW = dZ X^T, db = sum dZ over the samples: per Linear one 256 x 256 (or smaller) output
//                          held in the accumulators of a workgroup, the sample axis split over workgroups, partial
//                          sums left in the context and added up in a fixed order by weight_grad_reduce_kernel;
//   repack_kernel          flat fp32 parameters -> the packed operand streams (after every optimizer step);
//   adam_kernel            torch.optim.Adam's update on the flat vectors (train.py:113-118).
//
// The chain kernels of every family are written with ChainTile's blocks inside chain_kernel's frame, and index the saved
// tensors through train_slots.hpp.
//
// LANE <-> SAMPLE here (not ray): a training batch is a few thousand rays (baseline.yaml:32), so the sample
// axis, not the ray axis, has to fill the chip; compositing and its backward are the staged kernels.
#pragma once
#include <algorithm>

#include "fused_impl.hpp"
#include "train_core.hpp"
#include "train_slots.hpp"

namespace nrf {

struct TrainKArgs {
    NetArgs net;              // forward: forward stream + bias table; backward: the transposed stream
    const float* x_enc;       // V1: (P, pe_dim)
    const float* pos;         // V2: (P,3)
    const float* dir;         // V2: (P,3)
    const float* dino;        // V3: (P, dino_dim) per-sample features
    int64_t n;                // samples
    int64_t n_tiles;          // workgroup tiles of WAVES*32 samples
    float* out4;              // V1 forward: (P,4) written; backward: the same tensor, read (sigmoid')
    const float* g_out4;      // V1 backward: dL/d out4 (P,4)
    float* rgb;               // V2: (P,3) written by forward, read by backward
    float* density;           // V2: (P,1)
    const float* g_rgb;       // V2 backward: dL/d rgb (P,3)
    const float* g_density;   // V2 backward: dL/d density (P,1)
    char* ctx;                // saved tensors
    int64_t slot_off[kMaxSlots];
    int slot_tiles[kMaxSlots];
    int64_t mask_off[kMaxMaskSlots];   // ReLU-mask bit planes: kMaskBytes per sample tile each
    int64_t aux_off;                   // V3: (padded samples, 2) fp32 softmax gate
    int64_t partial_off;               // weight-gradient partial sums: one kPartialFloats block per workgroup
};

// the arguments of the ray-input forward kernels: the staged kernels' and, behind them, the ray source (no existing kernel sees it)
struct TrainRayKArgs : TrainKArgs {
    TrainRaysDev rays;
};

// the ray-input forward on compacted rows: row j < n is sample index[j] of the ray batch (strictly inside it: the caller's duty)
struct TrainRayIndexKArgs : TrainRayKArgs {
    const int32_t* index;
};

// The input source of the saving forward bodies (their last template argument; train_forward*_body, instantiated by the kernel
// pairs *_kernel / *_rays_kernel).  StagedInputs: the caller's per-sample tensors
// (x_enc | pos, dir, dino), as nrf_mlp_forward_train* documents them.  RayInputs: rays (or a camera and pixel ids) in P.rays;
// RaySample below derives what the staged tensors would have held.
// IndexedRayInputs: RayInputs on a compacted sample list (nerfhip.h: nrf_mlp_forward_train_rays_indexed) -- row j of the outputs and
// of the context is sample P.index[j] of the ray batch, its depth is read back from rays.z_vals (the compaction left it there), and
// the kernel stores none of the ray source's outputs.
struct StagedInputs { static constexpr bool kRays = false, kIndexed = false; typedef TrainKArgs KArgs; };
struct RayInputs { static constexpr bool kRays = true, kIndexed = false; typedef TrainRayKArgs KArgs; };
struct IndexedRayInputs { static constexpr bool kRays = true, kIndexed = true; typedef TrainRayIndexKArgs KArgs; };

// ---- host-side helpers shared by the training translation units ---------------------------------------------
constexpr int kWgSamples = 256;          // the context is laid out for whole 256-sample groups, whatever the geometry

inline int64_t tiles32(int64_t n) { return (n + kWgSamples - 1) / kWgSamples * (kWgSamples / 32); }

inline int tile_bytes_of(int mode) { return mode == NRF_MMA_F32 ? 4 * kFragBytes : 2 * kFragBytes; }

// Weight-gradient grid (weight_grad_kernel): one workgroup per CU (128 KiB of LDS); small batches get ONE round of
// workgroups, large ones two.  The workgroups of a round are dealt to the jobs in proportion to the bytes a job reads per
// sample (KT + MT saved tiles, with a floor: a stage costs a load latency + a barrier however few tiles it moves), so that
// all of them finish together and the grid never exceeds the round (a 257th workgroup would run alone after the other 256).
// Returns the grid size; first_block[j] .. first_block[j+1] are job j's workgroups.
constexpr int kPartialFloats = 8 * 8 * 16 * 64 + 8 * 32;      // a workgroup's 256 x 256 accumulators + its 8 bias rows of 32

inline int wgrad_grid(const TrainDev& t, int mode, int64_t n_tiles32, int* first_block) {
    const int ST = mode == NRF_MMA_F32 ? 1 : 2;
    const int rounds = n_tiles32 >= 8192 ? 2 : 1;
    constexpr int min_stages = 4, cost_floor = 10;
    const int64_t max_splits = std::max<int64_t>(1, (n_tiles32 + min_stages * ST - 1) / (min_stages * ST));
    const int budget = rounds * t.cu_count;      // fewer workgroups were measured slower at every batch size (75 %: equal, 50 %: +10 %)
    auto cost = [&](int j) { return std::max(t.job_KT[j] + t.job_MT[j], cost_floor); };
    int cost_sum = 0;
    for (int j = 0; j < t.n_jobs; ++j) cost_sum += cost(j);
    int next = 0;
    for (int j = 0; j < t.n_jobs; ++j) {
        int64_t sp = (int64_t)budget * cost(j) / std::max(cost_sum, 1);      // floor: the sum stays within the budget
        sp = std::max<int64_t>(1, std::min<int64_t>(sp, max_splits));
        if (first_block) first_block[j] = next;
        next += (int)sp;
    }
    if (first_block) first_block[t.n_jobs] = next;
    return next;
}

inline bool fill_slots(const TrainDev& t, int mode, int64_t n, TrainKArgs& k, std::string& err) {
    if (t.n_slots < 1 || t.n_slots > kMaxSlots) { err = "training plan missing"; return false; }
    const int64_t nt = tiles32(n);
    int64_t off = 0;
    for (int i = 0; i < t.n_slots; ++i) {
        k.slot_off[i] = off;
        k.slot_tiles[i] = t.slot_tiles[i];
        off += nt * t.slot_tiles[i] * tile_bytes_of(mode);
    }
    if (t.n_mask_slots < 0 || t.n_mask_slots > kMaxMaskSlots) { err = "training plan: too many masked layers"; return false; }
    for (int i = 0; i < t.n_mask_slots; ++i) {
        k.mask_off[i] = off;
        off += nt * kFragBytes;
    }
    k.aux_off = off;
    off += nt * 32 * (int64_t)t.aux_floats * 4;
    k.partial_off = off;
    return true;
}

// Geometry of the chain kernels: 8 waves x 32 samples per workgroup (two waves per SIMD) is the throughput shape; a batch
// that does not even give every CU one such workgroup runs 4 waves x 32 instead (twice the workgroups, one wave per SIMD:
// the pass of a lone wave is latency, not throughput, and the reference's last schedule stage is 512 rays x 64 samples).
inline bool small_batch(const DeviceNet& net, int64_t n) { return tiles32(n) / 4 <= net.cu_count; }

namespace {

// f(ChainGeo<Mode, WAVES>{}): the chain kernels' instantiation for `mode` and n samples -- the 16-bit modes at 4 or 8 waves
// (small_batch), the fp32 mode at 4
template <class M, int W>
struct ChainGeo {
    typedef M Mode;
    static constexpr int kWaves = W;
};

template <class F>
int dispatch_chain(const DeviceNet& net, int mode, int64_t n, F&& f) {
    const bool small = small_batch(net, n);
    switch (mode) {
        case NRF_MMA_BF16: return small ? f(ChainGeo<ModeBF16, 4>{}) : f(ChainGeo<ModeBF16, 8>{});
        case NRF_MMA_F16:  return small ? f(ChainGeo<ModeF16, 4>{}) : f(ChainGeo<ModeF16, 8>{});
        default:           return f(ChainGeo<ModeF32, 4>{});
    }
}

// the backward chains stream the transposed weights
NetArgs backward_net_args(const DeviceNet& net, const TrainDev& t, int mode) {
    NetArgs n = net_args(net, mode);
    n.stream = t.bstream[mode];
    n.n_chunks = t.n_bchunks[mode];
    return n;
}

}  // namespace

inline bool check_train_common(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (mode < 0 || mode > 2) { err = "unknown mma_mode"; return false; }
    if (net.arch.pos_freq != (net.arch.net == NRF_NET_V3 ? 12 : 10)) { err = "the training path is built for pos_freq 10 (V1, V2) and 12 (V3)"; return false; }
    if (!t.bstream[mode] || !t.maps) { err = "model not prepared for training"; return false; }
    if (net.n_bias > kBiasMaxFloats) { err = "bias table exceeds the LDS carve-out"; return false; }
    return true;
}

// the family checks of the chain launchers (train_v*.hip and the indexed ray forwards beside them)
inline bool check_train_v1(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return false;
    if (net.arch.net != NRF_NET_V1) { err = "nrf_mlp_*_train_v1 needs a V1 model"; return false; }
    return true;
}
inline bool check_train_v2(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return false;
    if (net.arch.net != NRF_NET_V2 || net.arch.dir_freq != 4) { err = "nrf_mlp_forward_train / nrf_mlp_backward need a V2 model with dir_freq 4"; return false; }
    return true;
}
inline bool check_train_v3(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return false;
    if (net.arch.net != NRF_NET_V3 || net.arch.dir_freq != 4 || (net.arch.dino_dim != 64 && net.arch.dino_dim != 128)) {
        err = "V3 training needs dir_freq 4 and dino_dim 64 or 128";
        return false;
    }
    if (net.arch.n_layers > 8) { err = "V3 training: at most 8 trunk layers (saved-tensor slot table)"; return false; }
    return true;
}

// dW/db of every Linear from the saved tensors (defined in train_shared.hip; network independent)
int launch_weight_grad(const DeviceNet& net, const TrainDev& t, int mode, const TrainKArgs& k, float* grad, hipStream_t s, std::string& err);

// One sample of a RayInputs kernel: row `ray` of the call and sample `s` of it (n < 2^31: 32-bit division), with the operations of
// get_rays_kernel / sample_kernel (staged_kernels.hip) in their order, so that depths, points and directions are theirs to the bit.
// Only `ray` stays live across the network: the colour branch asks for the direction again (two L2 hits or ~20 VALU
// instructions against three registers held through the trunk).
struct RaySample {
    uint32_t ray;
    int s;
    __device__ __forceinline__ RaySample(const TrainRaysDev& R, int64_t sid) {
        ray = (uint32_t)sid / (uint32_t)R.lad.S;
        s = (int)((uint32_t)sid - ray * (uint32_t)R.lad.S);
    }
    __device__ __forceinline__ void origin_dir(const TrainRaysDev& R, float (&o)[3], float (&d)[3]) const {
        if (R.pixels) {
            camera_ray(R.cam, R.pixels[ray], o, d);
            // the origin is the camera's translation, a load from the kernel arguments: left as one, the compiler merges it with the
            // other branch's load into ONE load through a selected pointer and parks the selection in scratch (12 bytes per lane)
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] = uniform_f(o[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) { o[k] = R.rays_o[(int64_t)ray * 3 + k]; d[k] = R.rays_d[(int64_t)ray * 3 + k]; }
        }
    }
    __device__ __forceinline__ void dir(const TrainRaysDev& R, float (&d)[3]) const {
        float o[3];
        origin_dir(R, o, d);
    }
    __device__ __forceinline__ float depth(const TrainRaysDev& R, int64_t sid) const {
        if (R.z_in) return R.z_in[sid];
        if (!R.perturb) return ladder_z(R.lad, s);
        const float u = R.t_rand ? R.t_rand[sid] : counter_uniform(R.seed, (uint64_t)ray, (uint32_t)s);
        return ladder_z_jitter(R.lad, s, u);
    }
    // the position of a sample whose depth the compaction has left in z_vals (IndexedRayInputs): nothing drawn, nothing stored
    __device__ __forceinline__ void position_kept(const TrainRaysDev& R, int64_t sid, float (&p)[3]) const {
        float o[3], d[3];
        origin_dir(R, o, d);
        const float z = R.z_vals[sid];
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = point_on_ray(o[k], d[k], z);
    }
    // the sample's position; `writer` lanes (lane half 0 of a real sample) leave z_vals, points_out and, at s == 0, rays_d_out
    __device__ __forceinline__ void position(const TrainRaysDev& R, int64_t sid, bool writer, float (&p)[3]) const {
        float o[3], d[3];
        origin_dir(R, o, d);
        const float z = depth(R, sid);
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = point_on_ray(o[k], d[k], z);
        if (writer) {
            R.z_vals[sid] = z;
            if (R.points_out) {
#pragma unroll
                for (int k = 0; k < 3; ++k) R.points_out[sid * 3 + k] = p[k];
            }
            if (R.rays_d_out && s == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) R.rays_d_out[(int64_t)ray * 3 + k] = d[k];
            }
        }
    }
};

__device__ __forceinline__ i32x4* mask_ptr(const TrainKArgs& P, int mslot, int64_t st, int lane) {
    return (i32x4*)(P.ctx + P.mask_off[mslot] + st * (int64_t)kMaskBytes + lane * 16);
}

template <class Mode>
__device__ __forceinline__ char* tile_ptr(const TrainKArgs& P, int slot, int64_t st, int t, int lane) {
    return P.ctx + P.slot_off[slot] + ((st * P.slot_tiles[slot] + t) * (int64_t)tile_bytes<Mode>()) + lane * 16;
}

// ---------------------------------------------------------------------------------------------
// the chain kernels' building blocks (slots and planes: train_slots.hpp)
// ---------------------------------------------------------------------------------------------
// One wave's 32-sample tile of a chain kernel.  `bias` is the bias table in the saving forward chains and 32 * 8 zeros in the
// dZ chains, which have no bias (their accumulators start at 0, boff stays 0).
template <class Mode, int WAVES>
struct ChainTile {
    typedef typename Mode::Act Act;
    typedef ActIO<Mode> IO;
    typedef Act Tiles[8][1];              // 256 features
    const TrainKArgs& P;
    Pipe<WAVES>& pipe;
    const NRF_LDS float* bias;
    const int lane, c, h;
    const int64_t st, raw, sid;           // sample tile; this lane's sample; the sample it reads (past the end: the last one)
    // dZ chains: ReLU' of the layer being produced, from the forward's bit planes (train_core.hpp), and that of the layer after
    // it, loaded one layer ahead of its use
    i32x4 mcur, mnext;

    __device__ __forceinline__ ChainTile(const TrainKArgs& P_, Pipe<WAVES>& pipe_, const NRF_LDS float* bias_, int lane_, int c_, int h_,
                                         int64_t st_)
        : P(P_), pipe(pipe_), bias(bias_), lane(lane_), c(c_), h(h_), st(st_), raw(st_ * 32 + c_), sid(raw < P_.n ? raw : P_.n - 1) {}

    __device__ __forceinline__ void save(int slot, int t, const Act& a) const { IO::store_g(tile_ptr<Mode>(P, slot, st, t, lane), a); }
    __device__ __forceinline__ i32x4 bits(int plane) const { return *mask_ptr(P, plane, st, lane); }

    // Linear + ReLU: out = relu(W in + b), saved into `slot`, its ReLU bits into `plane`
    template <int KT, int MT>
    __device__ __forceinline__ void relu_layer(const Act (&in)[KT][1], Act (&out)[MT][1], int slot, int plane, int boff) {
        i32x4 mw = {};
        dense<Mode, KT, MT, 1>(pipe, bias + boff, h, in, [&](auto m_, f32x16(&acc)[1]) {
            constexpr int m = decltype(m_)::value;
            out[m][0] = Mode::template to_act<true>(acc[0]);
            __builtin_amdgcn_sched_barrier(0);   // relu_bits is inline asm: it must come after a compiler-visible read of the accumulators (MFMA -> VALU hazard)
            put_bits<m>(mw, relu_bits(acc[0]));
            save(slot, m, out[m][0]);
            if constexpr (m == MT - 1) *mask_ptr(P, plane, st, lane) = mw;
        });
    }
    // Linear without activation (feature_head, output_proj; in the dZ chains: the transpose of a layer that had none),
    // MT output tiles into out[0 .. MT-1], saved into `slot`
    template <int MT, int KT, int NO>
    __device__ __forceinline__ void linear(const Act (&in)[KT][1], Act (&out)[NO][1], int slot, int boff) {
        dense<Mode, KT, MT, 1>(pipe, bias + boff, h, in, [&](auto m_, f32x16(&acc)[1]) {
            constexpr int m = decltype(m_)::value;
            out[m][0] = Mode::template to_act<false>(acc[0]);
            save(slot, m, out[m][0]);
        });
    }
    // dZ chain: dZ = (W^T in) under the ReLU bits in mcur, saved into `slot`
    template <int KT, int MT>
    __device__ __forceinline__ void masked_layer(const Act (&in)[KT][1], Act (&out)[MT][1], int slot) {
        dense<Mode, KT, MT, 1>(pipe, bias, h, in, [&](auto m_, f32x16(&acc)[1]) {
            constexpr int m = decltype(m_)::value;
            out[m][0] = masked_act<Mode, m>(acc[0], mcur);
            save(slot, m, out[m][0]);
        });
    }

    // Forward trunk: layers j .. end-1 (8 -> 8 tiles, Linear + ReLU, bias at boff, which moves past them), ping-ponging
    // between A and B from A, each saved into s.trunk(j) / s.plane(j).  then(X) continues on the buffer holding the last
    // output: a compile-time choice, so that neither buffer is indexed at run time.
    template <class S, class Then>
    __device__ __forceinline__ void trunk_forward(const S& s, int j, int end, Tiles& A, Tiles& B, int& boff, Then&& then) {
        auto layer = [&](const Tiles& in, Tiles& out) {
            relu_layer(in, out, s.trunk(j), s.plane(j), boff);
            ++j;
            boff += 32 * 8;
        };
        const int count = end - j;
        for (int p = 0; p < count / 2; ++p) {
            layer(A, B);
            layer(B, A);
        }
        if (count & 1) {
            layer(A, B);
            then(B);
        } else {
            then(A);
        }
    }
    // dZ chain through the trunk of n layers: top (head^T, or [feature_head | density_head]^T) -> dZ of layer n-1 into A under
    // mcur, then layer j^T -> dZ of layer j-1 down to dZ of layer 0, each under bits loaded while the layer before runs.
    // then(X, Y): X holds dZ of layer 0, Y is the other buffer (compile-time choice, as in trunk_forward).
    template <class S, int KT, class Then>
    __device__ __forceinline__ void trunk_backward(const S& s, int n, const Act (&top)[KT][1], Tiles& A, Tiles& B, Then&& then) {
        int below = n - 2;                // trunk layer whose bits come next
        auto prefetch = [&]() { if (below >= 0) mnext = bits(s.plane(below)); --below; };
        prefetch();
        masked_layer(top, A, s.dz_trunk(n - 1));
        mcur = mnext;
        const int hidden = n - 1;
        int j = n - 2;                    // the layer whose dZ is produced
        auto layer = [&](const Tiles& in, Tiles& out) {
            prefetch();
            masked_layer(in, out, s.dz_trunk(j));
            mcur = mnext;
            --j;
        };
        for (int p = 0; p < hidden / 2; ++p) {
            layer(A, B);
            layer(B, A);
        }
        if (hidden & 1) {
            masked_layer(A, B, s.dz_trunk(j));
            then(B, A);
        } else {
            then(A, B);
        }
    }

    // V2 / V3 colour branch on the trunk output X (nets.hpp:NetV2::tail with stores): density_head, feature_head, PE(dir),
    // colour layers 0 / 2 / 4, with the bias of density_head at boff; write_rgb_density() stores the results.  Src: the kernel's
    // input source -- the sample's direction is row sid of P.dir or that of its ray in *rays (IndexedRayInputs: of sample index[sid],
    // asked for again here rather than held through the trunk, as the ray is).
    template <int LD, class Src = StagedInputs>
    __device__ __forceinline__ void colour_forward(const ColourSlots& cs, const Tiles& X, int boff, float& dens_raw, float (&logit)[3],
                                                   const TrainRaysDev* rays = nullptr, const int32_t* index = nullptr) {
        {
            f32x16 dens[1];
            dense_head<Mode, 8, 1>(pipe, bias + boff, h, X, dens);
            dens_raw = dens[0][0];
        }
        Act in9[9][1];
        linear<8>(X, in9, cs.in(), boff + 32);
        {
            float dd[3];
            if constexpr (Src::kIndexed) {
                RaySample(*rays, index[sid]).dir(*rays, dd);
            } else if constexpr (Src::kRays) {
                RaySample(*rays, sid).dir(*rays, dd);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) dd[k] = P.dir[sid * 3 + k];
            }
            Act t1[pe_tiles(LD)];
            encode3<Mode, LD>(dd, h, t1);
            in9[8][0] = t1[0];
            save(cs.in(), 8, t1[0]);
        }
        Act c0[4][1], c1[2][1];
        relu_layer(in9, c0, cs.c0(), cs.plane_c0(), boff + 32 + 32 * 8);
        relu_layer(c0, c1, cs.c2(), cs.plane_c2(), boff + 32 + 32 * 8 + 16 * 8);
        f32x16 rgb[1];
        dense_head<Mode, 2, 1>(pipe, bias + boff + 32 + 32 * 8 + 16 * 8 + 8 * 8, h, c1, rgb);
        logit[0] = rgb[0][0]; logit[1] = rgb[0][1]; logit[2] = rgb[0][2];
    }
    __device__ __forceinline__ void write_rgb_density(float dens_raw, const float (&logit)[3]) const {
        if (h == 0 && raw < P.n) {
            P.rgb[raw * 3 + 0] = sigmoid_sel<Mode::FAST_EXP>(logit[0]);
            P.rgb[raw * 3 + 1] = sigmoid_sel<Mode::FAST_EXP>(logit[1]);
            P.rgb[raw * 3 + 2] = sigmoid_sel<Mode::FAST_EXP>(logit[2]);
            P.density[raw] = fmaxf(dens_raw, 0.0f);                                 // nerf_mlp.py:63
        }
    }
    // V2 / V3 colour branch, dZ chain: d rgb -> d logits (sigmoid'), relu' of density_head, colour layers 4^T and 2^T under
    // their bits, 0^T (feature columns) without: feature_vec has no activation.  Leaves in9 = [d feature_vec | dZ density_head],
    // the operand of the trunk's top layer, and mcur = the bits of trunk plane top_plane.
    __device__ __forceinline__ void colour_backward(const ColourSlots& cs, int top_plane, Act (&in9)[9][1]) {
        mcur = bits(cs.plane_c2());
        mnext = bits(cs.plane_c0());
        Act G[1][1], d1[2][1], d0[4][1];
        {
            f32x16 e = {};
            float ds = 0.0f;
            if (h == 0 && raw < P.n) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float o = P.rgb[raw * 3 + k];
                    e[k] = P.g_rgb[raw * 3 + k] * o * (1.0f - o);
                }
                ds = P.density[raw] > 0.0f ? P.g_density[raw] : 0.0f;          // relu' of density_head (nerf_mlp.py:63)
            }
            G[0][0] = Mode::template to_act<false>(e);
            save(cs.d_logits(), 0, G[0][0]);
            f32x16 e2 = {};
            e2[0] = ds;
            in9[8][0] = Mode::template to_act<false>(e2);
            save(cs.dz_density(), 0, in9[8][0]);
        }
        masked_layer(G, d1, cs.dz_c2());
        mcur = mnext;
        mnext = bits(top_plane);
        masked_layer(d1, d0, cs.dz_c0());
        mcur = mnext;
        linear<8>(d0, in9, cs.d_feature(), 0);
    }
};

// The frame of every chain kernel: the LDS carve-out, the bias table (FORWARD) or the zero bias of the dZ chains, the weight
// pipe, and the persistent walk over this workgroup's tiles; body(T) runs one tile of this wave (a ChainTile).
template <class Mode, int WAVES, bool FORWARD, class Body>
__device__ __forceinline__ void chain_kernel(const TrainKArgs& P, Body&& body) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    NRF_LDS char* lds = (NRF_LDS char*)smem;
    NRF_LDS float* bias = (NRF_LDS float*)(lds + kLdsRing);
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if constexpr (FORWARD) {
        load_bias_table(bias, P.net.bias, P.net.n_bias);
    } else {
        for (int i = threadIdx.x; i < 32 * 8; i += blockDim.x) bias[i] = 0.0f;
        __syncthreads();
    }
    Pipe<WAVES> pipe;
    pipe.init(P.net.stream, P.net.n_chunks, lds);
    pipe.start();
    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        ChainTile<Mode, WAVES> T(P, pipe, bias, lane, c, h, tile * WAVES + wave);
        body(T);
    }
    pipe.drain();
}

namespace {

// The launch body of every family's chain launchers (train_v*.hip): F::check, then the chain kernel
// F::forward<ChainGeo> / F::backward<ChainGeo> at the mode's geometry; the dZ chains stream the transposed weights and are
// followed by the weight gradients.
template <class F, bool FORWARD, class Src = StagedInputs>
int run_chain(const DeviceNet& net, const TrainDev& t, int mode, typename Src::KArgs k, float* grad, hipStream_t s, std::string& err) {
    if (!F::check(net, t, mode, err)) return NRF_EINVAL;
    const int64_t n = k.n;
    if (n <= 0) return NRF_OK;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const int r = dispatch_chain(net, mode, n, [&](auto g) {
        typedef decltype(g) G;
        if constexpr (FORWARD && Src::kIndexed)
            return launch_persistent<F::template forward_indexed<G>, G::kWaves>(net, net_args(net, mode), k, tiles32(n) / G::kWaves, s,
                                                                                "train forward (indexed rays)", err);
        else if constexpr (FORWARD && Src::kRays)
            return launch_persistent<F::template forward_rays<G>, G::kWaves>(net, net_args(net, mode), k, tiles32(n) / G::kWaves, s,
                                                                             "train forward (rays)", err);
        else if constexpr (FORWARD)
            return launch_persistent<F::template forward<G>, G::kWaves>(net, net_args(net, mode), k, tiles32(n) / G::kWaves, s, "train forward", err);
        else
            return launch_persistent<F::template backward<G>, G::kWaves>(net, backward_net_args(net, t, mode), k, tiles32(n) / G::kWaves, s,
                                                                         "train backward", err);
    });
    if (FORWARD || r != NRF_OK) return r;
    return launch_weight_grad(net, t, mode, k, grad, s, err);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// V1 forward
// ---------------------------------------------------------------------------------------------
template <class Mode, int WAVES, int LP, class Src>
__device__ __forceinline__ void train_forward_body(const typename Src::KArgs& P) {
    typedef typename Mode::Act Act;
    constexpr int KT0 = pe_tiles(LP), PE = pe_dim(LP);
    chain_kernel<Mode, WAVES, true>(P, [&](ChainTile<Mode, WAVES>& T) {
        const int h = T.h;
        Act A[8][1], B[8][1];
        if constexpr (Src::kRays) {                              // the encoding of the fused renderer's V1 (nets.hpp:encode3) in place of a (n,63) tensor
            float p[3];
            if constexpr (Src::kIndexed) {
                const int64_t id = P.index[T.sid];
                RaySample(P.rays, id).position_kept(P.rays, id, p);
            } else {
                RaySample(P.rays, T.sid).position(P.rays, T.sid, h == 0 && T.raw < P.n, p);
            }
            Act e1[KT0], enc[KT0][1];
            encode3<Mode, LP>(p, h, e1);
#pragma unroll
            for (int t = 0; t < KT0; ++t) {
                enc[t][0] = e1[t];
                T.save(SlotsV1::input(), t, e1[t]);
            }
            T.relu_layer(enc, A, SlotsV1::trunk(0), SlotsV1::plane(0), 0);
        } else {
            Act enc[KT0][1];
            const float* xin = P.x_enc + T.sid * PE;
            f32x16 e[KT0];
            static_for<16 * KT0>([&](auto u_) {                  // positional_encoding.py order -> operand order (feature_map.hpp)
                constexpr int u = decltype(u_)::value;
                constexpr int i0 = pe_ref_index(LP, u, 0), i1 = pe_ref_index(LP, u, 1);
                float val = 0.0f;
                if constexpr (i0 >= 0 && i1 >= 0) val = xin[h ? i1 : i0];
                else if constexpr (i0 >= 0) val = h ? 0.0f : xin[i0];
                else if constexpr (i1 >= 0) val = h ? xin[i1] : 0.0f;
                e[u / 16][u % 16] = val;
            });
#pragma unroll
            for (int t = 0; t < KT0; ++t) {
                enc[t][0] = Mode::template to_act<false>(e[t]);
                T.save(SlotsV1::input(), t, enc[t][0]);
            }
            T.relu_layer(enc, A, SlotsV1::trunk(0), SlotsV1::plane(0), 0);
        }
        const SlotsV1 S{P.net.n_layers};
        int boff = 32 * 8;
        f32x16 head[1];
        T.trunk_forward(S, 1, S.n, A, B, boff, [&](const Act (&X)[8][1]) { dense_head<Mode, 8, 1>(T.pipe, T.bias + boff, h, X, head); });
        if (h == 0 && T.raw < P.n) {
            const float r = sigmoid_sel<Mode::FAST_EXP>(head[0][0]), g = sigmoid_sel<Mode::FAST_EXP>(head[0][1]),
                        b = sigmoid_sel<Mode::FAST_EXP>(head[0][2]);
            *(float4*)(P.out4 + T.raw * 4) = make_float4(r, g, b, head[0][3]);      // nerf_model.py:22-24
        }
    });
}

template <class Mode, int WAVES, int LP>
__global__ void __launch_bounds__(WAVES * 64) train_forward_kernel(const TrainKArgs P) {
    train_forward_body<Mode, WAVES, LP, StagedInputs>(P);
}

template <class Mode, int WAVES, int LP>
__global__ void __launch_bounds__(WAVES * 64) train_forward_rays_kernel(const TrainRayKArgs P) {
    train_forward_body<Mode, WAVES, LP, RayInputs>(P);
}

template <class Mode, int WAVES, int LP>
__global__ void __launch_bounds__(WAVES * 64) train_forward_rays_indexed_kernel(const TrainRayIndexKArgs P) {
    train_forward_body<Mode, WAVES, LP, IndexedRayInputs>(P);
}

// ---------------------------------------------------------------------------------------------
// V1 backward chain
// ---------------------------------------------------------------------------------------------
template <class Mode, int WAVES, int LP>
__global__ void __launch_bounds__(WAVES * 64) train_backward_kernel(const TrainKArgs P) {
    typedef typename Mode::Act Act;
    chain_kernel<Mode, WAVES, false>(P, [&](ChainTile<Mode, WAVES>& T) {
        const SlotsV1 S{P.net.n_layers};
        T.mcur = T.mnext = T.bits(S.plane(S.n - 1));
        Act G[1][1];
        {   // d out4 -> d [rgb logits, sigma]: rows 0..3 of one operand tile (registers 0..3 of lane half 0)
            f32x16 e = {};
            if (T.h == 0 && T.raw < P.n) {
                const float4 o = *(const float4*)(P.out4 + T.raw * 4);
                const float4 g = *(const float4*)(P.g_out4 + T.raw * 4);
                e[0] = g.x * o.x * (1.0f - o.x);                                    // sigmoid'
                e[1] = g.y * o.y * (1.0f - o.y);
                e[2] = g.z * o.z * (1.0f - o.z);
                e[3] = g.w;                                                         // sigma_out has no activation
            }
            G[0][0] = Mode::template to_act<false>(e);
            T.save(S.dz_head(), 0, G[0][0]);
        }
        Act A[8][1], B[8][1];
        T.trunk_backward(S, S.n, G, A, B, [](const Act (&)[8][1], const Act (&)[8][1]) {});
    });
}

// ---------------------------------------------------------------------------------------------
// weight gradients
// ---------------------------------------------------------------------------------------------
struct GradJob {
    int64_t x_off, dz_off;      // slot bases inside the context
    int KT, MT;                 // feature tiles of X / of dZ used by this job
    int x_stride, dz_stride;    // feature tiles per sample tile of the two slots
    int x_first;                // first X tile of the window (a Linear fed by a concatenation is split into windows of <= 8 tiles)
    int map_off;                // this job's row_w | row_b | col tables inside `maps` (ints)
};

struct GradKArgs {
    const char* ctx;
    float* partial;             // per-workgroup partial sums (kPartialFloats each), reduced by weight_grad_reduce_kernel
    float* grad;                // flat gradient vector, accumulated into
    const int32_t* maps;
    GradJob jobs[kMaxJobs];
    int first_block[kMaxJobs + 1];   // job j owns workgroups [first_block[j], first_block[j+1]): its slabs of the sample axis
    int n_jobs;
    int64_t n_tiles32;          // 32-sample tiles
};

// One workgroup (8 waves) = one Linear x one slab of samples; its 256 x 256 fp32 output lives in the accumulators
// (wave w: rows 64*(w&3).., columns 128*(w>>2)..).  HBM-bound: 1 KiB of saved operands per sample and layer against
// 131 kFLOP.  Per stage of ST sample tiles, wave w transposes dZ tile w and X tile w of every sample tile on the
// matrix core (train_core.hpp) -- each tile exactly once per workgroup -- and parks the transposed operand tiles in
// LDS, where all waves read the 2 + 4 tiles their outputs need; the saved tiles of the next stage are already in
// flight (registers) while the current one is multiplied.  Two LDS buffers, one barrier per stage.  (Two stages in flight per
// wave measured the same: profiles/r03_ab_wgrad_prefetch.txt.)
template <class Mode, int ST>
__global__ void __launch_bounds__(512) weight_grad_kernel(const GradKArgs P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename Mode::Act Act;
    typedef ActIO<Mode> IO;
    constexpr int RT = 2, CT = 4;
    constexpr int TB = tile_bytes<Mode>();
    constexpr int kStageBytes = ST * 16 * TB;
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int job = 0;
    while (job + 1 < P.n_jobs && (int)blockIdx.x >= P.first_block[job + 1]) ++job;
    const int split = blockIdx.x - P.first_block[job], splits = P.first_block[job + 1] - P.first_block[job];
    const GradJob J = P.jobs[job];
    const int row0 = (wave & 3) * RT, col0 = (wave >> 2) * CT;
    const bool has_z = wave < J.MT, has_x = wave < J.KT;            // transposition duty: dZ tile `wave`, X tile `wave`

    Transposer<Mode> tr;
    tr.init(lane);
    f32x16 acc[RT][CT];
    float bsum = 0.0f;
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = f32x16{};

    const int64_t per = (P.n_tiles32 + splits - 1) / splits;
    const int64_t t0 = split * per, t1 = (t0 + per < P.n_tiles32) ? t0 + per : P.n_tiles32;
    const char* xb = P.ctx + J.x_off + lane * 16;
    const char* zb = P.ctx + J.dz_off + lane * 16;
    const Act zero = Mode::template to_act<false>(f32x16{});
    Act rz[ST], rx[ST];
    auto fetch = [&](int64_t st0) {
#pragma unroll
        for (int q = 0; q < ST; ++q) {
            const bool in = st0 + q < t1;
            rz[q] = (in && has_z) ? IO::template load_g<Act>(zb + ((st0 + q) * J.dz_stride + wave) * (int64_t)TB) : zero;
            rx[q] = (in && has_x) ? IO::template load_g<Act>(xb + ((st0 + q) * J.x_stride + J.x_first + wave) * (int64_t)TB) : zero;
        }
    };
    // one stage: transpose + park the registers, refill them with the next stage, multiply
    auto stage_step = [&](int64_t st0, int buf) {
        char* stage = smem + buf * kStageBytes + lane * 16;
#pragma unroll
        for (int q = 0; q < ST; ++q) {
            if (has_z) {
                const f32x16 t = tr.run(rz[q]);
                float s = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) s += t[r];
                bsum += s;
                IO::store(stage + (q * 16 + wave) * TB, Mode::template to_act<false>(t));
            }
            if (has_x) IO::store(stage + (q * 16 + 8 + wave) * TB, Mode::template to_act<false>(tr.run(rx[q])));
        }
        if (st0 + ST < t1) fetch(st0 + ST);                       // the next stage's saved tiles: in flight across the barrier and the MFMAs
        __syncthreads();
#pragma unroll
        for (int q = 0; q < ST; ++q) {
            Act tz[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i)
                if (row0 + i < J.MT) tz[i] = IO::template load<Act>(stage + (q * 16 + row0 + i) * TB);
#pragma unroll
            for (int j = 0; j < CT; ++j) {
                if (col0 + j >= J.KT) continue;
                const Act tx = IO::template load<Act>(stage + (q * 16 + 8 + col0 + j) * TB);
#pragma unroll
                for (int i = 0; i < RT; ++i)
                    if (row0 + i < J.MT) OuterMma<Mode>::run(acc[i][j], tz[i], tx);
            }
        }
    };
    if (t0 < t1) fetch(t0);
    int buf = 0;
    for (int64_t st0 = t0; st0 < t1; st0 += ST) {
        stage_step(st0, buf);
        buf ^= 1;
    }
    // hand the partial sums over: [wave][tile i*CT+j][register group of 4][lane][4 floats], 16 B per lane and store
    float* part = P.partial + (int64_t)blockIdx.x * kPartialFloats;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        if (row0 + i >= J.MT) continue;
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            if (col0 + j >= J.KT) continue;
            f32x4* dst = (f32x4*)(part + ((wave * 8 + i * CT + j) * 16) * 64) + lane;
#pragma unroll
            // plain stores: the 61 MB of partial sums are read back by the very next kernel and fit the MALL (streaming them -- like
            // the saved tiles -- made the reduction 2.4 us slower)
            for (int q = 0; q < 4; ++q) dst[q * 64] = f32x4{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        }
    }
    if (has_z) {                                                   // bias: the wave that transposed dZ tile `wave` summed it
        const float s = bsum + __shfl_xor(bsum, 32, 64);
        if (h == 0) part[8 * 8 * 16 * 64 + 32 * wave + c] = s;
    }
}

}  // namespace nrf
