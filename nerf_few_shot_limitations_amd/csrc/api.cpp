// api.cpp -- the extern "C" surface of libnerfhip.so (include/nerfhip.h).
// Argument checking happens here, on the host, before any kernel is launched: a
// launch only goes out once every shape the kernel and its grid assume has been
// verified.  No C++ exception leaves this file.
// Layout: the model, one namespace of helpers (every check that two entries share stands there once), one extern "C" block.
// An entry looks at what its arguments alone decide first, then at what needs the model, then at the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/nerfhip.h"
#include "freq_mask.hpp"
#include "kernels.hpp"
#include "packing.hpp"
#include "ray_deal.hpp"

struct nrf_model {
    nrf_arch arch{};
    int device = 0;
    nrf::NetPlan plan;
    std::vector<nrf::HostLinear> lin;
    nrf::PackedStream h_stream[nrf::kModes];
    std::vector<float> h_bias;
    void* d_stream[nrf::kModes] = {nullptr, nullptr, nullptr, nullptr};
    float* d_bias = nullptr;
    unsigned long long* d_queues = nullptr;
    nrf::DeviceNet net{};
    // training path (built on first use: ensure_train)
    bool train_ready = false;
    bool lin_stale = false;                 // parameters were last set from a device vector: the host copy `lin` is old
    bool bfresh[3] = {false, false, false}; // backward stream of the mode matches the current parameters
    nrf::ParamLayout layout;
    nrf::NetPlan bplan;                     // the dZ chain's layers, and behind them the post-chain gradient kernels' (ensure_train: the riders):
                                            // one device stream, one gather table, one re-pack, one freshness flag
    nrf::TrainPlan tplan;
    nrf::TrainDev train{};
    void* d_bstream[3] = {nullptr, nullptr, nullptr};
    int32_t* d_maps = nullptr;
    int32_t* d_src[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};   // [forward|backward][packing.hpp stream kind] element sources
    int64_t n_src[2][3] = {{0, 0, 0}, {0, 0, 0}};                                        // (no backward stream in the split mode)
    int32_t* d_bias_src = nullptr;
    // frequency mask (freq_mask.hpp): the recorded one takes effect at the next pack; each mode remembers what its streams were
    // last packed with, and its weight gradients scale with that (train.freq[mode]), so a forward, its backward and its weight
    // gradients always agree
    nrf::FreqMaskArgs freq{};
    bool freq_active = false;
    nrf::FreqMaskArgs freq_packed[nrf::kModes]{};
    bool freq_packed_active[nrf::kModes] = {false, false, false, false};
    int8_t* d_freq_ids = nullptr;
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(NRF_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define NRF_HIP(call)                                    \
    do {                                                 \
        const hipError_t e_ = (call);                    \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

// the last line of an entry: what a launcher returned, with the entry's text (or the launcher's own) on a failure
int launched(int r, const char* what) { return r == NRF_OK ? NRF_OK : fail(r, what); }
int launched(int r, const std::string& what) { return launched(r, what.c_str()); }

// any of the pointers has one of the mask's address bits set (a NULL has none)
bool misaligned(uintptr_t mask, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & mask) != 0;
}

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) return;
        ok = (prev == dev) || (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// what an entry answers when its guard is not ok
int no_device() { return fail(NRF_EHIP, "cannot select the model's device"); }

bool copy_linears(const nrf_linear* in, int n, std::vector<nrf::HostLinear>& out, std::string& err) {
    out.resize(n);
    for (int i = 0; i < n; ++i) {
        if (!in[i].weight || !in[i].bias || in[i].out_f <= 0 || in[i].in_f <= 0) {
            err = "linear " + std::to_string(i) + ": null pointer or non-positive shape";
            return false;
        }
        out[i].out_f = in[i].out_f;
        out[i].in_f = in[i].in_f;
        out[i].w.assign(in[i].weight, in[i].weight + (size_t)in[i].out_f * in[i].in_f);
        out[i].b.assign(in[i].bias, in[i].bias + in[i].out_f);
    }
    return true;
}

nrf::Camera make_camera(int H, int W, float focal, const float c2w[12]) {
    nrf::Camera c;
    c.H = H; c.W = W; c.focal = focal;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) c.r[i][j] = c2w[4 * i + j];
        c.t[i] = c2w[4 * i + 3];
    }
    return c;
}

// the pinhole camera of the entries that generate their rays, and the ray range [ray_begin, ray_end) within its image
int check_camera(int H, int W, float focal, const float* c2w) {
    if (H < 1 || W < 1 || !(focal > 0.0f) || !c2w) return fail(NRF_EINVAL, "bad camera");
    return NRF_OK;
}
int check_ray_range(int H, int W, int64_t ray_begin, int64_t ray_end) {
    if (ray_begin < 0 || ray_end < ray_begin || ray_end > (int64_t)H * W) return fail(NRF_EINVAL, "ray range outside the image");
    return NRF_OK;
}

bool make_dino(const nrf_dino* in, int want_c, nrf::DinoDev& d, std::string& err) {
    if (!in || !in->features) { err = "dino side channel missing (features == NULL)"; return false; }
    if (in->Hp < 1 || in->Wp < 1 || in->C < 1 || in->H < 1 || in->W < 1) { err = "dino: bad map / image size"; return false; }
    if (want_c > 0 && in->C != want_c) { err = "dino: channel count differs from the model's dino_dim"; return false; }
    d.features = in->features; d.Hp = in->Hp; d.Wp = in->Wp; d.C = in->C;
    std::memcpy(d.inv_pose, in->inv_pose, sizeof(float) * 12);
    d.focal = in->focal; d.H = in->H; d.W = in->W;
    return true;
}

// the streams of `mode` now hold the recorded mask
void mark_packed(nrf_model* m, int mode) {
    m->freq_packed[mode] = m->freq;
    m->freq_packed_active[mode] = m->freq_active;
    if (mode < 3) m->train.freq[mode] = m->freq_active ? &m->freq_packed[mode] : nullptr;
}

bool same_mask(const nrf::FreqMaskArgs& a, const nrf::FreqMaskArgs& b) { return std::memcmp(a.scale, b.scale, sizeof(a.scale)) == 0; }

// what the host packer reads: the Linears themselves, or under a mask a copy with the masked columns multiplied in fp32
const std::vector<nrf::HostLinear>& pack_source(const nrf_model* m, bool active, const nrf::FreqMaskArgs& f, std::vector<nrf::HostLinear>& scaled) {
    if (!active) return m->lin;
    scaled = m->lin;
    nrf::freq_scale_linears(m->arch, scaled, f.scale);
    return scaled;
}

int upload(nrf_model* m, hipStream_t s, bool allocate) {
    std::vector<nrf::HostLinear> scaled;
    const std::vector<nrf::HostLinear>& lin = pack_source(m, m->freq_active, m->freq, scaled);
    for (int mode = 0; mode < nrf::kModes; ++mode) {
        m->h_stream[mode] = nrf::pack_stream(m->plan, lin, mode);
        const size_t bytes = m->h_stream[mode].bytes.size();
        if (allocate) NRF_HIP(hipMalloc(&m->d_stream[mode], bytes));
        NRF_HIP(hipMemcpyAsync(m->d_stream[mode], m->h_stream[mode].bytes.data(), bytes, hipMemcpyHostToDevice, s));
        m->net.stream[mode] = m->d_stream[mode];
        m->net.n_chunks[mode] = m->h_stream[mode].n_chunks;
        mark_packed(m, mode);
    }
    m->lin_stale = false;
    if (m->train_ready) {
        for (int mode = 0; mode < 3; ++mode) {
            const nrf::PackedStream ps = nrf::pack_stream(m->bplan, lin, mode);         // (with the W0d^T layer: ensure_train)
            NRF_HIP(hipMemcpyAsync(m->d_bstream[mode], ps.bytes.data(), ps.bytes.size(), hipMemcpyHostToDevice, s));
            NRF_HIP(hipStreamSynchronize(s));
            m->bfresh[mode] = true;
        }
    }
    m->h_bias = nrf::pack_bias(m->plan, m->lin);
    if (allocate) NRF_HIP(hipMalloc((void**)&m->d_bias, m->h_bias.size() * sizeof(float)));
    if (allocate) {
        NRF_HIP(hipMalloc((void**)&m->d_queues, nrf::kQueueSlots * sizeof(unsigned long long)));
        m->net.queues = m->d_queues;
    }
    NRF_HIP(hipMemcpyAsync(m->d_bias, m->h_bias.data(), m->h_bias.size() * sizeof(float), hipMemcpyHostToDevice, s));
    NRF_HIP(hipStreamSynchronize(s));     // pageable staging: the host vectors may be re-packed right after
    m->net.bias = m->d_bias;
    m->net.n_bias = m->plan.n_bias;
    m->net.flops_per_sample = m->plan.flops_per_sample;
    return NRF_OK;
}

// device-side element sources of the forward streams + bias table (needed by nrf_model_update_device)
int ensure_sources(nrf_model* m) {
    if (m->d_src[0][0]) return NRF_OK;
    m->layout = nrf::param_layout(m->lin);
    for (int kind = 0; kind < 3; ++kind) {
        const std::vector<int32_t> src = nrf::stream_sources(m->plan, m->layout, kind);
        NRF_HIP(hipMalloc((void**)&m->d_src[0][kind], src.size() * sizeof(int32_t)));
        NRF_HIP(hipMemcpy(m->d_src[0][kind], src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        m->n_src[0][kind] = (int64_t)src.size();
    }
    const std::vector<int32_t> bsrc = nrf::bias_sources(m->plan, m->layout);
    NRF_HIP(hipMalloc((void**)&m->d_bias_src, bsrc.size() * sizeof(int32_t)));
    NRF_HIP(hipMemcpy(m->d_bias_src, bsrc.data(), bsrc.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // flat parameter index -> scale id of the frequency mask: one table for every segment of the masked re-pack and for the
    // masked weight-gradient reduce
    const std::vector<int8_t> ids = nrf::freq_scale_ids(m->arch, m->layout);
    NRF_HIP(hipMalloc((void**)&m->d_freq_ids, ids.size()));
    NRF_HIP(hipMemcpy(m->d_freq_ids, ids.data(), ids.size(), hipMemcpyHostToDevice));
    m->freq.ids = m->d_freq_ids;
    for (int mode = 0; mode < nrf::kModes; ++mode) m->freq_packed[mode].ids = m->d_freq_ids;
    return NRF_OK;
}

// backward streams, weight-gradient maps: everything the training kernels need beyond the forward model
int ensure_train(nrf_model* m) {
    if (m->train_ready) return NRF_OK;
    int rc = ensure_sources(m);
    if (rc != NRF_OK) return rc;
    std::string err;
    if (!nrf::make_backward_plan(m->arch, m->lin, m->bplan, err) || !nrf::make_train_plan(m->arch, m->plan, m->layout, m->tplan, err))
        return fail(NRF_EUNSUPPORTED, err);
    if ((int)m->tplan.slot_tiles.size() > nrf::kMaxSlots || (int)m->tplan.jobs.size() > nrf::kMaxJobs || m->tplan.n_mask_slots > nrf::kMaxMaskSlots)
        return fail(NRF_EUNSUPPORTED, "network too deep for the training path");
    // The riders: layers of the post-chain gradient kernels (train_post_grad_core.hpp) behind the chain's layers in the same
    // stream -- the chain kernels wrap at n_bchunks and never see them.  First (V3) W0d^T of dino_grad_kernel, then the input
    // gradient's: W0^T and (V2) color_layers.0^T restricted to the encodings (train_input_grad_impl.hpp), on V3 W0p^T and
    // color_layers.0^T's direction tile (train_input_grad_v3_impl.hpp).
    const bool v3 = m->arch.net == NRF_NET_V3;
    nrf::NetPlan gplan, iplan;
    if (v3 && !nrf::make_dino_grad_plan(m->arch, m->lin, gplan, err)) return fail(NRF_EUNSUPPORTED, err);
    if (!(v3 ? nrf::make_input_grad_v3_plan : nrf::make_input_grad_plan)(m->arch, m->lin, iplan, err)) return fail(NRF_EUNSUPPORTED, err);
    std::vector<int> rider_frags16;              // 16-bit fragments of each rider; the first gplan.layers.size() are gstream's
    for (const nrf::NetPlan* p : {&gplan, &iplan})
        for (const nrf::LayerPlan& L : p->layers) {
            rider_frags16.push_back(L.MT * L.KT * 2);
            m->bplan.layers.push_back(L);
        }
    for (int mode = 0; mode < 3; ++mode) {
        // under the mask the mode's forward stream holds; current only if that is also the recorded one
        std::vector<nrf::HostLinear> scaled;
        const nrf::PackedStream ps = nrf::pack_stream(m->bplan, pack_source(m, m->freq_packed_active[mode], m->freq_packed[mode], scaled), mode);
        NRF_HIP(hipMalloc(&m->d_bstream[mode], ps.bytes.size()));
        NRF_HIP(hipMemcpy(m->d_bstream[mode], ps.bytes.data(), ps.bytes.size(), hipMemcpyHostToDevice));
        // 16 fragments per chunk, twice the fragments in fp32; every layer starts on a chunk boundary (packing.cpp:stream_sources)
        uint32_t g_chunks = 0, i_chunks = 0;
        for (size_t r = 0; r < rider_frags16.size(); ++r)
            (r < gplan.layers.size() ? g_chunks : i_chunks) += (uint32_t)((rider_frags16[r] * (mode == NRF_MMA_F32 ? 2 : 1) + 15) / 16);
        m->train.bstream[mode] = m->d_bstream[mode];
        m->train.n_bchunks[mode] = ps.n_chunks - g_chunks - i_chunks;
        m->train.gstream[mode] = g_chunks ? static_cast<const char*>(m->d_bstream[mode]) + (size_t)m->train.n_bchunks[mode] * 16 * 1024 : nullptr;
        m->train.istream[mode] = i_chunks ? static_cast<const char*>(m->d_bstream[mode]) + ((size_t)m->train.n_bchunks[mode] + g_chunks) * 16 * 1024 : nullptr;
        m->bfresh[mode] = !m->lin_stale && same_mask(m->freq_packed[mode], m->freq);
        m->train.freq[mode] = m->freq_packed_active[mode] ? &m->freq_packed[mode] : nullptr;
    }
    for (int f32 = 0; f32 < 2; ++f32) {
        const std::vector<int32_t> src = nrf::stream_sources(m->bplan, m->layout, f32);
        NRF_HIP(hipMalloc((void**)&m->d_src[1][f32], src.size() * sizeof(int32_t)));
        NRF_HIP(hipMemcpy(m->d_src[1][f32], src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        m->n_src[1][f32] = (int64_t)src.size();
    }
    const int nj = (int)m->tplan.jobs.size();
    std::vector<int32_t> maps((size_t)nj * nrf::kMapStride, -1);
    for (int j = 0; j < nj; ++j) {
        const nrf::GradJobPlan& J = m->tplan.jobs[j];
        if (J.row_w.size() > 320 || J.col.size() > 320) return fail(NRF_EUNSUPPORTED, "layer too wide for the weight-gradient maps");
        std::copy(J.row_w.begin(), J.row_w.end(), maps.begin() + (size_t)j * nrf::kMapStride);
        std::copy(J.row_b.begin(), J.row_b.end(), maps.begin() + (size_t)j * nrf::kMapStride + 320);
        std::copy(J.col.begin(), J.col.end(), maps.begin() + (size_t)j * nrf::kMapStride + 640);
        m->train.job_x_slot[j] = J.x_slot; m->train.job_dz_slot[j] = J.dz_slot; m->train.job_KT[j] = J.KT; m->train.job_MT[j] = J.MT; m->train.job_x_first[j] = J.x_first;
    }
    NRF_HIP(hipMalloc((void**)&m->d_maps, maps.size() * sizeof(int32_t)));
    NRF_HIP(hipMemcpy(m->d_maps, maps.data(), maps.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    m->train.maps = m->d_maps;
    m->train.n_jobs = nj;
    m->train.n_slots = (int)m->tplan.slot_tiles.size();
    for (int i = 0; i < m->train.n_slots; ++i) m->train.slot_tiles[i] = m->tplan.slot_tiles[i];
    m->train.n_mask_slots = m->tplan.n_mask_slots;
    m->train.aux_floats = m->tplan.aux_floats;
    m->train.cu_count = m->net.cu_count;
    m->train.n_params = m->layout.total;
    m->train_ready = true;
    return NRF_OK;
}

int check_opts(const nrf_render_opts* o) {
    if (!o) return fail(NRF_EINVAL, "opts is NULL");
    if (o->n_samples < 1 || o->n_samples > 4096) return fail(NRF_EINVAL, "n_samples must be in 1..4096");
    if (!(o->near > 0.0f) || !(o->far > o->near) || !std::isfinite(o->far)) return fail(NRF_EINVAL, "need 0 < near < far");
    if (o->mma_mode < 0 || o->mma_mode >= nrf::kModes) return fail(NRF_EINVAL, "unknown mma_mode");
    if (!(o->ert_eps >= 0.0f) || o->ert_eps >= 1.0f) return fail(NRF_EINVAL, "ert_eps must be in [0,1)");
    return NRF_OK;
}

// out_rgbd rows are written with one 16-byte store per ray: refuse a misaligned base before anything else of the render is looked at
// (only the grid of an _occ entry comes in front of it; a C caller passing a float-aligned sub-view would otherwise get a GPU memory
// fault instead of an error code)
bool rgbd_misaligned(const nrf_render_opts* o, const float* rgb) {
    return o && o->out_rgbd && rgb && (reinterpret_cast<uintptr_t>(rgb) & 15u) != 0;
}
const char* const kRgbdAlign = "out_rgbd: rgb must be 16-byte aligned ((R,4) rows written with one 16-byte store per ray)";

void fill_common(nrf::RenderArgs& a, const nrf_render_opts* o, float* rgb, float* depth, float* weights, float* z_vals) {
    a.near = o->near; a.far = o->far; a.n_samples = o->n_samples; a.lindisp = o->lindisp; a.perturb = o->perturb;
    a.t_rand = o->perturb ? o->t_rand : nullptr; a.z_ladder = o->z_ladder; a.z_in = o->z_in; a.seed = o->rng_seed;
    a.ert_eps = o->ert_eps; a.white_bkgd = o->white_bkgd;
    a.interleaved = o->out_rgbd ? 1 : 0;
    a.rgb = rgb; a.depth = depth; a.weights = weights; a.z_vals = z_vals;
}

// the tail description of a *_tail entry point against the call's options and ray count (nerfhip.h: nrf_tail)
int check_tail(const nrf_render_opts* o, const nrf_tail* t, int64_t n_rays) {
    if (!t) return fail(NRF_EINVAL, "tail is NULL");
    if (t->mode != NRF_MMA_F16X3) return fail(NRF_EINVAL, "tail mode must be NRF_MMA_F16X3");
    if (o->mma_mode != NRF_MMA_BF16 && o->mma_mode != NRF_MMA_F16)
        return fail(NRF_EINVAL, "a tail render needs a 16-bit base mode (NRF_MMA_BF16 or NRF_MMA_F16): the parity modes have no last-sample flips to repair");
    if (o->ert_eps > 0.0f) return fail(NRF_EINVAL, "a tail render takes ert_eps == 0: the ray-queue kernel is not part of the tail mode");
    if (!t->workspace) return fail(NRF_EINVAL, "tail workspace is NULL");
    if (misaligned(15, {t->workspace})) return fail(NRF_EINVAL, "tail workspace must be 16-byte aligned");
    if (t->workspace_bytes < nrf_render_tail_bytes(n_rays)) return fail(NRF_EINVAL, "tail workspace smaller than nrf_render_tail_bytes");
    return NRF_OK;
}

// the box of a grid (nerfhip.h: nrf_occupancy): res, lo and scale as the render entry points and the marking entry points take them
int check_occ_box(const int32_t res[3], const float lo[3], const float scale[3]) {
    for (int k = 0; k < 3; ++k) {
        if (res[k] < 1 || res[k] > 512) return fail(NRF_EINVAL, "nrf_occupancy: res must be in 1..512 on every axis");
        if (!std::isfinite(lo[k])) return fail(NRF_EINVAL, "nrf_occupancy: lo must be finite");
        if (!std::isfinite(scale[k]) || !(scale[k] > 0.0f)) return fail(NRF_EINVAL, "nrf_occupancy: scale must be finite and > 0");
    }
    if (res[0] % 32 != 0) return fail(NRF_EINVAL, "nrf_occupancy: res[0] must be a multiple of 32");
    return NRF_OK;
}

// the grid of a *_occ entry point and the call's ray count (nerfhip.h: nrf_occupancy): everything the arguments alone decide,
// looked at before the model
int check_occ(const nrf_occupancy* g, int64_t n_rays) {
    if (!g) return fail(NRF_EINVAL, "occ is NULL");
    if (g->struct_bytes != (int32_t)sizeof(nrf_occupancy)) return fail(NRF_EINVAL, "nrf_occupancy: struct_bytes is not sizeof(nrf_occupancy)");
    if (g->outside != 0 && g->outside != 1) return fail(NRF_EINVAL, "nrf_occupancy: outside must be 0 (evaluate) or 1 (skip)");
    if (!g->bits || misaligned(3, {g->bits})) return fail(NRF_EINVAL, "nrf_occupancy: bits is NULL or not 4-byte aligned");
    if (check_occ_box(g->res, g->lo, g->scale) != NRF_OK) return NRF_EINVAL;
    if (n_rays >= (int64_t)1 << 31) return fail(NRF_EINVAL, "a render with a grid runs on the ray queue: launch too large (>= 2^31 rays)");
    return NRF_OK;
}

nrf::OccDev make_occ(const nrf_occupancy* g) {
    nrf::OccDev d{};
    d.bits = g->bits; d.outside = g->outside; d.stats = g->stats;
    for (int k = 0; k < 3; ++k) { d.res[k] = g->res[k]; d.lo[k] = g->lo[k]; d.scale[k] = g->scale[k]; }
    return d;
}

// the extra output of the *_emit entry points: raw4 (n_rays, n_samples, 4); raw_only: nothing else is stored
struct EmitOut {
    float* raw4;
    int raw_only;
};

// what the emitting entries refuse, looked at once the options are known to be sane
int check_emit(const nrf_render_opts* o, const EmitOut* e) {
    if (!e->raw4 || misaligned(15, {e->raw4})) return fail(NRF_EINVAL, "raw4 is NULL or not 16-byte aligned (one 16-byte row per sample)");
    if (o->ert_eps > 0.0f) return fail(NRF_EINVAL, "an emitting render takes ert_eps == 0: a terminated ray would leave rows unwritten");
    return NRF_OK;
}

// The opening of the three renders: an emitting call with raw_only stores nothing but raw4 (the other outputs are dropped here and
// `raw_only` says so), out_rgbd wants rgb aligned, and there is a model.
int render_head(const nrf_model* m, const nrf_render_opts* opts, const EmitOut* emit, float*& rgb, float*& depth, float*& weights, float*& z_vals,
                bool& raw_only) {
    raw_only = emit && emit->raw_only;
    if (raw_only) rgb = depth = weights = z_vals = nullptr;
    if (rgbd_misaligned(opts, rgb)) return fail(NRF_EINVAL, kRgbdAlign);
    if (!m) return fail(NRF_EINVAL, "model is NULL");
    return NRF_OK;
}

// The end of the three renders, behind their own checks and their rays in `a`: the options and outputs, the side channel of the
// V3 network, the device, and the launch -- plain, emitting, with a grid, or prefix + tail through the caller's workspace.
int render_tail(const nrf_model* m, const nrf_render_opts* opts, const nrf_tail* tail, const nrf_occupancy* occ, const EmitOut* emit, nrf::RenderArgs& a,
                float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    fill_common(a, opts, rgb, depth, weights, z_vals);
    std::string err;
    if (m->arch.net == NRF_NET_V3 && !make_dino(opts->dino, m->arch.dino_dim, a.dino, err)) return fail(NRF_EINVAL, err);
    DeviceGuard guard(m->device);
    if (!guard.ok) return no_device();
    hipStream_t s = (hipStream_t)stream;
    if (emit) return launched(nrf::launch_render_emit(m->net, opts->mma_mode, a, emit->raw4, s, err), err);
    if (occ) return launched(nrf::launch_render_occ(m->net, opts->mma_mode, a, make_occ(occ), s, err), err);
    if (tail) return launched(nrf::launch_render_tail(m->net, opts->mma_mode, a, static_cast<float*>(tail->workspace), s, err), err);
    return launched(nrf::launch_render(m->net, opts->mma_mode, a, s, err), err);
}

// what the two marking entry points share: everything but the rays (nerfhip.h: nrf_occupancy_mark_rays)
int mark_any(const char* who, const float* rays_o, const float* rays_d, const nrf::Camera* cam, int64_t ray_begin, int64_t n_rays, int n_samples,
             const float* z_vals, const float* weights, const int32_t res[3], const float lo[3], const float scale[3], float weight_threshold,
             float seen_eps, uint32_t* hit_bits, uint32_t* seen_bits, void* stream) {
    const std::string w(who);
    if (n_rays < 0) return fail(NRF_EINVAL, w + ": n_rays < 0");
    if (n_rays >= (int64_t)1 << 31) return fail(NRF_EINVAL, w + ": launch too large (>= 2^31 rays)");
    if (n_samples < 1) return fail(NRF_EINVAL, w + ": n_samples must be >= 1");
    if (!res || !lo || !scale) return fail(NRF_EINVAL, w + ": res, lo or scale is NULL");
    if (check_occ_box(res, lo, scale) != NRF_OK) return NRF_EINVAL;
    if (!std::isfinite(weight_threshold) || weight_threshold < 0.0f) return fail(NRF_EINVAL, w + ": weight_threshold must be finite and >= 0");
    if (!(seen_eps >= 0.0f) || seen_eps >= 1.0f) return fail(NRF_EINVAL, w + ": seen_eps must be in [0,1)");
    if (!hit_bits && !seen_bits) return fail(NRF_EINVAL, w + ": hit_bits and seen_bits are both NULL");
    if (misaligned(3, {hit_bits, seen_bits})) return fail(NRF_EINVAL, w + ": hit_bits / seen_bits must be 4-byte aligned");
    if (!z_vals || !weights) return fail(NRF_EINVAL, w + ": z_vals or weights is NULL");
    if (!cam && (!rays_o || !rays_d)) return fail(NRF_EINVAL, w + ": null ray pointer");
    if (n_rays == 0) return NRF_OK;
    const int r3[3] = {res[0], res[1], res[2]};
    const int r = nrf::launch_occupancy_mark(rays_o, rays_d, cam, ray_begin, n_rays, n_samples, z_vals, weights, r3, lo, scale, weight_threshold,
                                             seen_eps, hit_bits, seen_bits, (hipStream_t)stream);
    return launched(r, "occupancy_mark launch failed");
}

// The three render entry points, plain (tailed == false) and with a tail (nerfhip.h: nrf_tail), which is checked once the call's
// ray count is known.
int render_rays_any(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays, const nrf_render_opts* opts,
                    const nrf_tail* tail, bool tailed, const nrf_occupancy* occ, float* rgb, float* depth, float* weights, float* z_vals, void* stream,
                    const EmitOut* emit = nullptr) {
    bool raw_only;
    if (render_head(m, opts, emit, rgb, depth, weights, z_vals, raw_only) != NRF_OK) return NRF_EINVAL;
    if (n_rays < 0) return fail(NRF_EINVAL, "n_rays < 0");
    if (n_rays == 0) return NRF_OK;
    const int rc = check_opts(opts);
    if (rc != NRF_OK) return rc;
    if (emit && check_emit(opts, emit) != NRF_OK) return NRF_EINVAL;
    if (!rays_o || !rays_d || (!raw_only && (!rgb || (!depth && !opts->out_rgbd)))) return fail(NRF_EINVAL, "nrf_render_rays: null ray or output pointer");
    if ((int64_t)opts->n_samples * n_rays > (int64_t)1 << 40) return fail(NRF_EINVAL, "ray-sample count too large");
    if (tailed && check_tail(opts, tail, n_rays) != NRF_OK) return NRF_EINVAL;
    nrf::RenderArgs a{};
    a.rays_o = rays_o; a.rays_d = rays_d; a.camera_mode = 0; a.ray_begin = 0; a.n_rays = n_rays;
    a.n_cams = 1; a.rays_per_cam = n_rays; a.tile_rays = n_rays; a.tile_stride = 0;
    return render_tail(m, opts, tail, occ, emit, a, rgb, depth, weights, z_vals, stream);
}

int render_camera_any(const nrf_model* m, int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                      const nrf_render_opts* opts, const nrf_tail* tail, bool tailed, const nrf_occupancy* occ, float* rgb, float* depth, float* weights, float* z_vals,
                      void* stream, const EmitOut* emit = nullptr) {
    bool raw_only;
    if (render_head(m, opts, emit, rgb, depth, weights, z_vals, raw_only) != NRF_OK) return NRF_EINVAL;
    if (check_camera(H, W, focal, c2w) != NRF_OK || check_ray_range(H, W, ray_begin, ray_end) != NRF_OK) return NRF_EINVAL;
    if (ray_end == ray_begin) return NRF_OK;
    const int rc = check_opts(opts);
    if (rc != NRF_OK) return rc;
    if (emit && check_emit(opts, emit) != NRF_OK) return NRF_EINVAL;
    if (!raw_only && (!rgb || (!depth && !opts->out_rgbd))) return fail(NRF_EINVAL, "nrf_render_camera: null output pointer");
    if (tailed && check_tail(opts, tail, ray_end - ray_begin) != NRF_OK) return NRF_EINVAL;
    nrf::RenderArgs a{};
    a.camera_mode = 1; a.n_cams = 1; a.cams[0] = make_camera(H, W, focal, c2w); a.ray_begin = ray_begin; a.n_rays = ray_end - ray_begin;
    a.rays_per_cam = a.n_rays; a.tile_rays = a.n_rays; a.tile_stride = 0;
    return render_tail(m, opts, tail, occ, emit, a, rgb, depth, weights, z_vals, stream);
}

int render_cameras_tiles_any(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams, int64_t tile_rays,
                             int64_t first_tile, int64_t tile_step, int64_t n_tiles, const nrf_render_opts* opts, const nrf_tail* tail,
                             bool tailed, const nrf_occupancy* occ, float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    bool raw_only;                                            // (no emitting form: always false)
    if (render_head(m, opts, nullptr, rgb, depth, weights, z_vals, raw_only) != NRF_OK) return NRF_EINVAL;
    if (check_camera(H, W, focal, c2w) != NRF_OK) return NRF_EINVAL;
    if (n_cams < 1 || n_cams > nrf::kMaxCams) return fail(NRF_EINVAL, "n_cams must be in 1..8 per call");
    if (tile_rays < 1 || first_tile < 0 || tile_step < 1 || n_tiles < 0) return fail(NRF_EINVAL, "bad tile description");
    if (n_tiles == 0) return NRF_OK;
    if (first_tile * tile_rays >= (int64_t)H * W) return fail(NRF_EINVAL, "first tile lies outside the image");
    const int rc = check_opts(opts);
    if (rc != NRF_OK) return rc;
    if (!rgb || (!depth && !opts->out_rgbd)) return fail(NRF_EINVAL, "nrf_render_cameras_tiles: null output pointer");
    if (opts->t_rand || opts->z_in) return fail(NRF_EINVAL, "tile rendering takes no per-ray inputs (t_rand and z_in must be NULL)");
    if (tailed && check_tail(opts, tail, n_tiles * tile_rays * n_cams) != NRF_OK) return NRF_EINVAL;
    nrf::RenderArgs a{};
    a.camera_mode = 1; a.n_cams = n_cams;
    for (int c = 0; c < n_cams; ++c) a.cams[c] = make_camera(H, W, focal, c2w + 12 * c);
    a.ray_begin = first_tile * tile_rays; a.rays_per_cam = n_tiles * tile_rays; a.n_rays = a.rays_per_cam * n_cams;
    a.tile_rays = tile_rays; a.tile_stride = tile_step * tile_rays;
    return render_tail(m, opts, tail, occ, nullptr, a, rgb, depth, weights, z_vals, stream);
}

// The prologue of the four training entries, in this order: the model, n and the mode, nothing to do (n == 0), null pointers,
// the entry's family check `wrong` (an error text or NULL), the device, the training set-up, the context size and, before a
// dZ chain, the freshness of the transposed weights; then launch(err).
template <class Wrong, class Launch>
int train_entry(nrf_model* m, int mma_mode, int64_t n, bool null_ptr, int64_t ctx_bytes, bool backward, Wrong&& wrong, Launch&& launch) {
    if (!m) return fail(NRF_EINVAL, "model is NULL");
    if (n < 0 || mma_mode < 0 || mma_mode > 2) return fail(NRF_EINVAL, "bad n / mma_mode (the training path is built for bf16, f16 and f32)");
    if (n == 0) return NRF_OK;
    if (null_ptr) return fail(NRF_EINVAL, "null pointer");
    if (const char* w = wrong()) return fail(NRF_EINVAL, w);
    DeviceGuard guard(m->device);
    if (!guard.ok) return no_device();
    const int rc = ensure_train(m);
    if (rc != NRF_OK) return rc;
    if (ctx_bytes < nrf::train_ctx_bytes(m->train, mma_mode, n)) return fail(NRF_EINVAL, "context buffer smaller than nrf_train_context_bytes");
    if (backward && !m->bfresh[mma_mode])
        return fail(NRF_EINVAL, "backward weights of this mode are older than the parameters: call nrf_model_update_device (with this mode) first");
    std::string err;
    return launched(launch(err), err);
}

const char* any_family() { return nullptr; }      // the V1 entries: the launcher checks the family

// The ray source of the entries that train from rays (nerfhip.h: nrf_train_rays) with the call's options and ray count: what the
// arguments alone decide, in front of the model.  `who` names the entry; two texts differ between the entries: what a training
// step does with every sample (the ert_eps refusal) and the refusal of a missing z_vals.
int check_ray_source(const char* who, const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts, const char* step_does,
                     const char* no_z_vals) {
    if (!rays) return fail(NRF_EINVAL, std::string(who) + ": rays is NULL");
    if (rays->struct_bytes != (int32_t)sizeof(nrf_train_rays)) return fail(NRF_EINVAL, "nrf_train_rays: struct_bytes is not sizeof(nrf_train_rays)");
    if (n_rays < 0) return fail(NRF_EINVAL, std::string(who) + ": n_rays < 0");
    const int rc = check_opts(opts);
    if (rc != NRF_OK) return rc;
    if (opts->ert_eps > 0.0f) return fail(NRF_EINVAL, std::string(who) + " takes ert_eps == 0: a training step " + step_does);
    const bool by_rays = rays->rays_o || rays->rays_d, by_pixels = rays->pixels != nullptr;
    if (by_rays == by_pixels) return fail(NRF_EINVAL, "nrf_train_rays: give either rays_o and rays_d or pixels, not both and not neither");
    if (by_rays && (!rays->rays_o || !rays->rays_d)) return fail(NRF_EINVAL, "nrf_train_rays: rays_o and rays_d come together");
    if (by_pixels && (rays->H < 1 || rays->W < 1 || !(rays->focal > 0.0f))) return fail(NRF_EINVAL, "nrf_train_rays: bad camera for the pixels");
    if (!rays->z_vals) return fail(NRF_EINVAL, no_z_vals);
    if (by_pixels && !rays->rays_d_out) return fail(NRF_EINVAL, "nrf_train_rays: output rays_d_out is required in pixel mode");
    if ((int64_t)opts->n_samples * n_rays > (int64_t)INT32_MAX) return fail(NRF_EINVAL, "ray-sample count too large (n_rays * n_samples < 2^31)");
    return NRF_OK;
}
const char* const kNoZVals = "nrf_train_rays: output z_vals is required";

// The checked ray source as the kernels take it (r.dino is the caller's).  sampling: the call draws the depths and writes the
// nrf_train_rays outputs; without it the kernel takes S from the ladder and reads the depths from z_vals, and the rest stays zero.
void fill_ray_source(nrf::TrainRaysDev& r, const nrf_train_rays* rays, const nrf_render_opts* opts, bool sampling) {
    r.rays_o = rays->rays_o; r.rays_d = rays->rays_d; r.pixels = rays->pixels;
    if (rays->pixels) r.cam = make_camera(rays->H, rays->W, rays->focal, rays->c2w);
    r.lad = nrf::make_ladder(opts->near, opts->far, opts->n_samples, opts->lindisp, opts->z_ladder);
    r.z_vals = rays->z_vals;
    if (!sampling) return;
    r.perturb = opts->perturb; r.t_rand = opts->perturb ? opts->t_rand : nullptr; r.z_in = opts->z_in; r.seed = opts->rng_seed;
    r.rays_d_out = rays->rays_d_out; r.points_out = rays->points_out;
}

// nrf_ray_reg as the launches take it; false (with the message set) on a refusal
bool ray_reg_terms(const nrf_ray_reg* reg, nrf::RayRegTerms& rt) {
    if (!reg) return fail(NRF_EINVAL, "reg is NULL"), false;
    if (reg->struct_bytes != (int32_t)sizeof(nrf_ray_reg)) return fail(NRF_EINVAL, "nrf_ray_reg.struct_bytes is not sizeof(nrf_ray_reg)"), false;
    if (!(reg->dist_weight >= 0.0f) || !(reg->occ_weight >= 0.0f) || !std::isfinite(reg->dist_weight) || !std::isfinite(reg->occ_weight))
        return fail(NRF_EINVAL, "dist_weight and occ_weight must be finite and >= 0"), false;
    if (reg->dist_weight > 0.0f && !(std::isfinite(reg->dist_inv_span) && reg->dist_inv_span > 0.0f))
        return fail(NRF_EINVAL, "dist_inv_span must be finite and > 0 when dist_weight > 0"), false;
    if (reg->occ_weight > 0.0f && reg->occ_samples < 1) return fail(NRF_EINVAL, "occ_samples must be >= 1 when occ_weight > 0"), false;
    rt.dist_weight = reg->dist_weight; rt.dist_inv_span = reg->dist_inv_span; rt.occ_weight = reg->occ_weight; rt.occ_samples = reg->occ_samples;
    return true;
}

// nrf_patch_reg as the launches take it, checked against the batch it splits; false (with the message set) on a refusal
bool patch_reg_terms(const nrf_patch_reg* patch, int64_t n_rays, nrf::PatchRegTerms& pt) {
    if (!patch) return fail(NRF_EINVAL, "patch is NULL"), false;
    if (patch->struct_bytes != (int32_t)sizeof(nrf_patch_reg)) return fail(NRF_EINVAL, "nrf_patch_reg.struct_bytes is not sizeof(nrf_patch_reg)"), false;
    if (!(patch->depth_smooth_weight >= 0.0f) || !std::isfinite(patch->depth_smooth_weight))
        return fail(NRF_EINVAL, "depth_smooth_weight must be finite and >= 0"), false;
    if (patch->patch_size < 2 || patch->patch_size > 16) return fail(NRF_EINVAL, "patch_size must be in 2 ... 16"), false;
    if (patch->n_patches < 0) return fail(NRF_EINVAL, "n_patches must be >= 0"), false;
    if ((int64_t)patch->n_patches * patch->patch_size * patch->patch_size >= n_rays)
        return fail(NRF_EINVAL, "n_patches * patch_size^2 must be < n_rays: a batch needs at least one supervised ray"), false;
    pt.depth_smooth_weight = patch->depth_smooth_weight; pt.patch_size = patch->patch_size; pt.n_patches = patch->n_patches;
    return true;
}

// nrf_info_reg as the launches take it, checked against the patches it acts on; false (with the message set) on a refusal
bool info_reg_terms(const nrf_info_reg* info, const nrf::PatchRegTerms& pt, int n_samples, nrf::InfoRegTerms& it) {
    if (!info) return fail(NRF_EINVAL, "info is NULL"), false;
    if (info->struct_bytes != (int32_t)sizeof(nrf_info_reg)) return fail(NRF_EINVAL, "nrf_info_reg.struct_bytes is not sizeof(nrf_info_reg)"), false;
    for (const float v : {info->ent_weight, info->ent_threshold, info->kl_weight})
        if (!(v >= 0.0f) || !std::isfinite(v)) return fail(NRF_EINVAL, "ent_weight, ent_threshold and kl_weight must be finite and >= 0"), false;
    if (info->kl_weight > 0.0f && pt.n_patches < 1) return fail(NRF_EINVAL, "kl_weight > 0 needs n_patches > 0: the KL term acts on patch rays"), false;
    if (info->kl_weight > 0.0f && (int64_t)pt.patch_size * pt.patch_size * n_samples > NRF_INFO_KL_MAX_LDS_FLOATS)
        return fail(NRF_EINVAL, "kl_weight > 0: patch_size^2 * n_samples exceeds NRF_INFO_KL_MAX_LDS_FLOATS"), false;
    it.ent_weight = info->ent_weight; it.ent_threshold = info->ent_threshold; it.kl_weight = info->kl_weight;
    return true;
}

// nrf_loss_opts as the launches take it, for the entry `who`; false (with the message set) on a refusal
bool loss_terms(const char* who, const nrf_loss_opts* loss, nrf::LossTerms& lt) {
    if (!loss) return fail(NRF_EINVAL, std::string(who) + ": loss is NULL"), false;
    if (loss->struct_bytes != (int32_t)sizeof(nrf_loss_opts)) return fail(NRF_EINVAL, "nrf_loss_opts.struct_bytes is not sizeof(nrf_loss_opts)"), false;
    if (!(loss->rgb_weight >= 0.0f) || !(loss->reg_weight >= 0.0f) || !(loss->depth_weight >= 0.0f) || !std::isfinite(loss->rgb_weight) ||
        !std::isfinite(loss->reg_weight) || !std::isfinite(loss->depth_weight))
        return fail(NRF_EINVAL, "loss weights must be finite and >= 0"), false;
    lt.rgb_weight = loss->rgb_weight; lt.reg_weight = loss->reg_weight; lt.depth_weight = loss->depth_weight;
    lt.target_depth = loss->target_depth; lt.noise_std = loss->noise_std; lt.noise = loss->noise; lt.rng_seed = loss->rng_seed;
    return true;
}

bool slot_aligned(const char* who, const int32_t* slot) {
    if (misaligned(3, {slot})) return fail(NRF_EINVAL, std::string(who) + ": slot must be 4-byte aligned"), false;
    return true;
}

bool sizes_ok(const char* who, int64_t n_rays, int n_samples) {
    if (n_rays <= 0 || n_rays > ((int64_t)1 << 30) || n_samples < 1 || n_samples > 4096) return fail(NRF_EINVAL, std::string(who) + ": bad sizes"), false;
    return true;
}

// The sizes and strides of the compositor's backward forms.  The loss launches (who != NULL: the text names the entry) take
// 1 .. 2^30 rays; the plain backward forms take any n_rays >= 0 and return early on an empty batch.
int check_composite(const char* who, int64_t n_rays, int n_samples, int rgb_stride, int sigma_stride, int d_rgb_stride, int d_sigma_stride) {
    if (who && !sizes_ok(who, n_rays, n_samples)) return NRF_EINVAL;
    if (!who && (n_rays < 0 || n_samples < 1 || n_samples > 4096)) return fail(NRF_EINVAL, "bad sizes");
    if (rgb_stride < 3 || sigma_stride < 1 || d_rgb_stride < 3 || d_sigma_stride < 1) return fail(NRF_EINVAL, "bad strides");
    return NRF_OK;
}

int check_adam(float beta1, float beta2, float eps) {
    if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f)) return fail(NRF_EINVAL, "bad Adam constants");
    return NRF_OK;
}

// What the entries with regularisers hand over on top of the common arguments: rt != NULL: nrf_composite_reg_loss_backward (ray_terms
// holds five rows); pt != NULL (with rt): nrf_composite_patch_loss_backward; it != NULL (with both): nrf_composite_info_loss_backward
struct LossRegs {
    const nrf::RayRegTerms* rt; const nrf::PatchRegTerms* pt; const nrf::InfoRegTerms* it;
    float *patch_terms, *patch_depth, *info_terms, *patch_kl;
};

// nrf_composite_loss_backward and its indexed form (slot != NULL: rgb / sigma / d_rgb / d_sigma hold compacted rows), and the entries
// with regularisers
int composite_loss_backward_any(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals, const float* rays_d,
                                int64_t n_rays, int n_samples, int white_bkgd, const float* target, const nrf_loss_opts* loss, const int32_t* slot,
                                float* pred, float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf,
                                int64_t zero_n, void* stream, const LossRegs& g) {
    nrf::LossLaunch a{rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target, {}, slot, pred,
                      d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, (hipStream_t)stream};
    if (!loss_terms("nrf_composite_loss_backward", loss, a.lt)) return NRF_EINVAL;
    if (!(loss->noise_std >= 0.0f) || !std::isfinite(loss->noise_std)) return fail(NRF_EINVAL, "noise_std must be finite and >= 0");
    if (check_composite("nrf_composite_loss_backward", n_rays, n_samples, rgb_stride, sigma_stride, d_rgb_stride, d_sigma_stride) != NRF_OK) return NRF_EINVAL;
    if (!rgb || !sigma || !z_vals || !rays_d || !target || !d_rgb || !d_sigma || !ray_terms) return fail(NRF_EINVAL, "null pointer");
    if (zero_n < 0 || (zero_n > 0 && !zero_buf)) return fail(NRF_EINVAL, "zero_buf is NULL");
    int r;
    if (g.it) r = nrf::launch_composite_info_loss_backward(a, *g.rt, *g.pt, *g.it, g.patch_terms, g.patch_depth, g.info_terms, g.patch_kl);
    else if (g.pt) r = nrf::launch_composite_patch_loss_backward(a, *g.rt, *g.pt, g.patch_terms, g.patch_depth);
    else if (g.rt) r = nrf::launch_composite_reg_loss_backward(a, *g.rt);
    else r = nrf::launch_composite_loss_backward(a);
    return launched(r, "composite + loss + backward launch failed");
}

int composite_merge_any(nrf::MergeArgs& a, int mma_mode, int out_rgbd, void* stream) {
    if (a.n_rays < 0 || a.S < 1 || a.Ni < 0) return fail(NRF_EINVAL, "bad sizes");
    if (mma_mode < 0 || mma_mode >= nrf::kModes) return fail(NRF_EINVAL, "unknown mma_mode");
    if (a.n_rays == 0) return NRF_OK;
    if (!a.z_coarse || !a.raw_coarse || (a.Ni > 0 && (!a.z_new || !a.raw_new)) || !a.rgb) return fail(NRF_EINVAL, "null pointer");
    if (misaligned(15, {a.raw_coarse, a.raw_new}))
        return fail(NRF_EINVAL, "raw rows must be 16-byte aligned (read with one 16-byte load per sample)");
    if (out_rgbd && misaligned(15, {a.rgb})) return fail(NRF_EINVAL, kRgbdAlign);
    a.interleaved = out_rgbd ? 1 : 0;
    // the compositor's exp / sigmoid follow the arithmetic mode that emitted the rows (mlp_core.hpp: Mode::FAST_EXP)
    const int r = nrf::launch_composite_merge(a, mma_mode == NRF_MMA_BF16, (hipStream_t)stream);
    return launched(r, "composite_merge launch failed");
}

// the checks the two fetch adjoints share; 1 = nothing to do
int fetch_backward_check(int Hp, int Wp, int C, const void* points, int64_t n, const float* d_feats, float* d_map, int accumulate, void* ws,
                         int64_t ws_bytes) {
    if (n < 0 || Hp < 1 || Wp < 1 || C < 1) return fail(NRF_EINVAL, "bad sizes");
    if (!d_map) return fail(NRF_EINVAL, "null pointer");
    if (n == 0 && accumulate) return 1;
    if (n > 0 && (!points || !d_feats)) return fail(NRF_EINVAL, "null pointer");
    if (!ws) return fail(NRF_EINVAL, "fetch backward workspace is NULL");
    if (misaligned(3, {ws})) return fail(NRF_EINVAL, "fetch backward workspace must be 4-byte aligned");
    if (ws_bytes < 4 * nrf::fetch_backward_ws_floats(Hp, Wp, C, n)) return fail(NRF_EINVAL, "workspace smaller than nrf_fetch_backward_workspace_bytes");
    return NRF_OK;
}

// ---- the debug entries: host functions that hand out what the packers and the planners make ----
using Linears = std::vector<nrf::HostLinear>;
// a plan of the copied Linears: NRF_OK, or the code to refuse with and its text in err
using PlanMaker = int (*)(const nrf_arch&, const Linears&, nrf::NetPlan&, std::string&);
template <bool (*Make)(const nrf_arch&, const Linears&, nrf::NetPlan&, std::string&)>
int planned(const nrf_arch& a, const Linears& lin, nrf::NetPlan& plan, std::string& err) { return Make(a, lin, plan, err) ? NRF_OK : NRF_EINVAL; }
// the transposed chain: the forward plan has to stand before its backward plan is made
int planned_backward(const nrf_arch& a, const Linears& lin, nrf::NetPlan& bplan, std::string& err) {
    nrf::NetPlan plan;
    if (!nrf::make_plan(a, lin, plan, err)) return NRF_EINVAL;
    return nrf::make_backward_plan(a, lin, bplan, err) ? NRF_OK : NRF_EUNSUPPORTED;
}

int debug_args(const char* who, const nrf_arch* arch, const nrf_linear* linears, int n_linear) {
    if (!arch || !linears || n_linear <= 0) return fail(NRF_EINVAL, std::string(who) + ": null argument");
    return NRF_OK;
}

int debug_plan(const nrf_arch* arch, const nrf_linear* linears, int n_linear, PlanMaker make, Linears& lin, nrf::NetPlan& plan) {
    std::string err;
    if (!copy_linears(linears, n_linear, lin, err)) return fail(NRF_EINVAL, err);
    const int rc = make(*arch, lin, plan, err);
    if (rc != NRF_OK) return fail(rc, err);
    return NRF_OK;
}

// the close of every debug entry: all of src, into a buffer of cap elements if one is given
template <class T>
int copy_out(T* dst, int64_t cap, const std::vector<T>& src, const char* too_small) {
    if (!dst) return NRF_OK;
    if (cap < (int64_t)src.size()) return fail(NRF_EINVAL, too_small);
    std::memcpy(dst, src.data(), src.size() * sizeof(T));
    return NRF_OK;
}

// nrf_debug_pack alone: the bias table follows the stream
struct BiasOut {
    float* out;
    int64_t cap;
    int64_t* n;
};

// The five stream packers: the plan that `make` gives, packed in one of the first n_modes modes.  Both sizes are reported before
// either buffer is looked at.
int debug_pack(const char* who, PlanMaker make, int n_modes, const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode,
               uint8_t* stream_out, int64_t stream_cap, int64_t* stream_bytes, const BiasOut* bias = nullptr) {
    if (debug_args(who, arch, linears, n_linear) != NRF_OK) return NRF_EINVAL;
    if (mma_mode < 0 || mma_mode >= n_modes) return fail(NRF_EINVAL, "unknown mma_mode");
    Linears lin;
    nrf::NetPlan plan;
    int rc = debug_plan(arch, linears, n_linear, make, lin, plan);
    if (rc != NRF_OK) return rc;
    const nrf::PackedStream ps = nrf::pack_stream(plan, lin, mma_mode);
    const std::vector<float> b = bias ? nrf::pack_bias(plan, lin) : std::vector<float>();
    if (stream_bytes) *stream_bytes = (int64_t)ps.bytes.size();
    if (bias && bias->n) *bias->n = (int64_t)b.size();
    rc = copy_out(stream_out, stream_cap, ps.bytes, "stream_out too small");
    return rc == NRF_OK && bias ? copy_out(bias->out, bias->cap, b, "bias_out too small") : rc;
}

}  // namespace

extern "C" {

int nrf_abi_version(void) { return NRF_ABI_VERSION; }

int nrf_abi_sizeof(int which) {
    switch (which) {
        case 0: return (int)sizeof(nrf_arch);
        case 1: return (int)sizeof(nrf_linear);
        case 2: return (int)sizeof(nrf_dino);
        case 3: return (int)sizeof(nrf_render_opts);
        case 4: return (int)sizeof(nrf_tail);
        default: return -1;
    }
}

const char* nrf_last_error(void) { return g_err.c_str(); }

int nrf_model_create(nrf_model** out, int device, const nrf_arch* arch, const nrf_linear* linears, int n_linear) {
    if (!out || !arch || !linears || n_linear <= 0) return fail(NRF_EINVAL, "nrf_model_create: null argument");
    *out = nullptr;
    nrf_model* m = new (std::nothrow) nrf_model();
    if (!m) return fail(NRF_ENOMEM, "out of host memory");
    m->arch = *arch;
    m->device = device;
    std::string err;
    if (!copy_linears(linears, n_linear, m->lin, err) || !nrf::make_plan(*arch, m->lin, m->plan, err)) {
        delete m;
        return fail(NRF_EINVAL, err);
    }
    DeviceGuard guard(device);
    if (!guard.ok) { delete m; return fail(NRF_EHIP, "cannot select device " + std::to_string(device)); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { delete m; return fail(NRF_EHIP, "hipGetDeviceProperties failed"); }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        delete m;
        return fail(NRF_EUNSUPPORTED, std::string("libnerfhip is built for gfx950 only, device is ") + prop.gcnArchName);
    }
    for (float& v : m->freq.scale) v = 1.0f;
    m->net.arch = *arch;
    m->net.device = device;
    m->net.cu_count = prop.multiProcessorCount;
    const int rc = upload(m, nullptr, true);
    if (rc != NRF_OK) { nrf_model_destroy(m); return rc; }
    *out = m;
    return NRF_OK;
}

int nrf_model_update(nrf_model* m, const nrf_linear* linears, int n_linear, void* stream) {
    if (!m || !linears) return fail(NRF_EINVAL, "nrf_model_update: null argument");
    std::string err;
    std::vector<nrf::HostLinear> lin;
    nrf::NetPlan plan;
    if (!copy_linears(linears, n_linear, lin, err) || !nrf::make_plan(m->arch, lin, plan, err)) return fail(NRF_EINVAL, err);
    m->lin.swap(lin);
    m->plan = plan;
    DeviceGuard guard(m->device);
    if (!guard.ok) return no_device();
    return upload(m, (hipStream_t)stream, false);
}

void nrf_model_destroy(nrf_model* m) {
    if (!m) return;
    DeviceGuard guard(m->device);
    for (int i = 0; i < nrf::kModes; ++i)
        if (m->d_stream[i]) (void)hipFree(m->d_stream[i]);
    if (m->d_bias) (void)hipFree(m->d_bias);
    if (m->d_queues) (void)hipFree(m->d_queues);
    for (int i = 0; i < 3; ++i)
        if (m->d_bstream[i]) (void)hipFree(m->d_bstream[i]);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j)
            if (m->d_src[i][j]) (void)hipFree(m->d_src[i][j]);
    if (m->d_maps) (void)hipFree(m->d_maps);
    if (m->d_bias_src) (void)hipFree(m->d_bias_src);
    if (m->d_freq_ids) (void)hipFree(m->d_freq_ids);
    delete m;
}

int64_t nrf_model_flops_per_sample(const nrf_model* m) { return m ? m->plan.flops_per_sample : 0; }

int64_t nrf_render_tail_bytes(int64_t n_rays) {
    if (n_rays < 0) { (void)fail(NRF_EINVAL, "nrf_render_tail_bytes: n_rays < 0"); return -1; }
    return (nrf::render_tail_floats(n_rays) * (int64_t)sizeof(float) + 15) & ~(int64_t)15;
}

int nrf_render_rays(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays, const nrf_render_opts* opts,
                    float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    return render_rays_any(m, rays_o, rays_d, n_rays, opts, nullptr, false, nullptr, rgb, depth, weights, z_vals, stream);
}
int nrf_render_rays_tail(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays, const nrf_render_opts* opts,
                         const nrf_tail* tail, float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    return render_rays_any(m, rays_o, rays_d, n_rays, opts, tail, true, nullptr, rgb, depth, weights, z_vals, stream);
}
int nrf_render_camera(const nrf_model* m, int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                      const nrf_render_opts* opts, float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    return render_camera_any(m, H, W, focal, c2w, ray_begin, ray_end, opts, nullptr, false, nullptr, rgb, depth, weights, z_vals, stream);
}
int nrf_render_camera_tail(const nrf_model* m, int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                           const nrf_render_opts* opts, const nrf_tail* tail, float* rgb, float* depth, float* weights, float* z_vals,
                           void* stream) {
    return render_camera_any(m, H, W, focal, c2w, ray_begin, ray_end, opts, tail, true, nullptr, rgb, depth, weights, z_vals, stream);
}
int nrf_render_rays_emit(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays, const nrf_render_opts* opts,
                         float* rgb, float* depth, float* weights, float* z_vals, float* raw4, int raw_only, void* stream) {
    const EmitOut e{raw4, raw_only};
    return render_rays_any(m, rays_o, rays_d, n_rays, opts, nullptr, false, nullptr, rgb, depth, weights, z_vals, stream, &e);
}
int nrf_render_camera_emit(const nrf_model* m, int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                           const nrf_render_opts* opts, float* rgb, float* depth, float* weights, float* z_vals, float* raw4, int raw_only,
                           void* stream) {
    const EmitOut e{raw4, raw_only};
    return render_camera_any(m, H, W, focal, c2w, ray_begin, ray_end, opts, nullptr, false, nullptr, rgb, depth, weights, z_vals, stream, &e);
}
int nrf_render_cameras_tiles(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams, int64_t tile_rays,
                             int64_t first_tile, int64_t tile_step, int64_t n_tiles, const nrf_render_opts* opts, float* rgb, float* depth,
                             float* weights, float* z_vals, void* stream) {
    return render_cameras_tiles_any(m, H, W, focal, c2w, n_cams, tile_rays, first_tile, tile_step, n_tiles, opts, nullptr, false, nullptr, rgb, depth,
                                    weights, z_vals, stream);
}
int nrf_render_cameras_tiles_tail(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams, int64_t tile_rays,
                                  int64_t first_tile, int64_t tile_step, int64_t n_tiles, const nrf_render_opts* opts, const nrf_tail* tail,
                                  float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    return render_cameras_tiles_any(m, H, W, focal, c2w, n_cams, tile_rays, first_tile, tile_step, n_tiles, opts, tail, true, nullptr, rgb, depth,
                                    weights, z_vals, stream);
}

// with a grid: the grid and the ray count are checked first (they need no model), then the plain entry's own checks
int nrf_render_rays_occ(const nrf_model* m, const float* rays_o, const float* rays_d, int64_t n_rays, const nrf_render_opts* opts,
                        const nrf_occupancy* occ, float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    if (check_occ(occ, n_rays) != NRF_OK) return NRF_EINVAL;
    return render_rays_any(m, rays_o, rays_d, n_rays, opts, nullptr, false, occ, rgb, depth, weights, z_vals, stream);
}
int nrf_render_camera_occ(const nrf_model* m, int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end,
                          const nrf_render_opts* opts, const nrf_occupancy* occ, float* rgb, float* depth, float* weights, float* z_vals,
                          void* stream) {
    if (check_occ(occ, ray_end - ray_begin) != NRF_OK) return NRF_EINVAL;
    return render_camera_any(m, H, W, focal, c2w, ray_begin, ray_end, opts, nullptr, false, occ, rgb, depth, weights, z_vals, stream);
}
int nrf_render_cameras_tiles_occ(const nrf_model* m, int H, int W, float focal, const float* c2w, int n_cams, int64_t tile_rays,
                                 int64_t first_tile, int64_t tile_step, int64_t n_tiles, const nrf_render_opts* opts, const nrf_occupancy* occ,
                                 float* rgb, float* depth, float* weights, float* z_vals, void* stream) {
    // (the product is formed in floating point: a tile description that overflows int64 is refused like any other launch too large)
    const double rays = (double)(n_tiles > 0 ? n_tiles : 0) * (double)(tile_rays > 0 ? tile_rays : 0) * (double)(n_cams > 0 ? n_cams : 0);
    if (check_occ(occ, rays >= 2147483648.0 ? (int64_t)1 << 31 : (int64_t)rays) != NRF_OK) return NRF_EINVAL;
    return render_cameras_tiles_any(m, H, W, focal, c2w, n_cams, tile_rays, first_tile, tile_step, n_tiles, opts, nullptr, false, occ, rgb, depth,
                                    weights, z_vals, stream);
}

int nrf_occupancy_pack(const float* density, int64_t n_cells, int k, float threshold, uint32_t* bits, void* stream) {
    if (n_cells < 0 || n_cells % 32 != 0 || k < 1) return fail(NRF_EINVAL, "nrf_occupancy_pack: n_cells must be a non-negative multiple of 32 and k >= 1");
    if (n_cells == 0) return NRF_OK;
    if (!density || !bits) return fail(NRF_EINVAL, "nrf_occupancy_pack: null pointer");
    const int r = nrf::launch_occupancy_pack(density, n_cells, k, threshold, bits, (hipStream_t)stream);
    return launched(r, "occupancy_pack launch failed");
}

int nrf_occupancy_dilate(const uint32_t* bits_in, const int32_t res[3], uint32_t* bits_out, void* stream) {
    if (!bits_in || !bits_out || !res || bits_in == bits_out) return fail(NRF_EINVAL, "nrf_occupancy_dilate: null pointer, or bits_out is bits_in");
    for (int k = 0; k < 3; ++k)
        if (res[k] < 1 || res[k] > 512) return fail(NRF_EINVAL, "nrf_occupancy_dilate: res must be in 1..512 on every axis");
    if (res[0] % 32 != 0) return fail(NRF_EINVAL, "nrf_occupancy_dilate: res[0] must be a multiple of 32");
    const int r3[3] = {res[0], res[1], res[2]};
    const int r = nrf::launch_occupancy_dilate(bits_in, r3, bits_out, (hipStream_t)stream);
    return launched(r, "occupancy_dilate launch failed");
}

int nrf_occupancy_mark_rays(const float* rays_o, const float* rays_d, int64_t n_rays, int n_samples, const float* z_vals, const float* weights,
                            const int32_t res[3], const float lo[3], const float scale[3], float weight_threshold, float seen_eps,
                            uint32_t* hit_bits, uint32_t* seen_bits, void* stream) {
    return mark_any("nrf_occupancy_mark_rays", rays_o, rays_d, nullptr, 0, n_rays, n_samples, z_vals, weights, res, lo, scale, weight_threshold, seen_eps,
                    hit_bits, seen_bits, stream);
}

int nrf_occupancy_mark_camera(int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end, int n_samples, const float* z_vals,
                              const float* weights, const int32_t res[3], const float lo[3], const float scale[3], float weight_threshold,
                              float seen_eps, uint32_t* hit_bits, uint32_t* seen_bits, void* stream) {
    if (check_camera(H, W, focal, c2w) != NRF_OK || check_ray_range(H, W, ray_begin, ray_end) != NRF_OK) return NRF_EINVAL;
    const nrf::Camera cam = make_camera(H, W, focal, c2w);
    return mark_any("nrf_occupancy_mark_camera", nullptr, nullptr, &cam, ray_begin, ray_end - ray_begin, n_samples, z_vals, weights, res, lo, scale,
                    weight_threshold, seen_eps, hit_bits, seen_bits, stream);
}

int nrf_get_rays(int H, int W, float focal, const float c2w[12], int64_t ray_begin, int64_t ray_end, float* rays_o, float* rays_d,
                 void* stream) {
    if (check_camera(H, W, focal, c2w) != NRF_OK || check_ray_range(H, W, ray_begin, ray_end) != NRF_OK) return NRF_EINVAL;
    if (ray_end > ray_begin && (!rays_o || !rays_d)) return fail(NRF_EINVAL, "null output");
    const int r = nrf::launch_get_rays(make_camera(H, W, focal, c2w), ray_begin, ray_end - ray_begin, rays_o, rays_d, (hipStream_t)stream);
    return launched(r, "get_rays launch failed");
}

int nrf_sample_along_rays(const float* rays_o, const float* rays_d, int64_t n_rays, float near, float far, int n_samples, int lindisp,
                          int perturb, const float* t_rand, const float* z_ladder, uint64_t rng_seed, float* pts, float* z_vals,
                          void* stream) {
    if (n_rays < 0 || n_samples < 1) return fail(NRF_EINVAL, "bad sizes");
    if (n_rays == 0) return NRF_OK;
    if (!rays_o || !rays_d || (!pts && !z_vals)) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_sample(rays_o, rays_d, n_rays, near, far, n_samples, lindisp, perturb, perturb ? t_rand : nullptr, z_ladder, rng_seed,
                                     pts, z_vals, (hipStream_t)stream);
    return launched(r, "sample launch failed");
}

int nrf_encode(const float* x, int64_t n, int dim, int num_freqs, int include_input, const float* freq_bands, float* out, void* stream) {
    if (n < 0 || dim < 1 || num_freqs < 0 || (num_freqs > 31 && !freq_bands)) return fail(NRF_EINVAL, "bad sizes");
    if (n == 0) return NRF_OK;
    if (!x || !out) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_encode(x, n, dim, num_freqs, include_input, freq_bands, out, (hipStream_t)stream);
    return launched(r, "encode launch failed");
}

int nrf_mlp_forward_v1(const nrf_model* m, int mma_mode, const float* x_enc, int64_t n, float* out4, void* stream) {
    if (!m) return fail(NRF_EINVAL, "model is NULL");
    if (n < 0) return fail(NRF_EINVAL, "n < 0");
    if (n == 0) return NRF_OK;
    if (!x_enc || !out4) return fail(NRF_EINVAL, "null pointer");
    DeviceGuard guard(m->device);
    if (!guard.ok) return no_device();
    std::string err;
    const int r = nrf::launch_forward_v1(m->net, mma_mode, x_enc, n, out4, (hipStream_t)stream, err);
    return launched(r, err);
}

int nrf_mlp_forward(const nrf_model* m, int mma_mode, const float* positions, const float* directions, const float* dino, int64_t n,
                    float* rgb, float* density, void* stream) {
    if (!m) return fail(NRF_EINVAL, "model is NULL");
    if (n < 0) return fail(NRF_EINVAL, "n < 0");
    if (n == 0) return NRF_OK;
    if (!positions || !directions || !rgb || !density) return fail(NRF_EINVAL, "null pointer");
    if (m->arch.net == NRF_NET_V3 && !dino) return fail(NRF_EINVAL, "V3 needs dino features");
    DeviceGuard guard(m->device);
    if (!guard.ok) return no_device();
    std::string err;
    const int r = nrf::launch_forward(m->net, mma_mode, positions, directions, dino, n, rgb, density, (hipStream_t)stream, err);
    return launched(r, err);
}

int nrf_composite(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals, const float* rays_d,
                  int64_t n_rays, int n_samples, int white_bkgd, float* out_rgb, float* out_depth, float* out_weights, void* stream) {
    if (n_rays < 0 || n_samples < 1) return fail(NRF_EINVAL, "bad sizes");
    if (rgb_stride < 3 || sigma_stride < 1) return fail(NRF_EINVAL, "bad strides");
    if (n_rays == 0) return NRF_OK;
    if (!rgb || !sigma || !z_vals || !rays_d || !out_rgb) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_composite(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, out_rgb,
                                        out_depth, out_weights, (hipStream_t)stream);
    return launched(r, "composite launch failed");
}

int64_t nrf_param_count(const nrf_model* m) {
    if (!m) return 0;
    int64_t n = 0;
    for (const auto& l : m->lin) n += (int64_t)l.out_f * l.in_f + l.out_f;
    return n;
}

int nrf_model_update_device(nrf_model* m, const float* flat_params, int mode_mask, void* stream) {
    if (!m || !flat_params) return fail(NRF_EINVAL, "nrf_model_update_device: null argument");
    if (mode_mask <= 0 || mode_mask >= (1 << nrf::kModes)) return fail(NRF_EINVAL, "mode_mask must select at least one of the NRF_MMA_* modes");
    DeviceGuard guard(m->device);
    if (!guard.ok) return no_device();
    int rc = ensure_sources(m);
    if (rc != NRF_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    // one launch per mode in the mask: its forward stream, its backward stream (once training is set up; the split mode has none)
    // and, with the first mode, the bias table
    bool bias = true;
    for (int mode = 0; mode < nrf::kModes; ++mode) {
        if (!(mode_mask & (1 << mode))) continue;
        const int kind = nrf::stream_kind(mode);
        const bool bwd = m->train_ready && mode < 3;
        const int32_t* src[3] = {m->d_src[0][kind], bwd ? m->d_src[1][kind] : nullptr, bias ? m->d_bias_src : nullptr};
        const int64_t n[3] = {m->n_src[0][kind], bwd ? m->n_src[1][kind] : 0, bias ? m->plan.n_bias : 0};
        const int modes[3] = {mode, mode, NRF_MMA_F32};
        void* out[3] = {m->d_stream[mode], bwd ? m->d_bstream[mode] : nullptr, bias ? m->d_bias : nullptr};
        rc = nrf::launch_repack3(flat_params, src, n, modes, out, s, m->freq_active ? &m->freq : nullptr);
        if (rc != NRF_OK) return fail(rc, "repack launch failed");
        mark_packed(m, mode);
        bias = false;
    }
    m->lin_stale = true;
    for (int k = 0; k < 3; ++k) m->bfresh[k] = (mode_mask & (1 << k)) && m->train_ready;
    return NRF_OK;
}

int nrf_model_set_freq_mask(nrf_model* m, const float* pos_scale, const float* dir_scale) {
    if (!m) return fail(NRF_EINVAL, "nrf_model_set_freq_mask: model is NULL");
    if (dir_scale && m->arch.net == NRF_NET_V1) return fail(NRF_EINVAL, "nrf_model_set_freq_mask: a V1 model reads no direction encoding (dir_scale must be NULL)");
    const int np = nrf::freq_pos_cols(m->arch), nd = nrf::freq_dir_cols(m->arch);
    if (np + nd > nrf::kFreqCols) return fail(NRF_EUNSUPPORTED, "nrf_model_set_freq_mask: too many encoding columns");
    nrf::FreqMaskArgs f = m->freq;
    for (float& v : f.scale) v = 1.0f;
    bool active = false;
    for (int part = 0; part < 2; ++part) {
        const float* in = part ? dir_scale : pos_scale;
        const int n = part ? nd : np, id0 = part ? np : 0;
        for (int c = 0; in && c < n; ++c) {
            if (!std::isfinite(in[c]) || in[c] < 0.0f || in[c] > 1.0f) return fail(NRF_EINVAL, "nrf_model_set_freq_mask: scales must be finite and in [0,1]");
            f.scale[id0 + c] = in[c] == 0.0f ? 0.0f : in[c];            // (-0 is recorded as +0)
            active = active || in[c] != 1.0f;
        }
    }
    if (same_mask(f, m->freq)) return NRF_OK;
    m->freq = f;
    m->freq_active = active;
    for (int k = 0; k < 3; ++k) m->bfresh[k] = false;           // every mode's backward weights are older than the mask now
    return NRF_OK;
}

int nrf_model_get_freq_mask(const nrf_model* m, float* pos_scale, float* dir_scale, int* active) {
    if (!m) return fail(NRF_EINVAL, "nrf_model_get_freq_mask: model is NULL");
    const int np = nrf::freq_pos_cols(m->arch), nd = nrf::freq_dir_cols(m->arch);
    if (pos_scale) std::memcpy(pos_scale, m->freq.scale, sizeof(float) * np);
    if (dir_scale) std::memcpy(dir_scale, m->freq.scale + np, sizeof(float) * nd);
    if (active) *active = m->freq_active ? 1 : 0;
    return NRF_OK;
}

int64_t nrf_train_context_bytes(nrf_model* m, int mma_mode, int64_t n) {
    if (!m || n < 0 || mma_mode < 0 || mma_mode > 2) { (void)fail(NRF_EINVAL, "nrf_train_context_bytes: bad argument"); return -1; }
    DeviceGuard guard(m->device);
    if (!guard.ok) { (void)no_device(); return -1; }
    if (ensure_train(m) != NRF_OK) return -1;
    return nrf::train_ctx_bytes(m->train, mma_mode, n);
}

int nrf_mlp_forward_train_v1(nrf_model* m, int mma_mode, const float* x_enc, int64_t n, float* out4, void* ctx, int64_t ctx_bytes,
                             void* stream) {
    return train_entry(m, mma_mode, n, !x_enc || !out4 || !ctx, ctx_bytes, false, any_family, [&](std::string& err) {
        return nrf::launch_train_forward(m->net, m->train, mma_mode, x_enc, n, out4, ctx, (hipStream_t)stream, err);
    });
}

int nrf_mlp_backward_v1(nrf_model* m, int mma_mode, const float* out4, const float* g_out4, int64_t n, void* ctx, int64_t ctx_bytes,
                        float* flat_grad, void* stream) {
    return train_entry(m, mma_mode, n, !out4 || !g_out4 || !ctx || !flat_grad, ctx_bytes, true, any_family, [&](std::string& err) {
        return nrf::launch_train_backward(m->net, m->train, mma_mode, out4, g_out4, n, ctx, flat_grad, (hipStream_t)stream, err);
    });
}

int nrf_mlp_forward_train(nrf_model* m, int mma_mode, const float* positions, const float* directions, const float* dino, int64_t n, float* rgb,
                          float* density, void* ctx, int64_t ctx_bytes, void* stream) {
    auto wrong = [&]() -> const char* {
        if (m->arch.net == NRF_NET_V1) return "V1 models take encoded inputs: nrf_mlp_forward_train_v1";
        if (m->arch.net == NRF_NET_V3 && !dino) return "V3 needs per-sample dino features";
        return nullptr;
    };
    return train_entry(m, mma_mode, n, !positions || !directions || !rgb || !density || !ctx, ctx_bytes, false, wrong, [&](std::string& err) {
        return m->arch.net == NRF_NET_V3
            ? nrf::launch_train_forward_v3(m->net, m->train, mma_mode, positions, directions, dino, n, rgb, density, ctx, (hipStream_t)stream, err)
            : nrf::launch_train_forward_v2(m->net, m->train, mma_mode, positions, directions, n, rgb, density, ctx, (hipStream_t)stream, err);
    });
}

int nrf_mlp_backward(nrf_model* m, int mma_mode, const float* rgb, const float* density, const float* g_rgb, const float* g_density, int64_t n,
                     void* ctx, int64_t ctx_bytes, float* flat_grad, void* stream) {
    auto wrong = [&]() -> const char* { return m->arch.net == NRF_NET_V1 ? "V1 models: nrf_mlp_backward_v1" : nullptr; };
    return train_entry(m, mma_mode, n, !rgb || !density || !g_rgb || !g_density || !ctx || !flat_grad, ctx_bytes, true, wrong,
                       [&](std::string& err) {
        return m->arch.net == NRF_NET_V3
            ? nrf::launch_train_backward_v3(m->net, m->train, mma_mode, rgb, density, g_rgb, g_density, n, ctx, flat_grad, (hipStream_t)stream, err)
            : nrf::launch_train_backward_v2(m->net, m->train, mma_mode, rgb, density, g_rgb, g_density, n, ctx, flat_grad, (hipStream_t)stream, err);
    });
}

int nrf_mlp_backward_dino(nrf_model* m, int mma_mode, int64_t n, void* ctx, int64_t ctx_bytes, float* d_dino, void* stream) {
    auto wrong = [&]() -> const char* {
        if (m->arch.net != NRF_NET_V3) return "nrf_mlp_backward_dino: only the V3 network has DINO feature inputs";
        if (misaligned(15, {d_dino})) return "nrf_mlp_backward_dino: d_dino must be 16-byte aligned";
        return nullptr;
    };
    return train_entry(m, mma_mode, n, !ctx || !d_dino, ctx_bytes, true, wrong, [&](std::string& err) {
        return nrf::launch_dino_grad(m->net, m->train, mma_mode, n, ctx, d_dino, (hipStream_t)stream, err);
    });
}

int nrf_mlp_backward_inputs(nrf_model* m, int mma_mode, int64_t n, void* ctx, int64_t ctx_bytes, const float* positions, const float* directions,
                            float* d_x_enc, float* d_positions, float* d_directions, void* stream) {
    auto wrong = [&]() -> const char* {
        if (m->arch.net == NRF_NET_V3)
            return "nrf_mlp_backward_inputs: the V3 network also needs the adjoint of the projection and the bilinear fetch with respect to the points "
                   "(nrf_mlp_backward_inputs_v3, then nrf_project_fetch_backward_points)";
        if (m->arch.net != NRF_NET_V1 && m->arch.net != NRF_NET_V2) return "nrf_mlp_backward_inputs: unknown network family";
        if (!d_x_enc && !d_positions && !d_directions) return "nrf_mlp_backward_inputs: no output asked for";
        if (d_x_enc && m->arch.net != NRF_NET_V1) return "nrf_mlp_backward_inputs: d_x_enc belongs to the V1 network (encoded inputs)";
        if (d_directions && m->arch.net == NRF_NET_V1) return "nrf_mlp_backward_inputs: the V1 network has no direction input";
        if (d_positions && !positions) return "nrf_mlp_backward_inputs: d_positions needs the positions";
        if (d_directions && !directions) return "nrf_mlp_backward_inputs: d_directions needs the directions";
        if (misaligned(3, {d_x_enc, d_positions, d_directions, positions, directions}))
            return "nrf_mlp_backward_inputs: float tensors must be 4-byte aligned";
        return nullptr;
    };
    return train_entry(m, mma_mode, n, !ctx, ctx_bytes, true, wrong, [&](std::string& err) {
        return nrf::launch_input_grad(m->net, m->train, mma_mode, n, ctx, positions, directions, d_x_enc, d_positions, d_directions,
                                      (hipStream_t)stream, err);
    });
}

int nrf_mlp_backward_inputs_v3(nrf_model* m, int mma_mode, int64_t n, void* ctx, int64_t ctx_bytes, const float* positions, const float* directions,
                               float* d_positions, float* d_directions, void* stream) {
    auto wrong = [&]() -> const char* {
        if (m->arch.net != NRF_NET_V3) return "nrf_mlp_backward_inputs_v3: only the V3 network (V1 / V2: nrf_mlp_backward_inputs)";
        if (!d_positions && !d_directions) return "nrf_mlp_backward_inputs_v3: no output asked for";
        if (d_positions && !positions) return "nrf_mlp_backward_inputs_v3: d_positions needs the positions";
        if (d_directions && !directions) return "nrf_mlp_backward_inputs_v3: d_directions needs the directions";
        if (misaligned(3, {d_positions, d_directions, positions, directions}))
            return "nrf_mlp_backward_inputs_v3: float tensors must be 4-byte aligned";
        return nullptr;
    };
    return train_entry(m, mma_mode, n, !ctx, ctx_bytes, true, wrong, [&](std::string& err) {
        return nrf::launch_input_grad_v3(m->net, m->train, mma_mode, n, ctx, positions, directions, d_positions, d_directions, (hipStream_t)stream, err);
    });
}

int nrf_mlp_forward_train_rays(nrf_model* m, const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts, float* out_a, float* out_b,
                               void* ctx, int64_t ctx_bytes, void* stream) {
    // what the arguments alone decide comes first, then what needs the model, then the device (context size)
    const int rc = check_ray_source("nrf_mlp_forward_train_rays", rays, n_rays, opts, "evaluates every sample", kNoZVals);
    if (rc != NRF_OK) return rc;
    if (!m) return fail(NRF_EINVAL, "model is NULL");
    const int mode = opts->mma_mode == NRF_MMA_F16X3 ? NRF_MMA_F32 : opts->mma_mode;      // the split mode trains in exact fp32
    const bool v1 = m->arch.net == NRF_NET_V1;
    nrf::TrainRaysDev r{};
    std::string derr;
    if (m->arch.net == NRF_NET_V3 && !make_dino(opts->dino, m->arch.dino_dim, r.dino, derr)) return fail(NRF_EINVAL, "nrf_mlp_forward_train_rays: " + derr);
    if (n_rays == 0) return NRF_OK;
    const int64_t n = n_rays * opts->n_samples;
    fill_ray_source(r, rays, opts, true);
    auto wrong = [&]() -> const char* {
        if (v1 && out_b) return "nrf_mlp_forward_train_rays: a V1 model writes out_a (n,4) alone, out_b must be NULL";
        return nullptr;
    };
    return train_entry(m, mode, n, !out_a || (!v1 && !out_b) || !ctx, ctx_bytes, false, wrong, [&](std::string& err) {
        hipStream_t s = (hipStream_t)stream;
        switch (m->arch.net) {
            case NRF_NET_V1: return nrf::launch_train_forward_rays_v1(m->net, m->train, mode, r, n, out_a, ctx, s, err);
            case NRF_NET_V3: return nrf::launch_train_forward_rays_v3(m->net, m->train, mode, r, n, out_a, out_b, ctx, s, err);
            default:         return nrf::launch_train_forward_rays_v2(m->net, m->train, mode, r, n, out_a, out_b, ctx, s, err);
        }
    });
}

int nrf_mlp_forward_train_rays_indexed(nrf_model* m, const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts, const int32_t* index,
                                       int64_t n_rows, float* out_a, float* out_b, void* ctx, int64_t ctx_bytes, void* stream) {
    // the order of nrf_mlp_forward_train_rays, with the row list behind the ray source
    const int rc = check_ray_source("nrf_mlp_forward_train_rays_indexed", rays, n_rays, opts, "evaluates every kept sample",
                                    "nrf_mlp_forward_train_rays_indexed: rays->z_vals is required (the depths nrf_occupancy_compact_rays left there)");
    if (rc != NRF_OK) return rc;
    if (!index) return fail(NRF_EINVAL, "nrf_mlp_forward_train_rays_indexed: index is NULL");
    if (misaligned(3, {index})) return fail(NRF_EINVAL, "nrf_mlp_forward_train_rays_indexed: index must be 4-byte aligned");
    if (n_rows < 0) return fail(NRF_EINVAL, "nrf_mlp_forward_train_rays_indexed: n_rows < 0");
    if (n_rows > (int64_t)opts->n_samples * n_rays) return fail(NRF_EINVAL, "nrf_mlp_forward_train_rays_indexed: n_rows exceeds n_rays * n_samples");
    if (!m) return fail(NRF_EINVAL, "model is NULL");
    const int mode = opts->mma_mode == NRF_MMA_F16X3 ? NRF_MMA_F32 : opts->mma_mode;      // the split mode trains in exact fp32
    const bool v1 = m->arch.net == NRF_NET_V1;
    nrf::TrainRaysDev r{};
    std::string derr;
    if (m->arch.net == NRF_NET_V3 && !make_dino(opts->dino, m->arch.dino_dim, r.dino, derr))
        return fail(NRF_EINVAL, "nrf_mlp_forward_train_rays_indexed: " + derr);
    if (n_rows == 0) return NRF_OK;
    fill_ray_source(r, rays, opts, false);                      // z_vals is read, never written
    auto wrong = [&]() -> const char* {
        if (v1 && out_b) return "nrf_mlp_forward_train_rays_indexed: a V1 model writes out_a (n_rows,4) alone, out_b must be NULL";
        return nullptr;
    };
    return train_entry(m, mode, n_rows, !out_a || (!v1 && !out_b) || !ctx, ctx_bytes, false, wrong, [&](std::string& err) {
        hipStream_t s = (hipStream_t)stream;
        switch (m->arch.net) {
            case NRF_NET_V1: return nrf::launch_train_forward_rays_indexed_v1(m->net, m->train, mode, r, index, n_rows, out_a, ctx, s, err);
            case NRF_NET_V3: return nrf::launch_train_forward_rays_indexed_v3(m->net, m->train, mode, r, index, n_rows, out_a, out_b, ctx, s, err);
            default:         return nrf::launch_train_forward_rays_indexed_v2(m->net, m->train, mode, r, index, n_rows, out_a, out_b, ctx, s, err);
        }
    });
}

int nrf_composite_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals, const float* rays_d,
                           int64_t n_rays, int n_samples, int white_bkgd, const float* g_rgb, const float* g_depth, const float* g_weights,
                           float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, void* stream) {
    if (check_composite(nullptr, n_rays, n_samples, rgb_stride, sigma_stride, d_rgb_stride, d_sigma_stride) != NRF_OK) return NRF_EINVAL;
    if (n_rays == 0) return NRF_OK;
    if (!rgb || !sigma || !z_vals || !rays_d || !d_rgb || !d_sigma) return fail(NRF_EINVAL, "null pointer");
    if (!g_rgb && !g_depth && !g_weights) return fail(NRF_EINVAL, "no incoming gradient");
    const int r = nrf::launch_composite_backward(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, g_rgb,
                                                 g_depth, g_weights, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, (hipStream_t)stream);
    return launched(r, "composite backward launch failed");
}

int nrf_composite_backward_geom(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals, const float* rays_d,
                                int64_t n_rays, int n_samples, int white_bkgd, const float* g_rgb, const float* g_depth, const float* g_weights,
                                float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* d_z, float* d_rays_d, void* stream) {
    if (check_composite(nullptr, n_rays, n_samples, rgb_stride, sigma_stride, d_rgb_stride, d_sigma_stride) != NRF_OK) return NRF_EINVAL;
    if (n_rays == 0) return NRF_OK;
    if (!rgb || !sigma || !z_vals || !rays_d || !d_rgb || !d_sigma || !d_z || !d_rays_d) return fail(NRF_EINVAL, "null pointer");
    if (!g_rgb && !g_depth && !g_weights) return fail(NRF_EINVAL, "no incoming gradient");
    const int r = nrf::launch_composite_backward_geom(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, g_rgb,
                                                      g_depth, g_weights, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, d_z, d_rays_d,
                                                      (hipStream_t)stream);
    return launched(r, "composite backward (geometry) launch failed");
}

int nrf_ray_grad(const float* d_points, const float* d_dirs, const float* z_vals, const float* rays_d, const float* d_z_in,
                 const float* d_rays_d_in, int64_t n_rays, int n_samples, float* d_rays_o, float* d_rays_d, float* d_z_out, void* stream) {
    if (n_rays < 0 || n_samples < 1 || n_samples > 4096) return fail(NRF_EINVAL, "bad sizes");
    if (n_rays == 0) return NRF_OK;
    if (!d_points || !z_vals || !rays_d) return fail(NRF_EINVAL, "null pointer");
    if (!d_rays_o && !d_rays_d && !d_z_out) return fail(NRF_EINVAL, "nrf_ray_grad: no output asked for");
    const int r = nrf::launch_ray_grad(d_points, d_dirs, z_vals, rays_d, d_z_in, d_rays_d_in, n_rays, n_samples, d_rays_o, d_rays_d, d_z_out,
                                       (hipStream_t)stream);
    return launched(r, "ray_grad launch failed");
}

int nrf_mse_grad(const float* pred, const float* target, int64_t n, float weight, float* g_pred, float* loss, void* stream) {
    if (n <= 0 || n > ((int64_t)1 << 22)) return fail(NRF_EINVAL, "nrf_mse_grad: n must be in 1 .. 2^22");
    if (!pred || !target || !g_pred || !loss) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_mse_grad(pred, target, n, weight, g_pred, loss, (hipStream_t)stream);
    return launched(r, "mse launch failed");
}

int nrf_composite_mse_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals, const float* rays_d,
                               int64_t n_rays, int n_samples, int white_bkgd, const float* target, float weight, float* pred, float* d_rgb,
                               int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_loss, float* zero_buf, int64_t zero_n,
                               void* stream) {
    if (check_composite("nrf_composite_mse_backward", n_rays, n_samples, rgb_stride, sigma_stride, d_rgb_stride, d_sigma_stride) != NRF_OK) return NRF_EINVAL;
    if (!rgb || !sigma || !z_vals || !rays_d || !target || !d_rgb || !d_sigma || !ray_loss) return fail(NRF_EINVAL, "null pointer");
    if (zero_n < 0 || (zero_n > 0 && !zero_buf)) return fail(NRF_EINVAL, "zero_buf is NULL");
    const int r = nrf::launch_composite_mse_backward(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target,
                                                     weight, pred, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_loss, zero_buf, zero_n,
                                                     (hipStream_t)stream);
    return launched(r, "composite + mse + backward launch failed");
}

int nrf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, void* stream) {
    if (n < 0 || step < 1) return fail(NRF_EINVAL, "bad n / step");
    if (n == 0) return NRF_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq) return fail(NRF_EINVAL, "null pointer");
    if (check_adam(beta1, beta2, eps) != NRF_OK) return NRF_EINVAL;
    const int r = nrf::launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, nullptr, 0, 0.0f, nullptr,
                                   (hipStream_t)stream);
    return launched(r, "adam launch failed");
}

int nrf_adam_step_loss(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int step, const float* ray_loss, int64_t n_rays, float loss_weight, float* loss,
                       void* stream) {
    if (n <= 0 || step < 1) return fail(NRF_EINVAL, "bad n / step");
    if (!params || !grads || !exp_avg || !exp_avg_sq) return fail(NRF_EINVAL, "null pointer");
    if (check_adam(beta1, beta2, eps) != NRF_OK) return NRF_EINVAL;
    if (!ray_loss || !loss || n_rays <= 0) return fail(NRF_EINVAL, "nrf_adam_step_loss: ray_loss / loss missing");
    const int r = nrf::launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, ray_loss, n_rays, loss_weight,
                                   loss, (hipStream_t)stream);
    return launched(r, "adam launch failed");
}

int nrf_composite_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals, const float* rays_d,
                                int64_t n_rays, int n_samples, int white_bkgd, const float* target, const nrf_loss_opts* loss, float* pred,
                                float* d_rgb, int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf,
                                int64_t zero_n, void* stream) {
    return composite_loss_backward_any(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target, loss, nullptr,
                                       pred, d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, stream, {});
}

int nrf_composite_loss_backward_indexed(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals,
                                        const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd, const float* target,
                                        const nrf_loss_opts* loss, const int32_t* slot, float* pred, float* d_rgb, int d_rgb_stride,
                                        float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf, int64_t zero_n, void* stream) {
    if (!slot) return fail(NRF_EINVAL, "nrf_composite_loss_backward_indexed: slot is NULL");
    if (!slot_aligned("nrf_composite_loss_backward_indexed", slot)) return NRF_EINVAL;
    return composite_loss_backward_any(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target, loss, slot, pred,
                                       d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, stream, {});
}

int nrf_composite_reg_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals,
                                    const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd, const float* target,
                                    const nrf_loss_opts* loss, const nrf_ray_reg* reg, const int32_t* slot, float* pred, float* d_rgb,
                                    int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf, int64_t zero_n,
                                    void* stream) {
    nrf::RayRegTerms rt{};
    if (!ray_reg_terms(reg, rt)) return NRF_EINVAL;
    if (!slot_aligned("nrf_composite_reg_loss_backward", slot)) return NRF_EINVAL;
    return composite_loss_backward_any(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target, loss, slot, pred,
                                       d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, stream, {&rt});
}

int nrf_ray_terms_finish(const float* ray_terms, int64_t n_rays, const nrf_ray_reg* reg, const float* losses4, float* losses6, void* stream) {
    nrf::RayRegTerms rt{};
    if (!ray_reg_terms(reg, rt)) return NRF_EINVAL;
    if (n_rays <= 0 || n_rays > ((int64_t)1 << 30)) return fail(NRF_EINVAL, "nrf_ray_terms_finish: bad sizes");
    if (!ray_terms || !losses4 || !losses6) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_ray_terms_finish(ray_terms, n_rays, rt.dist_weight, rt.occ_weight, losses4, losses6, (hipStream_t)stream);
    return launched(r, "ray terms finish launch failed");
}

int nrf_composite_patch_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals,
                                      const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd, const float* target,
                                      const nrf_loss_opts* loss, const nrf_ray_reg* reg, const int32_t* slot, float* pred, float* d_rgb,
                                      int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf, int64_t zero_n,
                                      void* stream, const nrf_patch_reg* patch, float* patch_terms, float* patch_depth) {
    nrf::RayRegTerms rt{};
    if (!ray_reg_terms(reg, rt)) return NRF_EINVAL;
    nrf::PatchRegTerms pt{};
    if (!patch_reg_terms(patch, n_rays, pt)) return NRF_EINVAL;
    if (pt.n_patches > 0 && !patch_terms) return fail(NRF_EINVAL, "nrf_composite_patch_loss_backward: patch_terms is NULL");
    if (!slot_aligned("nrf_composite_patch_loss_backward", slot)) return NRF_EINVAL;
    return composite_loss_backward_any(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target, loss, slot, pred,
                                       d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, stream,
                                       {&rt, &pt, nullptr, patch_terms, patch_depth});
}

int nrf_patch_terms_finish(const float* ray_terms, int64_t n_rays, int n_samples, const nrf_loss_opts* loss, const nrf_ray_reg* reg,
                           const nrf_patch_reg* patch, const float* patch_terms, float* losses7, void* stream) {
    nrf::RayRegTerms rt{};
    if (!ray_reg_terms(reg, rt)) return NRF_EINVAL;
    nrf::PatchRegTerms pt{};
    if (!patch_reg_terms(patch, n_rays, pt)) return NRF_EINVAL;
    nrf::LossTerms lt{};
    if (!loss_terms("nrf_patch_terms_finish", loss, lt)) return NRF_EINVAL;          // (loss->target_depth: a flag here, not read)
    if (!sizes_ok("nrf_patch_terms_finish", n_rays, n_samples)) return NRF_EINVAL;
    if (!ray_terms || !losses7 || (pt.n_patches > 0 && !patch_terms)) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_patch_terms_finish(ray_terms, n_rays, n_samples, lt, rt, pt, patch_terms, losses7, (hipStream_t)stream);
    return launched(r, "patch terms finish launch failed");
}

int nrf_composite_info_loss_backward(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* z_vals,
                                     const float* rays_d, int64_t n_rays, int n_samples, int white_bkgd, const float* target,
                                     const nrf_loss_opts* loss, const nrf_ray_reg* reg, const int32_t* slot, float* pred, float* d_rgb,
                                     int d_rgb_stride, float* d_sigma, int d_sigma_stride, float* ray_terms, float* zero_buf, int64_t zero_n,
                                     void* stream, const nrf_patch_reg* patch, float* patch_terms, float* patch_depth, const nrf_info_reg* info,
                                     float* info_terms, float* patch_kl) {
    nrf::RayRegTerms rt{};
    if (!ray_reg_terms(reg, rt)) return NRF_EINVAL;
    nrf::PatchRegTerms pt{};
    if (!patch_reg_terms(patch, n_rays, pt)) return NRF_EINVAL;
    nrf::InfoRegTerms it{};
    if (!info_reg_terms(info, pt, n_samples, it)) return NRF_EINVAL;
    if (pt.n_patches > 0 && !patch_terms) return fail(NRF_EINVAL, "nrf_composite_info_loss_backward: patch_terms is NULL");
    if (it.ent_weight > 0.0f && !info_terms) return fail(NRF_EINVAL, "nrf_composite_info_loss_backward: info_terms is NULL with ent_weight > 0");
    if (it.kl_weight > 0.0f && !patch_kl) return fail(NRF_EINVAL, "nrf_composite_info_loss_backward: patch_kl is NULL with kl_weight > 0");
    if (!slot_aligned("nrf_composite_info_loss_backward", slot)) return NRF_EINVAL;
    return composite_loss_backward_any(rgb, rgb_stride, sigma, sigma_stride, z_vals, rays_d, n_rays, n_samples, white_bkgd, target, loss, slot, pred,
                                       d_rgb, d_rgb_stride, d_sigma, d_sigma_stride, ray_terms, zero_buf, zero_n, stream,
                                       {&rt, &pt, &it, patch_terms, patch_depth, info_terms, patch_kl});
}

int nrf_info_terms_finish(const float* ray_terms, int64_t n_rays, int n_samples, const nrf_loss_opts* loss, const nrf_ray_reg* reg,
                          const nrf_patch_reg* patch, const float* patch_terms, const nrf_info_reg* info, const float* info_terms,
                          const float* patch_kl, float* losses9, void* stream) {
    nrf::RayRegTerms rt{};
    if (!ray_reg_terms(reg, rt)) return NRF_EINVAL;
    nrf::PatchRegTerms pt{};
    if (!patch_reg_terms(patch, n_rays, pt)) return NRF_EINVAL;
    nrf::InfoRegTerms it{};
    if (!info_reg_terms(info, pt, n_samples, it)) return NRF_EINVAL;
    nrf::LossTerms lt{};
    if (!loss_terms("nrf_info_terms_finish", loss, lt)) return NRF_EINVAL;
    if (!sizes_ok("nrf_info_terms_finish", n_rays, n_samples)) return NRF_EINVAL;
    if (!ray_terms || !losses9 || (pt.n_patches > 0 && !patch_terms) || (it.ent_weight > 0.0f && !info_terms) || (it.kl_weight > 0.0f && !patch_kl))
        return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_info_terms_finish(ray_terms, n_rays, n_samples, lt, rt, pt, it, patch_terms, info_terms, patch_kl, losses9,
                                                (hipStream_t)stream);
    return launched(r, "info terms finish launch failed");
}

int64_t nrf_hier_train_workspace_bytes(int64_t n_rays, int n_samples, int n_importance) {
    if (n_rays < 0 || n_samples < 1 || n_importance < 1 || (int64_t)n_samples + n_importance > 4096) {
        (void)fail(NRF_EINVAL, "nrf_hier_train_workspace_bytes: bad sizes");
        return -1;
    }
    return nrf::hier_train_ws_bytes(n_rays, n_samples, n_importance);
}

int nrf_composite_hier_loss_backward(const nrf_hier_loss* a, int64_t n_rays, int n_samples, int n_importance, void* stream) {
    const std::string w = "nrf_composite_hier_loss_backward";
    if (!a) return fail(NRF_EINVAL, w + ": a is NULL");
    if (a->struct_bytes != (int32_t)sizeof(nrf_hier_loss)) return fail(NRF_EINVAL, w + ": nrf_hier_loss: struct_bytes is not sizeof(nrf_hier_loss)");
    if (n_rays < 0 || n_rays > ((int64_t)1 << 30)) return fail(NRF_EINVAL, w + ": n_rays < 0 or too large");
    if (n_samples < 1) return fail(NRF_EINVAL, w + ": n_samples < 1");
    if (n_importance < 1) return fail(NRF_EINVAL, w + ": n_importance < 1");
    if ((int64_t)n_samples + n_importance > 4096) return fail(NRF_EINVAL, w + ": n_samples + n_importance > 4096");
    if (a->rgb_stride < 3 || a->sigma_stride < 1) return fail(NRF_EINVAL, w + ": bad strides");
    if (!(a->w_coarse >= 0.0f) || !(a->w_fine >= 0.0f) || !std::isfinite(a->w_coarse) || !std::isfinite(a->w_fine))
        return fail(NRF_EINVAL, w + ": w_coarse and w_fine must be finite and >= 0");
    if (!a->rgb_coarse || !a->sigma_coarse || !a->rgb_new || !a->sigma_new || !a->z_coarse || !a->z_new || !a->rays_d || !a->target ||
        !a->d_rgb_coarse || !a->d_sigma_coarse || !a->d_rgb_new || !a->d_sigma_new)
        return fail(NRF_EINVAL, w + ": null pointer");
    if (!a->ray_loss) return fail(NRF_EINVAL, w + ": ray_loss is NULL");
    if (misaligned(3, {a->rgb_coarse, a->sigma_coarse, a->rgb_new, a->sigma_new, a->z_coarse, a->z_new, a->rays_d, a->target, a->d_rgb_coarse,
                       a->d_sigma_coarse, a->d_rgb_new, a->d_sigma_new, a->pred_coarse, a->pred_fine, a->ray_loss, a->ray_parts, a->z_union,
                       a->weights_fine, a->zero_buf}))
        return fail(NRF_EINVAL, w + ": float tensors must be 4-byte aligned");
    if (a->zero_n < 0 || (a->zero_n > 0 && !a->zero_buf)) return fail(NRF_EINVAL, w + ": zero_buf is NULL");
    if (!a->workspace) return fail(NRF_EINVAL, w + ": workspace is NULL");
    if (misaligned(15, {a->workspace})) return fail(NRF_EINVAL, w + ": workspace must be 16-byte aligned");
    if (a->workspace_bytes < nrf::hier_train_ws_bytes(n_rays, n_samples, n_importance))
        return fail(NRF_EINVAL, w + ": workspace smaller than nrf_hier_train_workspace_bytes");
    if (n_rays == 0) return NRF_OK;
    nrf::HierTrainArgs h{};
    h.white_bkgd = a->white_bkgd; h.rgb_stride = a->rgb_stride; h.sigma_stride = a->sigma_stride;
    h.rgb_coarse = a->rgb_coarse; h.sigma_coarse = a->sigma_coarse; h.rgb_new = a->rgb_new; h.sigma_new = a->sigma_new;
    h.z_coarse = a->z_coarse; h.z_new = a->z_new; h.rays_d = a->rays_d; h.target = a->target;
    h.w_coarse = a->w_coarse; h.w_fine = a->w_fine;
    h.d_rgb_coarse = a->d_rgb_coarse; h.d_sigma_coarse = a->d_sigma_coarse; h.d_rgb_new = a->d_rgb_new; h.d_sigma_new = a->d_sigma_new;
    h.pred_coarse = a->pred_coarse; h.pred_fine = a->pred_fine; h.ray_loss = a->ray_loss; h.ray_parts = a->ray_parts;
    h.z_union = a->z_union; h.weights_fine = a->weights_fine; h.zero_buf = a->zero_buf; h.zero_n = a->zero_n; h.workspace = a->workspace;
    const int r = nrf::launch_hier_loss_backward(h, n_rays, n_samples, n_importance, (hipStream_t)stream);
    return launched(r, "nrf_composite_hier_loss_backward: launch failed");
}

int64_t nrf_occupancy_compact_workspace_bytes(int64_t n_rays) {
    if (n_rays < 0) { (void)fail(NRF_EINVAL, "nrf_occupancy_compact_workspace_bytes: n_rays < 0"); return -1; }
    return nrf::occupancy_compact_ws_bytes(n_rays);
}

int nrf_occupancy_compact_rays(const nrf_train_rays* rays, int64_t n_rays, const nrf_render_opts* opts, const nrf_occupancy* occ,
                               const nrf_compact* out, void* stream) {
    // the order of nrf_mlp_forward_train_rays: the ray source and the options, then the grid, then the outputs
    const int rc = check_ray_source("nrf_occupancy_compact_rays", rays, n_rays, opts, "composites every sample of the ladder", kNoZVals);
    if (rc != NRF_OK) return rc;
    if (check_occ(occ, n_rays) != NRF_OK) return NRF_EINVAL;
    if (!out) return fail(NRF_EINVAL, "nrf_occupancy_compact_rays: out is NULL");
    if (out->struct_bytes != (int32_t)sizeof(nrf_compact)) return fail(NRF_EINVAL, "nrf_compact: struct_bytes is not sizeof(nrf_compact)");
    if (!out->index || !out->slot || !out->positions || !out->count)
        return fail(NRF_EINVAL, "nrf_compact: outputs index, slot, positions and count are required");
    if (out->capacity < (int64_t)opts->n_samples * n_rays)
        return fail(NRF_EINVAL, "nrf_compact: capacity is below n_rays * n_samples (M is not known before the call)");
    if (misaligned(3, {out->index, out->slot, out->positions, out->directions, rays->z_vals, rays->rays_d_out, out->workspace}))
        return fail(NRF_EINVAL, "nrf_compact: index, slot, positions, directions, z_vals, rays_d_out and workspace must be 4-byte aligned");
    if (misaligned(7, {out->count})) return fail(NRF_EINVAL, "nrf_compact: count must be 8-byte aligned");
    if (!out->workspace) return fail(NRF_EINVAL, "nrf_compact: workspace is NULL");
    if (out->workspace_bytes < nrf::occupancy_compact_ws_bytes(n_rays))
        return fail(NRF_EINVAL, "nrf_compact: workspace smaller than nrf_occupancy_compact_workspace_bytes");
    if (n_rays == 0) return NRF_OK;
    nrf::TrainRaysDev r{};
    fill_ray_source(r, rays, opts, true);
    r.points_out = nullptr;                                     // (rays->points_out is not used: nerfhip.h)
    const int rl = nrf::launch_occupancy_compact(r, n_rays, make_occ(occ), out->capacity, out->index, out->slot, out->positions, out->directions,
                                                 out->count, out->workspace, (hipStream_t)stream);
    return launched(rl, "occupancy_compact launch failed");
}

int64_t nrf_grad_sqnorm_workspace_bytes(int64_t n) {
    if (n <= 0) { (void)fail(NRF_EINVAL, "nrf_grad_sqnorm_workspace_bytes: n must be positive"); return -1; }
    return 4 * (int64_t)nrf::sqnorm_partials(n);
}

int nrf_grad_sqnorm_partials(const float* grads, int64_t n, void* workspace, int64_t workspace_bytes, void* stream) {
    if (n <= 0) return fail(NRF_EINVAL, "nrf_grad_sqnorm_partials: n must be positive");
    if (!grads) return fail(NRF_EINVAL, "null pointer");
    if (!workspace) return fail(NRF_EINVAL, "norm workspace is NULL");
    if (misaligned(3, {workspace})) return fail(NRF_EINVAL, "norm workspace must be 4-byte aligned");
    if (workspace_bytes < 4 * (int64_t)nrf::sqnorm_partials(n)) return fail(NRF_EINVAL, "norm workspace smaller than nrf_grad_sqnorm_workspace_bytes");
    const int r = nrf::launch_grad_sqnorm_partials(grads, n, (float*)workspace, (hipStream_t)stream);
    return launched(r, "norm partials launch failed");
}

int nrf_adamw_step_loss(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int step, int decoupled, float max_norm, const float* sqnorm_partials, float* grad_norm,
                        const float* ray_terms, int64_t n_rays, int n_samples, float rgb_weight, float depth_weight, float reg_weight,
                        float* losses, void* stream) {
    if (n <= 0 || step < 1) return fail(NRF_EINVAL, "bad n / step");
    if (!params || !grads || !exp_avg || !exp_avg_sq) return fail(NRF_EINVAL, "null pointer");
    if (check_adam(beta1, beta2, eps) != NRF_OK) return NRF_EINVAL;
    if (std::isnan(max_norm)) return fail(NRF_EINVAL, "max_norm is NaN");
    if (max_norm > 0.0f && !sqnorm_partials) return fail(NRF_EINVAL, "max_norm > 0 needs the partial sums of nrf_grad_sqnorm_partials");
    if (grad_norm && !sqnorm_partials) return fail(NRF_EINVAL, "grad_norm needs the partial sums of nrf_grad_sqnorm_partials");
    if ((ray_terms == nullptr) != (losses == nullptr)) return fail(NRF_EINVAL, "nrf_adamw_step_loss: ray_terms and losses go together");
    if (ray_terms && (n_rays <= 0 || n_samples < 1)) return fail(NRF_EINVAL, "nrf_adamw_step_loss: bad n_rays / n_samples");
    if (ray_terms && (!(rgb_weight >= 0.0f) || !(depth_weight >= 0.0f) || !(reg_weight >= 0.0f))) return fail(NRF_EINVAL, "loss weights must be >= 0");
    nrf::AdamExt e{};
    e.decoupled = decoupled ? 1 : 0; e.max_norm = max_norm; e.partials = sqnorm_partials; e.grad_norm = grad_norm;
    e.ray_terms = ray_terms; e.n_rays = n_rays; e.n_samples = n_samples;
    e.rgb_weight = rgb_weight; e.depth_weight = depth_weight; e.reg_weight = reg_weight; e.losses = losses;
    const int r = nrf::launch_adamw(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, e, (hipStream_t)stream);
    return launched(r, "adamw launch failed");
}

int nrf_sample_pdf(const float* z_vals, const float* weights, int64_t n_rays, int n_samples, int n_importance, const float* u, int64_t u_ray_stride,
                   float* samples, float* z_union, void* stream) {
    if (n_rays < 0 || n_samples < 2 || n_importance < 1) return fail(NRF_EINVAL, "bad sizes");
    if (n_rays == 0) return NRF_OK;
    if (!z_vals || !weights || (!samples && !z_union)) return fail(NRF_EINVAL, "null pointer");
    if (u && u_ray_stride != 0 && u_ray_stride < n_importance) return fail(NRF_EINVAL, "u_ray_stride must be 0 (one shared row) or >= n_importance");
    const int r = nrf::launch_sample_pdf(z_vals, weights, n_rays, n_samples, n_importance, u, u_ray_stride, samples, z_union, (hipStream_t)stream);
    return launched(r, r == NRF_EINVAL ? "n_samples + n_importance too large for one LDS row" : "sample_pdf launch failed");
}

int nrf_sample_pdf_sorted(const float* z_vals, const float* weights, int64_t n_rays, int n_samples, int n_importance, const float* u,
                          int64_t u_ray_stride, float* samples, float* samples_sorted, float* z_union, void* stream) {
    if (n_rays < 0 || n_samples < 2 || n_importance < 1) return fail(NRF_EINVAL, "bad sizes");
    if (n_rays == 0) return NRF_OK;
    if (!z_vals || !weights || (!samples && !samples_sorted && !z_union)) return fail(NRF_EINVAL, "null pointer");
    if (u && u_ray_stride != 0 && u_ray_stride < n_importance) return fail(NRF_EINVAL, "u_ray_stride must be 0 (one shared row) or >= n_importance");
    const int r = nrf::launch_sample_pdf_sorted(z_vals, weights, n_rays, n_samples, n_importance, u, u_ray_stride, samples, samples_sorted, z_union,
                                                (hipStream_t)stream);
    return launched(r, r == NRF_EINVAL ? "n_samples + n_importance too large for one LDS row" : "sample_pdf launch failed");
}

int64_t nrf_hier_workspace_bytes(int64_t n_rays, int n_samples, int n_importance) {
    if (n_rays < 0 || n_samples < 1 || n_importance < 0) { (void)fail(NRF_EINVAL, "nrf_hier_workspace_bytes: bad sizes"); return -1; }
    // coarse depths, weights and rows; new depths and rows
    return n_rays * ((int64_t)n_samples * (4 + 4 + 16) + (int64_t)n_importance * (4 + 16));
}

int nrf_composite_merge(const float* z_coarse, const float* raw_coarse, const float* z_new, const float* raw_new, const float* rays_d,
                        int64_t n_rays, int n_samples, int n_importance, int mma_mode, int white_bkgd, int out_rgbd, float* rgb, float* depth,
                        float* weights, float* z_union, void* stream) {
    if (n_rays > 0 && !rays_d) return fail(NRF_EINVAL, "null pointer");
    nrf::MergeArgs a{};
    a.z_coarse = z_coarse; a.raw_coarse = raw_coarse; a.z_new = z_new; a.raw_new = raw_new; a.rays_d = rays_d;
    a.n_rays = n_rays; a.S = n_samples; a.Ni = n_importance; a.white_bkgd = white_bkgd;
    a.rgb = rgb; a.depth = depth; a.weights = weights; a.z_union = z_union;
    return composite_merge_any(a, mma_mode, out_rgbd, stream);
}

int nrf_composite_merge_camera(const float* z_coarse, const float* raw_coarse, const float* z_new, const float* raw_new, int H, int W, float focal,
                               const float c2w[12], int64_t ray_begin, int64_t ray_end, int n_samples, int n_importance, int mma_mode,
                               int white_bkgd, int out_rgbd, float* rgb, float* depth, float* weights, float* z_union, void* stream) {
    if (check_camera(H, W, focal, c2w) != NRF_OK || check_ray_range(H, W, ray_begin, ray_end) != NRF_OK) return NRF_EINVAL;
    nrf::MergeArgs a{};
    a.z_coarse = z_coarse; a.raw_coarse = raw_coarse; a.z_new = z_new; a.raw_new = raw_new; a.rays_d = nullptr;
    a.cam = make_camera(H, W, focal, c2w); a.ray_begin = ray_begin;
    a.n_rays = ray_end - ray_begin; a.S = n_samples; a.Ni = n_importance; a.white_bkgd = white_bkgd;
    a.rgb = rgb; a.depth = depth; a.weights = weights; a.z_union = z_union;
    return composite_merge_any(a, mma_mode, out_rgbd, stream);
}

int nrf_debug_pack(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode, uint8_t* stream_out, int64_t stream_cap,
                   int64_t* stream_bytes, float* bias_out, int64_t bias_cap, int64_t* n_bias) {
    const BiasOut bias{bias_out, bias_cap, n_bias};
    return debug_pack("nrf_debug_pack", planned<nrf::make_plan>, nrf::kModes, arch, linears, n_linear, mma_mode, stream_out, stream_cap, stream_bytes, &bias);
}

int nrf_sample_features(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, float* feats, void* stream) {
    if (n < 0 || Hp < 1 || Wp < 1 || C < 1) return fail(NRF_EINVAL, "bad sizes");
    if (n == 0) return NRF_OK;
    if (!features || !points_2d || !feats) return fail(NRF_EINVAL, "null pointer");
    const int r = nrf::launch_sample_features(features, Hp, Wp, C, points_2d, n, feats, (hipStream_t)stream);
    return launched(r, "sample_features launch failed");
}

int64_t nrf_fetch_backward_workspace_bytes(int Hp, int Wp, int C, int64_t n) {
    if (n < 0 || Hp < 1 || Wp < 1 || C < 1) { (void)fail(NRF_EINVAL, "nrf_fetch_backward_workspace_bytes: bad sizes"); return -1; }
    return 4 * nrf::fetch_backward_ws_floats(Hp, Wp, C, n);
}

int nrf_project_fetch_backward(const nrf_dino* dino, const float* points, int64_t n, const float* d_feats, float* d_map, int accumulate, void* ws,
                               int64_t ws_bytes, void* stream) {
    if (!dino) return fail(NRF_EINVAL, "dino is NULL");
    if (dino->Hp < 1 || dino->Wp < 1 || dino->C < 1 || dino->H < 1 || dino->W < 1) return fail(NRF_EINVAL, "dino: bad map / image size");
    const int c = fetch_backward_check(dino->Hp, dino->Wp, dino->C, points, n, d_feats, d_map, accumulate, ws, ws_bytes);
    if (c != NRF_OK) return c == 1 ? NRF_OK : c;
    nrf::DinoDev d{};                                       // the map itself (dino->features) is not read
    d.Hp = dino->Hp; d.Wp = dino->Wp; d.C = dino->C;
    std::memcpy(d.inv_pose, dino->inv_pose, sizeof(float) * 12);
    d.focal = dino->focal; d.H = dino->H; d.W = dino->W;
    const int r = nrf::launch_project_fetch_backward(d, points, n, d_feats, d_map, accumulate, (float*)ws, (hipStream_t)stream);
    return launched(r, "project_fetch backward launch failed");
}

int nrf_sample_features_backward(int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats, float* d_map, int accumulate,
                                 void* ws, int64_t ws_bytes, void* stream) {
    const int c = fetch_backward_check(Hp, Wp, C, points_2d, n, d_feats, d_map, accumulate, ws, ws_bytes);
    if (c != NRF_OK) return c == 1 ? NRF_OK : c;
    const int r = nrf::launch_sample_features_backward(Hp, Wp, C, points_2d, n, d_feats, d_map, accumulate, (float*)ws, (hipStream_t)stream);
    return launched(r, "sample_features backward launch failed");
}

int nrf_project_fetch_backward_points(const nrf_dino* dino, const float* points, int64_t n, const float* d_feats, float* d_points, int accumulate,
                                      void* stream) {
    if (n < 0) return fail(NRF_EINVAL, "n < 0");
    if (n == 0) return NRF_OK;
    if (!points || !d_feats || !d_points) return fail(NRF_EINVAL, "null pointer");
    if (misaligned(3, {points, d_feats, d_points}))
        return fail(NRF_EINVAL, "nrf_project_fetch_backward_points: float tensors must be 4-byte aligned");
    nrf::DinoDev d{};
    std::string err;
    if (!make_dino(dino, 0, d, err)) return fail(NRF_EINVAL, err);
    if (misaligned(3, {d.features})) return fail(NRF_EINVAL, "nrf_project_fetch_backward_points: float tensors must be 4-byte aligned");
    const int r = nrf::launch_project_fetch_backward_points(d, points, n, d_feats, d_points, accumulate, (hipStream_t)stream);
    return launched(r, "project_fetch backward (points) launch failed");
}

int nrf_sample_features_backward_points(const float* features, int Hp, int Wp, int C, const float* points_2d, int64_t n, const float* d_feats,
                                        float* d_xy, void* stream) {
    if (n < 0 || Hp < 1 || Wp < 1 || C < 1) return fail(NRF_EINVAL, "bad sizes");
    if (n == 0) return NRF_OK;
    if (!features || !points_2d || !d_feats || !d_xy) return fail(NRF_EINVAL, "null pointer");
    if (misaligned(3, {features, points_2d, d_feats, d_xy}))
        return fail(NRF_EINVAL, "nrf_sample_features_backward_points: float tensors must be 4-byte aligned");
    const int r = nrf::launch_sample_features_backward_points(features, Hp, Wp, C, points_2d, n, d_feats, d_xy, (hipStream_t)stream);
    return launched(r, "sample_features backward (points) launch failed");
}

int nrf_debug_pack_dino_grad(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode, uint8_t* stream_out, int64_t stream_cap,
                             int64_t* stream_bytes) {
    return debug_pack("nrf_debug_pack_dino_grad", planned<nrf::make_dino_grad_plan>, 3, arch, linears, n_linear, mma_mode, stream_out, stream_cap, stream_bytes);
}

int nrf_debug_pack_input_grad(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode, uint8_t* stream_out, int64_t stream_cap,
                              int64_t* stream_bytes) {
    return debug_pack("nrf_debug_pack_input_grad", planned<nrf::make_input_grad_plan>, 3, arch, linears, n_linear, mma_mode, stream_out, stream_cap, stream_bytes);
}

int nrf_debug_pack_input_grad_v3(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode, uint8_t* stream_out, int64_t stream_cap,
                                 int64_t* stream_bytes) {
    return debug_pack("nrf_debug_pack_input_grad_v3", planned<nrf::make_input_grad_v3_plan>, 3, arch, linears, n_linear, mma_mode, stream_out, stream_cap, stream_bytes);
}

int nrf_debug_pack_backward(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int mma_mode, uint8_t* stream_out, int64_t stream_cap,
                            int64_t* stream_bytes) {
    return debug_pack("nrf_debug_pack_backward", planned_backward, 3, arch, linears, n_linear, mma_mode, stream_out, stream_cap, stream_bytes);
}

int nrf_debug_train_plan(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int32_t* out, int64_t cap, int64_t* n_ints) {
    if (debug_args("nrf_debug_train_plan", arch, linears, n_linear) != NRF_OK) return NRF_EINVAL;
    Linears lin;
    nrf::NetPlan plan;
    nrf::TrainPlan tp;
    const int rc = debug_plan(arch, linears, n_linear, planned<nrf::make_plan>, lin, plan);
    if (rc != NRF_OK) return rc;
    std::string err;
    if (!nrf::make_train_plan(*arch, plan, nrf::param_layout(lin), tp, err)) return fail(NRF_EUNSUPPORTED, err);
    std::vector<int32_t> v;
    v.push_back((int32_t)tp.slot_tiles.size());
    v.insert(v.end(), tp.slot_tiles.begin(), tp.slot_tiles.end());
    v.push_back((int32_t)tp.jobs.size());
    for (const auto& J : tp.jobs) {
        v.push_back(J.x_slot); v.push_back(J.dz_slot); v.push_back(J.KT); v.push_back(J.MT); v.push_back(J.x_first);
        v.insert(v.end(), J.row_w.begin(), J.row_w.end());
        v.insert(v.end(), J.row_b.begin(), J.row_b.end());
        v.insert(v.end(), J.col.begin(), J.col.end());
    }
    v.push_back(tp.n_mask_slots);
    if (n_ints) *n_ints = (int64_t)v.size();
    return copy_out(out, cap, v, "out too small");
}

int nrf_debug_freq_mask_ids(const nrf_arch* arch, const nrf_linear* linears, int n_linear, int8_t* out, int64_t cap, int64_t* n_ids) {
    if (debug_args("nrf_debug_freq_mask_ids", arch, linears, n_linear) != NRF_OK) return NRF_EINVAL;
    Linears lin;
    nrf::NetPlan plan;
    const int rc = debug_plan(arch, linears, n_linear, planned<nrf::make_plan>, lin, plan);
    if (rc != NRF_OK) return rc;
    const std::vector<int8_t> ids = nrf::freq_scale_ids(*arch, nrf::param_layout(lin));
    if (n_ids) *n_ids = (int64_t)ids.size();
    return copy_out(out, cap, ids, "out too small");
}

int nrf_debug_ray_deal(int64_t n_rays, int n_samples, int cols_per_wave, int n_cu, int64_t* head, int64_t* items, int64_t cap, int64_t* n_items) {
    if (n_rays <= 0 || n_samples <= 0 || n_cu <= 0 || (cols_per_wave != 32 && cols_per_wave != 64) || !head)
        return fail(NRF_EINVAL, "nrf_debug_ray_deal: bad argument");
    constexpr int waves = 4;                                  // both renderers run 4 waves
    const int whole = waves * cols_per_wave;
    const nrf::Deal d = nrf::pick_deal(n_rays, n_samples, waves, cols_per_wave, n_cu);
    const int64_t grid = d.items < n_cu ? d.items : n_cu;
    head[0] = d.even; head[1] = d.spw_log2; head[2] = grid; head[3] = d.passes;
    int64_t n = 0;
    auto put = [&](int64_t b, int64_t first, int64_t rays, int l) {
        if (items && n < cap) { items[4 * n] = b; items[4 * n + 1] = first; items[4 * n + 2] = rays; items[4 * n + 3] = l; }
        ++n;
    };
    for (int64_t b = 0; b < grid; ++b) {                     // the walk of render_march
        if (d.even) {
            nrf::DealRange r = nrf::deal_range(d.items, grid, b, waves);
            while (r.rays > 0) {
                const int l = nrf::deal_split(r.rays, whole);
                put(b, r.first, whole >> l, l);
                r.first += whole >> l;
                r.rays -= whole >> l;
            }
        } else {
            const int64_t tile = whole >> d.spw_log2;
            for (int64_t t = b; t < d.items; t += grid) put(b, t * tile, tile, d.spw_log2);
        }
    }
    if (n_items) *n_items = n;
    if (items && cap < n) return fail(NRF_EINVAL, "items too small");
    return NRF_OK;
}

int nrf_project_fetch(const nrf_dino* dino, const float* points, int64_t n, float* feats, float* xy, void* stream) {
    if (n < 0) return fail(NRF_EINVAL, "n < 0");
    if (n == 0) return NRF_OK;
    if (!points || !feats) return fail(NRF_EINVAL, "null pointer");
    nrf::DinoDev d{};
    std::string err;
    if (!make_dino(dino, 0, d, err)) return fail(NRF_EINVAL, err);
    const int r = nrf::launch_project_fetch(d, points, n, feats, xy, (hipStream_t)stream);
    return launched(r, "project_fetch launch failed");
}

}  // extern "C"
