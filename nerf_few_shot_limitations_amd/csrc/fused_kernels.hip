// fused_kernels.hip -- host-side routing of the fused renderer / staged MLP forward to the per-family objects (fused_inst.hip)
#include "fused_impl.hpp"

namespace nrf {

namespace {

// A family as the routers see it: the arch it serves (dino_dim 0: any) and its entry point of every kind.
struct Family {
    int net, pos_freq, dino_dim;
    decltype(&render_v1) render;
    decltype(&forward_v1) forward;
    decltype(&render_occ_v1) render_occ;
    decltype(&render_emit_v1) render_emit;
    decltype(&render_hold_v1_16) render_hold;
    decltype(&render_tail_v1) render_tail;
};
#define NRF_FAMILY_ROW(fam, NETT, LP, NET, PF, DD) {NET, PF, DD, render_##fam, forward_##fam, render_occ_##fam, render_emit_##fam, render_hold_##fam##_16, render_tail_##fam},
const Family kFamilies[] = {NRF_FAMILIES(NRF_FAMILY_ROW)};

// the family built for this arch, or nullptr
const Family* family_of(const nrf_arch& arch) {
    for (const Family& f : kFamilies)
        if (arch.net == f.net && arch.pos_freq == f.pos_freq && (f.dino_dim == 0 || arch.dino_dim == f.dino_dim)) return &f;
    return nullptr;
}

const char* const kNoRenderer = "no fused renderer built for this (net, pos_freq): see nrf_render_rays";

}  // namespace

int launch_render(const DeviceNet& net, int mode, const RenderArgs& a, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    if (const Family* f = family_of(net.arch)) return f->render(net, mode, a, s, err);
    err = "no fused renderer built for this (net, pos_freq): V1/V2 with pos_freq 10 (baseline.yaml) and V3 with pos_freq 12 and dino_dim 64/128 (dino_nerf.yaml, lora.yaml, multiscale.yaml) are";
    return NRF_EUNSUPPORTED;
}

int launch_render_occ(const DeviceNet& net, int mode, const RenderArgs& a, const OccDev& g, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    if (const Family* f = family_of(net.arch)) return f->render_occ(net, mode, a, g, s, err);
    err = kNoRenderer;
    return NRF_EUNSUPPORTED;
}

int launch_render_emit(const DeviceNet& net, int mode, const RenderArgs& a, float* raw4, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    if (const Family* f = family_of(net.arch)) return f->render_emit(net, mode, a, raw4, s, err);
    err = kNoRenderer;
    return NRF_EUNSUPPORTED;
}

int launch_render_tail(const DeviceNet& net, int base_mode, const RenderArgs& a, float* carry, hipStream_t s, std::string& err) {
    if (!check_net(net, base_mode, err) || !check_net(net, NRF_MMA_F16X3, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    const bool prefix = a.n_samples > 1;       // n_samples == 1: the state is the reset state and the render is the tail launch alone
    if (const Family* f = family_of(net.arch)) {
        const int rc = prefix ? f->render_hold(net, base_mode, a, carry, s, err) : NRF_OK;
        return rc != NRF_OK ? rc : f->render_tail(net, a, carry, s, err);
    }
    err = kNoRenderer;
    return NRF_EUNSUPPORTED;
}

int launch_forward_v1(const DeviceNet& net, int mode, const float* x_enc, int64_t n, float* out4, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (net.arch.net != NRF_NET_V1) { err = "nrf_mlp_forward_v1 needs a V1 model"; return NRF_EINVAL; }
    if (n <= 0) return NRF_OK;
    ForwardKArgs k{};
    k.x_enc = x_enc; k.n = n; k.out4 = out4;
    if (const Family* f = family_of(net.arch)) return f->forward(net, mode, k, s, err);
    err = "no V1 forward built for this pos_freq";
    return NRF_EUNSUPPORTED;
}

// (a V1 model goes through launch_forward_v1: its kernel reads encoded inputs)
int launch_forward(const DeviceNet& net, int mode, const float* pos, const float* dir, const float* dino, int64_t n,
                   float* rgb, float* density, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    ForwardKArgs k{};
    k.pos = pos; k.dir = dir; k.dino = dino; k.n = n; k.rgb = rgb; k.density = density;
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && !dino) { err = "V3 forward needs per-sample dino features"; return NRF_EINVAL; }
    const Family* f = net.arch.net == NRF_NET_V1 ? nullptr : family_of(net.arch);
    if (f) return f->forward(net, mode, k, s, err);
    err = "no forward built for this (net, pos_freq)";
    return NRF_EUNSUPPORTED;
}

}  // namespace nrf
