// fused_kernels.hip -- host-side routing of the fused renderer / staged MLP forward to the per-family translation units
#include "fused_impl.hpp"

namespace nrf {

int launch_render(const DeviceNet& net, int mode, const RenderArgs& a, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    if (net.arch.net == NRF_NET_V1 && net.arch.pos_freq == 10) return render_v1(net, mode, a, s, err);
    if (net.arch.net == NRF_NET_V2 && net.arch.pos_freq == 10) return render_v2(net, mode, a, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 64) return render_v3(net, mode, a, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 128) return render_v3w(net, mode, a, s, err);
    err = "no fused renderer built for this (net, pos_freq): V1/V2 with pos_freq 10 (baseline.yaml) and V3 with pos_freq 12 and dino_dim 64/128 (dino_nerf.yaml, lora.yaml, multiscale.yaml) are";
    return NRF_EUNSUPPORTED;
}

int launch_render_occ(const DeviceNet& net, int mode, const RenderArgs& a, const OccDev& g, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    if (net.arch.net == NRF_NET_V1 && net.arch.pos_freq == 10) return render_occ_v1(net, mode, a, g, s, err);
    if (net.arch.net == NRF_NET_V2 && net.arch.pos_freq == 10) return render_occ_v2(net, mode, a, g, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 64) return render_occ_v3(net, mode, a, g, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 128) return render_occ_v3w(net, mode, a, g, s, err);
    err = "no fused renderer built for this (net, pos_freq): see nrf_render_rays";
    return NRF_EUNSUPPORTED;
}

int launch_render_emit(const DeviceNet& net, int mode, const RenderArgs& a, float* raw4, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    if (net.arch.net == NRF_NET_V1 && net.arch.pos_freq == 10) return render_emit_v1(net, mode, a, raw4, s, err);
    if (net.arch.net == NRF_NET_V2 && net.arch.pos_freq == 10) return render_emit_v2(net, mode, a, raw4, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 64) return render_emit_v3(net, mode, a, raw4, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 128) return render_emit_v3w(net, mode, a, raw4, s, err);
    err = "no fused renderer built for this (net, pos_freq): see nrf_render_rays";
    return NRF_EUNSUPPORTED;
}

int launch_render_tail(const DeviceNet& net, int base_mode, const RenderArgs& a, float* carry, hipStream_t s, std::string& err) {
    if (!check_net(net, base_mode, err) || !check_net(net, NRF_MMA_F16X3, err)) return NRF_EINVAL;
    if (a.n_rays <= 0) return NRF_OK;
    const bool prefix = a.n_samples > 1;       // n_samples == 1: the state is the reset state and the render is the tail launch alone
    int rc = NRF_OK;
    if (net.arch.net == NRF_NET_V1 && net.arch.pos_freq == 10) {
        if (prefix) rc = render_hold_v1_16(net, base_mode, a, carry, s, err);
        return rc != NRF_OK ? rc : render_tail_v1(net, a, carry, s, err);
    }
    if (net.arch.net == NRF_NET_V2 && net.arch.pos_freq == 10) {
        if (prefix) rc = render_hold_v2_16(net, base_mode, a, carry, s, err);
        return rc != NRF_OK ? rc : render_tail_v2(net, a, carry, s, err);
    }
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 64) {
        if (prefix) rc = render_hold_v3_16(net, base_mode, a, carry, s, err);
        return rc != NRF_OK ? rc : render_tail_v3(net, a, carry, s, err);
    }
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12 && net.arch.dino_dim == 128) {
        if (prefix) rc = render_hold_v3w_16(net, base_mode, a, carry, s, err);
        return rc != NRF_OK ? rc : render_tail_v3w(net, a, carry, s, err);
    }
    err = "no fused renderer built for this (net, pos_freq): see nrf_render_rays";
    return NRF_EUNSUPPORTED;
}

int launch_forward_v1(const DeviceNet& net, int mode, const float* x_enc, int64_t n, float* out4, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (net.arch.net != NRF_NET_V1) { err = "nrf_mlp_forward_v1 needs a V1 model"; return NRF_EINVAL; }
    if (n <= 0) return NRF_OK;
    ForwardKArgs k{};
    k.x_enc = x_enc; k.n = n; k.out4 = out4;
    if (net.arch.pos_freq == 10) return forward_v1(net, mode, k, s, err);
    err = "no V1 forward built for this pos_freq";
    return NRF_EUNSUPPORTED;
}

int launch_forward(const DeviceNet& net, int mode, const float* pos, const float* dir, const float* dino, int64_t n,
                   float* rgb, float* density, hipStream_t s, std::string& err) {
    if (!check_net(net, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    ForwardKArgs k{};
    k.pos = pos; k.dir = dir; k.dino = dino; k.n = n; k.rgb = rgb; k.density = density;
    if (net.arch.net == NRF_NET_V2 && net.arch.pos_freq == 10) return forward_v2(net, mode, k, s, err);
    if (net.arch.net == NRF_NET_V3 && net.arch.pos_freq == 12) {
        if (!dino) { err = "V3 forward needs per-sample dino features"; return NRF_EINVAL; }
        if (net.arch.dino_dim == 64) return forward_v3(net, mode, k, s, err);
        if (net.arch.dino_dim == 128) return forward_v3w(net, mode, k, s, err);
    }
    err = "no forward built for this (net, pos_freq)";
    return NRF_EUNSUPPORTED;
}

}  // namespace nrf
