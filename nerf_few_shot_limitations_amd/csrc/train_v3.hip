// train_v3.hip -- host entry points of the V3 (NeRFWithDINO) training kernels (pos_freq 12, dir_freq 4, dino_dim 64 / 128)
#include "train_v3_impl.hpp"

namespace nrf {

namespace {

bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return false;
    if (net.arch.net != NRF_NET_V3 || net.arch.dir_freq != 4 || (net.arch.dino_dim != 64 && net.arch.dino_dim != 128)) {
        err = "V3 training needs dir_freq 4 and dino_dim 64 or 128";
        return false;
    }
    if (net.arch.n_layers > 8) { err = "V3 training: at most 8 trunk layers (saved-tensor slot table)"; return false; }
    return true;
}

// f(ChainGeo, DT): dispatch_chain with the feature width as DT = dino_dim / 32 operand tiles
template <class F>
int dispatch_v3(const DeviceNet& net, int mode, int64_t n, F&& f) {
    if (net.arch.dino_dim == 64) return dispatch_chain(net, mode, n, [&](auto g) { return f(g, std::integral_constant<int, 2>{}); });
    return dispatch_chain(net, mode, n, [&](auto g) { return f(g, std::integral_constant<int, 4>{}); });
}

}  // namespace

int launch_train_forward_v3(const DeviceNet& net, const TrainDev& t, int mode, const float* pos, const float* dir, const float* dino, int64_t n,
                            float* rgb, float* density, void* ctx, hipStream_t s, std::string& err) {
    if (!check(net, t, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    k.pos = pos; k.dir = dir; k.dino = dino; k.n = n; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    return dispatch_v3(net, mode, n, [&](auto g, auto dt) {
        typedef decltype(g) G;
        return launch_persistent<train_forward_v3_kernel<typename G::Mode, G::kWaves, 12, 4, decltype(dt)::value>, G::kWaves>(
            net, net_args(net, mode), k, tiles32(n) / G::kWaves, s, "train forward", err);
    });
}

int launch_train_backward_v3(const DeviceNet& net, const TrainDev& t, int mode, const float* rgb, const float* density,
                             const float* g_rgb, const float* g_density, int64_t n, void* ctx, float* grad, hipStream_t s, std::string& err) {
    if (!check(net, t, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    k.n = n; k.rgb = const_cast<float*>(rgb); k.density = const_cast<float*>(density); k.g_rgb = g_rgb; k.g_density = g_density;
    k.ctx = (char*)ctx;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const int r = dispatch_v3(net, mode, n, [&](auto g, auto dt) {
        typedef decltype(g) G;
        return launch_persistent<train_backward_v3_kernel<typename G::Mode, G::kWaves, 12, decltype(dt)::value>, G::kWaves>(
            net, backward_net_args(net, t, mode), k, tiles32(n) / G::kWaves, s, "train backward", err);
    });
    if (r != NRF_OK) return r;
    return launch_weight_grad(net, t, mode, k, grad, s, err);
}

}  // namespace nrf
