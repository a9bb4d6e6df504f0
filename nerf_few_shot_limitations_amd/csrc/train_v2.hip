// train_v2.hip -- host entry points of the V2 training kernels (pos_freq 10, dir_freq 4): train_v2_impl.hpp
#include "train_v2_impl.hpp"

namespace nrf {

namespace {

bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return false;
    if (net.arch.net != NRF_NET_V2 || net.arch.dir_freq != 4) { err = "nrf_mlp_forward_train / nrf_mlp_backward need a V2 model with dir_freq 4"; return false; }
    return true;
}

}  // namespace

int launch_train_forward_v2(const DeviceNet& net, const TrainDev& t, int mode, const float* pos, const float* dir, int64_t n, float* rgb,
                            float* density, void* ctx, hipStream_t s, std::string& err) {
    if (!check(net, t, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    k.pos = pos; k.dir = dir; k.n = n; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    return dispatch_chain(net, mode, n, [&](auto g) {
        typedef decltype(g) G;
        return launch_persistent<train_forward_v2_kernel<typename G::Mode, G::kWaves, 10, 4>, G::kWaves>(net, net_args(net, mode), k,
                                                                                                        tiles32(n) / G::kWaves, s, "train forward", err);
    });
}

int launch_train_backward_v2(const DeviceNet& net, const TrainDev& t, int mode, const float* rgb, const float* density,
                             const float* g_rgb, const float* g_density, int64_t n, void* ctx, float* grad, hipStream_t s, std::string& err) {
    if (!check(net, t, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    k.n = n; k.rgb = const_cast<float*>(rgb); k.density = const_cast<float*>(density); k.g_rgb = g_rgb; k.g_density = g_density;
    k.ctx = (char*)ctx;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const int r = dispatch_chain(net, mode, n, [&](auto g) {
        typedef decltype(g) G;
        return launch_persistent<train_backward_v2_kernel<typename G::Mode, G::kWaves, 10>, G::kWaves>(net, backward_net_args(net, t, mode), k,
                                                                                                      tiles32(n) / G::kWaves, s, "train backward", err);
    });
    if (r != NRF_OK) return r;
    return launch_weight_grad(net, t, mode, k, grad, s, err);
}

}  // namespace nrf
