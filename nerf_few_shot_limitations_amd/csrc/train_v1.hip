// train_v1.hip -- host entry points of the V1 training kernels (pos_freq 10): train_impl.hpp
#include "train_impl.hpp"

namespace nrf {

namespace {

bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) {
    if (!check_train_common(net, t, mode, err)) return false;
    if (net.arch.net != NRF_NET_V1) { err = "nrf_mlp_*_train_v1 needs a V1 model"; return false; }
    return true;
}

}  // namespace

int launch_train_forward(const DeviceNet& net, const TrainDev& t, int mode, const float* x_enc, int64_t n, float* out4, void* ctx,
                         hipStream_t s, std::string& err) {
    if (!check(net, t, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    k.x_enc = x_enc; k.n = n; k.out4 = out4; k.ctx = (char*)ctx;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    return dispatch_chain(net, mode, n, [&](auto g) {
        typedef decltype(g) G;
        return launch_persistent<train_forward_kernel<typename G::Mode, G::kWaves, 10>, G::kWaves>(net, net_args(net, mode), k, tiles32(n) / G::kWaves,
                                                                                                  s, "train forward", err);
    });
}

int launch_train_backward(const DeviceNet& net, const TrainDev& t, int mode, const float* out4, const float* g_out4, int64_t n,
                          void* ctx, float* grad, hipStream_t s, std::string& err) {
    if (!check(net, t, mode, err)) return NRF_EINVAL;
    if (n <= 0) return NRF_OK;
    TrainKArgs k{};
    k.n = n; k.out4 = const_cast<float*>(out4); k.g_out4 = g_out4; k.ctx = (char*)ctx;
    if (!fill_slots(t, mode, n, k, err)) return NRF_EINVAL;
    const int r = dispatch_chain(net, mode, n, [&](auto g) {
        typedef decltype(g) G;
        return launch_persistent<train_backward_kernel<typename G::Mode, G::kWaves, 10>, G::kWaves>(net, backward_net_args(net, t, mode), k,
                                                                                                   tiles32(n) / G::kWaves, s, "train backward", err);
    });
    if (r != NRF_OK) return r;
    return launch_weight_grad(net, t, mode, k, grad, s, err);
}

}  // namespace nrf
