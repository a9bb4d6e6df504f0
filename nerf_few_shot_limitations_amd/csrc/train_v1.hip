// train_v1.hip -- host entry points of the V1 training kernels (pos_freq 10): train_impl.hpp
#include "train_impl.hpp"

namespace nrf {

namespace {

struct V1 {
    static bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) { return check_train_v1(net, t, mode, err); }
    template <class G> static constexpr auto forward = train_forward_kernel<typename G::Mode, G::kWaves, 10>;
    template <class G> static constexpr auto forward_rays = train_forward_rays_kernel<typename G::Mode, G::kWaves, 10>;
    template <class G> static constexpr auto backward = train_backward_kernel<typename G::Mode, G::kWaves, 10>;
};

}  // namespace

int launch_train_forward(const DeviceNet& net, const TrainDev& t, int mode, const float* x_enc, int64_t n, float* out4, void* ctx,
                         hipStream_t s, std::string& err) {
    TrainKArgs k{};
    k.x_enc = x_enc; k.n = n; k.out4 = out4; k.ctx = (char*)ctx;
    return run_chain<V1, true>(net, t, mode, k, nullptr, s, err);
}

int launch_train_forward_rays_v1(const DeviceNet& net, const TrainDev& t, int mode, const TrainRaysDev& r, int64_t n, float* out4, void* ctx,
                                 hipStream_t s, std::string& err) {
    TrainRayKArgs k{};
    k.rays = r; k.n = n; k.out4 = out4; k.ctx = (char*)ctx;
    return run_chain<V1, true, RayInputs>(net, t, mode, k, nullptr, s, err);
}

int launch_train_backward(const DeviceNet& net, const TrainDev& t, int mode, const float* out4, const float* g_out4, int64_t n,
                          void* ctx, float* grad, hipStream_t s, std::string& err) {
    TrainKArgs k{};
    k.n = n; k.out4 = const_cast<float*>(out4); k.g_out4 = g_out4; k.ctx = (char*)ctx;
    return run_chain<V1, false>(net, t, mode, k, grad, s, err);
}

}  // namespace nrf
