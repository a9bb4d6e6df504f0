// train_v2.hip -- host entry points of the V2 training kernels (pos_freq 10, dir_freq 4): train_v2_impl.hpp
#include "train_v2_impl.hpp"

namespace nrf {

namespace {

struct V2 {
    static bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) { return check_train_v2(net, t, mode, err); }
    template <class G> static constexpr auto forward = train_forward_v2_kernel<typename G::Mode, G::kWaves, 10, 4>;
    template <class G> static constexpr auto forward_rays = train_forward_v2_rays_kernel<typename G::Mode, G::kWaves, 10, 4>;
    template <class G> static constexpr auto backward = train_backward_v2_kernel<typename G::Mode, G::kWaves, 10>;
};

}  // namespace

int launch_train_forward_v2(const DeviceNet& net, const TrainDev& t, int mode, const float* pos, const float* dir, int64_t n, float* rgb,
                            float* density, void* ctx, hipStream_t s, std::string& err) {
    TrainKArgs k{};
    k.pos = pos; k.dir = dir; k.n = n; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    return run_chain<V2, true>(net, t, mode, k, nullptr, s, err);
}

int launch_train_forward_rays_v2(const DeviceNet& net, const TrainDev& t, int mode, const TrainRaysDev& r, int64_t n, float* rgb,
                                 float* density, void* ctx, hipStream_t s, std::string& err) {
    TrainRayKArgs k{};
    k.rays = r; k.n = n; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    return run_chain<V2, true, RayInputs>(net, t, mode, k, nullptr, s, err);
}

int launch_train_backward_v2(const DeviceNet& net, const TrainDev& t, int mode, const float* rgb, const float* density,
                             const float* g_rgb, const float* g_density, int64_t n, void* ctx, float* grad, hipStream_t s, std::string& err) {
    TrainKArgs k{};
    k.n = n; k.rgb = const_cast<float*>(rgb); k.density = const_cast<float*>(density); k.g_rgb = g_rgb; k.g_density = g_density;
    k.ctx = (char*)ctx;
    return run_chain<V2, false>(net, t, mode, k, grad, s, err);
}

}  // namespace nrf
