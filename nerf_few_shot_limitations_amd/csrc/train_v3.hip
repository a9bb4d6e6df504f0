// train_v3.hip -- host entry points of the V3 (NeRFWithDINO) training kernels (pos_freq 12, dir_freq 4, dino_dim 64 / 128)
#include "train_v3_impl.hpp"

namespace nrf {

namespace {

// DT = dino_dim / 32 operand tiles of per-sample features
template <int DT>
struct V3 {
    static bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) { return check_train_v3(net, t, mode, err); }
    template <class G> static constexpr auto forward = train_forward_v3_kernel<typename G::Mode, G::kWaves, 12, 4, DT>;
    template <class G> static constexpr auto forward_rays = train_forward_v3_rays_kernel<typename G::Mode, G::kWaves, 12, 4, DT>;
    template <class G> static constexpr auto backward = train_backward_v3_kernel<typename G::Mode, G::kWaves, 12, DT>;
};

}  // namespace

int launch_train_forward_v3(const DeviceNet& net, const TrainDev& t, int mode, const float* pos, const float* dir, const float* dino, int64_t n,
                            float* rgb, float* density, void* ctx, hipStream_t s, std::string& err) {
    TrainKArgs k{};
    k.pos = pos; k.dir = dir; k.dino = dino; k.n = n; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    return net.arch.dino_dim == 64 ? run_chain<V3<2>, true>(net, t, mode, k, nullptr, s, err) : run_chain<V3<4>, true>(net, t, mode, k, nullptr, s, err);
}

int launch_train_forward_rays_v3(const DeviceNet& net, const TrainDev& t, int mode, const TrainRaysDev& r, int64_t n, float* rgb,
                                 float* density, void* ctx, hipStream_t s, std::string& err) {
    TrainRayKArgs k{};
    k.rays = r; k.n = n; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    return net.arch.dino_dim == 64 ? run_chain<V3<2>, true, RayInputs>(net, t, mode, k, nullptr, s, err)
                                   : run_chain<V3<4>, true, RayInputs>(net, t, mode, k, nullptr, s, err);
}

int launch_train_backward_v3(const DeviceNet& net, const TrainDev& t, int mode, const float* rgb, const float* density,
                             const float* g_rgb, const float* g_density, int64_t n, void* ctx, float* grad, hipStream_t s, std::string& err) {
    TrainKArgs k{};
    k.n = n; k.rgb = const_cast<float*>(rgb); k.density = const_cast<float*>(density); k.g_rgb = g_rgb; k.g_density = g_density;
    k.ctx = (char*)ctx;
    return net.arch.dino_dim == 64 ? run_chain<V3<2>, false>(net, t, mode, k, grad, s, err) : run_chain<V3<4>, false>(net, t, mode, k, grad, s, err);
}

}  // namespace nrf
