// train_rays_indexed_v3.hip -- the V3 ray-input saving forward on a compacted sample list, dino_dim 64 / 128 (train_impl.hpp:
// IndexedRayInputs; nerfhip.h: nrf_mlp_forward_train_rays_indexed).  A unit of its own (build.py).
#include "train_v3_impl.hpp"

namespace nrf {

namespace {

// DT = dino_dim / 32 operand tiles of per-sample features
template <int DT>
struct V3Indexed {
    static bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) { return check_train_v3(net, t, mode, err); }
    template <class G> static constexpr auto forward_indexed = train_forward_v3_rays_indexed_kernel<typename G::Mode, G::kWaves, 12, 4, DT>;
};

}  // namespace

int launch_train_forward_rays_indexed_v3(const DeviceNet& net, const TrainDev& t, int mode, const TrainRaysDev& r, const int32_t* index,
                                         int64_t n_rows, float* rgb, float* density, void* ctx, hipStream_t s, std::string& err) {
    TrainRayIndexKArgs k{};
    k.rays = r; k.index = index; k.n = n_rows; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    return net.arch.dino_dim == 64 ? run_chain<V3Indexed<2>, true, IndexedRayInputs>(net, t, mode, k, nullptr, s, err)
                                   : run_chain<V3Indexed<4>, true, IndexedRayInputs>(net, t, mode, k, nullptr, s, err);
}

}  // namespace nrf
