// train_rays_indexed_v2.hip -- the V2 ray-input saving forward on a compacted sample list (train_impl.hpp: IndexedRayInputs;
// nerfhip.h: nrf_mlp_forward_train_rays_indexed).  A unit of its own (build.py).
#include "train_v2_impl.hpp"

namespace nrf {

namespace {

struct V2Indexed {
    static bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) { return check_train_v2(net, t, mode, err); }
    template <class G> static constexpr auto forward_indexed = train_forward_v2_rays_indexed_kernel<typename G::Mode, G::kWaves, 10, 4>;
};

}  // namespace

int launch_train_forward_rays_indexed_v2(const DeviceNet& net, const TrainDev& t, int mode, const TrainRaysDev& r, const int32_t* index,
                                         int64_t n_rows, float* rgb, float* density, void* ctx, hipStream_t s, std::string& err) {
    TrainRayIndexKArgs k{};
    k.rays = r; k.index = index; k.n = n_rows; k.rgb = rgb; k.density = density; k.ctx = (char*)ctx;
    return run_chain<V2Indexed, true, IndexedRayInputs>(net, t, mode, k, nullptr, s, err);
}

}  // namespace nrf
