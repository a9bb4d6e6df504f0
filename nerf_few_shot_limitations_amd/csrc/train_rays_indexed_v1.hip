// train_rays_indexed_v1.hip -- the V1 ray-input saving forward on a compacted sample list (train_impl.hpp: IndexedRayInputs;
// nerfhip.h: nrf_mlp_forward_train_rays_indexed).  A unit of its own (build.py).
#include "train_impl.hpp"

namespace nrf {

namespace {

struct V1Indexed {
    static bool check(const DeviceNet& net, const TrainDev& t, int mode, std::string& err) { return check_train_v1(net, t, mode, err); }
    template <class G> static constexpr auto forward_indexed = train_forward_rays_indexed_kernel<typename G::Mode, G::kWaves, 10>;
};

}  // namespace

int launch_train_forward_rays_indexed_v1(const DeviceNet& net, const TrainDev& t, int mode, const TrainRaysDev& r, const int32_t* index,
                                         int64_t n_rows, float* out4, void* ctx, hipStream_t s, std::string& err) {
    TrainRayIndexKArgs k{};
    k.rays = r; k.index = index; k.n = n_rows; k.out4 = out4; k.ctx = (char*)ctx;
    return run_chain<V1Indexed, true, IndexedRayInputs>(net, t, mode, k, nullptr, s, err);
}

}  // namespace nrf
