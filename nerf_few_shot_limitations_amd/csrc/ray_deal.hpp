// ray_deal.hpp -- how a render launch's rays are dealt to the persistent workgroups of render_kernel / render_hold_kernel
// (fused_impl.hpp: render_march).  Shared by the launchers, the kernel's own walk and nrf_debug_ray_deal (api.cpp), which lets the
// CPU tests replay the deal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

namespace nrf {

// Samples per ray and pass (log2; render_kernel): the work items of the uniform deal are tiles of WAVES * COLS/SPW rays marched in
// ceil(S/SPW) passes, dealt to the CUs in whole rounds -- pick the SPW = 1, 2, 4 ... COLS (a wave's columns: ONE ray per wave at the
// far end) with the least rounds x passes.  What a wider split costs is the owner lane's serial composite of its SPW samples
// per pass (~0.15 % of an MLP pass per sample: measured, profiles/r03_small_frames.txt); ties go to the smaller SPW.  Small frames live
// off the far end: 100 x 100 x 32 (BASELINE config 1) is 157 tiles x 8 passes at SPW = 4 -- one round, 61 % of the CUs -- and
// 1250 tiles x 1 pass = 5 rounds at SPW = 32; a 64 x 64 x 48 validation frame drops from 12 pass-times to 3.  Every choice is exact:
// a ray's sequence of operations does not depend on it.  NRF_SPW=0..6 pins it (A/B runs).
constexpr double kCompositePerSample = 0.0015;
inline double pass_cost(int64_t passes, int l) { return (double)passes * (1.0 + kCompositePerSample * (double)(1 << l)); }

// -1: not pinned
inline int pinned_spw_log2() {
    const char* env = getenv("NRF_SPW");                 // read per launch: tests walk through every split inside one process
    return (env && *env) ? atoi(env) : -1;
}

inline int pick_spw_log2(int64_t n_rays, int S, int waves, int cols_per_wave, int cu, int64_t* passes = nullptr, double* cost = nullptr) {
    const int pinned = pinned_spw_log2();
    int max_l = 0;
    while ((2 << max_l) <= cols_per_wave) ++max_l;
    int best = -1;
    double best_t = 0.0;
    for (int l = 0; l <= max_l; ++l) {
        if (pinned >= 0 && l != (pinned < max_l ? pinned : max_l)) continue;
        const int64_t tile = (int64_t)waves * (cols_per_wave >> l);
        const int64_t tiles = (n_rays + tile - 1) / tile;
        const int64_t rounds = (tiles + cu - 1) / cu;
        const int64_t n = rounds * (int64_t)((S + (1 << l) - 1) >> l);
        const double t = pass_cost(n, l);
        if (best < 0 || t < best_t * (1.0 - 1e-9)) {
            best_t = t; best = l;
            if (passes) *passes = n;
            if (cost) *cost = t;
        }
    }
    return best;
}

// The even deal.  The uniform deal pays for its last, partly empty round and applies one split -- and its composite overhead -- to
// every ray: 800 x 800 x 64 is 79 rounds x 8 passes = 632 passes (639.6 pass-times in the model above) against 160 000
// column-filling passes / 256 CUs = 625.  The even deal cuts the rays, in units of `waves` rays (the smallest tile: one ray per
// wave), into one contiguous range per workgroup, the ranges differing by at most one unit (deal_range); a workgroup marches its
// range as whole tiles of waves * COLS rays at SPW = 1 and the rest as the binary decomposition of its ray count: tiles of 1/2,
// 1/4 ... of a whole one at SPW = 2, 4 ... (deal_split), every pass filling all columns: 2500 rays = 9 x 256 + 128 + 64 + 4
// -> 576 + 32 + 16 + 1 = 625 passes.  It is taken where its longest workgroup needs fewer passes AND less model time than the
// uniform deal's (small frames -- one short tile per workgroup either way -- keep the uniform one); NRF_SPW pins the uniform
// deal.  Exact like every split: a ray's sequence of operations depends on neither its tile nor its split.
struct DealRange {
    int64_t first;      // first ray of the workgroup's range
    int64_t rays;       // its length: a multiple of `waves` (the launch's last unit may reach past n_rays: those columns store nothing)
};

__host__ __device__ inline DealRange deal_range(int64_t units, int64_t grid, int64_t b, int waves) {
    const int64_t per = units / grid, extra = units % grid;
    return {(b * per + (b < extra ? b : extra)) * waves, (per + (b < extra ? 1 : 0)) * waves};
}

// log2 of the split of the next tile of a range with `left` rays to go (left >= waves, a multiple of it): the largest tile of
// whole >> l rays that fits (whole = waves * COLS, a power of two times waves)
__host__ __device__ inline int deal_split(int64_t left, int whole) {
    int l = 0;
    while ((int64_t)(whole >> l) > left) ++l;
    return l;
}

struct Deal {
    int spw_log2 = 0;        // uniform deal: the launch's split
    bool even = false;
    int64_t items = 0;       // uniform: tiles; even: units of `waves` rays
    int64_t passes = 0;      // MLP passes of the launch's longest workgroup
};

// passes / model time of a range of `rays` under the even deal
inline void even_range_cost(int64_t rays, int S, int whole, int64_t& passes, double& cost) {
    passes = (rays / whole) * S;
    cost = pass_cost(passes, 0);
    for (int64_t left = rays % whole; left > 0;) {
        const int l = deal_split(left, whole);
        const int64_t n = (S + (1 << l) - 1) >> l;
        passes += n;
        cost += pass_cost(n, l);
        left -= whole >> l;
    }
}

inline Deal pick_deal(int64_t n_rays, int S, int waves, int cols_per_wave, int cu) {
    Deal d;
    double uni_cost = 0.0;
    d.spw_log2 = pick_spw_log2(n_rays, S, waves, cols_per_wave, cu, &d.passes, &uni_cost);
    const int64_t tile = (int64_t)waves * (cols_per_wave >> d.spw_log2);
    d.items = (n_rays + tile - 1) / tile;
    if (pinned_spw_log2() >= 0 || n_rays <= 0 || S <= 0) return d;
    const int64_t units = (n_rays + waves - 1) / waves;
    const int64_t grid = units < cu ? units : cu;
    int64_t passes;
    double cost;
    even_range_cost(deal_range(units, grid, 0, waves).rays, S, waves * cols_per_wave, passes, cost);     // a longest range ...
    if (units % grid) {                                  // ... and a shortest: with ceil(S/SPW) passes per tile one unit less can cost more
        int64_t p2;
        double c2;
        even_range_cost(deal_range(units, grid, grid - 1, waves).rays, S, waves * cols_per_wave, p2, c2);
        if (p2 > passes) passes = p2;
        if (c2 > cost) cost = c2;
    }
    if (passes < d.passes && cost < uni_cost) {
        d.even = true;
        d.items = units;
        d.passes = passes;
    }
    return d;
}

}  // namespace nrf
