// hier_train.hip -- the stage between the two forwards and the two backwards of the hierarchical training step
// (nerfhip.h: nrf_composite_hier_loss_backward).  The step holds the network rows of a ray's S coarse samples and of its Ni new
// samples in two separate row sets; the fine image composites their sorted union.  Two kernels move rows between those layouts,
// and the compositor, the loss and the compositor backward in between are the library's own composite_loss_backward_kernel
// (staged_kernels.hip), launched once on the coarse rows and once on the gathered union -- so the fine term's numbers are that
// kernel's on the gathered rows by construction, not by a second copy of its arithmetic:
//
//   merge_gather_kernel : one thread per sample.  Its place in the union is its merge rank, sample_pdf_rows' rule
//                         (sample_pdf_impl.hpp) -- coarse a: a + #{new < z_a}; new k: k + #{coarse <= z_k}: a coarse depth goes in
//                         front of an equal new one, equal new depths keep their order -- found by a binary search of the other
//                         (ascending) list.  The thread stores its depth, its [r,g,b,sigma] row (one 16-byte store) and its rank
//                         at that place.
//   scatter_add_kernel  : one thread per sample again: the fine term's d row at the sample's rank goes back to the sample's own
//                         row set -- stored for a new sample, added to the coarse term's d row (one fp32 addition) for a coarse one
//                         -- and the first R threads form ray_loss = w_coarse * se_c + w_fine * se_f.
//
// Every output element is written by exactly one thread and the two kernels are separated from the compositor launches by kernel
// boundaries: no atomics, no cross-lane traffic through memory, two runs give the same bits.  Both kernels are HBM-bound copies
// (40 B per sample each); all stores are vector stores.
#include "kernels.hpp"

namespace nrf {

namespace {

constexpr int kBlock = 256;

inline unsigned grid_for(int64_t n, int block, int64_t cap) {
    int64_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// how many of the ascending a[0..n) are <= v (LE) or < v: the first index whose element is not.  A NaN compares false either way:
// the count is 0 and the rank stays inside the ray's M places.
template <bool LE>
__device__ __forceinline__ int count_below(const float* __restrict__ a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float x = a[mid];
        if (LE ? x <= v : x < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kBlock) merge_gather_kernel(const HierTrainArgs a, int64_t n_rays, int S, int Ni, float* __restrict__ z_union,
                                                              float4* __restrict__ rows, int32_t* __restrict__ rank_out) {
    const int M = S + Ni;
    const int64_t total = n_rays * M;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / M;
        const int j = (int)(i - r * M);
        const bool coarse = j < S;
        float v;
        int rank;
        int64_t row;
        if (coarse) {
            row = r * S + j;
            v = a.z_coarse[row];
            rank = j + count_below<false>(a.z_new + r * Ni, Ni, v);
        } else {
            row = r * Ni + (j - S);
            v = a.z_new[row];
            rank = (j - S) + count_below<true>(a.z_coarse + r * S, S, v);
        }
        const float* rgb = coarse ? a.rgb_coarse : a.rgb_new;
        const float* sigma = coarse ? a.sigma_coarse : a.sigma_new;
        const int64_t o = r * M + rank;                  // rank <= (S - 1) + Ni, (Ni - 1) + S: inside the ray's M places
        z_union[o] = v;
        rows[o] = make_float4(rgb[row * a.rgb_stride], rgb[row * a.rgb_stride + 1], rgb[row * a.rgb_stride + 2], sigma[row * a.sigma_stride]);
        rank_out[i] = rank;
    }
}

__global__ void __launch_bounds__(kBlock) scatter_add_kernel(const HierTrainArgs a, int64_t n_rays, int S, int Ni, const float4* __restrict__ d_rows,
                                                             const int32_t* __restrict__ rank_in, const float* __restrict__ parts,
                                                             float* __restrict__ ray_loss) {
    const int M = S + Ni;
    const int64_t total = n_rays * M;
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        if (i < n_rays) ray_loss[i] = __fadd_rn(__fmul_rn(a.w_coarse, parts[i]), __fmul_rn(a.w_fine, parts[n_rays + i]));
        const int64_t r = i / M;
        const int j = (int)(i - r * M);
        const float4 g = d_rows[r * M + rank_in[i]];
        if (j < S) {
            const int64_t row = r * S + j;
            float* d_rgb = a.d_rgb_coarse + row * a.rgb_stride;
            float* d_sigma = a.d_sigma_coarse + row * a.sigma_stride;
            d_rgb[0] = __fadd_rn(d_rgb[0], g.x); d_rgb[1] = __fadd_rn(d_rgb[1], g.y); d_rgb[2] = __fadd_rn(d_rgb[2], g.z);
            d_sigma[0] = __fadd_rn(d_sigma[0], g.w);
        } else {
            const int64_t row = r * Ni + (j - S);
            float* d_rgb = a.d_rgb_new + row * a.rgb_stride;
            d_rgb[0] = g.x; d_rgb[1] = g.y; d_rgb[2] = g.z;
            a.d_sigma_new[row * a.sigma_stride] = g.w;
        }
    }
}

}  // namespace

// the workspace, in floats, for N = n_rays * (S + Ni) samples: gathered rows (4N) | their d rows (4N) | merged depths (N) | ranks (N,
// int32) | the two squared errors per ray (2 n_rays) | the image of the optional weights launch (3 n_rays)
int64_t hier_train_ws_bytes(int64_t n_rays, int S, int Ni) {
    const int64_t N = n_rays * ((int64_t)S + Ni);
    return ((4 * (10 * N + 5 * n_rays) + 15) / 16) * 16;
}

int launch_hier_loss_backward(const HierTrainArgs& a, int64_t n_rays, int S, int Ni, hipStream_t s) {
    if (n_rays <= 0 || S < 1 || Ni < 1 || S + Ni > 4096) return NRF_EINVAL;
    const int M = S + Ni;
    const int64_t N = n_rays * M;
    float* ws = (float*)a.workspace;
    float* rows = ws;
    float* d_rows = ws + 4 * N;
    float* z_union = a.z_union ? a.z_union : ws + 8 * N;
    int32_t* rank = (int32_t*)(ws + 9 * N);
    float* parts = a.ray_parts ? a.ray_parts : ws + 10 * N;
    // 1. the coarse term: compositor, loss and compositor backward on the coarse rows as they lie (and the clearing side job)
    int r = launch_composite_mse_backward(a.rgb_coarse, a.rgb_stride, a.sigma_coarse, a.sigma_stride, a.z_coarse, a.rays_d, n_rays, S, a.white_bkgd,
                                          a.target, a.w_coarse, a.pred_coarse, a.d_rgb_coarse, a.rgb_stride, a.d_sigma_coarse, a.sigma_stride, parts,
                                          a.zero_buf, a.zero_n, s);
    if (r != NRF_OK) return r;
    // 2. the union: depths and rows in the merged order
    hipLaunchKernelGGL(merge_gather_kernel, dim3(grid_for(N, kBlock, 16384)), dim3(kBlock), 0, s, a, n_rays, S, Ni, z_union, (float4*)rows, rank);
    if (hipGetLastError() != hipSuccess) return NRF_EHIP;
    // 3. the fine term on it
    r = launch_composite_mse_backward(rows, 4, rows + 3, 4, z_union, a.rays_d, n_rays, M, a.white_bkgd, a.target, a.w_fine, a.pred_fine, d_rows, 4,
                                      d_rows + 3, 4, parts + n_rays, nullptr, 0, s);
    if (r != NRF_OK) return r;
    if (a.weights_fine) {
        // the loss kernel keeps no weights: a caller that asks for them pays one compositor launch (its image goes to the workspace)
        r = launch_composite(rows, 4, rows + 3, 4, z_union, a.rays_d, n_rays, M, a.white_bkgd, ws + 10 * N + 2 * n_rays, nullptr, a.weights_fine, s);
        if (r != NRF_OK) return r;
    }
    // 4. the fine term's d rows back to the two row sets, and the rays' loss terms
    hipLaunchKernelGGL(scatter_add_kernel, dim3(grid_for(N, kBlock, 16384)), dim3(kBlock), 0, s, a, n_rays, S, Ni, (const float4*)d_rows, rank, parts,
                       a.ray_loss);
    if (hipGetLastError() != hipSuccess) return NRF_EHIP;
    return NRF_OK;
}

}  // namespace nrf
