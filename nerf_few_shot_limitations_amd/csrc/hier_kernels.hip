// hier_kernels.hip -- the staged kernels of the hierarchical render that evaluates only the new samples in its fine pass: the
// resampling that also hands out the new samples in ascending order, and the merging compositor (kernels.hpp: MergeArgs).
#include "kernels.hpp"
#include "sample_pdf_impl.hpp"

namespace nrf {

namespace {

constexpr int kBlock = 256;

__global__ void sample_pdf_sorted_kernel(const float* __restrict__ z, const float* __restrict__ w, int64_t n_rays, int S, int Ni,
                                         const float* __restrict__ u_in, int64_t u_ray_stride, float* __restrict__ samples,
                                         float* __restrict__ z_union, float* __restrict__ samples_sorted) {
    sample_pdf_rows(z, w, n_rays, S, Ni, u_in, u_ray_stride, samples, z_union, samples_sorted);
}

// ---- the hierarchical fine pass from kept rows (kernels.hpp: MergeArgs) --------------------------------------------------
// LANE <-> RAY: one lane walks its ray's two ascending depth lists with two pointers -- the coarse sample is taken while
// z_coarse <= z_new, sample_pdf_kernel's rule for the sorted union -- and composites the merged order front to back with the
// operations of render_march's SPW = 1 branch in its order (no wave scan: composite_kernel's summation order differs).  dist goes
// to the next element of the merged order, the last one gets 1e10 |d|.  A ray's rows are about 3 KB at 128 + 64; the 16-byte row
// loads of a lane use every byte of a cache line over eight steps.
template <bool FAST>
__global__ void __launch_bounds__(kBlock) composite_merge_kernel(const MergeArgs A) {
    const int S = A.S, Ni = A.Ni, U = S + Ni;
    for (int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x; r < A.n_rays; r += (int64_t)gridDim.x * kBlock) {
        float d[3];
        if (A.rays_d) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = A.rays_d[r * 3 + k];
        } else {
            float o[3];
            camera_ray(A.cam, A.ray_begin + r, o, d);
        }
        const float norm = ray_norm(d);
        const float* zc = A.z_coarse + r * S;
        const float* zn = A.z_new + r * Ni;               // (never read with Ni == 0)
        const float4* rc = (const float4*)A.raw_coarse + r * S;
        const float4* rn = (const float4*)A.raw_new + r * Ni;
        float* wo = A.weights ? A.weights + r * U : nullptr;
        float* zu = A.z_union ? A.z_union + r * U : nullptr;
        Composite comp;
        comp.reset();
        int i = 0, j = 0;
        // head of the merged order: (depth, is it the coarse list's)
        auto head = [&](bool& coarse) -> float {
            const float a = i < S ? zc[i] : 0.0f, b = j < Ni ? zn[j] : 0.0f;
            coarse = j >= Ni || (i < S && a <= b);
            return coarse ? a : b;
        };
        bool coarse;
        float zo = head(coarse);
        for (int k = 0; k < U; ++k) {
            const float4 v = coarse ? rc[i] : rn[j];
            if (coarse) ++i; else ++j;
            const bool last = k + 1 == U;
            float zn_next = 0.0f;
            if (!last) zn_next = head(coarse);
            const float dist = last ? __fmul_rn(1e10f, norm) : __fmul_rn(__fsub_rn(zn_next, zo), norm);
            const float w = comp.template add<FAST>(v.w, sigmoid_sel<FAST>(v.x), sigmoid_sel<FAST>(v.y), sigmoid_sel<FAST>(v.z), zo, dist);
            if (wo) wo[k] = w;
            if (zu) zu[k] = zo;
            zo = zn_next;
        }
        float cr = comp.r, cg = comp.g, cb = comp.b;
        if (A.white_bkgd) {                                      // nerf_mlp.py:209-212
            const float bg = __fsub_rn(1.0f, comp.acc);
            cr = __fadd_rn(cr, bg); cg = __fadd_rn(cg, bg); cb = __fadd_rn(cb, bg);
        }
        if (A.interleaved) {
            *(float4*)(A.rgb + r * 4) = make_float4(cr, cg, cb, comp.depth);
        } else {
            A.rgb[r * 3 + 0] = cr; A.rgb[r * 3 + 1] = cg; A.rgb[r * 3 + 2] = cb;
            if (A.depth) A.depth[r] = comp.depth;
        }
    }
}

}  // namespace

int launch_composite_merge(const MergeArgs& m, bool fast_exp, hipStream_t s) {
    if (m.n_rays <= 0) return NRF_OK;
    const int64_t blocks = (m.n_rays + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(blocks < 16384 ? blocks : 16384));
    if (fast_exp) hipLaunchKernelGGL(composite_merge_kernel<true>, grid, dim3(kBlock), 0, s, m);
    else hipLaunchKernelGGL(composite_merge_kernel<false>, grid, dim3(kBlock), 0, s, m);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

int launch_sample_pdf_sorted(const float* z, const float* w, int64_t n_rays, int S, int Ni, const float* u, int64_t u_ray_stride, float* samples,
                             float* samples_sorted, float* z_union, hipStream_t s) {
    if (n_rays <= 0) return NRF_OK;
    SamplePdfGrid g;
    if (!sample_pdf_grid(n_rays, S, Ni, g)) return NRF_EINVAL;
    hipLaunchKernelGGL(sample_pdf_sorted_kernel, dim3((unsigned)g.blocks), dim3(g.waves * 64), g.lds_bytes, s, z, w, n_rays, S, Ni, u, u_ray_stride,
                       samples, z_union, samples_sorted);
    return hipGetLastError() == hipSuccess ? NRF_OK : NRF_EHIP;
}

}  // namespace nrf
