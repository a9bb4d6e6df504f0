// mfma_shape_probe_fused.hip -- 32x32x16 against 16x16x32 f16 MFMAs in the step composition of the fused renderer's pinned walk
// (mlp_core.hpp:dense_pinned), where tools/mfma_shape_probe.hip runs bare loops:
//   * 256 workgroups of 4 waves, one wave per SIMD, 64 sample columns per wave;
//   * a "layer" is 128 fragment steps; a step reads ONE 1-KiB A fragment (ds_read_b128, issued 3 steps ahead) and feeds it to
//     2 x 32x32x16 (two column tiles of 32) in one arm and to 4 x 16x16x32 (four column tiles of 16) in the other: 64 MFMA cycles
//     and 65 536 FLOP per step either way;
//   * the B operands (the layer's input activations: 128 registers in both arms) stay in registers; two accumulator sets
//     alternate per output tile (16 K-steps of 16 / 8 K-steps of 32) and are re-armed with a zero C operand, so nothing grows;
//   * every step converts two registers of the finished accumulator set: 2 v_add_f32 (bias), v_cvt_pkrtz_f16_f32, v_pk_max_i16
//     (ReLU on the packed bits) -- the 256 output registers of a 256 x 64 layer over its 128 steps, in both arms;
//   * operands as in the renderer: weights ~ N(0, 2/256) in f16, activations |N(0,1)| with every other one zero (after ReLU).
// The two arms alternate in one process after 2 s of warm-up (each launch ~0.2 s, so each runs at its own settled clock);
// median and minimum wall per arm, and the spread between repeated launches of the same arm, are printed.
// Build: hipcc --offload-arch=gfx950 -O3 tools/mfma_shape_probe_fused.hip -o tools/mfma_shape_probe_fused
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
#define LDS __attribute__((address_space(3)))

constexpr int kFrags = 128;                 // fragments of a 256 x 256 layer
constexpr int kThreads = 256;
constexpr int kBlocks = 256;
constexpr int kWeights = kFrags * 64;       // f16x8 per lane and fragment
constexpr int kActs = kThreads * 32;        // f16x8: 32 operand words of 8 halves per thread

__device__ __forceinline__ int relu_pack(float x0, float x1, float b0, float b1) {
    const f16x2 h = __builtin_bit_cast(f16x2, __builtin_amdgcn_cvt_pkrtz(x0 + b0, x1 + b1));
    const i16x2 z = {0, 0};
    return __builtin_bit_cast(int, __builtin_elementwise_max(__builtin_bit_cast(i16x2, h), z));
}

template <int SHAPE>
__global__ void __launch_bounds__(kThreads) probe(const f16x8* __restrict__ w, const f16x8* __restrict__ acts, int* out, int iters) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    LDS f16x8* lds = (LDS f16x8*)smem;
    for (int i = threadIdx.x; i < kWeights; i += kThreads) lds[i] = w[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    f16x8 b[32];                              // SHAPE 32: [k-step 0..15][column tile 0..1]; SHAPE 16: [k-step 0..7][column tile 0..3]
#pragma unroll
    for (int k = 0; k < 32; ++k) b[k] = acts[(threadIdx.x * 32 + k) % kActs];
    const float bias0 = 0.01f * (float)(lane & 7), bias1 = -0.02f * (float)(lane & 3);
    int sink = 0;
    constexpr int NT = SHAPE == 32 ? 2 : 4;             // column tiles
    constexpr int KS = SHAPE == 32 ? 16 : 8;            // K-steps per output tile
    constexpr int R = SHAPE == 32 ? 16 : 4;             // accumulator registers per tile
    typedef typename std::conditional<SHAPE == 32, f32x16, f32x4>::type Acc;
    Acc acc[2][NT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[s][n][r] = 0.f;
    for (int it = 0; it < iters; ++it) {
        asm volatile("" ::: "memory");                  // the fragment reads are re-issued every layer
        f16x8 a[4];
        a[0] = lds[0 * 64 + lane]; a[1] = lds[1 * 64 + lane]; a[2] = lds[2 * 64 + lane];
#pragma unroll
        for (int f = 0; f < kFrags; ++f) {
            __builtin_amdgcn_sched_barrier(0);
            a[(f + 3) & 3] = lds[((f + 3) % kFrags) * 64 + lane];          // fragment f + 3 (wraps into the next layer's first ones)
            const int tile = f / KS, k = f % KS, set = tile & 1;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                Acc c = acc[set][n];
                if (k == 0)
#pragma unroll
                    for (int r = 0; r < R; ++r) c[r] = 0.f;                 // re-armed: a zero C operand
                if constexpr (SHAPE == 32) acc[set][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[f & 3], b[k * NT + n], c, 0, 0, 0);
                else acc[set][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[f & 3], b[k * NT + n], c, 0, 0, 0);
            }
            // one epilogue slice: two registers of the finished set (NT * R registers over KS steps = 2 per step)
            const int e = 2 * k, en = e / R, er = e % R;
            sink ^= relu_pack(acc[set ^ 1][en][er], acc[set ^ 1][en][er + 1], bias0, bias1);
        }
    }
    out[blockIdx.x * kThreads + threadIdx.x] = sink;
}

template <int SHAPE>
float launch(const f16x8* w, const f16x8* acts, int* out, int iters, hipEvent_t e0, hipEvent_t e1) {
    (void)hipEventRecord(e0);
    probe<SHAPE><<<kBlocks, kThreads, kWeights * 16>>>(w, acts, out, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms;
}

static unsigned short f16_bits(float f) { _Float16 h = (_Float16)f; unsigned short u; memcpy(&u, &h, 2); return u; }

int main() {
    unsigned x = 12345;
    auto uni = [&]() { x = x * 1664525u + 1013904223u; return ((x >> 8) & 0xFFFFFF) / 16777216.0f; };
    auto gauss = [&]() { float s = 0.f; for (int i = 0; i < 12; ++i) s += uni(); return s - 6.0f; };
    std::vector<unsigned short> hw((size_t)kWeights * 8), ha((size_t)kActs * 8);
    for (auto& v : hw) v = f16_bits(gauss() * sqrtf(2.0f / 256.0f));
    for (size_t i = 0; i < ha.size(); ++i) { const float g = fabsf(gauss()); ha[i] = f16_bits(uni() < 0.5f ? 0.0f : g); }
    f16x8 *w, *acts;
    int* out;
    if (hipMalloc(&w, hw.size() * 2) != hipSuccess || hipMalloc(&acts, ha.size() * 2) != hipSuccess || hipMalloc(&out, kBlocks * kThreads * 4) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 1;
    }
    (void)hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(acts, ha.data(), ha.size() * 2, hipMemcpyHostToDevice);
    (void)hipFuncSetAttribute((const void*)probe<32>, hipFuncAttributeMaxDynamicSharedMemorySize, kWeights * 16);
    (void)hipFuncSetAttribute((const void*)probe<16>, hipFuncAttributeMaxDynamicSharedMemorySize, kWeights * 16);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    const int iters = 40000, rounds = 9;                 // ~0.2 s per launch
    float warm = 0.f;
    for (int i = 0; i < 40 && warm < 2000.f; ++i) warm += launch<32>(w, acts, out, iters, e0, e1) + launch<16>(w, acts, out, iters, e0, e1);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess || warm < 2000.f) { printf("warm-up failed (%.0f ms)\n", warm); return 1; }
    std::vector<float> t32, t16;
    for (int r = 0; r < rounds; ++r) {
        t32.push_back(launch<32>(w, acts, out, iters, e0, e1));
        t16.push_back(launch<16>(w, acts, out, iters, e0, e1));
        printf("round %d: 32x32x16 %.3f ms   16x16x32 %.3f ms\n", r, t32.back(), t16.back());
    }
    if (hipDeviceSynchronize() != hipSuccess) { printf("device error: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    const double flop = (double)kBlocks * 4 * iters * kFrags * 65536.0;
    auto report = [&](const char* name, std::vector<float> t) {
        std::sort(t.begin(), t.end());
        const float med = t[t.size() / 2];
        printf("%s: median %.3f ms (%.0f TFLOP/s)  min %.3f  max %.3f  spread %.2f %%\n", name, med, flop / (med * 1e-3) / 1e12, t.front(), t.back(),
               100.0 * (t.back() - t.front()) / med);
        return med;
    };
    const float m32 = report("2 x 32x32x16 per fragment", t32), m16 = report("4 x 16x16x32 per fragment", t16);
    printf("16x16x32 vs 32x32x16: %+.2f %% wall (negative = 16x16x32 faster)\n", 100.0 * (m16 - m32) / m32);
    return 0;
}
