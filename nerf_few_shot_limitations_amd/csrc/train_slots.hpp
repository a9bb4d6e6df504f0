// train_slots.hpp -- the saved-tensor layout of the training path, written down once: which context slot holds which
// layer's operand tiles (train_core.hpp) and which ReLU bit plane holds which layer's mask, as functions of the trunk depth
// n.  packing.cpp:make_train_plan builds the slot sizes, plane count and weight-gradient jobs from these names; the chain
// kernels (train_impl.hpp, train_v2_impl.hpp, train_v3_impl.hpp) index the context by the same numbers.  Standard C++ plus
// the __host__ / __device__ annotations only: the packer is also built without HIP (tests/test_packing_sanitize.py).
#pragma once

namespace nrf {

// The colour branch of V2 and V3 (DensityMLP's heads and ColorMLP, nerf_mlp.py:41-84), from three bases:
//   fwd+0  [feature_vec | PE(dir)] (9 tiles)     bwd+0  dZ density_head (1 tile, row 0)       plane+0  colour layer 0
//   fwd+1  colour layer 0 output (4)             bwd+1  dZ feature_head = d feature_vec (8)   plane+1  colour layer 2
//   fwd+2  colour layer 2 output (2)             bwd+2  dZ color_layers.0 (4)
//                                                bwd+3  dZ color_layers.2 (2)
//                                                bwd+4  dZ color_layers.4 = d rgb logits (1)
// density_head and feature_head read the trunk output, the slot before fwd.
struct ColourSlots {
    int fwd, bwd, plane;
    constexpr __host__ __device__ int in() const { return fwd; }
    constexpr __host__ __device__ int c0() const { return fwd + 1; }
    constexpr __host__ __device__ int c2() const { return fwd + 2; }
    constexpr __host__ __device__ int dz_density() const { return bwd; }
    constexpr __host__ __device__ int d_feature() const { return bwd + 1; }
    constexpr __host__ __device__ int dz_c0() const { return bwd + 2; }
    constexpr __host__ __device__ int dz_c2() const { return bwd + 3; }
    constexpr __host__ __device__ int d_logits() const { return bwd + 4; }
    constexpr __host__ __device__ int plane_c0() const { return plane; }
    constexpr __host__ __device__ int plane_c2() const { return plane + 1; }
};

// V1 (nerf_model.py:16-24), n = layers:
//   0        PE(x) (KT0 tiles)              n+1+j  dZ of layers.j (8)              plane j  layers.j
//   1+j      layers.j output (8)            2n+1   dZ of the head = d out4 (1)
struct SlotsV1 {
    int n;
    static constexpr __host__ __device__ int input() { return 0; }
    static constexpr __host__ __device__ int trunk(int j) { return 1 + j; }
    constexpr __host__ __device__ int dz_trunk(int j) const { return n + 1 + j; }
    constexpr __host__ __device__ int dz_head() const { return 2 * n + 1; }
    constexpr __host__ __device__ int count() const { return 2 * n + 2; }
    static constexpr __host__ __device__ int plane(int j) { return j; }
    constexpr __host__ __device__ int planes() const { return n; }
};

// V2 (nerf_mlp.py:41-84 without DINO), n = density layers:
//   0        PE(pos) (KT0 tiles)            n+4+j  dZ of density_layers.j (8)      plane j  density_layers.j
//   1+j      density_layers.j output (8)    2n+4   colour branch, backward         n, n+1   colour branch
//   n+1      colour branch, forward
struct SlotsV2 {
    int n;
    static constexpr __host__ __device__ int input() { return 0; }
    static constexpr __host__ __device__ int trunk(int j) { return 1 + j; }
    constexpr __host__ __device__ int dz_trunk(int j) const { return n + 4 + j; }
    constexpr __host__ __device__ ColourSlots colour() const { return ColourSlots{n + 1, 2 * n + 4, n}; }
    constexpr __host__ __device__ int count() const { return 2 * n + 9; }
    static constexpr __host__ __device__ int plane(int j) { return j; }
    constexpr __host__ __device__ int planes() const { return n + 2; }
};

// V3 (nerf_mlp.py:86-158, the fusion block of lora_dino.py:146-193 in front of the V2 body), n = trunk layers, D = 11 + n:
//   0    [pe | dino] (KT0)           4    [pe*w0 | dino*w1] (KT0)       8+j   trunk layer j output (8)
//   1    fusion.0 out, pass 1 (8)    5    fusion.0 out, pass 2 (8)      8+n   colour branch, forward
//   2    fusion.2 out = fused (8)    6    fusion.2 out, pass 2 (8)
//   3    attention.0 out (2)         7    output_proj out (8)
//   D+0  dZ fusion.0 p1   D+1 dZ fusion.2 p1   D+2 dZ attention.0 (2)   D+3 dZ attention.2 = d gate logits (1)
//   D+4  dZ fusion.0 p2   D+5 dZ fusion.2 p2   D+6 dZ output_proj       D+7+j dZ trunk j     D+7+n colour branch, backward
// ReLU bit planes: 0 fusion.0 p1, 1 fusion.2 p1, 2 attention.0, 3 fusion.0 p2, 4 fusion.2 p2, 5+j trunk j, 5+n colour branch.
// Aux: the gate (w0, w1) per sample.
struct SlotsV3 {
    int n;
    static constexpr __host__ __device__ int input(int pass) { return 4 * pass; }
    static constexpr __host__ __device__ int fusion0(int pass) { return 1 + 4 * pass; }
    static constexpr __host__ __device__ int fusion2(int pass) { return 2 + 4 * pass; }
    static constexpr __host__ __device__ int attention0() { return 3; }
    static constexpr __host__ __device__ int proj() { return 7; }
    static constexpr __host__ __device__ int trunk(int j) { return 8 + j; }
    constexpr __host__ __device__ int dz_fusion0(int pass) const { return 11 + n + 4 * pass; }
    constexpr __host__ __device__ int dz_fusion2(int pass) const { return 12 + n + 4 * pass; }
    constexpr __host__ __device__ int dz_attention0() const { return 13 + n; }
    constexpr __host__ __device__ int d_gate() const { return 14 + n; }
    constexpr __host__ __device__ int dz_proj() const { return 17 + n; }
    constexpr __host__ __device__ int dz_trunk(int j) const { return 18 + n + j; }
    constexpr __host__ __device__ ColourSlots colour() const { return ColourSlots{8 + n, 18 + 2 * n, 5 + n}; }
    constexpr __host__ __device__ int count() const { return 23 + 2 * n; }
    static constexpr __host__ __device__ int plane_fusion0(int pass) { return 3 * pass; }
    static constexpr __host__ __device__ int plane_fusion2(int pass) { return 1 + 3 * pass; }
    static constexpr __host__ __device__ int plane_attention0() { return 2; }
    static constexpr __host__ __device__ int plane(int j) { return 5 + j; }
    constexpr __host__ __device__ int planes() const { return 7 + n; }
};

}  // namespace nrf
