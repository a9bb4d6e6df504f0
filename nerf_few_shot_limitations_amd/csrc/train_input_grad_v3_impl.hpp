// train_input_grad_v3_impl.hpp -- dL/d (positions, directions) of the V3 network through the positional encodings, from what a
// finished dZ chain (train_v3_impl.hpp: train_backward_v3_kernel) left in the context.  Notation of train_slots.hpp and
// train_dino_grad_impl.hpp: fusion.0 has weight W0 = [W0p | W0d] (256 x (PE + C)) and runs twice, on [pe | f] and on
// [pe w0 | f w1]; the chain saved
//     d1 = dZ(fusion.0, pass 1)   in slot SlotsV3::dz_fusion0(0)   (it already contains the whole gate path)
//     d2 = dZ(fusion.0, pass 2)   in slot SlotsV3::dz_fusion0(1)
//     dZc = dZ(color_layers.0)    in slot ColourSlots::dz_c0()     (4 tiles)
// and the gate (w0, w1) per sample, so that
//     dL/d e(p) = W0p^T d1 + w0 (W0p^T d2)          dL/d e(d) = C0[:, 256 + pe]^T dZc
// and the epilogue applies the adjoint of the encoding (train_post_grad_core.hpp: encoding_adjoint_tile, L = 12 over three
// accumulator tiles for the positions, the run-time dir_freq over one for the directions).  The two products are kept apart down
// to the fp32 join acc1 + w0 * acc2: forming d1 + w0 d2 in front of the MFMA would round a gradient to 16 bits a second time.
// This is the share of dL/d positions that flows through the encoding only; the share through the fetched features -- the
// adjoint of the projection and of the bilinear fetch applied to nrf_mlp_backward_dino's dL/df -- is
// fetch_points_backward_kernel (staged_kernels.hip), which adds onto this kernel's output.
// The A operands are two small fragment streams of the packer (packing.cpp:make_input_grad_v3_plan: 3 x 8 and 1 x 4 tile pairs,
// 48 + 8 KiB in the 16-bit modes, twice that in fp32).  HBM-bound: 2 x 8 + 4 saved tiles, the gate and 24 bytes of coordinates
// read, 24 B written per sample.  Built from train_post_grad_core.hpp.
#pragma once
#include "train_post_grad_core.hpp"

namespace nrf {

struct InputGradV3Args {
    const void* wstream;        // (3 * 8 + 4) * Mode::SUB fragments: W0p^T, then color_layers.0^T's direction tile, (m, t, s) order
    const char* ctx;
    int64_t dz1_off, dz2_off;   // context offsets of the two fusion.0 dZ slots (8 feature tiles per sample tile)
    int64_t dzc_off;            // ... of color_layers.0's (4)
    int64_t aux_off;            // the gate
    int64_t n;                  // samples
    int64_t n_tiles;            // 32-sample tiles that hold a sample
    const float* positions;     // (n,3), read when d_positions is asked for
    const float* directions;    // (n,3), read when d_directions is asked for
    float* d_positions;         // (n,3) or NULL
    float* d_directions;        // (n,3) or NULL
    int dir_freq;               // 1..4
};

constexpr int kInputGradV3PosFreq = 12;                         // the V3 training path's pos_freq (check_train_common)
constexpr int kInputGradV3PT = pe_tiles(kInputGradV3PosFreq);   // 3

template <class Mode, bool POS, bool DIR>
__global__ void __launch_bounds__(kPostGradWaves * 64) input_grad_v3_kernel(const InputGradV3Args P) {
    constexpr int PT = kInputGradV3PT;
    constexpr int64_t TB = tile_bytes<Mode>();
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const NRF_LDS char* frags = post_grad_resident<post_grad_frags<Mode, PT, true>()>(P.wstream, lane, wave);
    for (int64_t st = (int64_t)blockIdx.x * kPostGradWaves + wave; st < P.n_tiles; st += (int64_t)gridDim.x * kPostGradWaves) {
        const PostGradRow row(st, c, P.n);
        if constexpr (POS) {
            f32x16 acc1[PT], acc2[PT];
            post_grad_walk<Mode, PT>(frags, P.ctx + P.dz1_off + st * 8 * TB + lane * 16, P.ctx + P.dz2_off + st * 8 * TB + lane * 16, acc1, acc2);
            const float w0 = ((const float2*)(P.ctx + P.aux_off))[row.sid].x;
#pragma unroll
            for (int m = 0; m < PT; ++m) acc1[m] = acc1[m] + acc2[m] * w0;        // (two roundings: the build sets -ffp-contract=off)
            encoding_adjoint_store<PT>(acc1, P.positions, kInputGradV3PosFreq, row, h, P.d_positions);
        }
        if constexpr (DIR)
            post_grad_directions<Mode, post_grad_dir_frag0<Mode, PT>()>(frags, P.ctx + P.dzc_off + st * 4 * TB + lane * 16, P.directions, P.dir_freq, row,
                                                                        h, P.d_directions);
    }
}

}  // namespace nrf
