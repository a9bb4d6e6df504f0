// train_input_grad_impl.hpp -- dL/d (inputs of the field) of the V1 and V2 networks, from what a finished dZ chain
// (train_impl.hpp: train_backward_kernel, train_v2_impl.hpp) left in the context.  Notation of train_slots.hpp: the first Linear
// has weight W0 (256 x pe_dim), color_layers.0 has weight C0 (128 x (256 + dir pe_dim)); the chain saved
//     dZ0 = dZ(first Linear)      in slot dz_trunk(0)           (8 tiles)
//     dZc = dZ(color_layers.0)    in slot ColourSlots::dz_c0()  (4 tiles, V2)
// so that, with the encodings e(p) and e(d) of feature_map.hpp,
//     dL/d e(p) = W0[:, pe]^T dZ0          dL/d e(d) = C0[:, 256 + pe]^T dZc
// and the epilogue applies the adjoint of the encoding (train_post_grad_core.hpp: encoding_adjoint_tile -- the sum runs in slot
// order).  The A operands are two small fragment streams of the packer (packing.cpp:make_input_grad_plan: PT x 8 and 1 x 4 tile
// pairs, 32 + 8 KiB in the 16-bit modes, twice that in fp32).  HBM-bound: 8 (+ 4) saved tiles and 12 (+ 12) bytes of coordinates
// read, 12 .. 24 B (or 4 pe_dim B) written per sample.  Built from train_post_grad_core.hpp.
#pragma once
#include "train_post_grad_core.hpp"

namespace nrf {

struct InputGradArgs {
    const void* wstream;        // (PT * 8 + 4) * Mode::SUB fragments: W0^T, then (V2) C0^T's direction tile, (m, t, s) order
    const char* ctx;
    int64_t dz0_off, dzc_off;   // context offsets of the two dZ slots (8 | 4 feature tiles per sample tile)
    int64_t n;                  // samples
    int64_t n_tiles;            // 32-sample tiles that hold a sample
    const float* positions;     // (n,3), read when d_positions is asked for
    const float* directions;    // (n,3), read when d_directions is asked for
    float* d_x_enc;             // V1: (n, pe_dim) in the reference's column order, or NULL
    float* d_positions;         // (n,3) or NULL
    float* d_directions;        // V2: (n,3) or NULL
    int dir_freq;               // V2: 1..4
};

constexpr int kInputGradPosFreq = 10;                       // the training path's pos_freq (check_train_common)
constexpr int kInputGradPT = pe_tiles(kInputGradPosFreq);   // 2

template <class Mode, bool V2>
__global__ void __launch_bounds__(kPostGradWaves * 64) input_grad_kernel(const InputGradArgs P) {
    constexpr int PT = kInputGradPT;
    constexpr int64_t TB = tile_bytes<Mode>();
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const NRF_LDS char* frags = post_grad_resident<post_grad_frags<Mode, PT, V2>()>(P.wstream, lane, wave);
    for (int64_t st = (int64_t)blockIdx.x * kPostGradWaves + wave; st < P.n_tiles; st += (int64_t)gridDim.x * kPostGradWaves) {
        const PostGradRow row(st, c, P.n);
        {
            f32x16 acc[PT];
            post_grad_walk<Mode, PT>(frags, P.ctx + P.dz0_off + st * 8 * TB + lane * 16, acc);
            if constexpr (!V2) {
                if (P.d_x_enc && row.live) {
                    float* out = P.d_x_enc + row.raw * pe_dim(kInputGradPosFreq);
#pragma unroll
                    for (int u = 0; u < 16 * PT; ++u) {
                        const int idx = pe_ref_index(kInputGradPosFreq, u, h);
                        if (idx >= 0) out[idx] = acc[u >> 4][u & 15];
                    }
                }
            }
            if (P.d_positions) encoding_adjoint_store<PT>(acc, P.positions, kInputGradPosFreq, row, h, P.d_positions);
        }
        if constexpr (V2) {
            if (P.d_directions)
                post_grad_directions<Mode, post_grad_dir_frag0<Mode, PT>()>(frags, P.ctx + P.dzc_off + st * 4 * TB + lane * 16, P.directions, P.dir_freq,
                                                                            row, h, P.d_directions);
        }
    }
}

}  // namespace nrf
