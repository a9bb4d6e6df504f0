// freq_mask.hpp -- the per-column scale of the positional encodings (nerfhip.h: nrf_model_set_freq_mask; FreeNeRF's frequency
// mask in its general form).  A scale m on an encoding is a column scale of the Linears that read it, W (m . enc) = (W diag m) enc,
// so the mask lives where the weights are packed and where their gradient is scattered (freq_mask.hip), and nowhere else:
//
//   family | position encoding read by                       | direction encoding read by
//   V1     | layers.0 (linear 0), all columns                | --
//   V2     | density_layers.0 (linear 0), all columns        | color_layers.0 (linear n+2), columns [hidden, hidden + dir_dim)
//   V3     | dino_fusion.fusion.0 (linear 0), [0, pos_dim)   | color_layers.0 (linear n+7), columns [hidden, hidden + dir_dim)
//
// Scale ids: position column c is id c, direction column c is id pos_cols + c; one vector of kFreqCols floats holds both and
// travels by value in the kernels' arguments.
#pragma once
#include <cstdint>
#include <vector>

#include "packing.hpp"

namespace nrf {

constexpr int kFreqCols = 120;          // 3 (2 * 15 + 1) position columns (make_plan: pos_freq <= 15) + 3 (2 * 4 + 1) direction columns

struct FreqMaskArgs {
    const int8_t* ids;                  // device, one per flat parameter: scale id, -1 = none
    float scale[kFreqCols];
};

inline int freq_pos_cols(const nrf_arch& a) { return 3 * (2 * a.pos_freq + 1); }
inline int freq_dir_cols(const nrf_arch& a) { return a.net == NRF_NET_V1 ? 0 : 3 * (2 * a.dir_freq + 1); }

// (linear index, first column, columns, first scale id) of the at most two masked column ranges
struct FreqRange { int lin, col0, n, id0; };
inline int freq_ranges(const nrf_arch& a, FreqRange out[2]) {
    out[0] = {0, 0, freq_pos_cols(a), 0};
    if (a.net == NRF_NET_V1) return 1;
    out[1] = {(a.net == NRF_NET_V3 ? 5 : 0) + a.n_layers + 2, a.hidden, freq_dir_cols(a), freq_pos_cols(a)};
    return 2;
}

// flat parameter index -> scale id (-1 = none)
inline std::vector<int8_t> freq_scale_ids(const nrf_arch& a, const ParamLayout& lay) {
    std::vector<int8_t> ids((size_t)lay.total, (int8_t)-1);
    FreqRange r[2];
    const int nr = freq_ranges(a, r);
    for (int k = 0; k < nr; ++k) {
        const int64_t rows = (lay.b_off[r[k].lin] - lay.w_off[r[k].lin]) / lay.in_f[r[k].lin];
        for (int64_t o = 0; o < rows; ++o)
            for (int c = 0; c < r[k].n; ++c) ids[(size_t)(lay.w_off[r[k].lin] + o * lay.in_f[r[k].lin] + r[k].col0 + c)] = (int8_t)(r[k].id0 + c);
    }
    return ids;
}

// the Linears with the masked columns multiplied in fp32: what the host packer reads under a mask
inline void freq_scale_linears(const nrf_arch& a, std::vector<HostLinear>& lin, const float* scale) {
    FreqRange r[2];
    const int nr = freq_ranges(a, r);
    for (int k = 0; k < nr; ++k) {
        HostLinear& l = lin[r[k].lin];
        for (int o = 0; o < l.out_f; ++o)
            for (int c = 0; c < r[k].n; ++c) l.w[(size_t)o * l.in_f + r[k].col0 + c] *= scale[r[k].id0 + c];       // one rounded fp32 product
    }
}

}  // namespace nrf
