// Host-only harness for the packer's part of the input gradient (csrc/packing.cpp: make_input_grad_plan), built under
// AddressSanitizer + UBSan by tests/test_input_grad_sanitize.py: the W0^T (positional-encoding tiles) and, V2, color_layers.0^T
// (direction-encoding tile) plan, its streams and gather tables, alone and appended to the backward chain's plan as the device
// holds it (api.cpp: ensure_train), for V1 / V2, trunk depths 2 / 8, dir_freq 1 / 4 and the three training modes; the V3 family and
// a malformed list must be refused.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nerf_few_shot_limitations_amd/csrc/feature_map.hpp"
#include "../../nerf_few_shot_limitations_amd/csrc/packing.hpp"

using namespace nrf;

static std::vector<HostLinear> linears(const std::vector<std::pair<int, int>>& shapes) {
    std::vector<HostLinear> out;
    unsigned s = 777u;
    for (auto& sh : shapes) {
        HostLinear l;
        l.out_f = sh.first; l.in_f = sh.second;
        l.w.resize((size_t)l.out_f * l.in_f); l.b.resize(l.out_f);
        for (auto& v : l.w) { s = s * 1664525u + 1013904223u; v = (float)((int)((s >> 8) & 0xFF) - 128); }       // integers: exact in every mode
        for (auto& v : l.b) v = 0.0f;
        out.push_back(l);
    }
    return out;
}

static std::vector<std::pair<int, int>> shapes_of(int net, int n, int dir_freq) {
    std::vector<std::pair<int, int>> sh = {{256, 63}};
    for (int i = 1; i < n; ++i) sh.push_back({256, 256});
    if (net == NRF_NET_V1) { sh.push_back({1, 256}); sh.push_back({3, 256}); return sh; }
    sh.push_back({1, 256}); sh.push_back({256, 256});
    sh.push_back({128, 256 + pe_dim(dir_freq)}); sh.push_back({64, 128}); sh.push_back({3, 64});
    return sh;
}

static int run(int net, int n, int dir_freq) {
    const nrf_arch a{net, 10, net == NRF_NET_V2 ? dir_freq : 0, 256, n, 0};
    std::string err;
    std::vector<HostLinear> lin = linears(shapes_of(net, n, dir_freq));
    NetPlan g, b;
    if (!make_input_grad_plan(a, lin, g, err)) { std::printf("make_input_grad_plan: %s\n", err.c_str()); return 1; }
    const size_t n_layers = net == NRF_NET_V2 ? 2 : 1;
    if (g.layers.size() != n_layers || g.layers[0].MT != 2 || g.layers[0].KT != 8 || !g.layers[0].transposed) { std::printf("unexpected plan\n"); return 1; }
    if (n_layers == 2 && (g.layers[1].MT != 1 || g.layers[1].KT != 4 || !g.layers[1].transposed)) { std::printf("unexpected direction layer\n"); return 1; }
    const ParamLayout lay = param_layout(lin);
    // every non-zero element of the fp32 gather table is one element of W0 (all of its 63 columns) or of the direction columns of
    // color_layers.0, each exactly once
    const int de = pe_dim(dir_freq), c0 = n + 2;
    const std::vector<int32_t> src = stream_sources(g, lay, kStreamF32);
    std::vector<int> seen0((size_t)256 * 63, 0), seen1((size_t)128 * de, 0);
    for (int32_t v : src) {
        if (v < 0) continue;
        if (v >= lay.w_off[0] && v < lay.w_off[0] + 256 * 63) { ++seen0[(size_t)(v - lay.w_off[0])]; continue; }
        if (net != NRF_NET_V2) { std::printf("source outside the first Linear\n"); return 1; }
        const int64_t rel = v - lay.w_off[c0];
        const int row = (int)(rel / (256 + de)), col = (int)(rel % (256 + de));
        if (rel < 0 || row >= 128 || col < 256) { std::printf("source outside the direction columns of color_layers.0\n"); return 1; }
        ++seen1[(size_t)row * de + col - 256];
    }
    for (int c : seen0) if (c != 1) { std::printf("an element of W0 packed %d times\n", c); return 1; }
    if (net == NRF_NET_V2) for (int c : seen1) if (c != 1) { std::printf("an element of the direction columns packed %d times\n", c); return 1; }
    size_t bytes = 0;
    for (int mode = 0; mode < 3; ++mode) {
        const PackedStream ps = pack_stream(g, lin, mode);
        const int SUB = mode == NRF_MMA_F32 ? 4 : 2;
        const size_t want = (size_t)(2 * 8 * SUB / 16 + (n_layers == 2 ? 1 : 0)) * 16 * 1024;      // every layer whole chunks
        if (ps.bytes.size() != want || ps.n_chunks * 16u * 1024u != want) { std::printf("stream size %zu != %zu\n", ps.bytes.size(), want); return 1; }
        bytes += want;
        // behind the chain's layers, as the device stream holds it: the tail of the combined stream is the stand-alone stream
        if (!make_backward_plan(a, lin, b, err)) { std::printf("make_backward_plan: %s\n", err.c_str()); return 1; }
        const size_t chain = pack_stream(b, lin, mode).bytes.size();
        for (const auto& l : g.layers) b.layers.push_back(l);
        const PackedStream both = pack_stream(b, lin, mode);
        if (both.bytes.size() != chain + want || std::memcmp(both.bytes.data() + chain, ps.bytes.data(), want) != 0) {
            std::printf("combined stream does not end in the input-gradient layers\n");
            return 1;
        }
        const std::vector<int32_t> s2 = stream_sources(b, lay, stream_kind(mode));
        for (int32_t v : s2) if (v >= lay.total || v < -1) { std::printf("source out of range\n"); return 1; }
    }
    std::printf("net=%d n=%d dir_freq=%d ok: %zu stream bytes\n", net, n, dir_freq, bytes);
    return 0;
}

int main() {
    int rc = 0;
    for (int n : {2, 8}) {
        rc |= run(NRF_NET_V1, n, 0);
        rc |= run(NRF_NET_V2, n, 4);
        rc |= run(NRF_NET_V2, n, 1);
    }
    std::string err;
    NetPlan plan;
    {   // the V3 family and a malformed list are refused, not walked
        const nrf_arch v3{NRF_NET_V3, 12, 4, 256, 2, 64};
        std::vector<HostLinear> l2 = linears(shapes_of(NRF_NET_V2, 2, 4));
        if (make_input_grad_plan(v3, l2, plan, err)) { std::printf("V3 accepted\n"); rc = 1; }
        const nrf_arch v1{NRF_NET_V1, 10, 0, 256, 2, 0};
        if (make_input_grad_plan(v1, l2, plan, err)) { std::printf("malformed V1 accepted\n"); rc = 1; }
        const nrf_arch v2bad{NRF_NET_V2, 10, 5, 256, 2, 0};
        std::vector<HostLinear> l5 = linears(shapes_of(NRF_NET_V2, 2, 5));
        if (make_input_grad_plan(v2bad, l5, plan, err)) { std::printf("dir_freq 5 accepted\n"); rc = 1; }
    }
    std::printf(rc ? "FAILED\n" : "sanitize ok\n");
    return rc;
}
