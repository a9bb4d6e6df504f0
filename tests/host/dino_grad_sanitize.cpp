// Host-only harness for the packer's part of the DINO feature gradient (csrc/packing.cpp: make_dino_grad_plan), built under
// AddressSanitizer + UBSan by tests/test_dino_grad_sanitize.py: the one-layer W0d^T plan, its streams and gather tables, alone and
// appended to the backward chain's plan as the device holds it (api.cpp: ensure_train), for dino_dim 64 / 128, trunk depths 1 / 8 and
// the three training modes; the other network families and a malformed list must be refused.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

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

static std::vector<std::pair<int, int>> v3_shapes(int n, int dd) {
    std::vector<std::pair<int, int>> sh = {{256, 75 + dd}, {256, 256}, {64, 256}, {2, 64}, {256, 256}};
    for (int i = 0; i < n; ++i) sh.push_back({256, 256});
    sh.push_back({1, 256}); sh.push_back({256, 256});
    sh.push_back({128, 256 + 27}); sh.push_back({64, 128}); sh.push_back({3, 64});
    return sh;
}

static int run(int n, int dd) {
    const nrf_arch a{NRF_NET_V3, 12, 4, 256, n, dd};
    std::string err;
    std::vector<HostLinear> lin = linears(v3_shapes(n, dd));
    NetPlan g, b;
    if (!make_dino_grad_plan(a, lin, g, err)) { std::printf("make_dino_grad_plan: %s\n", err.c_str()); return 1; }
    const int DT = dd / 32;
    if (g.layers.size() != 1 || g.layers[0].MT != DT || g.layers[0].KT != 8 || !g.layers[0].transposed) { std::printf("unexpected plan\n"); return 1; }
    const ParamLayout lay = param_layout(lin);
    // every element of the fp32 gather table is one element of W0's DINO columns, each exactly once
    const std::vector<int32_t> src = stream_sources(g, lay, kStreamF32);
    std::vector<int> seen((size_t)256 * dd, 0);
    for (int32_t v : src) {
        if (v < 0) { std::printf("zero element inside W0d^T\n"); return 1; }
        const int64_t rel = v - lay.w_off[0];
        const int row = (int)(rel / (75 + dd)), col = (int)(rel % (75 + dd));
        if (rel < 0 || row >= 256 || col < 75) { std::printf("source outside the DINO columns of fusion.0\n"); return 1; }
        ++seen[(size_t)row * dd + col - 75];
    }
    for (int c : seen) if (c != 1) { std::printf("an element of W0d packed %d times\n", c); return 1; }
    size_t bytes = 0;
    for (int mode = 0; mode < 3; ++mode) {
        const PackedStream ps = pack_stream(g, lin, mode);
        const size_t want = (size_t)DT * 8 * (mode == NRF_MMA_F32 ? 4 : 2) * 1024;
        if (ps.bytes.size() != want || ps.n_chunks * 16u * 1024u != want) { std::printf("stream size %zu != %zu\n", ps.bytes.size(), want); return 1; }
        bytes += want;
        // behind the chain's layers, as the device stream holds it: the tail of the combined stream is the stand-alone stream
        if (!make_backward_plan(a, lin, b, err)) { std::printf("make_backward_plan: %s\n", err.c_str()); return 1; }
        const size_t chain = pack_stream(b, lin, mode).bytes.size();
        b.layers.push_back(g.layers[0]);
        const PackedStream both = pack_stream(b, lin, mode);
        if (both.bytes.size() != chain + want || std::memcmp(both.bytes.data() + chain, ps.bytes.data(), want) != 0) {
            std::printf("combined stream does not end in the W0d^T layer\n");
            return 1;
        }
        const std::vector<int32_t> s2 = stream_sources(b, lay, stream_kind(mode));
        for (int32_t v : s2) if (v >= lay.total || v < -1) { std::printf("source out of range\n"); return 1; }
    }
    std::printf("v3 n=%d dino_dim=%d ok: %zu stream bytes\n", n, dd, bytes);
    return 0;
}

int main() {
    int rc = 0;
    for (int n : {1, 8})
        for (int dd : {64, 128}) rc |= run(n, dd);
    std::string err;
    NetPlan plan;
    {   // other families and a malformed list are refused, not walked
        const nrf_arch v2{NRF_NET_V2, 10, 4, 256, 2, 0};
        std::vector<HostLinear> l2 = linears({{256, 63}, {256, 256}, {1, 256}, {256, 256}, {128, 283}, {64, 128}, {3, 64}});
        if (make_dino_grad_plan(v2, l2, plan, err)) { std::printf("V2 accepted\n"); rc = 1; }
        const nrf_arch v3{NRF_NET_V3, 12, 4, 256, 2, 64};
        if (make_dino_grad_plan(v3, l2, plan, err)) { std::printf("malformed V3 accepted\n"); rc = 1; }
        const nrf_arch v3odd{NRF_NET_V3, 12, 4, 256, 2, 96};
        std::vector<HostLinear> l3 = linears(v3_shapes(2, 96));
        if (make_dino_grad_plan(v3odd, l3, plan, err)) { std::printf("dino_dim 96 accepted\n"); rc = 1; }
    }
    std::printf(rc ? "FAILED\n" : "sanitize ok\n");
    return rc;
}
