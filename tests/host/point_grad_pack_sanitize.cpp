// Host-only harness for the V3 input-gradient plan of the weight packer (csrc/packing.cpp:make_input_grad_v3_plan): the plan, its
// packed streams in the three training modes and its device re-pack source tables, alone and behind the dZ chain's and the
// feature gradient's layers as api.cpp:ensure_train strings them.  Built under AddressSanitizer + UBSan by
// tests/test_point_grad_host.py (sanitizers run on the CPU build only).
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../nerf_few_shot_limitations_amd/csrc/packing.hpp"

using namespace nrf;

static std::vector<HostLinear> linears(const std::vector<std::pair<int, int>>& shapes) {
    std::vector<HostLinear> out;
    unsigned s = 54321u;
    for (auto& sh : shapes) {
        HostLinear l;
        l.out_f = sh.first; l.in_f = sh.second;
        l.w.resize((size_t)l.out_f * l.in_f); l.b.resize(l.out_f);
        for (auto& v : l.w) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xFFFF) / 65536.0f - 0.5f; }
        for (auto& v : l.b) { s = s * 1664525u + 1013904223u; v = ((s >> 8) & 0xFFFF) / 65536.0f - 0.5f; }
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

int main() {
    int rc = 0;
    std::string err;
    for (int n = 1; n <= 8; n += (n == 1 ? 1 : 3))
        for (int dd = 64; dd <= 128; dd += 64) {
            nrf_arch a{NRF_NET_V3, 12, 4, 256, n, dd};
            const std::vector<HostLinear> lin = linears(v3_shapes(n, dd));
            const ParamLayout lay = param_layout(lin);
            NetPlan ip, gp, bp;
            if (!make_input_grad_v3_plan(a, lin, ip, err)) { std::printf("v3 n=%d d=%d: %s\n", n, dd, err.c_str()); rc = 1; continue; }
            if (ip.layers.size() != 2 || ip.layers[0].MT != 3 || ip.layers[0].KT != 8 || ip.layers[1].MT != 1 || ip.layers[1].KT != 4) {
                std::printf("v3 n=%d d=%d: unexpected plan shape\n", n, dd); rc = 1; continue;
            }
            if (!make_backward_plan(a, lin, bp, err) || !make_dino_grad_plan(a, lin, gp, err)) { std::printf("plans: %s\n", err.c_str()); rc = 1; continue; }
            bp.layers.push_back(gp.layers[0]);
            for (const auto& L : ip.layers) bp.layers.push_back(L);
            size_t bytes = 0;
            for (int mode = 0; mode < 3; ++mode) {
                const PackedStream alone = pack_stream(ip, lin, mode), behind = pack_stream(bp, lin, mode);
                const size_t want = (size_t)(mode == NRF_MMA_F32 ? 6 + 1 : 3 + 1) * 16 * 1024;
                if (alone.bytes.size() != want || behind.bytes.size() < want) { std::printf("v3 n=%d d=%d mode %d: stream size\n", n, dd, mode); rc = 1; }
                // the layers ride at the end of the chain's stream unchanged
                if (!std::equal(alone.bytes.begin(), alone.bytes.end(), behind.bytes.end() - (std::ptrdiff_t)alone.bytes.size())) {
                    std::printf("v3 n=%d d=%d mode %d: the riding layers differ from the plan packed alone\n", n, dd, mode); rc = 1;
                }
                bytes += behind.bytes.size();
            }
            for (int kind = 0; kind < 2; ++kind) {
                const std::vector<int32_t> src = stream_sources(bp, lay, kind);
                for (int32_t v : src) if (v >= lay.total || v < -1) { std::printf("source out of range\n"); rc = 1; break; }
            }
            std::printf("v3 n=%d d=%d ok: %zu stream bytes\n", n, dd, bytes);
        }
    // other families and malformed lists are refused, not walked
    NetPlan plan;
    nrf_arch v2{NRF_NET_V2, 10, 4, 256, 2, 0};
    const std::vector<HostLinear> l2 = linears({{256, 63}, {256, 256}, {1, 256}, {256, 256}, {128, 283}, {64, 128}, {3, 64}});
    if (make_input_grad_v3_plan(v2, l2, plan, err)) { std::printf("V2 accepted\n"); rc = 1; }
    nrf_arch v3{NRF_NET_V3, 12, 4, 256, 8, 64};
    if (make_input_grad_v3_plan(v3, l2, plan, err)) { std::printf("malformed V3 accepted\n"); rc = 1; }
    nrf_arch v3c{NRF_NET_V3, 12, 4, 256, 2, 96};
    if (make_input_grad_v3_plan(v3c, linears(v3_shapes(2, 96)), plan, err)) { std::printf("dino_dim 96 accepted\n"); rc = 1; }
    std::printf(rc ? "FAILED\n" : "sanitize ok\n");
    return rc;
}
