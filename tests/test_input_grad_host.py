"""Host-side checks of the input gradient (include/nerfhip.h: nrf_mlp_backward_inputs, nrf_composite_backward_geom, nrf_ray_grad):
the library exports the entry points with the declared signatures, the packer's W0^T / color_layers.0^T streams replayed through
the numpy model of the MFMA lane maps (tests/mfma_emulator.py) give W0[:, pe]^T dZ exactly in the kernel's slot order, the new
kernels spill nothing, and bad arguments are refused on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mfma_emulator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrf_mlp_backward_inputs", "nrf_composite_backward_geom", "nrf_ray_grad", "nrf_debug_pack_input_grad")
L_POS, L_DIR = 10, 4
PE, DE = 3 * (2 * L_POS + 1), 3 * (2 * L_DIR + 1)


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def linears(L, net, n_layers, dir_freq=L_DIR):
    """Small-integer, asymmetric weights (exact in bf16 and f16), as tests/test_dino_grad_host.py builds them."""
    de = 3 * (2 * dir_freq + 1)
    if net == 1:
        shapes = [(256, PE)] + [(256, 256)] * (n_layers - 1) + [(1, 256), (3, 256)]
    else:
        shapes = [(256, PE)] + [(256, 256)] * (n_layers - 1) + [(1, 256), (256, 256), (128, 256 + de), (64, 128), (3, 64)]
    arr = (L.nrf_linear * len(shapes))()
    keep, ws = [], []
    for i, (o, k) in enumerate(shapes):
        r, c = np.meshgrid(np.arange(o), np.arange(k), indexing="ij")
        w = np.ascontiguousarray((((3 * r + 5 * c + i) % 7) - 3).astype(np.float32))
        b = np.zeros(o, np.float32)
        keep += [w, b]
        ws.append(w)
        arr[i] = L.nrf_linear(w.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p), o, k)
    return arr, len(shapes), L.nrf_arch(net, L_POS, dir_freq if net == 2 else 0, 256, n_layers, 0), ws, keep


def input_grad_stream(L, arr, n, arch, mode):
    nb = C.c_int64()
    L.check(L.lib().nrf_debug_pack_input_grad(C.byref(arch), arr, n, L.MMA_MODES[mode], None, 0, C.byref(nb)))
    raw = (C.c_uint8 * nb.value)()
    L.check(L.lib().nrf_debug_pack_input_grad(C.byref(arch), arr, n, L.MMA_MODES[mode], raw, nb.value, None))
    return bytes(raw)


def ref_index(Lf, u, h):
    """feature_map.hpp: the reference's feature index of (slot u, lane half h), -1 = padding."""
    if u < 3 * Lf:
        return 3 + 6 * (u // 3) + 3 * h + (u % 3)
    if u == 3 * Lf:
        return 2 if h else 0
    if u == 3 * Lf + 1:
        return -1 if h else 1
    return -1


@pytest.mark.parametrize("Lf", [10, 4])
def test_slot_map_of_the_encoding(Lf):
    """slot u < 3L is (f = u / 3, c = u % 3), sine in lane half 0 and cosine in half 1; the raw coordinates sit in slots 3L (x | z)
    and 3L + 1 (y | -); every reference column appears exactly once."""
    seen = {}
    for u in range(16 * ((3 * Lf + 2 + 15) // 16)):
        for h in (0, 1):
            idx = ref_index(Lf, u, h)
            if idx < 0:
                assert u > 3 * Lf or (u == 3 * Lf + 1 and h == 1)
                continue
            assert idx not in seen
            seen[idx] = (u, h)
            if u < 3 * Lf:
                f, c = u // 3, u % 3
                # positional_encoding.py:27-33: [x, sin(2^0 x) (3), cos(2^0 x) (3), sin(2^1 x), ...]
                assert idx == 3 + 6 * f + (3 if h else 0) + c
    assert sorted(seen) == list(range(3 * (2 * Lf + 1)))
    assert seen[0] == (3 * Lf, 0) and seen[1] == (3 * Lf + 1, 0) and seen[2] == (3 * Lf, 1)


def test_library_exports_the_new_entry_points_with_the_declared_signatures(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if p.strip()]
        res, args = L.SIGNATURES[name]
        assert hasattr(lib, name) and len(args) == len(params), (name, len(args), params)
        assert res is C.c_int, name
        for p, a in zip(params, args):
            if "*" in p:
                assert a in (C.c_void_p,) or hasattr(a, "contents") or issubclass(a, C._Pointer), (name, p, a)
            elif "int64_t" in p:
                assert a is C.c_int64, (name, p, a)
            else:
                assert a is C.c_int, (name, p, a)
    assert lib.nrf_abi_version() == 5                            # additive: no existing struct or signature changed


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("n_layers", [2, 8])
@pytest.mark.parametrize("net", [1, 2])
def test_packed_stream_replays_to_the_input_gradient(L, net, n_layers, mode):
    """The kernel's walk (train_input_grad_impl.hpp) in numpy: per output tile m the fragments (m, t, s) against the saved dZ tiles
    of the first Linear; accumulator register r of lane half h in tile m is dL/d feature (slot 16 m + r, half h).  V2: then the
    direction layer, from the next chunk boundary, against the 4 dZ tiles of color_layers.0."""
    arr, n, arch, ws, keep = linears(L, net, n_layers)
    raw = input_grad_stream(L, arr, n, arch, mode)
    SUB = 4 if mode == "f32" else 2
    chunks = 2 * 8 * SUB // 16 + (1 if net == 2 else 0)         # the direction layer: 4 * SUB <= 16 fragments, one chunk
    assert len(raw) == chunks * 16 * 1024
    rng = np.random.default_rng(7)
    dz0 = rng.integers(-4, 5, (256, 32)).astype(np.float32)      # (feature, sample)
    st = E.Stream(raw, mode)
    acc = E.dense(st, np.zeros(64, np.float32), E.quantize(E.tiles_from_matrix(dz0), mode), 2, None)
    W0 = ws[0]
    want = W0.T.astype(np.float64) @ dz0                         # (PE, 32)
    got = np.full((PE, 32), np.nan)
    for lane in range(64):
        c, h = lane & 31, lane >> 5
        for u in range(32):
            idx = ref_index(L_POS, u, h)
            if idx >= 0:
                got[idx, c] = acc[u >> 4, lane, u & 15]
            else:
                assert acc[u >> 4, lane, u & 15] == 0            # padding rows of W0^T are zero
    assert np.abs(want).max() > 50 and np.array_equal(got, want)
    if net == 2:
        dzc = rng.integers(-4, 5, (128, 32)).astype(np.float32)
        accd = E.dense(st, np.zeros(32, np.float32), E.quantize(E.tiles_from_matrix(dzc), mode), 1, None)
        C0 = ws[n_layers + 2]
        wantd = C0[:, 256:].T.astype(np.float64) @ dzc           # (DE, 32)
        gotd = np.full((DE, 32), np.nan)
        for lane in range(64):
            c, h = lane & 31, lane >> 5
            for u in range(16):
                idx = ref_index(L_DIR, u, h)
                if idx >= 0:
                    gotd[idx, c] = accd[0, lane, u]
                else:
                    assert accd[0, lane, u] == 0
        assert np.abs(wantd).max() > 20 and np.array_equal(gotd, wantd)


def test_kernel_resources_of_the_new_kernels():
    """input_grad_kernel (every instantiation) and ray_grad_kernel: no spilled VGPRs / SGPRs, no scratch; the input gradient is a
    translation unit of its own and the chain kernels stay in theirs."""
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere)")
    assert any(src == "train_input_grad.hip" and name == "train_input_grad" for src, name, _ in B.SOURCES)
    res = B.kernel_resources()
    ks = {k: v for k, v in res.items() if "train_input_grad:" in k and "input_grad_kernel<" in k}
    assert len(ks) == 6, sorted(ks)                              # bf16, f16, f32 x V1, V2
    for mode in ("ModeBF16", "ModeF16,", "ModeF32"):
        for v2 in ("false", "true"):
            assert [k for k in ks if mode in k and v2 in k], (mode, v2)
    rg = {k: v for k, v in res.items() if "staged_kernels:" in k and "ray_grad_kernel(" in k}
    assert len(rg) == 1, sorted(rg)
    for name, r in {**ks, **rg}.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    geom = {k: v for k, v in res.items() if "staged_kernels:" in k and "composite_backward_geom_kernel(" in k}
    assert len(geom) == 1 and all(r["vgpr_spill"] == 0 and r["scratch"] == 0 for r in geom.values()), geom
    assert not [k for k in res if "input_grad_kernel" in k and "train_input_grad:" not in k]


def test_bad_arguments_are_refused_on_the_host(L):
    lib = L.lib()
    fake = C.c_void_p(4096)                                      # never dereferenced: every call below fails its checks first
    assert lib.nrf_mlp_backward_inputs(None, 0, 32, fake, 1 << 30, fake, None, None, fake, None, None) == -1 and b"model" in lib.nrf_last_error()
    # the compositor's geometric backward
    a = (fake, 4, fake, 4, fake, fake)
    assert lib.nrf_composite_backward_geom(*a, -1, 8, 0, fake, None, None, fake, 4, fake, 4, fake, fake, None) == -1
    assert lib.nrf_composite_backward_geom(*a, 4, 0, 0, fake, None, None, fake, 4, fake, 4, fake, fake, None) == -1
    assert lib.nrf_composite_backward_geom(*a, 4, 8, 0, fake, None, None, fake, 4, fake, 4, None, fake, None) == -1
    assert lib.nrf_composite_backward_geom(*a, 4, 8, 0, fake, None, None, fake, 4, fake, 4, fake, None, None) == -1
    assert lib.nrf_composite_backward_geom(*a, 4, 8, 0, None, None, None, fake, 4, fake, 4, fake, fake, None) == -1
    assert lib.nrf_composite_backward_geom(*a, 0, 8, 0, fake, None, None, fake, 4, fake, 4, fake, fake, None) == 0       # nothing to do
    # the adjoint of the points
    assert lib.nrf_ray_grad(fake, None, fake, fake, None, None, -1, 8, fake, fake, None, None) == -1
    assert lib.nrf_ray_grad(fake, None, fake, fake, None, None, 4, 0, fake, fake, None, None) == -1
    assert lib.nrf_ray_grad(None, None, fake, fake, None, None, 4, 8, fake, fake, None, None) == -1
    assert lib.nrf_ray_grad(fake, None, fake, fake, None, None, 4, 8, None, None, None, None) == -1 and b"no output" in lib.nrf_last_error()
    assert lib.nrf_ray_grad(None, None, None, None, None, None, 0, 8, None, None, None, None) == 0                       # nothing to do
    # the streams belong to the V1 and V2 networks, and to the three training modes
    arr, n, arch, ws, keep = linears(L, 2, 2)
    assert lib.nrf_debug_pack_input_grad(C.byref(arch), arr, n, 3, None, 0, None) == -1
    assert lib.nrf_debug_pack_input_grad(None, arr, n, 0, None, 0, None) == -1
    arch.net = 3
    assert lib.nrf_debug_pack_input_grad(C.byref(arch), arr, n, 0, None, 0, None) == -1
    arch.net = 1                                                 # a V2 list handed in as V1: malformed
    assert lib.nrf_debug_pack_input_grad(C.byref(arch), arr, n, 0, None, 0, None) == -1
