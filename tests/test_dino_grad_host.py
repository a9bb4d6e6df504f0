"""Host-side checks of the DINO feature gradient (include/nerfhip.h: nrf_mlp_backward_dino, nrf_project_fetch_backward,
nrf_sample_features_backward): the library exports the entry points with the declared signatures, the packer's W0d^T stream
replayed through the numpy model of the MFMA lane maps (tests/mfma_emulator.py) gives W0d^T d1 + w1 W0d^T d2 exactly, and bad
arguments are refused on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import mfma_emulator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrf_mlp_backward_dino", "nrf_fetch_backward_workspace_bytes", "nrf_project_fetch_backward", "nrf_sample_features_backward",
       "nrf_debug_pack_dino_grad")
PE = 3 * (2 * 12 + 1)


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def v3_linears(L, dino_dim, n_layers=1):
    """Small-integer, asymmetric weights: W0[k][j] differs from W0[j][k] and from its neighbours, exact in bf16 and f16."""
    shapes = [(256, PE + dino_dim), (256, 256), (64, 256), (2, 64), (256, 256)] + [(256, 256)] * n_layers + \
             [(1, 256), (256, 256), (128, 256 + 27), (64, 128), (3, 64)]
    arr = (L.nrf_linear * len(shapes))()
    keep, ws = [], []
    for i, (o, k) in enumerate(shapes):
        r, c = np.meshgrid(np.arange(o), np.arange(k), indexing="ij")
        w = np.ascontiguousarray((((3 * r + 5 * c + i) % 7) - 3).astype(np.float32))
        b = np.zeros(o, np.float32)
        keep += [w, b]
        ws.append(w)
        arr[i] = L.nrf_linear(w.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p), o, k)
    return arr, len(shapes), L.nrf_arch(3, 12, 4, 256, n_layers, dino_dim), ws, keep


def dino_grad_stream(L, arr, n, arch, mode):
    nb = C.c_int64()
    L.check(L.lib().nrf_debug_pack_dino_grad(C.byref(arch), arr, n, L.MMA_MODES[mode], None, 0, C.byref(nb)))
    raw = (C.c_uint8 * nb.value)()
    L.check(L.lib().nrf_debug_pack_dino_grad(C.byref(arch), arr, n, L.MMA_MODES[mode], raw, nb.value, None))
    return bytes(raw)


def test_library_exports_the_new_entry_points_with_the_declared_signatures(L):
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    for name in NEW:
        m = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(",") if p.strip()]
        res, args = L.SIGNATURES[name]
        assert hasattr(lib, name) and len(args) == len(params), (name, len(args), params)
        assert res is (C.c_int64 if m.group(1) == "int64_t" else C.c_int), name
        for p, a in zip(params, args):                         # int64_t <-> c_int64, pointers <-> pointer types, int <-> c_int
            if "*" in p:
                assert a in (C.c_void_p,) or hasattr(a, "contents") or issubclass(a, C._Pointer), (name, p, a)
            elif "int64_t" in p:
                assert a is C.c_int64, (name, p, a)
            else:
                assert a is C.c_int, (name, p, a)
    assert lib.nrf_abi_version() == 5                            # additive: no existing struct or signature changed


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("dino_dim", [64, 128])
def test_packed_stream_replays_to_the_feature_gradient(L, mode, dino_dim):
    """The kernel's walk (train_dino_grad_impl.hpp) in numpy: per output tile m the fragments (m, t, s) against the saved dZ tiles
    of fusion.0's two passes, two accumulator sets, acc1 + w1 * acc2 written at 32 m + 8 g + 4 h + q of the sample's row."""
    DT = dino_dim // 32
    arr, n, arch, ws, keep = v3_linears(L, dino_dim)
    raw = dino_grad_stream(L, arr, n, arch, mode)
    SUB = 4 if mode == "f32" else 2
    assert len(raw) == DT * 8 * SUB * 1024                       # exactly the layer: DT x 8 tile pairs, whole chunks
    rng = np.random.default_rng(5)
    d1 = rng.integers(-4, 5, (256, 32)).astype(np.float32)       # dZ fusion.0 pass 1 / pass 2: (feature, sample)
    d2 = rng.integers(-4, 5, (256, 32)).astype(np.float32)
    w1 = 0.25                                                    # a power of two: every operation below is exact
    zero = np.zeros(32 * DT, np.float32)
    acc1 = E.dense(E.Stream(raw, mode), zero, E.quantize(E.tiles_from_matrix(d1), mode), DT, None)
    acc2 = E.dense(E.Stream(raw, mode), zero, E.quantize(E.tiles_from_matrix(d2), mode), DT, None)
    out = np.full((32, dino_dim), np.nan, np.float32)            # (sample, channel) rows as the kernel writes them
    for lane in range(64):
        c, h = lane & 31, lane >> 5
        for m in range(DT):
            for g in range(4):
                for q in range(4):
                    out[c, 32 * m + 8 * g + 4 * h + q] = acc1[m, lane, 4 * g + q] + np.float32(w1) * acc2[m, lane, 4 * g + q]
    W0d = ws[0][:, PE:]                                          # (256, C): the DINO columns of fusion.0
    want = (W0d.T.astype(np.float64) @ d1 + w1 * (W0d.T.astype(np.float64) @ d2)).T
    assert np.abs(want).max() > 50 and np.array_equal(out.astype(np.float64), want)


def test_dino_grad_stream_is_the_transposed_dino_block_of_the_backward_stream(L):
    """Same fragments as the F0T layer of the backward chain restricted to the DINO tiles: the fp32 stream holds exactly the
    values of W0d (each once per (row, column)) and nothing of the position-encoding columns."""
    arr, n, arch, ws, keep = v3_linears(L, 64)
    frags = np.frombuffer(dino_grad_stream(L, arr, n, arch, "f32"), np.float32).reshape(2, 8, 4, 64, 4)      # (m, t, g, lane, e)
    W0 = ws[0]
    for m in range(2):
        for t in range(8):
            for g in range(4):
                for lane in (0, 17, 45, 63):
                    i, h = lane & 31, lane >> 5
                    for e in range(4):
                        assert frags[m, t, g, lane, e] == W0[32 * t + 8 * g + 4 * h + e, PE + 32 * m + i]


def test_bad_arguments_are_refused_on_the_host(L):
    lib = L.lib()
    assert lib.nrf_mlp_backward_dino(None, 0, 32, None, 0, None, None) == -1 and b"model" in lib.nrf_last_error()
    assert lib.nrf_fetch_backward_workspace_bytes(0, 9, 64, 10) == -1
    assert lib.nrf_fetch_backward_workspace_bytes(9, 9, 64, -1) == -1 and b"bad sizes" in lib.nrf_last_error()
    assert lib.nrf_fetch_backward_workspace_bytes(9, 9, 64, 0) >= 9 * 9 * 64 * 4
    # one slab copy of the map at least, and a function of the sizes alone
    assert lib.nrf_fetch_backward_workspace_bytes(9, 9, 64, 65536) % (9 * 9 * 64 * 4) == 0
    fake = C.c_void_p(4096)                                      # never dereferenced: every call below fails its checks first
    d = L.nrf_dino(None, 9, 9, 64, (C.c_float * 16)(), 100.0, 128, 128)
    assert lib.nrf_project_fetch_backward(None, fake, 4, fake, fake, 0, fake, 1 << 30, None) == -1
    assert lib.nrf_project_fetch_backward(C.byref(d), fake, -1, fake, fake, 0, fake, 1 << 30, None) == -1
    assert lib.nrf_project_fetch_backward(C.byref(d), fake, 4, fake, None, 0, fake, 1 << 30, None) == -1
    assert lib.nrf_project_fetch_backward(C.byref(d), fake, 4, None, fake, 0, fake, 1 << 30, None) == -1
    assert lib.nrf_project_fetch_backward(C.byref(d), fake, 4, fake, fake, 0, None, 1 << 30, None) == -1
    assert lib.nrf_project_fetch_backward(C.byref(d), fake, 4, fake, fake, 0, fake, 16, None) == -1 and b"workspace" in lib.nrf_last_error()
    assert lib.nrf_sample_features_backward(9, 9, 0, fake, 4, fake, fake, 0, fake, 1 << 30, None) == -1
    assert lib.nrf_sample_features_backward(9, 9, 64, fake, 4, fake, fake, 1, fake, 16, None) == -1
    assert lib.nrf_sample_features_backward(9, 9, 64, None, 0, None, fake, 1, None, 0, None) == 0      # nothing to add
    # the W0d^T stream belongs to the V3 network
    for net, nl in ((1, 2), (2, 2)):
        arr, n, arch, ws, keep = v3_linears(L, 64)
        arch.net = net
        assert lib.nrf_debug_pack_dino_grad(C.byref(arch), arr, n, 0, None, 0, None) == -1
    arr, n, arch, ws, keep = v3_linears(L, 64)
    assert lib.nrf_debug_pack_dino_grad(C.byref(arch), arr, n, 3, None, 0, None) == -1      # no split-f16 training mode
    assert lib.nrf_debug_pack_dino_grad(None, arr, n, 0, None, 0, None) == -1
