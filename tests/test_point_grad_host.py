"""Host-side checks of the V3 point gradient (include/nerfhip.h: nrf_mlp_backward_inputs_v3, nrf_project_fetch_backward_points,
nrf_sample_features_backward_points): the library exports the entry points with the declared signatures, the packer's W0p^T /
color_layers.0^T streams replayed through the numpy model of the MFMA lane maps (tests/mfma_emulator.py) give
W0p^T d1 + w0 W0p^T d2 exactly in the kernel's slot order, the new kernels spill nothing, bad arguments are refused on the host,
the closed form of the fetch adjoint that the header states agrees with autograd through the oracle, and the new plan is clean
under AddressSanitizer + UBSan (a stand-alone program: nothing sanitised is loaded into python)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import mfma_emulator as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrf_mlp_backward_inputs_v3", "nrf_project_fetch_backward_points", "nrf_sample_features_backward_points", "nrf_debug_pack_input_grad_v3")
L_POS, L_DIR = 12, 4
PE, DE = 3 * (2 * L_POS + 1), 3 * (2 * L_DIR + 1)


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def linears(L, n_layers, dino_dim):
    """Small-integer, asymmetric weights (exact in bf16 and f16), as tests/test_dino_grad_host.py builds them."""
    shapes = [(256, PE + dino_dim), (256, 256), (64, 256), (2, 64), (256, 256)] + [(256, 256)] * n_layers + \
             [(1, 256), (256, 256), (128, 256 + DE), (64, 128), (3, 64)]
    arr = (L.nrf_linear * len(shapes))()
    keep, ws = [], []
    for i, (o, k) in enumerate(shapes):
        r, c = np.meshgrid(np.arange(o), np.arange(k), indexing="ij")
        w = np.ascontiguousarray((((3 * r + 5 * c + i) % 7) - 3).astype(np.float32))
        b = np.zeros(o, np.float32)
        keep += [w, b]
        ws.append(w)
        arr[i] = L.nrf_linear(w.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p), o, k)
    return arr, len(shapes), L.nrf_arch(3, L_POS, L_DIR, 256, n_layers, dino_dim), ws, keep


def input_grad_v3_stream(L, arr, n, arch, mode):
    nb = C.c_int64()
    L.check(L.lib().nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, L.MMA_MODES[mode], None, 0, C.byref(nb)))
    raw = (C.c_uint8 * nb.value)()
    L.check(L.lib().nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, L.MMA_MODES[mode], raw, nb.value, None))
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


def test_slot_map_of_the_l12_encoding():
    """pos_freq 12: 38 slots in three 16-slot tiles; slot u < 36 is (f = u / 3, c = u % 3), sine in lane half 0 and cosine in half 1;
    the raw coordinates sit in slots 36 (x | z) and 37 (y | -); slots 38 .. 47 are padding; every reference column appears once."""
    assert (3 * L_POS + 2 + 15) // 16 == 3
    seen = {}
    for u in range(48):
        for h in (0, 1):
            idx = ref_index(L_POS, u, h)
            if idx < 0:
                assert u >= 38 or (u == 37 and h == 1)
                continue
            assert idx not in seen
            seen[idx] = (u, h)
            if u < 36:
                assert idx == 3 + 6 * (u // 3) + (3 if h else 0) + u % 3
    assert sorted(seen) == list(range(PE)) and PE == 75
    assert seen[0] == (36, 0) and seen[1] == (37, 0) and seen[2] == (36, 1)
    assert max(u // 3 for u in range(36)) == 11              # 2^11 is the largest frequency: the adjoint's 1 << f stays below 1 << 15


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
@pytest.mark.parametrize("dino_dim", [64, 128])
def test_packed_stream_replays_to_the_v3_input_gradient(L, dino_dim, n_layers, mode):
    """The kernel's walk (train_input_grad_v3_impl.hpp) in numpy: per output tile m the fragments (m, t, s) against the saved dZ
    tiles of BOTH fusion.0 passes, joined as acc1 + w0 acc2 with the sample's gate; accumulator register r of lane half h in tile m
    is dL/d feature (slot 16 m + r, half h).  Then the direction layer, from the next chunk boundary, against the 4 dZ tiles of
    color_layers.0.  Integer weights and gradients and a gate of quarters: every product and sum is exact, so equality is exact."""
    arr, n, arch, ws, keep = linears(L, n_layers, dino_dim)
    raw = input_grad_v3_stream(L, arr, n, arch, mode)
    SUB = 4 if mode == "f32" else 2
    assert len(raw) == (3 * 8 * SUB // 16 + 1) * 16 * 1024     # the direction layer: 4 * SUB <= 16 fragments, one chunk
    rng = np.random.default_rng(11)
    d1 = rng.integers(-4, 5, (256, 32)).astype(np.float32)      # (feature, sample)
    d2 = rng.integers(-4, 5, (256, 32)).astype(np.float32)
    w0 = (rng.integers(0, 5, 32) / 4.0).astype(np.float32)
    zero = np.zeros(96, np.float32)
    s1, s2 = E.Stream(raw, mode), E.Stream(raw, mode)
    acc1 = E.dense(s1, zero, E.quantize(E.tiles_from_matrix(d1), mode), 3, None)
    acc2 = E.dense(s2, zero, E.quantize(E.tiles_from_matrix(d2), mode), 3, None)
    W0p = ws[0][:, :PE].astype(np.float64)                       # the positional columns of fusion.0 come first (lora_dino.py:181)
    want = W0p.T @ d1 + w0[None, :].astype(np.float64) * (W0p.T @ d2)
    got = np.full((PE, 32), np.nan)
    for lane in range(64):
        c, h = lane & 31, lane >> 5
        for u in range(48):
            joined = np.float32(acc1[u >> 4, lane, u & 15]) + w0[c] * np.float32(acc2[u >> 4, lane, u & 15])
            idx = ref_index(L_POS, u, h)
            if idx >= 0:
                got[idx, c] = joined
            else:
                assert joined == 0                               # padding rows of W0p^T are zero
    assert np.abs(want).max() > 50 and np.array_equal(got, want)
    dzc = rng.integers(-4, 5, (128, 32)).astype(np.float32)
    accd = E.dense(s1, np.zeros(32, np.float32), E.quantize(E.tiles_from_matrix(dzc), mode), 1, None)
    C0 = ws[5 + n_layers + 2]
    wantd = C0[:, 256:].T.astype(np.float64) @ dzc               # (DE, 32)
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
    """input_grad_v3_kernel (three modes x positions / directions / both) and fetch_points_backward_kernel (16-byte and scalar
    loads): no spilled VGPRs / SGPRs, no scratch; the V3 input gradient is a translation unit of its own."""
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere)")
    assert any(src == "train_input_grad_v3.hip" and name == "train_input_grad_v3" for src, name, _ in B.SOURCES)
    res = B.kernel_resources()
    ks = {k: v for k, v in res.items() if "train_input_grad_v3:" in k and "input_grad_v3_kernel<" in k}
    assert len(ks) == 9, sorted(ks)
    for mode in ("ModeBF16", "ModeF16,", "ModeF32"):
        for which in ("true, true", "true, false", "false, true"):
            assert [k for k in ks if mode in k and which in k], (mode, which)
    fp = {k: v for k, v in res.items() if "staged_kernels:" in k and "fetch_points_backward_kernel<" in k}
    assert len(fp) == 2, sorted(fp)
    for name, r in {**ks, **fp}.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    assert not [k for k in res if "input_grad_v3_kernel" in k and "train_input_grad_v3:" not in k]
    assert not [k for k in res if "train_input_grad_v3:" in k and "input_grad_v3_kernel" not in k]      # no chain kernel moved here


def test_bad_arguments_are_refused_on_the_host(L):
    lib = L.lib()
    fake = C.c_void_p(4096)                                      # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(4098)
    assert lib.nrf_mlp_backward_inputs_v3(None, 0, 32, fake, 1 << 30, fake, fake, fake, fake, None) == -1 and b"model" in lib.nrf_last_error()
    # the adjoint of project + fetch with respect to the points
    d = L.nrf_dino()
    d.features, d.Hp, d.Wp, d.C, d.focal, d.H, d.W = 4096, 9, 9, 64, 100.0, 64, 64
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, -1, fake, fake, 0, None) == -1
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, 0, fake, fake, 0, None) == 0                        # nothing to do
    assert lib.nrf_project_fetch_backward_points(C.byref(d), None, 4, fake, fake, 0, None) == -1
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, 4, None, fake, 0, None) == -1
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, 4, fake, None, 1, None) == -1
    assert lib.nrf_project_fetch_backward_points(None, fake, 4, fake, fake, 0, None) == -1
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, 4, fake, odd, 0, None) == -1 and b"aligned" in lib.nrf_last_error()
    d.C = 0
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, 4, fake, fake, 0, None) == -1
    d.C, d.features = 64, None                                   # unlike the map's adjoint, this one reads the map
    assert lib.nrf_project_fetch_backward_points(C.byref(d), fake, 4, fake, fake, 0, None) == -1 and b"features" in lib.nrf_last_error()
    # the same for normalised image points
    assert lib.nrf_sample_features_backward_points(fake, 0, 9, 64, fake, 4, fake, fake, None) == -1
    assert lib.nrf_sample_features_backward_points(fake, 9, 9, 64, fake, -1, fake, fake, None) == -1
    assert lib.nrf_sample_features_backward_points(fake, 9, 9, 64, fake, 0, fake, fake, None) == 0
    assert lib.nrf_sample_features_backward_points(None, 9, 9, 64, fake, 4, fake, fake, None) == -1
    assert lib.nrf_sample_features_backward_points(fake, 9, 9, 64, fake, 4, fake, None, None) == -1
    assert lib.nrf_sample_features_backward_points(fake, 9, 9, 64, odd, 4, fake, fake, None) == -1 and b"aligned" in lib.nrf_last_error()
    # the streams belong to the V3 network with a feature width the kernels are built for, and to the three training modes
    arr, n, arch, ws, keep = linears(L, 2, 64)
    assert lib.nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, 3, None, 0, None) == -1
    assert lib.nrf_debug_pack_input_grad_v3(None, arr, n, 0, None, 0, None) == -1
    nb = C.c_int64()
    assert lib.nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, 0, None, 0, C.byref(nb)) == 0 and nb.value == 4 * 16 * 1024
    small = (C.c_uint8 * 16)()
    assert lib.nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, 0, small, 16, None) == -1
    arch.net = 2
    assert lib.nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, 0, None, 0, None) == -1
    arch.net, arch.dino_dim = 3, 128                             # a 64-d list handed in as 128-d: malformed
    assert lib.nrf_debug_pack_input_grad_v3(C.byref(arch), arr, n, 0, None, 0, None) == -1
    # the V1 / V2 packer still refuses V3: the new plan sits beside it, not in its place
    arch.dino_dim = 64
    assert lib.nrf_debug_pack_input_grad(C.byref(arch), arr, n, 0, None, 0, None) == -1


# ---- the closed form of the fetch adjoint (nerfhip.h: nrf_project_fetch_backward_points), restated in numpy -------------------------
def fetch_adjoint_numpy(fmap, pose, focal, H, W, pts, g):
    """d_points (n,3) and d_xy (n,2) of sum(feats * g) by the formulas of the header, in float64 on float32 inputs."""
    fm = np.asarray(fmap, np.float64)[0]
    Hp, Wp, Cc = fm.shape
    inv = np.linalg.inv(np.asarray(pose, np.float64))
    p = np.asarray(pts, np.float64)
    pc = p @ inv[:3, :3].T + inv[:3, 3]
    zi = pc[:, 2] + 1e-8
    xn = (pc[:, 0] / zi * focal + W / 2) / W * 2 - 1
    yn = (pc[:, 1] / zi * focal + H / 2) / H * 2 - 1
    gx, gy = ((xn + 1) * Wp - 1) / 2, ((yn + 1) * Hp - 1) / 2
    x0, y0 = np.floor(gx), np.floor(gy)
    tx, ty = gx - x0, gy - y0

    def tap(a, b):
        xi, yi = x0 + a, y0 + b
        ok = (xi >= 0) & (xi <= Wp - 1) & (yi >= 0) & (yi <= Hp - 1)
        rows = fm[np.clip(yi, 0, Hp - 1).astype(int), np.clip(xi, 0, Wp - 1).astype(int)]
        return np.where(ok[:, None], rows, 0.0)
    m00, m10, m01, m11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
    gg = np.asarray(g, np.float64)
    Gx = (gg * ((1 - ty)[:, None] * (m10 - m00) + ty[:, None] * (m11 - m01))).sum(1)
    Gy = (gg * ((1 - tx)[:, None] * (m01 - m00) + tx[:, None] * (m11 - m10))).sum(1)
    dxn, dyn = Gx * Wp / 2, Gy * Hp / 2
    dpc = np.stack([dxn * 2 * focal / (W * zi), dyn * 2 * focal / (H * zi),
                    -(dxn * 2 * focal * pc[:, 0] / W + dyn * 2 * focal * pc[:, 1] / H) / zi ** 2], 1)
    return dpc @ inv[:3, :3], np.stack([dxn, dyn], 1), np.stack([gx, gy], 1)


@pytest.mark.parametrize("view", ["orbit", "near"])
@pytest.mark.parametrize("shape", [(9, 9, 64), (14, 22, 64), (10, 12, 128)])
def test_closed_form_of_the_fetch_adjoint_agrees_with_autograd(golden, view, shape):
    """400 rays x 8 jittered samples of the rendered camera projected into another view, random maps: the formulas the header
    states against fp32 autograd through the oracle's projection and tap-by-tap fetch, within 1e-5 of the largest element over the
    samples more than 1e-3 texel from a texel edge (the fetch has a kink there).  Keeps the GPU tests' reference honest."""
    g = golden("dino_views")
    pose, focal, Hs, Ws = g[view + "_pose"], float(g[view + "_focal"]), int(g[view + "_H"]), int(g[view + "_W"])
    Hp, Wp, Cc = shape
    n = 400 * 8
    ro, rd = O.get_rays(20, 20, O.focal_for(20), torch.from_numpy(O.LEGO_LIKE_C2W.copy()))
    tr = torch.from_numpy(O.uniform01(401, n).reshape(400, 8)).float()
    pts, _ = O.sample_points_along_rays(ro.reshape(-1, 3), rd.reshape(-1, 3), 2.0, 6.0, 8, t_rand=tr)
    pts = pts.reshape(-1, 3).clone().requires_grad_(True)
    fmap = torch.from_numpy(O.uniform01(405, Hp * Wp * Cc).reshape(1, Hp, Wp, Cc) * 2 - 1).float()
    gf = torch.from_numpy(O.uniform01(406, n * Cc).reshape(n, Cc) - 0.5).float()
    xy = O.project_points_to_image(pts, torch.from_numpy(pose), focal, Hs, Ws)[0]
    xy.retain_grad()
    (O.sample_features_at_points(fmap, xy) * gf).sum().backward()
    d_pts, d_xy, gxy = fetch_adjoint_numpy(fmap.numpy(), pose, focal, Hs, Ws, pts.detach().numpy(), gf.numpy())
    frac = gxy - np.floor(gxy)
    keep = (np.minimum(frac, 1 - frac).min(1) > 1e-3)
    assert keep.mean() > 0.9, keep.mean()
    ref_p, ref_xy = pts.grad.numpy()[keep], xy.grad.numpy()[keep]
    assert np.abs(ref_p).max() > 0
    e_p = np.abs(d_pts[keep] - ref_p).max() / np.abs(ref_p).max()
    e_xy = np.abs(d_xy[keep] - ref_xy).max() / np.abs(ref_xy).max()
    print(f"closed form vs autograd ({view}, {shape}): d_points {e_p:.2e}, d_xy {e_xy:.2e} of the largest element; kept {keep.mean():.3f}")
    assert e_p < 1e-5 and e_xy < 1e-5, (e_p, e_xy)


def test_point_grad_fixture_is_consistent(golden):
    """point_grads.npz: the stored d_points_feat is the closed form applied to the stored d_feats, the rays' gradients are the
    adjoint of points = o + z d applied to the stored d_points (plus, for d and z, the compositor's own terms, hence only o here),
    and the feature path is far smaller than the whole -- which is why it is stored, and tested, on its own."""
    g = golden("point_grads")
    R, S = g["z"].shape
    pts = (g["rays_o"][:, None, :] + g["rays_d"][:, None, :] * g["z"][:, :, None]).reshape(-1, 3).astype(np.float32)
    d_pts, _, gxy = fetch_adjoint_numpy(g["fmap"], g["pose"], float(g["focal"]), int(g["H"]), int(g["W"]), pts, g["d_feats"])
    frac = gxy - np.floor(gxy)
    assert np.minimum(frac, 1 - frac).min() > 1e-3                # the rays were chosen clean
    scale = np.abs(g["d_points_feat"]).max()
    assert np.abs(d_pts - g["d_points_feat"]).max() < 1e-4 * scale
    assert np.allclose(g["d_points"].reshape(R, S, 3).sum(1), g["d_rays_o"], rtol=0, atol=2e-5 * np.abs(g["d_rays_o"]).max())
    assert 100 < np.abs(g["d_points"]).max() / scale < 3000
    assert g["d_points"].shape == (R * S, 3) and g["d_feats"].shape == (R * S, 64)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "point_grads.npz")) < 300 * 1024


def test_constructor_switches():
    """point_grad is the use_dino form's switch, input_grad the other forms': each refuses the other's place and says where to go."""
    import nerf_few_shot_limitations_amd as N
    m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64, point_grad=True)
    assert m.point_grad and not m.input_grad
    assert not N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64).point_grad
    with pytest.raises(ValueError, match="projection and the bilinear fetch"):
        N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64, input_grad=True)
    with pytest.raises(ValueError, match="point_grad"):
        N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64, input_grad=True)
    with pytest.raises(ValueError, match="input_grad"):
        N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=2, point_grad=True)
    with pytest.raises(ValueError, match="input_grad"):
        N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2, point_grad=True)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_v3_input_grad_plan_is_clean_under_asan_ubsan(tmp_path):
    """tests/host/point_grad_pack_sanitize.cpp: the new plan at trunk depths 1 / 2 / 5 / 8 and both feature widths, packed alone and
    behind the chain's layers in the three training modes, its source tables, and three refusals."""
    exe = str(tmp_path / "point_grad_pack_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D__host__=", "-D__device__=", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
           os.path.join(ROOT, "tests", "host", "point_grad_pack_sanitize.cpp"), os.path.join(ROOT, "nerf_few_shot_limitations_amd", "csrc", "packing.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr + b.stdout).lower() and "cannot find" in (b.stderr + b.stdout).lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "sanitize ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" ok:") == 8
