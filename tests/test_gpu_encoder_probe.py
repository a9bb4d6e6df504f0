"""The in-kernel positional encoders, feature by feature, in all four modes (run with -m gpu on an MI355X).

encode3 (csrc/nets.hpp) is read out through the selector networks of tests/encoder_probe.py -- exact wires from ONE encoder feature
to an output -- on that file's 1531 probe points (|x| <= 8, the zeros of sin and cos at every frequency, the rint / fract seams),
and every feature (the raw x, y, z rows included) of every point is held to the float64 encoding under the mode's bound; the
bounds, their derivations and the wires are in encoder_probe.py's docstring, the CPU half is tests/test_encoder_probe_host.py.

  V2 (L = 10), V3 (L = 12, dino_dim 64, random DINO input)   position features through nrf_mlp_forward (NeRFMLP(...)(positions,
                      directions, dino) under no_grad): 63 / 75 features, two forwards each (relu(e), relu(-e)).
  the training forward   the same observations through nrf_mlp_forward_train where the mode has one (f32, f16, bf16): torch.equal
                      to the inference forward, which pins the other kernel family's encoder.
  two launches        the V2 points cut at row 777 (ragged against 32 and 64): the bits are unchanged -- an encoder must not
                      depend on the lane's tile.
  directions (L = 4)  of V2, through color_layers and the sigmoid: 27 features, three per forward.
  V1 (L = 10)         through one-sample renders of the rays (0, p, 1) on the tile kernel (ert_eps = 0) and on the ray-queue kernel
                      (ert_eps = 1e-30): every weight is exactly 1, 63 features, three per render.

Every case prints a RECORD line: the worst |a - e| / bound, its feature and its input.

RECORD (MI355X, gfx950; measurements, not bounds; 26 tests in 3.6 s, the slowest 0.14 s).  Worst |a - e| / bound over every feature and point:
                      f32 (path 0: ocml)   f16x3 (path 2: polynomial)   f16 (path 1: v_sin)   bf16 (path 1: v_sin)
  V2 positions        0.241  cos f=5       0.713  sin f=6               0.985  cos f=5        0.842  cos f=7
  V3 positions        0.241  cos f=5       0.544  sin f=4               0.985  cos f=5        0.842  cos f=7
  V2 directions       0.272  cos f=0       0.250  cos f=2               0.982  sin f=1        0.019  (wiring only)
  V1, tile = queue    0.266  cos f=9       0.284  sin f=4               0.977  cos f=5        0.070  (wiring only)
  f16x3's worst V2 point, (7.314, ., .) at sin f = 6, is the worst point of the CPU model of the polynomial path (1.83e-7 there,
  tests/test_encoder_probe_host.py); the 16-bit figures and their points are those of that model rounded to the operand type: at
  most one flipped last bit of the operand type at |x| <= 8, every frequency.  The training forward and the two-launch split are
  bit-equal to the staged forward in every mode, the tile render to the ray-queue render.

HAND CHECK (once, on a scratch copy of the library with `+ p[c] * kInv2PiLo` taken out of nets.hpp: encode3; MI355X).  Of this file,
7 of 26 cases fail: V2 and V3 positions in f16x3 (from cos f = 0 upwards, 1.4 .. 2.5 of the bound at the low bands) and in f16 (from
f = 8, 1.9 of the bound there), V3 positions in bf16 (f = 11 only, 1.5 .. 1.6), V1 in f16x3 and f16 (both kernels); the f32 cases,
the directions (|x| <= 1) and the bit-equality cases pass, as they must.  The suite as it was is NOT blind to this fault everywhere:
with the same library 10 cases of tests/test_gpu_parity.py fail, every one of them in f16x3 (its 1.2e-5 .. 1e-4 bars on 'solid'
weights, 5e-5 .. 3.8e-4 seen), and the 8 f16 V3 cases of tests/test_gpu_train_stages.py (input.0 at 2.9 .. 3.0 of the encoder-stage
rule: L = 12 reaches f = 11 even at |x| <= 2).  What it did not see: f16 at L = 10 (V2, V1), bf16 anywhere, and in no case which
feature is wrong; both files pass with the library as it is.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import encoder_probe as E
from tests import render_probe as P

pytestmark = pytest.mark.gpu

CUT = 777                                       # ragged against 32 and 64, and not where the probe's special points end
TRAIN_MODES = ("f32", "f16", "bf16")


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def make_model(N, fam, mode):
    if fam == "v1":
        m, p = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2, mma_mode=mode), E.v1_selector()
    else:
        m = N.NeRFMLP(pos_freq=12 if fam == "v3" else 10, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=fam == "v3",
                      dino_dim=64 if fam == "v3" else 0, mma_mode=mode)
        p = E.v3_selector() if fam == "v3" else E.v2_selector()
    m.load_state_dict(p, strict=False)
    return m.cuda().eval()


def set_param(model, name, value):
    """In place, so that the parameter's version moves and the next call re-packs the streams."""
    with torch.no_grad():
        model.get_parameter(name).copy_(value.to("cuda"))


def inputs(fam):
    pts, dirs = torch.from_numpy(E.probe_points()).cuda(), torch.from_numpy(E.probe_dirs()).cuda()
    dino = None
    if fam == "v3":
        from oracle import nerf_oracle as O
        dino = (torch.from_numpy(O.uniform01(9, E.N_POINTS * 64).reshape(-1, 64)) * 2 - 1).cuda().contiguous()
    return pts, dirs, dino


def forward_train(model, pos, dirs, dino):
    """nrf_mlp_forward_train through the C ABI -> (rgb, density)."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = pos.device
    h, mode = _train_handle(model, dev)
    n = pos.shape[0]
    rgb, den = torch.empty((n, 3), device=dev), torch.empty((n, 1), device=dev)
    nbytes = L.lib().nrf_train_context_bytes(h, mode, n)
    assert nbytes > 0
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    L.check(L.lib().nrf_mlp_forward_train(h, mode, L.ptr(pos), L.ptr(dirs), L.ptr(dino), n, L.ptr(rgb), L.ptr(den), C.c_void_p(buf.data_ptr()),
                                          nbytes, L.stream_ptr()))
    torch.cuda.synchronize()
    return rgb, den


def position_densities(N, fam, mode):
    """{route: (F, 2, n) fp32 densities d+ / d- of every position feature}, routes 'eval', 'train' (where the mode trains) and,
    for V2, 'split' (two launches): one walk over the head rows."""
    model = make_model(N, fam, mode)
    pts, dirs, dino = inputs(fam)
    F = E.n_features(12 if fam == "v3" else 10)
    routes = ["eval"] + (["split"] if fam == "v2" else []) + (["train"] if mode in TRAIN_MODES else [])
    out = {r: torch.empty((F, 2, E.N_POINTS)) for r in routes}
    cut = lambda t, a, b: None if t is None else t[a:b].contiguous()
    for k in range(F):
        for s, sign in enumerate((1.0, -1.0)):
            set_param(model, "density_mlp.density_head.weight", E.density_row(k, sign))
            with torch.no_grad():
                out["eval"][k, s] = model(pts, dirs, dino)[1][:, 0].cpu()
                if "split" in out:
                    parts = [model(cut(pts, a, b), cut(dirs, a, b), cut(dino, a, b))[1][:, 0] for a, b in ((0, CUT), (CUT, E.N_POINTS))]
                    out["split"][k, s] = torch.cat(parts).cpu()
            if "train" in out:
                out["train"][k, s] = forward_train(model, pts, dirs, dino)[1][:, 0].cpu()
    return out


@pytest.fixture(scope="module")
def walk(N, request):
    """(family, mode, position_densities of them): one walk per (family, mode), shared by the tests that ask for the same pair."""
    fam, mode = request.param
    return fam, mode, position_densities(N, fam, mode)


def walks(fams, modes):
    return pytest.mark.parametrize("walk", [(fam, mode) for mode in modes for fam in fams], indirect=True, ids=lambda c: f"{c[1]}-{c[0]}")


def check(what, observed, points, L, mode, wire, sigmoid=False):
    findings = E.compare(observed, points, L, lambda e: E.bound(e, mode, wire, sigmoid), lambda e: E.target(e, mode))
    print("\n" + E.record(f"{what} {mode} (encoder path {E.TRIG[mode]})", findings))
    assert len(findings) == E.n_features(L)
    assert not E.failed(findings), E.failed(findings)


@walks(("v2", "v3"), E.MODES)
def test_position_features_through_the_staged_forward(walk):
    fam, mode, d = walk
    d = d["eval"]
    assert bool(((d[:, 0] == 0) | (d[:, 1] == 0)).all()) and bool((d >= 0).all()), "relu(e) and relu(-e) are never both open"
    e = (d[:, 0].double() - d[:, 1].double()).numpy().T
    check(f"{fam} positions", e, E.probe_points(), 12 if fam == "v3" else 10, mode, fam)


@walks(("v2", "v3"), TRAIN_MODES)
def test_training_forward_encodes_the_same_bits(walk):
    _, _, d = walk
    assert torch.equal(d["train"], d["eval"])


@walks(("v2",), E.MODES)
def test_two_launches_encode_the_same_bits(walk):
    _, _, d = walk
    assert torch.equal(d["split"], d["eval"])


@pytest.mark.parametrize("mode", E.MODES)
def test_direction_features(N, mode):
    model = make_model(N, "v2", mode)
    pts, dirs, _ = inputs("v2")
    cols = []
    for t in range(E.n_features(4) // 3):
        set_param(model, "color_mlp.color_layers.4.weight", E.colour_rows(t))
        with torch.no_grad():
            rgb, den = model(pts, dirs)
        assert bool((den == 0).all())
        cols.append(rgb.cpu())
    e = E.logit64(torch.cat(cols, 1).numpy())
    check("v2 directions", e, E.probe_dirs(), 4, mode, "dir", sigmoid=True)


@pytest.mark.parametrize("mode", E.MODES)
def test_v1_features_through_one_sample_renders(N, mode):
    model = make_model(N, "v1", mode)
    pts = E.probe_points()
    rd = torch.from_numpy(pts).cuda()
    ro, z = torch.zeros_like(rd), torch.ones((E.N_POINTS, 1), device="cuda")
    at = P.points32(ro, rd, z)[:, 0].numpy()
    assert np.array_equal(at, pts), "the rays (0, p, 1) reach the probe points themselves"
    seen = {}
    for route, eps in (("tile", 0.0), ("queue", 1e-30)):
        cols = []
        for t in range(E.n_features(10) // 3):
            set_param(model, "rgb_out.weight", E.v1_rgb_rows(t))
            out = N.render_rays(model, ro, rd, 0.5, 2.0, 1, z_in=z, white_bkgd=False, return_z=True, ert_eps=eps)
            assert torch.equal(out["z_vals"], z) and bool((out["weights"] == 1.0).all()), "alpha of the one-sample render is exactly 1"
            cols.append(out["rgb"].cpu())
        seen[route] = torch.cat(cols, 1)
        e = E.logit64(seen[route].numpy())
        e[:, :3] *= E.RAW_GAIN
        check(f"v1 {route} kernel", e, at, 10, mode, "v1", sigmoid=True)
    assert torch.equal(seen["tile"], seen["queue"])
