"""The hierarchical render that evaluates only the new samples in its fine pass (run with -m gpu).

A sample's network output depends on its ray and its depth alone, and the fine pass' sorted union holds the coarse depths bit for
bit, so the three-call route -- coarse render_rays, sample_pdf, render_rays on the union through z_in -- is a bit-for-bit oracle of
the reusing one.  Every comparison here is torch.equal; nothing in the feature needs a tolerance.

  1. emit equals plain     the emitting render's rgb, depth, weights, z_vals are render_rays' bits (ragged and tiny ray counts,
                           S = 2, 12, 70, ladder / lindisp / seeded jitter / explicit depths, every pinned split and the free deal)
  2. the compositor alone  nrf_composite_merge without new samples on the emitted rows reproduces that render (with and without a
                           white background): "same compositor", apart from "same merge"
  3. the route             render_hierarchical(reuse_coarse=True) == render_hierarchical() on every entry, ties at both ends of the
                           depth range included
  4. the camera route      render_camera_hierarchical does not depend on the cut into ray ranges and equals route 3 on get_rays
  5. evaluation            evaluate_views(N_importance=...) is the per-view camera route; N_importance = 0 is the existing path
  6. refusals              what the reusing route does not take raises ValueError
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import render_probe as P
from tests.test_gpu_render_link import make_model

pytestmark = pytest.mark.gpu

NETS = ["v1", "v2", "v3"]                    # v3: dino_dim 64, conditioned on the 'orbit' view (part of the samples project off its map)
MODES = ["f32", "f16x3", "f16", "bf16"]
KEYS = ("rgb", "depth", "weights", "z_vals")
R_RAGGED = 333                               # no multiple of 4 (the deal's unit), 64 or 256


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def g(golden):
    return golden("dino_views")


_models = {}


def model_of(N, net, mode):
    if (net, mode) not in _models:
        _models[(net, mode)] = make_model(N, net, mode)
    return _models[(net, mode)]


def source_of(g, net):
    src = P.source_view(g, net)
    return None if src is None else dict(src, features=src["features"].cuda().contiguous())


def rays(n):
    ro, rd = P.frame_rays()
    return ro[:n].cuda().contiguous(), rd[:n].cuda().contiguous()


def same(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def spw(monkeypatch, pin):
    if pin is None:
        monkeypatch.delenv("NRF_SPW", raising=False)
    else:
        monkeypatch.setenv("NRF_SPW", str(pin))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("net", NETS)
def test_emit_equals_plain_and_the_compositor_alone(N, g, net, mode, monkeypatch):
    """Cases 1 and 2 on the same emitted rows."""
    m, src = model_of(N, net, mode), source_of(g, net)
    for R in (R_RAGGED, 3):
        ro, rd = rays(R)
        for S in (2, 12, 70):
            samplings = {"ladder": {}, "lindisp": dict(lindisp=True), "jitter": dict(perturb=True, seed=5),
                         "z_in": dict(z_in=P.random_depths(R, S).cuda())}
            for name, kw in samplings.items():
                for pin in (None, 0, 3, 6):
                    spw(monkeypatch, pin)
                    what = (R, S, name, pin)
                    plain = N.render_rays(m, ro, rd, P.NEAR, P.FAR, S, return_z=True, dino=src, **kw)
                    emit = N.render_rays_emit(m, ro, rd, P.NEAR, P.FAR, S, dino=src, **kw)
                    same(emit, plain, KEYS, what)
                    assert emit["raw4"].shape == (R, S, 4) and torch.isfinite(emit["raw4"]).all(), what
                    if pin is None:
                        first = emit
                    else:                                    # the rows do not depend on the split either
                        assert torch.equal(emit["raw4"], first["raw4"]), what
                spw(monkeypatch, None)
                # case 2: the compositor alone, on the free deal's rows
                for white in (False, True):
                    ref = plain if not white else N.render_rays(m, ro, rd, P.NEAR, P.FAR, S, return_z=True, dino=src, white_bkgd=True, **kw)
                    alone = N.composite_merge(first["z_vals"], first["raw4"], rd, mma_mode=mode, white_bkgd=white)
                    same(alone, ref, KEYS, (R, S, name, "merge alone", white))
    # raw_only: nothing but the rows, and the same rows
    only = N.render_rays_emit(m, ro, rd, P.NEAR, P.FAR, 70, dino=src, raw_only=True, **samplings["z_in"])
    assert set(only) == {"raw4"} and torch.equal(only["raw4"], first["raw4"])


def repeated_u(R, Ni):
    """Inverse-cdf arguments with repeated values inside a row (equal new samples) and the two end points."""
    u = torch.from_numpy(O.uniform01(91 + Ni, R * Ni).reshape(R, Ni)).float()
    u = (u * 4).floor() / 4                                  # 0, .25, .5, .75: repeats in every row with Ni > 4
    u[:, 0] = 0.0
    u[: R // 2, -1] = 1.0
    return u.cuda().contiguous()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("net", NETS)
def test_reusing_route_equals_the_three_call_route(N, g, net, mode, monkeypatch):
    """Case 3."""
    m, src = model_of(N, net, mode), source_of(g, net)
    ro, rd = rays(R_RAGGED)
    for S, Ni in ((2, 1), (12, 5), (32, 16), (70, 70)):
        variants = [("default u", {}, None), ("repeated u", dict(u=repeated_u(R_RAGGED, Ni)), None), ("jitter", dict(perturb=True, seed=5), None),
                    ("lindisp", dict(lindisp=True), None), ("white", dict(white_bkgd=True), None), ("spw 0", {}, 0), ("spw 3", {}, 3)]
        for name, kw, pin in variants:
            spw(monkeypatch, pin)
            torch.manual_seed(17)                            # perturb without u: both routes draw the same u
            old = N.render_hierarchical(m, ro, rd, P.NEAR, P.FAR, S, Ni, dino=src, **kw)
            torch.manual_seed(17)
            new = N.render_hierarchical(m, ro, rd, P.NEAR, P.FAR, S, Ni, dino=src, reuse_coarse=True, **kw)
            what = (S, Ni, name)
            same(new, old, KEYS, what)
            same(new["coarse"], old["coarse"], KEYS, what + ("coarse",))
            assert set(new) == set(old) and set(new["coarse"]) == set(old["coarse"]), what
            assert new["z_vals"].shape == (R_RAGGED, S + Ni) and torch.all(new["z_vals"][:, 1:] >= new["z_vals"][:, :-1]), what
            if name == "default u":
                # u = 0 gives a new sample equal to the first coarse depth (the coarse one goes first), u = 1 one equal to the last --
                # which then is the ray's final, 1e10 sample: both ties are in the data
                zc = old["coarse"]["z_vals"]
                smp = N.sample_pdf(zc, old["coarse"]["weights"], Ni)[0]
                assert torch.equal(smp[:, 0], zc[:, 0]), what
                if Ni > 1:
                    assert bool((smp[:, -1] == zc[:, -1]).any()), what
                    tied = smp[:, -1] == zc[:, -1]
                    assert torch.equal(new["z_vals"][tied, -1], zc[tied, -1]) and torch.equal(new["z_vals"][tied, -2], zc[tied, -1]), what
    spw(monkeypatch, None)


def camera():
    return P.T(O.LEGO_LIKE_C2W), O.focal_for(P.W)


@pytest.mark.parametrize("net,mode", [("v1", "f16"), ("v1", "f16x3"), ("v2", "bf16"), ("v2", "f32"), ("v3", "f16"), ("v3", "f16x3")])
def test_camera_route(N, g, net, mode):
    """Case 4 on the 19 x 31 frame."""
    m, src = model_of(N, net, mode), source_of(g, net)
    c2w, focal = camera()
    H, W, S, Ni = P.H, P.W, 12, 5
    whole = N.render_camera_hierarchical(m, H, W, focal, c2w, P.NEAR, P.FAR, S, Ni, chunk_rays=H * W, dino=src)
    assert whole[0].shape == (H * W, 3) and whole[1].shape == (H * W,)
    for chunk in (64, 200):
        cut = N.render_camera_hierarchical(m, H, W, focal, c2w, P.NEAR, P.FAR, S, Ni, chunk_rays=chunk, dino=src)
        assert torch.equal(cut[0], whole[0]) and torch.equal(cut[1], whole[1]), chunk
    ro, rd = N.get_rays(H, W, focal, c2w)
    route = N.render_hierarchical(m, ro.reshape(-1, 3), rd.reshape(-1, 3), P.NEAR, P.FAR, S, Ni, dino=src, reuse_coarse=True)
    assert torch.equal(whole[0], route["rgb"]) and torch.equal(whole[1], route["depth"])
    three = N.render_hierarchical(m, ro.reshape(-1, 3), rd.reshape(-1, 3), P.NEAR, P.FAR, S, Ni, dino=src)
    assert torch.equal(whole[0], three["rgb"]) and torch.equal(whole[1], three["depth"])
    # a sub-range, into the caller's buffers, with a white background and disparity sampling
    b, e = 77, 401
    kw = dict(white_bkgd=True, lindisp=True, dino=src)
    full = N.render_camera_hierarchical(m, H, W, focal, c2w, P.NEAR, P.FAR, S, Ni, **kw)
    out_rgb, out_depth = torch.zeros((e - b, 3), device="cuda"), torch.zeros((e - b,), device="cuda")
    sub = N.render_camera_hierarchical(m, H, W, focal, c2w, P.NEAR, P.FAR, S, Ni, ray_begin=b, ray_end=e, chunk_rays=100, out_rgb=out_rgb,
                                       out_depth=out_depth, **kw)
    assert sub[0] is out_rgb and sub[1] is out_depth
    assert torch.equal(out_rgb, full[0][b:e]) and torch.equal(out_depth, full[1][b:e])
    # seeded coarse jitter is keyed by the global ray id: two cuts, one image -- and not the un-jittered one
    j1 = N.render_camera_hierarchical(m, H, W, focal, c2w, P.NEAR, P.FAR, S, Ni, chunk_rays=64, perturb=True, seed=5, dino=src)
    j2 = N.render_camera_hierarchical(m, H, W, focal, c2w, P.NEAR, P.FAR, S, Ni, chunk_rays=333, perturb=True, seed=5, dino=src)
    assert torch.equal(j1[0], j2[0]) and torch.equal(j1[1], j2[1])
    assert not torch.equal(j1[0], whole[0])


def test_evaluate_views_with_importance_samples(N):
    """Case 5."""
    m = model_of(N, "v1", "f16")
    H, W, S, Ni = 24, 20, 12, 16
    focal = O.focal_for(W)
    c2w = np.asarray(O.LEGO_LIKE_C2W, np.float32)
    c2w2 = c2w.copy()
    c2w2[:3, 3] = c2w2[:3, 3] * 0.9 + np.float32([0.2, -0.1, 0.15])
    poses = torch.from_numpy(np.stack([c2w, c2w2]))
    from nerf_few_shot_limitations_amd import evaluate_views
    res = evaluate_views(m, poses, H, W, focal, P.NEAR, P.FAR, S, N_importance=Ni, hier_chunk_rays=128, white_bkgd=True, targets=torch.zeros(2, H, W, 3))
    assert res["images"].shape == (2, H, W, 3) and res["depth"].shape == (2, H, W) and len(res["per_view"]) == 2
    for v in range(2):
        rgb, depth = N.render_camera_hierarchical(m, H, W, focal, poses[v], P.NEAR, P.FAR, S, Ni, white_bkgd=True)
        assert torch.equal(res["images"][v].reshape(-1, 3), rgb) and torch.equal(res["depth"][v].reshape(-1), depth), v
    assert not torch.equal(res["images"][0], res["images"][1])
    plain0 = evaluate_views(m, poses, H, W, focal, P.NEAR, P.FAR, S, N_importance=0)
    today = evaluate_views(m, poses, H, W, focal, P.NEAR, P.FAR, S)
    assert torch.equal(plain0["images"], today["images"]) and torch.equal(plain0["depth"], today["depth"])
    for v in range(2):
        rgb, depth = N.render_camera(m, H, W, focal, poses[v], P.NEAR, P.FAR, S)
        assert torch.equal(plain0["images"][v].reshape(-1, 3), rgb) and torch.equal(plain0["depth"][v].reshape(-1), depth), v
    with pytest.raises(ValueError):
        evaluate_views(m, poses, H, W, focal, P.NEAR, P.FAR, S, N_importance=Ni, ert_eps=1e-3)


def test_refusals(N):
    """Case 6: there is no silent fallback to the three-call route."""
    from nerf_few_shot_limitations_amd import OccupancyGrid, _lib as L
    m = model_of(N, "v1", "f16")
    ro, rd = rays(64)
    args = (m, ro, rd, P.NEAR, P.FAR, 12, 5)
    grid = OccupancyGrid.from_model(m, -P.FAR, P.FAR, resolution=32)
    for kw in (dict(tail_mode="f16x3"), dict(occupancy=grid), dict(return_stats=True), dict(ert_eps=1e-3)):
        with pytest.raises(ValueError):
            N.render_hierarchical(*args, reuse_coarse=True, **kw)
    N.render_hierarchical(*args, reuse_coarse=True, ert_eps=0.0)          # the values that mean "off" pass
    mt = make_model(N, "v1", "f16").train()
    with torch.enable_grad():
        with pytest.raises(ValueError):
            N.render_hierarchical(mt, ro, rd, P.NEAR, P.FAR, 12, 5, reuse_coarse=True)
    with torch.no_grad():                                                 # the same module under no_grad renders
        N.render_hierarchical(mt, ro, rd, P.NEAR, P.FAR, 12, 5, reuse_coarse=True)
    # the C entry refuses early termination with a message
    import ctypes as C
    from nerf_few_shot_limitations_amd.renderer import _opts
    opts = _opts(P.NEAR, P.FAR, 12, False, None, 0, False, 1e-3, False, "f16", None, ro.device)
    raw = torch.empty((64, 12, 4), device="cuda")
    rgb, depth = torch.empty((64, 3), device="cuda"), torch.empty((64,), device="cuda")
    rc = L.lib().nrf_render_rays_emit(m.handle(ro.device, "f16"), L.ptr(ro), L.ptr(rd), 64, C.byref(opts), L.ptr(rgb), L.ptr(depth), None, None,
                                      L.ptr(raw), 0, L.stream_ptr())
    assert rc == -1 and b"ert_eps" in L.lib().nrf_last_error()
