"""Tail mode (include/nerfhip.h: nrf_tail): a bf16 / f16 render whose LAST sample per ray -- the one the reference composites
with dists[-1] = 1e10, whose opacity is a step function of its density -- is evaluated in split-f16.  Every call goes through
the C ABI.  Definition under test:
  1. weights[:, :S-1] and z_vals are the plain 16-bit render's bits;
  2. sample S-1 is the split-f16 renderer's: with N_samples = 1 the whole render is bit-equal to mma_mode="f16x3";
  3. a ray's result does not depend on the work split, the batch cut, tiles or view batching.
The error bounds are the ones tests/test_gpu_parity.py::test_render_vs_oracle_100x100x32 holds on the "stable" rays (2x the
measured error, profiles/r02_mode_error_report.txt), asked here of EVERY ray.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

BASES = ["f16", "bf16"]


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def dino_map(dd=64):
    return torch.from_numpy(O.uniform01(7, 28 * 28 * dd).reshape(1, 28, 28, dd) * 2 - 1)


def make(N, net, mode, scene="solid"):
    """(model, oracle parameters, extra render keywords) of one of the four built families."""
    kw = {}
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
        p = O.make_weights("v1", 0, scene)
        m.load_state_dict(p)
    elif net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=mode)
        p = O.make_weights("v2", 1, scene)
        m.load_state_dict(p, strict=False)
    else:
        dd = 128 if net == "v3w" else 64
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=dd, mma_mode=mode)
        p = O.make_weights("v3", 2, scene) if dd == 64 else O.make_weights("v3", 3, scene, dino_dim=128)
        m.load_state_dict(p, strict=False)
        kw["dino"] = dict(features=dino_map(dd), pose=T(O.LEGO_LIKE_C2W), focal=O.focal_for(31), H=19, W=31)
    return m.cuda().eval(), p, kw


def rays(N, H, W):
    ro, rd = N.get_rays(H, W, O.focal_for(W), T(O.LEGO_LIKE_C2W))
    return ro.reshape(-1, 3), rd.reshape(-1, 3)


# ------------------------------------------------------------------ check 1: the flips are gone
def test_last_sample_flips_are_gone_100x100x32(N):
    """V1 "solid", 100 x 100 x 32 -- the frame of test_render_vs_oracle_100x100x32 -- against the oracle on ALL 10 000 rays.
    Bounds: f16 + tail rgb 1.2e-2 / depth 7e-2, bf16 + tail 9e-2 / 5.5e-1 (tests/test_gpu_parity.py:440-441: 2x the error measured
    on the stable rays); weights[:, S-1] within the rgb bound.  The frame bites: the PLAIN mode of the same call exceeds the rgb
    bound on at least one ray.  Should plain f16 not flip on this frame on the GPU, its "bites" assertion moves to the "fog" scene
    with the rays of oracle |sigma_last| < 1e-3 (at most 1 %) excluded."""
    H = W = 100; S = 32
    c2w = T(O.LEGO_LIKE_C2W)
    m, p, _ = make(N, "v1", "f16")
    ro, rd = O.get_rays(H, W, O.focal_for(W), c2w)
    ref = O.render_rays(p, "v1", ro, rd, 2.0, 6.0, S)
    sig_last = O.mlp_v1(p, O.positional_encoding(ro.reshape(-1, 3) + rd.reshape(-1, 3) * 6.0, 10))[:, 3]
    assert float(sig_last.abs().min()) > 1e-3                          # no ray of this frame sits on the step: nothing is excluded
    gro, grd = rays(N, H, W)
    f16_bites = None
    for mode, tol, dtol in (("f16", 1.2e-2, 7e-2), ("bf16", 9e-2, 5.5e-1)):
        rgb, depth = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, mma_mode=mode, tail_mode="f16x3")
        err = float((rgb.cpu() - ref["rgb"]).abs().max())
        derr = float((depth.cpu() - ref["depth"]).abs().max())
        out = N.render_rays(m, gro, grd, 2.0, 6.0, S, mma_mode=mode, tail_mode="f16x3")
        werr = float((out["weights"][:, S - 1].cpu() - ref["weights"][:, S - 1]).abs().max())
        plain, _ = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, mma_mode=mode)
        perr = float((plain.cpu() - ref["rgb"]).abs().max())
        print(f"tail {mode}: all-ray max rgb {err:.3e} depth {derr:.3e} w_last {werr:.3e}; plain max rgb {perr:.3e}")
        assert err <= tol and derr <= dtol, (mode, err, derr)
        assert werr <= tol, (mode, werr)
        if mode == "bf16":
            assert perr > tol, (mode, perr)
        else:
            f16_bites = perr > tol
    if not f16_bites:
        mf, pf, _ = make(N, "v1", "f16", "fog")
        reff = O.render_rays(pf, "v1", ro, rd, 2.0, 6.0, S)
        sl = O.mlp_v1(pf, O.positional_encoding(ro.reshape(-1, 3) + rd.reshape(-1, 3) * 6.0, 10))[:, 3]
        keep = sl.abs() >= 1e-3
        assert float((~keep).float().mean()) <= 0.01
        plain, _ = N.render_camera(mf, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, mma_mode="f16")
        tailed, dt = N.render_camera(mf, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, mma_mode="f16", tail_mode="f16x3")
        perr = float((plain.cpu() - reff["rgb"]).abs().max(-1).values[keep].max())
        terr = float((tailed.cpu() - reff["rgb"]).abs().max(-1).values[keep].max())
        print(f"fog f16: plain max rgb {perr:.3e}, tail {terr:.3e} on {int(keep.sum())} rays")
        assert perr > 1.2e-2 and terr <= 1.2e-2, (perr, terr)


# ------------------------------------------------------------------ check 2: the prefix is the plain render's
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("net", ["v1", "v2", "v3", "v3w"])
def test_prefix_weights_and_depths_are_the_plain_modes_bits(N, net, base):
    m, _, kw = make(N, net, base)
    ro, rd = rays(N, 19, 31)                                              # 589 rays: ragged tiles
    S = 12
    R = ro.shape[0]
    zin = torch.sort(T(O.uniform01(21, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values
    for cfg in (dict(), dict(perturb=True, seed=5), dict(lindisp=True), dict(perturb=True, seed=9, lindisp=True), dict(z_in=zin)):
        plain = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, **cfg, **kw)
        tail = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, tail_mode="f16x3", **cfg, **kw)
        assert torch.equal(tail["z_vals"], plain["z_vals"]), (net, base, cfg.keys())
        assert torch.equal(tail["weights"][:, :S - 1], plain["weights"][:, :S - 1]), (net, base, cfg.keys())
        assert torch.isfinite(tail["rgb"]).all() and torch.isfinite(tail["depth"]).all()
        # the last sample is the split mode's, not the base mode's: its weight is T_{S-1} (shared) x alpha_last
        w_last, T_last = tail["weights"][:, S - 1], 1.0 - plain["weights"][:, :S - 1].sum(-1)
        assert float((w_last - T_last.clamp(min=0)).max()) <= 1e-4


# ------------------------------------------------------------------ check 3: the tail is the split-f16 render's
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("net", ["v1", "v2", "v3", "v3w"])
def test_one_sample_render_is_the_split_mode_render(N, net, base):
    m, _, kw = make(N, net, base)
    ro, rd = rays(N, 19, 31)
    for white in (False, True):
        for cfg in (dict(), dict(perturb=True, seed=3)):
            want = N.render_rays(m, ro, rd, 2.0, 6.0, 1, mma_mode="f16x3", white_bkgd=white, return_z=True, **cfg, **kw)
            got = N.render_rays(m, ro, rd, 2.0, 6.0, 1, mma_mode=base, tail_mode="f16x3", white_bkgd=white, return_z=True, **cfg, **kw)
            for k in ("rgb", "depth", "weights", "z_vals"):
                assert torch.equal(got[k], want[k]), (net, base, white, k)


# ------------------------------------------------------------------ check 4: independence of the work split
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("net", ["v1", "v3"])
def test_camera_route_batch_cuts_and_rgbd_rows(N, net, base):
    from nerf_few_shot_limitations_amd import tiles
    H, W, S = 19, 31, 12
    c2w = T(O.LEGO_LIKE_C2W)
    m, _, kw = make(N, net, base)
    ro, rd = rays(N, H, W)
    whole = N.render_rays(m, ro, rd, 2.0, 6.0, S, tail_mode="f16x3", **kw)
    rgb, depth = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, tail_mode="f16x3", **kw)
    assert torch.equal(rgb, whole["rgb"]) and torch.equal(depth, whole["depth"])
    for cuts in ((1,), (63, 64, 65), (127, 129, 300), (31, 333, 588)):
        edges = (0,) + cuts + (ro.shape[0],)
        parts = [N.render_rays(m, ro[a:b], rd[a:b], 2.0, 6.0, S, tail_mode="f16x3", **kw) for a, b in zip(edges[:-1], edges[1:])]
        for key in ("rgb", "depth", "weights"):
            assert torch.equal(torch.cat([q[key] for q in parts]), whole[key]), (net, base, cuts, key)
    job = tiles.TileJob(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, 0, 1, H * W, tail_mode="f16x3", **kw)      # out_rgbd rows
    job.launch()
    assert torch.equal(job.buf[0, :, :3], rgb) and torch.equal(job.buf[0, :, 3], depth)


@pytest.mark.parametrize("base", BASES)
def test_every_samples_per_pass_split_gives_the_same_bits(N, base, monkeypatch):
    """The approach of tests/test_gpu_parity.py::test_every_samples_per_pass_split_gives_the_same_bits: every pinned split of the
    prefix launch (env NRF_SPW, read per launch; the tail launch is one sample per ray whatever it says) reproduces SPW = 1."""
    c2w = T(O.LEGO_LIKE_C2W)
    m, _, _ = make(N, "v2", base)
    monkeypatch.setenv("NRF_SPW", "0")
    ref = N.render_camera(m, 100, 100, O.focal_for(100), c2w, 2.0, 6.0, 32, tail_mode="f16x3")
    ro, rd = rays(N, 37, 29)                                              # 1073 rays, 21 samples: ragged at every split
    ref2 = N.render_rays(m, ro, rd, 2.0, 6.0, 21, perturb=True, seed=5, return_z=True, tail_mode="f16x3")
    for l in range(1, 7):
        monkeypatch.setenv("NRF_SPW", str(l))
        got = N.render_camera(m, 100, 100, O.focal_for(100), c2w, 2.0, 6.0, 32, tail_mode="f16x3")
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), l
        got2 = N.render_rays(m, ro, rd, 2.0, 6.0, 21, perturb=True, seed=5, return_z=True, tail_mode="f16x3")
        for k in ("rgb", "depth", "weights", "z_vals"):
            assert torch.equal(got2[k], ref2[k]), (l, k)
    monkeypatch.delenv("NRF_SPW")
    auto = N.render_camera(m, 100, 100, O.focal_for(100), c2w, 2.0, 6.0, 32, tail_mode="f16x3")
    assert torch.equal(auto[0], ref[0]) and torch.equal(auto[1], ref[1])


@pytest.mark.parametrize("perturb", [False, True])
def test_round_robin_tiles_and_view_batches_reassemble_bitwise(N, perturb):
    """Two virtual ranks' round-robin tiles x three views (one launch per rank when the deal is even, one per view otherwise)
    reassemble to the frames of single render_camera calls, jitter keyed by the global view index included."""
    from nerf_few_shot_limitations_amd import tiles
    H, W, S = 50, 36, 8
    c2w = T(O.LEGO_LIKE_C2W)
    poses = torch.stack([c2w.clone() for _ in range(3)])
    poses[1, 0, 3] += 0.3; poses[2, 1, 3] -= 0.2
    m, _, _ = make(N, "v1", "bf16")
    seed = 77
    full = [N.render_camera(m, H, W, O.focal_for(W), poses[v], 2.0, 6.0, S, perturb=perturb, seed=(seed + v * 0x51ED27), tail_mode="f16x3")
            for v in range(3)]
    for world, tile_rays in ((2, 5 * W), (2, 4 * W)):                    # 10 tiles: even deal; 13 tiles: padding, per-view launches
        locals_ = [tiles.render_tiles(m, H, W, O.focal_for(W), poses, 2.0, 6.0, S, r, world, tile_rays, perturb=perturb, seed=seed,
                                      tail_mode="f16x3") for r in range(world)]
        g = torch.stack(locals_)
        for v in range(3):
            frame = tiles.reassemble(g[:, v], H * W, world, tile_rays)
            assert torch.equal(frame[:, :3], full[v][0]) and torch.equal(frame[:, 3], full[v][1]), (world, tile_rays, v)
    rgb, depth = tiles.render_frame_sharded(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, tile_rows=4, perturb=perturb, seed=seed,
                                            tail_mode="f16x3")
    assert torch.equal(rgb.reshape(-1, 3), full[0][0]) and torch.equal(depth.reshape(-1), full[0][1])


# ------------------------------------------------------------------ check 5: hierarchical
@pytest.mark.parametrize("base", BASES)
def test_hierarchical_render_runs_both_passes_with_the_tail(N, base):
    H, W, S, Ni = 24, 20, 32, 16
    m, p, _ = make(N, "v1", base)
    ro, rd = rays(N, H, W)
    out = N.render_hierarchical(m, ro, rd, 2.0, 6.0, S, Ni, tail_mode="f16x3")
    coarse_plain = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True)
    coarse_tail = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, tail_mode="f16x3")
    for k in ("rgb", "depth", "weights", "z_vals"):
        assert torch.equal(out["coarse"][k], coarse_tail[k]), k                 # the coarse pass took the tail ...
    assert torch.equal(out["coarse"]["weights"][:, :S - 1], coarse_plain["weights"][:, :S - 1])
    union = out["z_vals"]
    assert union.shape == (H * W, S + Ni)
    fine_plain = N.render_rays(m, ro, rd, 2.0, 6.0, S + Ni, z_in=union, return_z=True)
    fine_tail = N.render_rays(m, ro, rd, 2.0, 6.0, S + Ni, z_in=union, return_z=True, tail_mode="f16x3")
    for k in ("rgb", "depth", "weights"):
        assert torch.equal(out[k], fine_tail[k]), k                             # ... and so did the fine pass (through z_in)
    assert torch.equal(out["weights"][:, :S + Ni - 1], fine_plain["weights"][:, :S + Ni - 1])
    assert torch.equal(fine_tail["z_vals"], fine_plain["z_vals"])


# ------------------------------------------------------------------ check 6: refusals
def test_refusals_and_the_untouched_plain_route(N):
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts
    m, _, _ = make(N, "v1", "f16")
    ro, rd = rays(N, 8, 8)
    R, S = ro.shape[0], 8
    lib = L.lib()
    h = m.handle(ro.device, "f16", also="f16x3")
    need = lib.nrf_render_tail_bytes(R)
    assert need == (24 * R + 15) // 16 * 16 and lib.nrf_render_tail_bytes(0) == 0 and lib.nrf_render_tail_bytes(-1) == -1
    ws = torch.zeros(need // 4 + 8, device="cuda")
    rgb, depth = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda")

    def call(mode="f16", ert=0.0, tail_mode=3, ptr=ws.data_ptr(), nbytes=need, tail=True):
        o = _opts(2.0, 6.0, S, False, None, 0, False, ert, False, mode, None, ro.device)
        t = L.nrf_tail(tail_mode, ptr, nbytes)
        return lib.nrf_render_rays_tail(h, L.ptr(ro), L.ptr(rd), R, C.byref(o), C.byref(t) if tail else None, L.ptr(rgb), L.ptr(depth),
                                        None, None, L.stream_ptr())

    assert call() == 0
    for bad, word in ((dict(ert=1e-3), "ert_eps"), (dict(mode="f32"), "base mode"), (dict(mode="f16x3"), "base mode"),
                      (dict(tail_mode=1), "NRF_MMA_F16X3"), (dict(ptr=None), "NULL"), (dict(ptr=ws.data_ptr() + 4), "aligned"),
                      (dict(nbytes=need - 16), "smaller"), (dict(tail=False), "NULL")):
        assert call(**bad) == -1, bad                                           # NRF_EINVAL
        assert word in lib.nrf_last_error().decode(), (bad, lib.nrf_last_error())
    torch.cuda.synchronize()
    # the camera and tile entry points check the same description against THEIR ray count
    o = _opts(2.0, 6.0, S, False, None, 0, False, 0.0, False, "f16", None, ro.device)
    c2w12 = (C.c_float * 12)(*T(O.LEGO_LIKE_C2W)[:3, :4].reshape(-1).tolist())
    short = L.nrf_tail(3, ws.data_ptr(), need - 16)
    assert lib.nrf_render_camera_tail(h, 8, 8, O.focal_for(8), c2w12, 0, R, C.byref(o), C.byref(short), L.ptr(rgb), L.ptr(depth), None, None,
                                      L.stream_ptr()) == -1
    assert lib.nrf_render_cameras_tiles_tail(h, 8, 8, O.focal_for(8), C.cast(c2w12, C.c_void_p), 1, 8, 0, 1, 8, C.byref(o), C.byref(short),
                                             L.ptr(rgb), L.ptr(depth), None, None, L.stream_ptr()) == -1
    # Python surface: bad names, and a tail under grad
    with pytest.raises(ValueError):
        N.render_rays(m, ro, rd, 2.0, 6.0, S, tail_mode="f32")
    with pytest.raises(ValueError):
        N.render_rays(m, ro, rd, 2.0, 6.0, S, mma_mode="f32", tail_mode="f16x3")
    with pytest.raises(L.NrfError):
        N.render_rays(m, ro, rd, 2.0, 6.0, S, ert_eps=1e-3, tail_mode="f16x3")
    m.train()
    from nerf_few_shot_limitations_amd.training import render_rays_train
    with pytest.raises(ValueError):
        N.render_rays(m, ro, rd, 2.0, 6.0, S, tail_mode="f16x3")
    with pytest.raises(ValueError):
        render_rays_train(m, ro, rd, 2.0, 6.0, S, tail_mode="f16x3")
    m.eval()
    # tail_mode=None is the call without the keyword
    a = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True)
    b = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, tail_mode=None)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ check 7: both streams current after training
def test_both_weight_streams_are_current_after_device_side_repacks(N):
    """A module whose parameters live in the flat device vector takes optimiser steps (FusedStep, f16) and is then rendered in
    eval() with a tail: the render must re-pack the f16 AND the split-f16 stream, the first time and after a further step."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    m, _, _ = make(N, "v1", "f16")
    c2w = T(O.LEGO_LIKE_C2W)
    Rn, S = 64, 16
    x = O.positional_encoding(T(O.uniform01(111, Rn * S * 3).reshape(Rn * S, 3) * 4 - 2).float(), 10).cuda()
    z = torch.sort(T(O.uniform01(112, Rn * S).reshape(Rn, S) * 4 + 2).float(), dim=-1).values.cuda()
    rd = T(O.uniform01(113, Rn * 3).reshape(Rn, 3) - 0.5).float().cuda()
    tgt = torch.ones(Rn, 3).cuda()
    step = FusedStep(m.train(), lr=1e-2)

    def fresh_copy_render():
        ref = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode="f16")
        ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        return N.render_camera(ref.cuda().eval(), 16, 16, O.focal_for(16), c2w, 2.0, 6.0, 16, tail_mode="f16x3")

    seen = []
    for n_steps in (2, 1):
        m.train()
        for _ in range(n_steps):
            step(x, z, rd, tgt)
        got = N.render_camera(m.eval(), 16, 16, O.focal_for(16), c2w, 2.0, 6.0, 16, tail_mode="f16x3")
        want = fresh_copy_render()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), n_steps
        seen.append(got[0])
    assert not torch.equal(seen[0], seen[1])                                    # the further step did change the weights
