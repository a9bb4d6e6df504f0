"""Occupancy grids pruned by the weights the training views render (include/nerfhip.h: nrf_occupancy_mark_rays /
nrf_occupancy_mark_camera, occupancy.py: OccupancyGrid.mark / from_views / prune).

Definition under test: per sample of a ray, the cell is the one the skipping renderer looks up (tests/test_gpu_occupancy.py:
host_cells on the points of nrf_sample_along_rays); `hit` is set iff !(w <= weight_threshold), `seen` iff
1 - sum(earlier weights) > seen_eps; a sample outside the box or at a non-finite position marks nothing.  The host replays that in
numpy float32.  The synthetic weights are multiples of 2^-12 with per-ray sums <= 1, so every order of the fp32 additions gives the
same bits and the replay of `seen` is exact; on rendered weights `hit` is still exact and `seen` is compared with a band around
seen_eps (tests 4 to 6; tests 5 and 6 also ask for the bits of the marker's ray entry on renders made through the ray route)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_occupancy import (C2W, FAR, NEAR, T, dilate_np, grid_of, host_cells, host_evaluated, model, points, rays, same,
                                      sphere_mask)

pytestmark = pytest.mark.gpu

LEGO = np.asarray(O.LEGO_LIKE_C2W, np.float32)
# a non-cubic grid over a box with unequal sides that cuts the frustum of the LEGO-like camera (its samples lie 2 .. 6 in front of
# (-0.05, 3.85, 1.21), looking at the origin)
RES1 = (64, 32, 96)
LO1, HI1 = (-1.5, -1.0, -2.0), (1.0, 2.5, 1.5)


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def empty_grid(N, res, lo, hi):
    rx, ry, rz = res
    return N.OccupancyGrid.from_mask(torch.zeros((rz, ry, rx), dtype=torch.bool), lo, hi).to("cuda")


def words_of(N, grid, cells):
    """int32 words (CPU) of a flat bool array over the cells of `grid`."""
    rx, ry, rz = grid.res
    return N.OccupancyGrid.from_mask(torch.from_numpy(np.ascontiguousarray(cells).reshape(rz, ry, rx)), grid.lo, grid.hi).bits


def mask_of(N, grid, words):
    return N.OccupancyGrid(words.cpu(), grid.res, grid.lo, grid.hi).to_mask().numpy().reshape(-1)


def synthetic_weights(n_rays, S, seed):
    """(n_rays, S) float32 multiples of 2^-12 with per-ray sums <= 1: rays 0 .. 2 are all zero, about a third of the samples are zero;
    the size of the draws goes round by ray, so that some rays stay below 1 and others reach a sum of exactly 1 well before their end
    (and are zero from there on)."""
    rng = np.random.default_rng(seed)
    top = np.array([1, 3, 8])[np.arange(n_rays) % 3] * 4096 // S + 2
    k = rng.integers(0, top[:, None], size=(n_rays, S))
    k[rng.random((n_rays, S)) < 0.35] = 0
    k[:3] = 0
    c = np.minimum(np.cumsum(k, axis=1), 4096)
    k = np.diff(np.concatenate([np.zeros((n_rays, 1), dtype=c.dtype), c], axis=1), axis=1)
    return (k.astype(np.float32) / np.float32(4096.0)).astype(np.float32)


def transmittance(w):
    """1 - the exclusive prefix sum of the rows of w, numpy float32 (front to back)."""
    w = np.asarray(w, np.float32)
    excl = np.concatenate([np.zeros_like(w[:, :1]), np.cumsum(w, axis=1, dtype=np.float32)[:, :-1]], axis=1)
    return (np.float32(1.0) - excl).astype(np.float32)


def replay(grid, pts, w, tau, eps):
    """(hit, seen) flat bool arrays over the cells of `grid`: the rule of nerfhip.h on the points pts (R,S,3) and weights w (R,S)."""
    with np.errstate(invalid="ignore"):
        inside, idx = host_cells(pts, grid)
        w = np.asarray(w, np.float32)
        hit_s = inside & ~(w <= np.float32(tau))
        seen_s = inside & (transmittance(w) > np.float32(eps))
    hit, seen = np.zeros(grid.n_cells, dtype=bool), np.zeros(grid.n_cells, dtype=bool)
    hit[idx[hit_s]] = True
    seen[idx[seen_s]] = True
    return hit, seen


def mark_raw(N, grid, ro, rd, z, w, tau, eps, want_hit=True, want_seen=True):
    """nrf_occupancy_mark_rays itself, with either output left out (NULL)."""
    from nerf_few_shot_limitations_amd import _lib as L
    hit = torch.zeros_like(grid.bits) if want_hit else None
    seen = torch.zeros_like(grid.bits) if want_seen else None
    L.check(L.lib().nrf_occupancy_mark_rays(L.ptr(ro), L.ptr(rd), w.shape[0], w.shape[1], L.ptr(z), L.ptr(w), (C.c_int32 * 3)(*grid.res),
                                            (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.scale), tau, eps,
                                            hit.data_ptr() if want_hit else None, seen.data_ptr() if want_seen else None, L.stream_ptr()))
    return hit, seen


# ------------------------------------------------------------------ 1: synthetic rows, exact
@pytest.mark.parametrize("S,jitter", [(1, False), (9, False), (64, False), (65, False), (65, True), (150, False)])
def test_synthetic_rows_match_the_host_replay_exactly(N, S, jitter):
    ro, rd = N.get_rays(5, 8, O.focal_for(8), T(LEGO))
    ro, rd = ro.reshape(-1, 3)[:37].clone(), rd.reshape(-1, 3)[:37].contiguous()
    ro[7, 1] = float("inf")                                                  # one ray without a finite position
    R = 37
    pts, z = N.sample_points_along_rays(ro, rd, NEAR, FAR, S, perturb=jitter, seed=17)
    pts = pts.cpu().numpy()
    w = synthetic_weights(R, S, 100 + S)
    w[5, min(3, S - 1)] = np.nan
    sums = np.nansum(w.astype(np.float64), axis=1)
    assert sums.max() <= 1.0 and (sums[:3] == 0).all()
    if S >= 9:
        full = (np.cumsum(np.nan_to_num(w).astype(np.float64), axis=1)[:, S // 2] == 1.0)
        assert full.sum() >= 3, full.sum()                                   # rays that sum to exactly 1 before their end
    grid = empty_grid(N, RES1, LO1, HI1)
    with np.errstate(invalid="ignore"):
        inside, _ = host_cells(pts, grid)
    assert not inside[7].any()
    if S >= 9:
        assert 0.15 < inside.mean() < 0.85, inside.mean()                    # the box cuts the frustum
    wt = torch.from_numpy(w).cuda()
    for tau in (0.0, 2.0 ** -6):
        for eps in (0.0, 2.0 ** -7):
            want_hit, want_seen = replay(grid, pts, w, tau, eps)
            hit, seen = grid.mark(ro, rd, z, wt, weight_threshold=tau, seen_eps=eps)
            assert hit.dtype == torch.int32 and hit.shape == grid.bits.shape and seen.shape == grid.bits.shape
            assert torch.equal(hit.cpu(), words_of(N, grid, want_hit)), (S, tau, eps)
            assert torch.equal(seen.cpu(), words_of(N, grid, want_seen)), (S, tau, eps)
            # either output alone
            only_hit, none = mark_raw(N, grid, ro, rd, z, wt, tau, eps, want_seen=False)
            assert none is None and torch.equal(only_hit, hit)
            none, only_seen = mark_raw(N, grid, ro, rd, z, wt, tau, eps, want_hit=False)
            assert none is None and torch.equal(only_seen, seen)
            # seen_eps=None: hit alone through the Python call
            h2, s2 = grid.mark(ro, rd, z, wt, weight_threshold=tau)
            assert s2 is None and torch.equal(h2, hit)
            print(f"S {S} jitter {jitter} tau {tau} eps {eps}: inside {inside.mean():.3f}, hit cells {int(want_hit.sum())}, seen cells {int(want_seen.sum())}")
            assert want_hit.sum() > 0 and want_seen.sum() > 0
            if S >= 9:
                assert (want_seen & ~want_hit).any()
    assert torch.equal(grid.bits, torch.zeros_like(grid.bits))                 # the grid's own bits play no part


# ------------------------------------------------------------------ 2: invariance
def test_marks_do_not_depend_on_the_cut_the_repetition_or_the_entry_point(N):
    from nerf_few_shot_limitations_amd import _lib as L
    H, W, S = 9, 61, 65
    R = H * W
    ro, rd = rays(N)
    _, z = N.sample_points_along_rays(ro, rd, NEAR, FAR, S, perturb=False)
    w = torch.from_numpy(synthetic_weights(R, S, 9)).cuda()
    grid = empty_grid(N, (64, 64, 64), -4.0, 4.0)
    tau, eps = 2.0 ** -6, 2.0 ** -7
    hit, seen = grid.mark(ro, rd, z, w, tau, eps)
    assert int(hit.ne(0).sum()) > 0 and int(seen.ne(0).sum()) > 0
    # two runs agree
    hit_b, seen_b = grid.mark(ro, rd, z, w, tau, eps)
    assert torch.equal(hit_b, hit) and torch.equal(seen_b, seen)
    # the two halves of the rays, accumulated into the same arrays
    h = R // 2 + 3
    hit_c, seen_c = grid.mark(ro[:h], rd[:h], z[:h], w[:h], tau, eps)
    assert not (torch.equal(hit_c, hit) and torch.equal(seen_c, seen))
    hit_c2, seen_c2 = grid.mark(ro[h:], rd[h:], z[h:], w[h:], tau, eps, hit=hit_c, seen=seen_c)
    assert hit_c2 is hit_c and seen_c2 is seen_c
    assert torch.equal(hit_c, hit) and torch.equal(seen_c, seen)
    # marking twice is marking once
    grid.mark(ro, rd, z, w, tau, eps, hit=hit_c, seen=seen_c)
    assert torch.equal(hit_c, hit) and torch.equal(seen_c, seen)
    # the camera entry over a ragged sub-range against the ray entry on get_rays' rows
    a, b = 37, 530
    want_hit, want_seen = grid.mark(ro[a:b], rd[a:b], z[a:b], w[a:b], tau, eps)
    got_hit, got_seen = torch.zeros_like(grid.bits), torch.zeros_like(grid.bits)
    c2w = (C.c_float * 12)(*C2W[:3, :4].reshape(-1).tolist())
    zc, wc = z[a:b].contiguous(), w[a:b].contiguous()
    L.check(L.lib().nrf_occupancy_mark_camera(H, W, O.focal_for(W), c2w, a, b, S, L.ptr(zc), L.ptr(wc), (C.c_int32 * 3)(*grid.res),
                                              (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.scale), tau, eps, got_hit.data_ptr(),
                                              got_seen.data_ptr(), L.stream_ptr()))
    assert torch.equal(got_hit, want_hit) and torch.equal(got_seen, want_seen)
    assert not torch.equal(want_hit, hit)


# ------------------------------------------------------------------ 3: weight_threshold = 0 changes no bit
FRAME = dict(H=24, W=24, S=32, res=64)


def frame(N, scene, mode):
    """The frame of tests/test_gpu_occupancy.py's zero-weights test: (model, rays, plain render, points, cell indices)."""
    m, _, _ = model(N, "v1", scene)
    ro, rd = rays(N, FRAME["H"], FRAME["W"])
    plain = N.render_rays(m, ro, rd, NEAR, FAR, FRAME["S"], mma_mode=mode, return_z=True)
    pts, _ = points(N, ro, rd, FRAME["S"])
    probe = empty_grid(N, (FRAME["res"],) * 3, -4.0, 4.0)
    inside, idx = host_cells(pts, probe)
    assert inside.all()                                                      # the box holds the whole frustum
    return m, ro, rd, plain, pts, idx, probe


def views_grid(N, m, mode, **kw):
    return N.OccupancyGrid.from_views(m, T(C2W), FRAME["H"], FRAME["W"], O.focal_for(FRAME["W"]), NEAR, FAR, FRAME["S"], -4.0, 4.0,
                                      resolution=FRAME["res"], mma_mode=mode, **kw)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32", "f16x3"])
@pytest.mark.parametrize("scene", ["fog", "smooth"])
def test_threshold_zero_grid_of_a_view_renders_that_view_bit_for_bit(N, scene, mode):
    m, ro, rd, plain, pts, idx, probe = frame(N, scene, mode)
    S = FRAME["S"]
    occ = np.zeros(probe.n_cells, dtype=bool)
    occ[idx[plain["weights"].cpu().numpy() != 0]] = True
    grid = views_grid(N, m, mode, unseen="drop", dilate=0)
    assert grid.bits.is_cuda and grid.res == probe.res and grid.outside == 0
    assert torch.equal(grid.bits.cpu(), words_of(N, probe, occ))
    kept = int(occ[idx].sum())
    share = 1.0 - kept / idx.size
    got = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, occupancy=grid, return_stats=True)
    print(f"from_views tau 0 {scene} {mode}: skipped share {share:.3f}, stats {got['stats'].tolist()}")
    assert 0.2 <= share <= 0.9, share
    same(got, plain)
    assert got["stats"][0].item() == kept
    plain_ert = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, ert_eps=1e-2)
    got_ert = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, ert_eps=1e-2, occupancy=grid)
    same(got_ert, plain_ert)


# ------------------------------------------------------------------ 4: weight_threshold > 0 and the guard
@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_positive_threshold_and_the_unseen_guard(N, mode):
    tau, eps, band = 1e-3, 1e-2, 1e-5
    m, ro, rd, plain, pts, idx, probe = frame(N, "smooth", mode)
    S = FRAME["S"]
    w = plain["weights"].cpu().numpy()
    hit = np.zeros(probe.n_cells, dtype=bool)
    hit[idx[~(w <= np.float32(tau))]] = True
    drop = views_grid(N, m, mode, weight_threshold=tau, seen_eps=eps, unseen="drop", dilate=0)
    assert torch.equal(drop.bits.cpu(), words_of(N, probe, hit))
    # seen: decided by the samples of a cell; a sample whose transmittance lies within `band` of seen_eps may fall either way (the
    # order of the kernel's fp32 additions is not the host's)
    Tr = transmittance(w)
    sure, maybe = np.zeros(probe.n_cells, dtype=bool), np.zeros(probe.n_cells, dtype=bool)
    sure[idx[Tr > np.float32(eps + band)]] = True
    maybe[idx[Tr > np.float32(eps - band)]] = True
    keep = views_grid(N, m, mode, weight_threshold=tau, seen_eps=eps, unseen="keep", dilate=0)
    got = mask_of(N, probe, keep.bits)
    least, most = hit | ~maybe, hit | ~sure
    undecided = int((least != most).sum())
    print(f"guard {mode}: cells undecided within {band} of seen_eps: {undecided} of {probe.n_cells}")
    assert undecided <= probe.n_cells // 1000
    assert not (least & ~got).any() and not (got & ~most).any()
    assert not (mask_of(N, probe, drop.bits) & ~got).any()                     # keeping the unseen cells only adds cells
    shares = {}
    for name, g in (("drop", drop), ("keep", keep)):
        r = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, occupancy=g, return_stats=True)
        count = int(host_evaluated(pts, g).sum())
        assert r["stats"][0].item() == count, (name, r["stats"].tolist(), count)
        shares[name] = count / idx.size
        print(f"guard {mode} unseen={name}: occupied cells {g.occupied_fraction:.4f}, evaluated share {shares[name]:.3f}, "
              f"max |rgb - rgb(no grid)| {float((r['rgb'] - plain['rgb']).abs().max()):.3e}")
        assert 0.3 <= shares[name] <= 0.8, (name, shares[name])
    assert shares["drop"] < shares["keep"]


# ------------------------------------------------------------------ 5: several views, a base grid, chunks, prune
BAND = 1e-5          # as in test 4: S <= 32 fp32 additions of partial sums <= 1 differ by far less between two orders (S * 2^-24 < 2e-6)


def view_replay(N, probe, m, pose, H, W, S, mode, tau, eps, base=None, **kw):
    """One view replayed outside from_views from its own render through the ray route (under `base` when given).  Returns
    hit, sure, maybe: flat bool arrays of the numpy replay -- hit is exact, seen lies between sure (transmittance > eps + BAND) and
    maybe (> eps - BAND); and (hit, seen) word tensors of the marker's ray entry on the same rows."""
    ro, rd = N.get_rays(H, W, O.focal_for(W), T(pose))
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    r = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, occupancy=base, **kw)
    pts, _ = points(N, ro, rd, S)
    w = r["weights"].cpu().numpy()
    hit, _ = replay(probe, pts, w, tau, eps)
    inside, idx = host_cells(pts, probe)
    Tr = transmittance(w)
    sure, maybe = np.zeros(probe.n_cells, dtype=bool), np.zeros(probe.n_cells, dtype=bool)
    sure[idx[inside & (Tr > np.float32(eps + BAND))]] = True
    maybe[idx[inside & (Tr > np.float32(eps - BAND))]] = True
    return hit, sure, maybe, probe.mark(ro, rd, r["z_vals"], r["weights"], tau, eps)


def between(N, probe, grid, least, most):
    """least <= the cells of grid <= most, and the two bounds differ in at most 0.1 % of the cells."""
    got = mask_of(N, probe, grid.bits)
    assert int((least != most).sum()) <= probe.n_cells // 1000, int((least != most).sum())
    assert not (least & ~got).any() and not (got & ~most).any()


def test_views_are_ored_and_a_base_grid_bounds_the_result(N):
    G = N.OccupancyGrid
    H, W, S, res, mode, tau, eps = 12, 16, 16, 32, "f32", 1e-3, 1e-2
    m, _, _ = model(N, "v1", "smooth")
    views = [C2W, np.asarray(O.LEGO_LIKE_C2W, np.float32)]
    poses = torch.stack([T(v) for v in views])
    probe = empty_grid(N, (res,) * 3, -4.0, 4.0)
    args = (H, W, O.focal_for(W), NEAR, FAR, S)
    cfg = dict(weight_threshold=tau, seen_eps=eps, mma_mode=mode)
    rep = [view_replay(N, probe, m, v, H, W, S, mode, tau, eps) for v in views]
    # hit of each view is the numpy replay from its own render's weights, exactly; two views give the OR
    one = [G.from_views(m, poses[v], *args, -4.0, 4.0, resolution=res, unseen="drop", dilate=0, **cfg) for v in range(2)]
    for v in range(2):
        assert torch.equal(one[v].bits.cpu(), words_of(N, probe, rep[v][0])), v
        assert rep[v][0].any()
    assert not torch.equal(one[0].bits, one[1].bits)
    both = G.from_views(m, poses, *args, -4.0, 4.0, resolution=res, unseen="drop", dilate=0, **cfg)
    assert torch.equal(both.bits, one[0].bits | one[1].bits)
    assert torch.equal(both.bits.cpu(), words_of(N, probe, rep[0][0] | rep[1][0]))
    # hit | ~seen: between the numpy bounds, and the bits of the marker's ray entry on the same renders
    hit_np, sure, maybe = (rep[0][k] | rep[1][k] for k in range(3))
    keep = G.from_views(m, poses, *args, -4.0, 4.0, resolution=res, dilate=0, **cfg)
    between(N, probe, keep, hit_np | ~maybe, hit_np | ~sure)
    kh, ks = rep[0][3][0] | rep[1][3][0], rep[0][3][1] | rep[1][3][1]
    assert torch.equal(keep.bits, kh | ~ks)
    hit, seen = probe._view_marks(m, poses, *args, **cfg)
    assert torch.equal(hit, kh) and torch.equal(seen, ks)
    # with a base grid: rendered under it, bounded by it, the formula replayed from renders made under occupancy=base
    base = grid_of(N, sphere_mask(res, 2.0)).to("cuda")
    base_np = mask_of(N, probe, base.bits)
    rep = [view_replay(N, probe, m, v, H, W, S, mode, tau, eps, base=base) for v in views]
    hit_np, sure, maybe = (rep[0][k] | rep[1][k] for k in range(3))
    assert not (hit_np & ~base_np).any()                                     # rendered under the base: no weight outside it
    grown = dilate_np(hit_np.reshape(res, res, res)).reshape(-1)
    dropped = G.from_views(m, poses, *args, -4.0, 4.0, resolution=res, base=base, dilate=1, unseen="drop", **cfg)
    assert torch.equal(dropped.bits.cpu(), words_of(N, probe, grown & base_np))
    got = G.from_views(m, poses, *args, -4.0, 4.0, resolution=res, base=base, dilate=1, **cfg)
    assert int((got.bits & ~base.bits).ne(0).sum()) == 0
    between(N, probe, got, (grown | ~maybe) & base_np, (grown | ~sure) & base_np)
    ks = rep[0][3][1] | rep[1][3][1]
    want = (grown | ~mask_of(N, probe, ks)) & base_np
    assert torch.equal(got.bits.cpu(), words_of(N, probe, want))
    assert 0 < want.sum() < base_np.sum()
    # ray ranges of 64 give the bits of one range
    chunked = G.from_views(m, poses, *args, -4.0, 4.0, resolution=res, base=base, dilate=1, chunk_rays=64, **cfg)
    assert torch.equal(chunked.bits, got.bits)
    # prune is from_views on the grid's own cells
    pruned = base.prune(m, poses, *args, dilate=1, **cfg)
    assert torch.equal(pruned.bits, got.bits) and (pruned.res, pruned.lo, pruned.hi, pruned.outside) == (base.res, base.lo, base.hi, base.outside)


# ------------------------------------------------------------------ 6: V3
def test_v3_grid_belongs_to_its_source_view(N):
    G = N.OccupancyGrid
    H, W, S, res, mode, tau, eps = 12, 16, 9, 32, "f16x3", 1e-3, 1e-2
    m, _, kw = model(N, "v3")
    probe = empty_grid(N, (res,) * 3, -4.0, 4.0)
    args = (H, W, O.focal_for(W), NEAR, FAR, S)
    cfg = dict(resolution=res, weight_threshold=tau, seen_eps=eps, dilate=0, mma_mode=mode)
    hit_np, sure, maybe, (kh, ks) = view_replay(N, probe, m, C2W, H, W, S, mode, tau, eps, **kw)
    drop = G.from_views(m, T(C2W), *args, -4.0, 4.0, unseen="drop", **cfg, **kw)
    assert torch.equal(drop.bits.cpu(), words_of(N, probe, hit_np))           # the numpy replay from its own render's weights
    assert hit_np.any()
    got = G.from_views(m, T(C2W), *args, -4.0, 4.0, **cfg, **kw)
    between(N, probe, got, hit_np | ~maybe, hit_np | ~sure)
    assert torch.equal(got.bits, kh | ~ks)
    assert 0.0 < got.occupied_fraction < 1.0
    with pytest.raises(ValueError, match="dino"):
        G.from_views(m, T(C2W), *args, -4.0, 4.0, resolution=res, mma_mode=mode)
    with pytest.raises(ValueError, match="dino"):
        probe._view_marks(m, T(C2W), *args, mma_mode=mode)


# ------------------------------------------------------------------ 7: refusals of the Python surface
def test_python_refusals(N):
    G = N.OccupancyGrid
    m, _, _ = model(N, "v1")
    ro, rd = rays(N)
    S = 8
    _, z = N.sample_points_along_rays(ro, rd, NEAR, FAR, S, perturb=False)
    w = torch.zeros_like(z)
    cpu = grid_of(N, torch.zeros((32, 32, 32), dtype=torch.bool))
    gpu = cpu.to("cuda")
    with pytest.raises(ValueError, match="GPU"):
        cpu.mark(ro, rd, z, w)
    with pytest.raises(ValueError, match="GPU"):
        cpu._view_marks(m, T(C2W), 4, 4, 10.0, NEAR, FAR, S)
    with pytest.raises(ValueError, match=r"\(R, S\)"):
        gpu.mark(ro, rd, z, w[:, :-1])
    with pytest.raises(ValueError, match=r"\(R, 3\)"):
        gpu.mark(ro[:-1], rd[:-1], z, w)
    with pytest.raises(ValueError, match="hit"):
        gpu.mark(ro, rd, z, w, hit=torch.zeros((7,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="seen"):
        gpu.mark(ro, rd, z, w, seen_eps=0.0, seen=torch.zeros_like(cpu.bits))
    args = (m, T(C2W), 4, 4, 10.0, NEAR, FAR, S, -4.0, 4.0)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_threshold"):
            gpu.mark(ro, rd, z, w, weight_threshold=bad)
        with pytest.raises(ValueError, match="weight_threshold"):
            G.from_views(*args, resolution=32, weight_threshold=bad)
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="seen_eps"):
            gpu.mark(ro, rd, z, w, seen_eps=bad)
        with pytest.raises(ValueError, match="seen_eps"):
            G.from_views(*args, resolution=32, seen_eps=bad)
    with pytest.raises(ValueError, match="unseen"):
        G.from_views(*args, resolution=32, unseen="maybe")
    with pytest.raises(ValueError, match="same res"):
        G.from_views(*args, resolution=64, base=gpu)
    with pytest.raises(ValueError):
        G.from_views(*args, resolution=48)
