"""Empty-space skipping (include/nerfhip.h: nrf_occupancy): the ray-queue renderer steps over every sample whose cell of an
occupancy bit grid is empty and composites it as density 0.  Definition under test: a render with a grid is, bit for bit, the
render in which the density of every sample in an empty cell is replaced by 0 -- so with an all-ones grid, or a grid that only
drops samples of weight 0, it is the plain render, bit for bit, in all four arithmetic modes.

Frame: 549 rays (9 x 61: more than two strips per wave of a 4-wave workgroup at 64 columns, ragged end), the pinhole camera at
(0, 0, 4) looking down -z, near 2, far 6, the box [-4, 4]^3.  The host replays the cell rule in numpy float32 on the points of
nrf_sample_along_rays (the renderer's own point_on_ray)."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

MODES = ["bf16", "f16", "f32", "f16x3"]
NETS = ["v1", "v2", "v3", "v3w"]
H, W = 9, 61
R = H * W
NEAR, FAR = 2.0, 6.0
C2W = np.eye(4, dtype=np.float32)
C2W[2, 3] = 4.0


def T(a):
    return torch.from_numpy(np.asarray(a))


def cols(mode):
    return 64 if mode in ("bf16", "f16") else 32


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def dino_map(dd=64):
    return torch.from_numpy(O.uniform01(7, 28 * 28 * dd).reshape(1, 28, 28, dd) * 2 - 1)


def make(N, net, mode, scene="fog"):
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


_models = {}


def model(N, net, scene="fog"):
    """One module per (family, scene) for the whole file; the arithmetic is chosen per call (mma_mode=)."""
    key = (net, scene)
    if key not in _models:
        _models[key] = make(N, net, "f32", scene)
    return _models[key]


def rays(N, h=H, w=W):
    ro, rd = N.get_rays(h, w, O.focal_for(w), T(C2W))
    return ro.reshape(-1, 3), rd.reshape(-1, 3)


def grid_of(N, mask, lo=-4.0, hi=4.0, outside=0):
    return N.OccupancyGrid.from_mask(torch.as_tensor(mask), lo, hi, outside=outside)


def host_cells(pts, grid):
    """The cell rule of nerfhip.h in numpy float32: (inside (…) bool, flat cell index (…) int64, 0 where not inside)."""
    pts = np.asarray(pts, np.float32)
    lo, scale, res = np.asarray(grid.lo, np.float32), np.asarray(grid.scale, np.float32), np.asarray(grid.res)
    t = (pts - lo) * scale                                                   # float32 - float32, float32 * float32: one rounding each
    assert t.dtype == np.float32
    inside = np.all((t >= 0) & (t < res.astype(np.float32)), axis=-1)
    i = np.floor(np.where(inside[..., None], t, 0)).astype(np.int64)
    return inside, (i[..., 2] * res[1] + i[..., 1]) * res[0] + i[..., 0]


def host_evaluated(pts, grid):
    """(…) bool: the samples a render with `grid` evaluates (all positions finite)."""
    inside, idx = host_cells(pts, grid)
    occ = grid.to_mask().cpu().numpy().reshape(-1)[idx]
    return np.where(inside, occ, grid.outside == 0)


def points(N, ro, rd, S):
    pts, z = N.sample_points_along_rays(ro, rd, NEAR, FAR, S, perturb=False)
    return pts.cpu().numpy(), z


def same(a, b, keys=("rgb", "depth", "weights", "z_vals")):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------ 1: an all-ones grid is the plain render
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("net", NETS)
def test_all_ones_grid_is_the_plain_render_bit_for_bit(N, net, mode):
    m, _, kw = model(N, net)
    ro, rd = rays(N)
    S = 9
    ones = grid_of(N, torch.ones((32, 32, 32), dtype=torch.bool))
    for ert in (0.0, 1e-2):
        cfg = dict(perturb=True, seed=11, ert_eps=ert, mma_mode=mode, return_z=True, **kw)
        plain = N.render_rays(m, ro, rd, NEAR, FAR, S, **cfg)
        got = N.render_rays(m, ro, rd, NEAR, FAR, S, occupancy=ones, return_stats=True, **cfg)
        same(got, plain)
        st = got["stats"].tolist()
        print(f"all-ones {net} {mode} ert {ert}: stats {st}, utilisation {st[0] / max(1, st[1] * cols(mode)):.3f}")
        if ert == 0.0:
            assert st[0] == R * S, st
        else:
            assert 0 < st[0] <= R * S, st
        assert st[1] * cols(mode) >= st[0]


# ------------------------------------------------------------------ 2: dropping only weight-0 samples changes no bit
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scene", ["fog", "smooth"])
def test_grid_from_the_plain_renders_zero_weights_changes_no_bit(N, scene, mode):
    """24 x 24 rays x 32 samples of V1; a 64^3 cell is occupied iff it holds a sample of non-zero weight in the plain render.  The
    fp32 oracle alone skips 0.65 ("fog") / 0.36 ("smooth") of the samples in this set-up; the share must lie in [0.2, 0.9]."""
    m, _, _ = model(N, "v1", scene)
    ro, rd = rays(N, 24, 24)
    S, res = 32, 64
    plain = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True)
    pts, _ = points(N, ro, rd, S)
    probe = grid_of(N, torch.zeros((res, res, res), dtype=torch.bool))
    inside, idx = host_cells(pts, probe)
    assert inside.all()                                              # the box holds the whole frustum
    occ = np.zeros(res ** 3, dtype=bool)
    occ[idx[plain["weights"].cpu().numpy() != 0]] = True
    grid = grid_of(N, occ.reshape(res, res, res))
    kept = int(occ[idx].sum())
    share = 1.0 - kept / idx.size
    got = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, occupancy=grid, return_stats=True)
    st = got["stats"].tolist()
    print(f"zero-weight grid {scene} {mode}: skipped share {share:.3f}, stats {st}, utilisation {st[0] / max(1, st[1] * cols(mode)):.3f}")
    assert 0.2 <= share <= 0.9, share
    same(got, plain)
    assert st[0] == kept, (st, kept)
    plain_ert = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, ert_eps=1e-2)
    got_ert = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, ert_eps=1e-2, occupancy=grid, return_stats=True)
    same(got_ert, plain_ert)
    assert got_ert["stats"][0].item() <= kept


# ------------------------------------------------------------------ 3: a geometric grid against the masked oracle
def oracle_outputs(p, net, ro, rd, S, kw):
    """Per-sample (rgb (R,S,3), sigma (R,S,1), z (R,S)) of the fp32 oracle (oracle.render_rays without its compositor)."""
    with torch.no_grad():
        pts, z = O.sample_points_along_rays(ro, rd, NEAR, FAR, S, None)
        n = ro.shape[0]
        pf = pts.reshape(-1, 3)
        df = rd[:, None, :].expand(-1, S, -1).reshape(-1, 3)
        if net == "v1":
            out = O.mlp_v1(p, O.positional_encoding(pf, 10))
            rgb, sig = out[:, :3], out[:, 3:4]
        elif net == "v2":
            rgb, sig = O.mlp_v2(p, pf, df, 10, 4)
        else:
            d = kw["dino"]
            xy, _, _ = O.project_points_to_image(pf, d["pose"], d["focal"], d["H"], d["W"])
            rgb, sig = O.mlp_v3(p, pf, df, O.sample_features_at_points(d["features"], xy), 12, 4)
    return rgb.reshape(n, S, 3), sig.reshape(n, S, 1), z


def masked_oracle(outs, evaluated, rd, white):
    rgb, sig, z = outs
    sig = torch.where(torch.from_numpy(evaluated)[..., None], sig, torch.zeros_like(sig))
    return O.volume_render(rgb, sig, z, rd, white)


def sphere_mask(res, radius, lo=-4.0, hi=4.0):
    c = lo + (np.arange(res, dtype=np.float64) + 0.5) * (hi - lo) / res
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    return (xx ** 2 + yy ** 2 + zz ** 2) <= radius ** 2


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("net", ["v1", "v2", "v3"])
def test_sphere_grid_against_the_masked_oracle(N, net, mode):
    """Cells whose centre lies within 1.5 of the origin, 32^3.  Expected: the oracle's network outputs with the density of the samples
    the host's cell rule calls empty set to 0, composited by oracle.volume_render.  Bound: the parity bar of these two modes, 1e-4."""
    m, p, kw = model(N, net)
    ro, rd = rays(N)
    S = 16
    grid = grid_of(N, sphere_mask(32, 1.5))
    pts, _ = points(N, ro, rd, S)
    ev = host_evaluated(pts, grid)
    share = ev.mean()
    print(f"sphere {net} {mode}: evaluated share {share:.3f}")
    assert share > 0.1 and 1.0 - share > 0.1, share
    oro, ord_ = O.get_rays(H, W, O.focal_for(W), T(C2W))
    outs = oracle_outputs(p, net, oro.reshape(-1, 3), ord_.reshape(-1, 3), S, kw)
    for white in (False, True):
        want = masked_oracle(outs, ev, ord_.reshape(-1, 3), white)
        got = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, white_bkgd=white, occupancy=grid, return_stats=True, **kw)
        errs = [float((got[k].cpu() - w).abs().max()) for k, w in zip(("rgb", "depth", "weights"), want)]
        print(f"sphere {net} {mode} white {white}: max err rgb {errs[0]:.3e} depth {errs[1]:.3e} weights {errs[2]:.3e}")
        assert max(errs) <= 1e-4, errs
        assert got["stats"][0].item() == int(ev.sum())


# ------------------------------------------------------------------ 4: an all-zero grid costs no network pass
@pytest.mark.parametrize("mode", MODES)
def test_all_zero_grid_renders_the_background_without_a_network_pass(N, mode):
    m, _, _ = model(N, "v1")
    ro, rd = rays(N)
    S = 9
    zero = grid_of(N, torch.zeros((32, 32, 32), dtype=torch.bool))
    plain = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, perturb=True, seed=4)
    for white in (False, True):
        got = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, return_z=True, perturb=True, seed=4, white_bkgd=white, occupancy=zero,
                            return_stats=True)
        assert torch.equal(got["rgb"], torch.full_like(got["rgb"], 1.0 if white else 0.0))
        assert torch.equal(got["depth"], torch.zeros_like(got["depth"]))
        assert torch.equal(got["weights"], torch.zeros_like(got["weights"]))
        assert torch.equal(got["z_vals"], plain["z_vals"])
        assert got["stats"].tolist() == [0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_passes_are_spent_on_the_occupied_rays_only(N, mode):
    """Occupied: the cells that only rays 0 .. 63 pass through (512 cells along y: finer than the spacing of the pixel rows, so row 0
    owns its cells).  Those rays fill one wave of 64 columns, or two of 32: no more than S passes each; every other ray is empty."""
    m, _, _ = model(N, "v1")
    ro, rd = rays(N)
    S = 9
    res = (32, 512, 32)                                                          # rx, ry, rz
    probe = N.OccupancyGrid.from_mask(torch.zeros((32, 512, 32), dtype=torch.bool), -4.0, 4.0)
    assert probe.res == res
    pts, _ = points(N, ro, rd, S)
    inside, idx = host_cells(pts, probe)
    assert inside.all()
    occ = np.zeros(32 * 512 * 32, dtype=bool)
    occ[idx[:64].reshape(-1)] = True
    occ[idx[64:].reshape(-1)] = False
    grid = N.OccupancyGrid.from_mask(torch.from_numpy(occ.reshape(32, 512, 32)), -4.0, 4.0)
    kept = occ[idx]
    assert kept[:64].sum() >= 61 * S and not kept[64:].any()
    got = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode=mode, occupancy=grid, return_stats=True)
    st = got["stats"].tolist()
    print(f"first-64 grid {mode}: stats {st}")
    assert st[0] == int(kept.sum())
    assert 0 < st[1] <= S * (64 // cols(mode)), st
    assert torch.equal(got["rgb"][64:], torch.zeros_like(got["rgb"][64:]))


# ------------------------------------------------------------------ 5: samples outside the box
@pytest.mark.parametrize("outside", [0, 1])
def test_outside_follows_the_flag(N, outside):
    """The box [-1, 1]^3 holds the middle of the frustum only.  outside = 0: the samples beyond it are evaluated; 1: skipped."""
    m, p, kw = model(N, "v1")
    ro, rd = rays(N)
    S = 16
    mask = T(O.uniform01(31, 32 ** 3).reshape(32, 32, 32)) < 0.5
    grid = grid_of(N, mask, -1.0, 1.0, outside=outside)
    pts, _ = points(N, ro, rd, S)
    inside, _ = host_cells(pts, grid)
    assert 0.2 < inside.mean() < 0.8, inside.mean()
    ev = host_evaluated(pts, grid)
    assert np.array_equal(ev[~inside], np.full(int((~inside).sum()), outside == 0))
    oro, ord_ = O.get_rays(H, W, O.focal_for(W), T(C2W))
    want = masked_oracle(oracle_outputs(p, "v1", oro.reshape(-1, 3), ord_.reshape(-1, 3), S, kw), ev, ord_.reshape(-1, 3), False)
    got = N.render_rays(m, ro, rd, NEAR, FAR, S, mma_mode="f32", occupancy=grid, return_stats=True)
    errs = [float((got[k].cpu() - w).abs().max()) for k, w in zip(("rgb", "depth", "weights"), want)]
    print(f"outside {outside}: evaluated {int(ev.sum())} of {ev.size}, max err {errs}")
    assert max(errs) <= 1e-4, errs
    assert got["stats"][0].item() == int(ev.sum())
    # a non-finite position is always evaluated, as in the plain render
    bad_o = ro.clone()
    bad_o[5, 0] = float("inf")
    got_bad = N.render_rays(m, bad_o, rd, NEAR, FAR, S, mma_mode="f32", occupancy=grid, return_stats=True)
    plain_bad = N.render_rays(m, bad_o, rd, NEAR, FAR, S, mma_mode="f32")
    assert got_bad["stats"][0].item() == int(ev.sum()) - int(ev[5].sum()) + S
    assert torch.equal(got_bad["weights"][5].isnan(), plain_bad["weights"][5].isnan())


# ------------------------------------------------------------------ 6: camera and tiles
@pytest.mark.parametrize("mode", ["f16", "f16x3"])
@pytest.mark.parametrize("net", ["v1", "v3"])
def test_camera_and_tile_routes_match_the_ray_route(N, net, mode):
    from nerf_few_shot_limitations_amd import tiles
    m, _, kw = model(N, net)
    S = 9
    grid = grid_of(N, sphere_mask(32, 1.5))
    ro, rd = rays(N)
    a, b = 37, 530                                                              # a ragged range of the image's rays
    want = N.render_rays(m, ro[a:b], rd[a:b], NEAR, FAR, S, mma_mode=mode, occupancy=grid, return_stats=True, ert_eps=1e-3, **kw)
    rgb, depth, st = N.render_camera(m, H, W, O.focal_for(W), T(C2W), NEAR, FAR, S, ray_begin=a, ray_end=b, mma_mode=mode, occupancy=grid,
                                     return_stats=True, ert_eps=1e-3, **kw)
    assert torch.equal(rgb, want["rgb"]) and torch.equal(depth, want["depth"])
    assert st[0].item() == want["stats"][0].item()
    # two views, rows [r,g,b,depth], 100-ray tiles: 6 tiles = 600 rows per view, the last 51 repeat the last ray
    poses = torch.stack([T(C2W).clone(), T(C2W).clone()])
    poses[1, 0, 3] += 0.3
    seed = 21
    job = tiles.TileJob(m, H, W, O.focal_for(W), poses, NEAR, FAR, S, 0, 1, 100, mma_mode=mode, occupancy=grid, return_stats=True,
                        perturb=True, seed=seed, **kw)
    job.launch()
    total = 0
    for v in range(2):
        rgb, depth, st = N.render_camera(m, H, W, O.focal_for(W), poses[v], NEAR, FAR, S, mma_mode=mode, occupancy=grid, return_stats=True,
                                         perturb=True, seed=seed + v * 0x51ED27, **kw)
        assert torch.equal(job.buf[v, :R, :3], rgb) and torch.equal(job.buf[v, :R, 3], depth), v
        assert torch.equal(job.buf[v, R:], job.buf[v, R - 1:R].expand(600 - R, 4)), v
        total += st[0].item()
    # (the padded rows are rays too: each repeats the last ray's samples)
    assert job.stats[0].item() >= total


# ------------------------------------------------------------------ 7: building a grid from a model
def dilate_np(mask):
    out = np.zeros_like(mask)
    p = np.pad(mask, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + mask.shape[0], dy:dy + mask.shape[1], dx:dx + mask.shape[2]]
    return out


@pytest.mark.parametrize("net,scene", [("v1", "smooth"), ("v2", "solid")])
def test_from_model_matches_a_numpy_recomputation(N, net, scene):
    m, _, _ = model(N, net, scene)
    G = N.OccupancyGrid
    res, k = 32, 2
    grid = G.from_model(m, -4.0, 4.0, resolution=res, threshold=0.0, samples_per_cell=k, dilate=1, chunk_cells=10000)   # several chunks, ragged
    pts = G.cell_points((res,) * 3, -4.0, 4.0, 0, res ** 3, k, 0, "cuda").reshape(-1, 3)
    centre = pts.reshape(res, res, res, k, 3)[3, 5, 7, 0].cpu().numpy()                      # cell (ix 7, iy 5, iz 3): sample 0 is its centre
    assert np.allclose(centre, -4.0 + (np.array([7, 5, 3]) + 0.5) * 0.25)
    cell = torch.arange(res ** 3, device="cuda")
    lo_c = torch.stack([cell % res, (cell // res) % res, cell // res ** 2], -1).float() * 0.25 - 4.0
    assert bool(((pts.reshape(-1, k, 3) >= lo_c[:, None]) & (pts.reshape(-1, k, 3) <= lo_c[:, None] + 0.25)).all())
    with torch.no_grad():
        if net == "v1":
            dens = m(N.PositionalEncoding(10)(pts))[:, 3]
        else:
            dirs = torch.zeros_like(pts)
            dirs[:, 2] = -1.0
            dens = m(pts, dirs)[1].reshape(-1)
    raw = (dens.reshape(-1, k).max(dim=1).values > 0.0).cpu().numpy().reshape(res, res, res)
    assert 0.0 < raw.mean() < 1.0, raw.mean()                        # both kinds of cell occur
    want = G.from_mask(torch.from_numpy(dilate_np(raw)), -4.0, 4.0)
    assert torch.equal(grid.bits.cpu(), want.bits)
    assert torch.equal(grid.to_mask().cpu(), torch.from_numpy(dilate_np(raw)))
    again = G.from_mask(grid.to_mask(), -4.0, 4.0)
    assert torch.equal(again.bits, grid.bits)
    # raising the threshold only clears bits
    low = G.from_model(m, -4.0, 4.0, resolution=res, threshold=0.0, samples_per_cell=k, dilate=0)
    assert torch.equal(low.to_mask().cpu(), torch.from_numpy(raw))
    high = G.from_model(m, -4.0, 4.0, resolution=res, threshold=max(float(dens.median()), 0.0) + 1.0, samples_per_cell=k, dilate=0)
    assert int((high.bits & ~low.bits).ne(0).sum()) == 0
    assert high.occupied_fraction < low.occupied_fraction
    # a NaN density makes its cell occupied (nrf_occupancy_pack on a hand-made density row)
    from nerf_few_shot_limitations_amd import _lib as L
    d = torch.full((64 * 3,), -1.0, device="cuda")
    d[3 * 5 + 1] = float("nan")
    d[3 * 40] = 0.5
    bits = torch.zeros((2,), dtype=torch.int32, device="cuda")
    L.check(L.lib().nrf_occupancy_pack(L.ptr(d), 64, 3, 0.25, bits.data_ptr(), L.stream_ptr()))
    assert bits.tolist() == [1 << 5, 1 << 8]


# ------------------------------------------------------------------ 8: refusals of the Python surface
def test_python_refusals(N):
    m, _, _ = model(N, "v1")
    ro, rd = rays(N)
    grid = grid_of(N, torch.ones((32, 32, 32), dtype=torch.bool))
    with pytest.raises(ValueError, match="tail_mode"):
        N.render_rays(m, ro, rd, NEAR, FAR, 8, mma_mode="f16", tail_mode="f16x3", occupancy=grid)
    with pytest.raises(ValueError, match="tail_mode"):
        N.render_camera(m, H, W, O.focal_for(W), T(C2W), NEAR, FAR, 8, mma_mode="f16", tail_mode="f16x3", occupancy=grid)
    with pytest.raises(ValueError, match="occupancy"):
        N.render_rays(m, ro, rd, NEAR, FAR, 8, return_stats=True)
    mt, _, _ = make(N, "v1", "f32")
    mt.train()
    with torch.enable_grad(), pytest.raises(ValueError, match="inference"):
        N.render_rays(mt, ro, rd, NEAR, FAR, 8, occupancy=grid)
    m3, _, _ = model(N, "v3")
    with pytest.raises(ValueError, match="dino"):
        N.OccupancyGrid.from_model(m3, -4.0, 4.0, resolution=32)
    # NeRFRenderer carries a grid to its evaluation renders
    r = N.NeRFRenderer(m, NEAR, FAR, occupancy=grid)
    out = r.render_rays(ro, rd)
    assert torch.equal(out["rgb"], N.render_rays(m, ro, rd, NEAR, FAR, 64)["rgb"])
