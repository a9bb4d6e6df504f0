"""GPU tests of the V3 renderer (NeRFWithDINO) conditioned on ANOTHER view's feature map, as the reference's evaluate() conditions
every test view on training view 0 (train.py:203-208).  With the rendered camera as the source view every sample of a ray projects
to the same map point, so a gather that used the wrong sample, column or held slot would go unnoticed; here the source views of
tests/golden/dino_views.npz (make_golden.py: dino_views) spread a ray's samples over the map, partly off it, off it altogether and
behind the source camera (camera-space Z > 0, projected mirrored), on non-square maps at dino_dim 64 and 128 (multiscale.yaml).
Run with -m gpu on an MI355X."""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # BASELINE.json north star, as tests/test_gpu_parity.py
PARITY = ["f32", "f16x3"]
POSES = ["orbit", "near"]
WIDTHS = [64, 128]


def T(a):
    return torch.from_numpy(np.asarray(a))


def maxdiff(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


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


def model(N, dd, mode, scene="fog"):
    m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=dd, mma_mode=mode)
    p = O.make_weights("v3", 2, scene) if dd == 64 else O.make_weights("v3", 3, scene, dino_dim=128)
    m.load_state_dict(p, strict=False)
    return m.cuda().eval(), p


def source(g, name, dd, features=None):
    """The train.py:203-214 side channel of a source view of the fixture: its map, pose and its own intrinsics (focal, H, W)."""
    return dict(features=T(g[f"map{dd}"]) if features is None else features, pose=T(g[f"{name}_pose"]),
                focal=float(g[f"{name}_focal"]), H=int(g[f"{name}_H"]), W=int(g[f"{name}_W"]))


def frame(g):
    """The fixture's rendered camera: (H, W, S, focal, c2w) and its rays (R,3) on the CPU (bit-equal to N.get_rays)."""
    H, W, S, f, c2w = int(g["H"]), int(g["W"]), int(g["S"]), float(g["focal"]), T(g["c2w"])
    ro, rd = O.get_rays(H, W, f, c2w)
    return H, W, S, f, c2w, ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()


def poisoned(g, dd):
    """The fixture's map with NaN at texel (0, 0), +Inf at (Hp-1, Wp-1) and NaN at one interior texel (the fixture lists the 64-d
    map's; the 128-d map gets the same pattern) -> (map, [(y, x)] of the bad texels)."""
    fm = g[f"map{dd}"].copy()
    Hp, Wp = fm.shape[1:3]
    bad = [tuple(int(v) for v in t) for t in g["bad_texels"]] if dd == 64 else [(0, 0), (Hp - 1, Wp - 1), (Hp // 2, Wp // 2)]
    assert bad[0] == (0, 0) and bad[1] == (Hp - 1, Wp - 1)
    for i, (y, x) in enumerate(bad):
        fm[0, y, x] = np.inf if i == 1 else np.nan
    return T(fm), bad


def census(src, pts):
    """Per sample point (n,3), with the oracle's projection (ray_utils.py:176-210) and the align_corners=False unnormalisation:
    number of the 4 bilinear taps on the map, camera-space Z, distance to the source camera centre, and (gx, gy)."""
    xy, z, _ = O.project_points_to_image(pts, src["pose"], src["focal"], src["H"], src["W"])
    Hp, Wp = src["features"].shape[1:3]
    gx, gy = ((xy[:, 0] + 1) * Wp - 1) / 2, ((xy[:, 1] + 1) * Hp - 1) / 2
    x0, y0 = torch.floor(gx), torch.floor(gy)
    n_on = torch.zeros(pts.shape[0], dtype=torch.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            n_on += ((x0 + dx >= 0) & (x0 + dx <= Wp - 1) & (y0 + dy >= 0) & (y0 + dy <= Hp - 1)).long()
    dist = (pts - src["pose"][:3, 3]).norm(dim=-1)
    return n_on, z, dist, gx, gy


def kernel_points(ro, rd, z):
    return (ro[:, None, :] + rd[:, None, :] * z.cpu()[..., None]).reshape(-1, 3)


# ------------------------------------------------------------------ the geometry really covers every case of the gather
# shares measured on the fixture's frame (plain / jittered sampling, 14x22 / 10x12 maps): orbit on 0.57-0.60, partly 0.115-0.16, off
# 0.27-0.29, nearest sample 2.7 from the source camera; near on 0.10-0.11, partly 0.03-0.06, off 0.84-0.85, Z > 0 0.45 of which
# 0.05-0.06 with taps on the map, nearest sample 1.0
GEOMETRY = {"orbit": dict(on=0.45, partly=0.08, off=0.2, behind=(0.0, 0.0), behind_on=0.0, min_dist=2.0),
            "near": dict(on=0.07, partly=0.02, off=0.7, behind=(0.35, 0.5), behind_on=0.03, min_dist=0.75)}


@pytest.mark.parametrize("dd", WIDTHS)
def test_cross_view_geometry_covers_every_tap_case(N, g, dd):
    """On the kernel's own sample points: samples with all four taps on the map, some on it, none on it, and behind the source
    camera (mirrored by the reference's projection, some of them back on the map) each above a stated share; every sample a stated
    distance from the source camera centre (near Z = 0 the projection is ill-conditioned and no fixed bar applies).  And the
    comparison can fail: the map rolled by one texel changes rgb by more than 100x the parity bar."""
    H, W, S, f, c2w, ro, rd = frame(g)
    m, _ = model(N, dd, "f16x3")
    for name, want in GEOMETRY.items():
        src = source(g, name, dd)
        for tr in (None, T(g["t_rand"])):
            out = N.render_rays(m, ro, rd, 2.0, 6.0, S, t_rand=tr, dino=src, return_z=True)
            n_on, z, dist, _, _ = census(src, kernel_points(ro, rd, out["z_vals"]))
            share = dict(on=float((n_on == 4).double().mean()), partly=float(((n_on > 0) & (n_on < 4)).double().mean()),
                         off=float((n_on == 0).double().mean()), behind=float((z > 0).double().mean()),
                         behind_on=float(((z > 0) & (n_on > 0)).double().mean()), min_dist=float(dist.min()))
            print(f"geometry d{dd} {name} {'jit' if tr is not None else 'plain'}: " + " ".join(f"{k} {v:.3f}" for k, v in share.items()))
            for k in ("on", "partly", "off", "behind_on", "min_dist"):
                assert share[k] >= want[k], (name, k, share)
            assert want["behind"][0] <= share["behind"] <= want["behind"][1], (name, share)
        rolled = torch.roll(src["features"], 1, dims=2)
        a = N.render_rays(m, ro, rd, 2.0, 6.0, S, dino=src)
        b = N.render_rays(m, ro, rd, 2.0, 6.0, S, dino=dict(src, features=rolled))
        assert maxdiff(a["rgb"], b["rgb"]) > 100 * TOL, (name, maxdiff(a["rgb"], b["rgb"]))


# ------------------------------------------------------------------ parity: the reference's renders and the oracle
@pytest.mark.parametrize("pmode", PARITY)
@pytest.mark.parametrize("dd", WIDTHS)
def test_cross_view_render_matches_the_reference(N, g, dd, pmode):
    """train.py:188-242 with another view's map, captured from the reference (dino_views.npz): rgb / depth / weights at 1e-4."""
    H, W, S, f, c2w, ro, rd = frame(g)
    m, _ = model(N, dd, pmode)
    for name in POSES:
        for tag, tr in (("plain", None), ("jit", T(g["t_rand"]))):
            out = N.render_rays(m, ro, rd, 2.0, 6.0, S, t_rand=tr, dino=source(g, name, dd))
            key = f"{name}_d{dd}_{tag}"
            assert maxdiff(out["rgb"], g[key + "_rgb"]) <= TOL, key
            assert maxdiff(out["depth"], g[key + "_depth"]) <= TOL, key
            assert maxdiff(out["weights"], g[key + "_w"]) <= TOL, key


@pytest.mark.parametrize("pmode", PARITY)
@pytest.mark.parametrize("dd", WIDTHS)
def test_cross_view_render_routes_match_the_oracle(N, g, dd, pmode):
    """Disparity spacing and white background on the 'solid' scene, through the tile kernel, the ray-queue kernel (a vanishing
    ert_eps: no ray stops early) and the in-kernel camera: the oracle (on the kernel's own depths) at 1e-4, the routes bit for bit."""
    H, W, S, f, c2w, ro, rd = frame(g)
    m, p = model(N, dd, pmode, "solid")
    for name in POSES:
        src = source(g, name, dd)
        kw = dict(lindisp=True, white_bkgd=True, dino=src)
        tile = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, **kw)
        assert maxdiff(tile["z_vals"], O.sample_points_along_rays(ro, rd, 2.0, 6.0, S, None, True)[1]) <= 2e-6
        ref = O.render_rays(p, "v3", ro, rd, 2.0, 6.0, S, white_bkgd=True, dino=src, z_in=tile["z_vals"].cpu())
        for k in ("rgb", "depth", "weights"):
            assert maxdiff(tile[k], ref[k]) <= TOL, (name, k, maxdiff(tile[k], ref[k]))
        queue = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, ert_eps=1e-30, **kw)
        for k in ("rgb", "depth", "weights", "z_vals"):
            assert maxdiff(queue[k], tile[k]) <= 1e-30, (name, k)
        cam = N.render_camera(m, H, W, f, c2w, 2.0, 6.0, S, **kw)
        assert torch.equal(cam[0], tile["rgb"]) and torch.equal(cam[1], tile["depth"]), name
        cam = N.render_camera(m, H, W, f, c2w, 2.0, 6.0, S, ert_eps=1e-30, **kw)
        assert maxdiff(cam[0], tile["rgb"]) <= 1e-30 and maxdiff(cam[1], tile["depth"]) <= 1e-30, name


@pytest.mark.parametrize("pmode", PARITY)
def test_cross_view_hierarchical_fine_pass(N, g, pmode):
    """Coarse pass, resampling, fine pass on the sorted union (as test_hierarchical_render_c3): the fine pass against the oracle on
    the SAME union depths -- whose samples sit elsewhere on the map than the coarse ones."""
    H, W, S, f, c2w, ro, rd = frame(g)
    Ni = 16
    for dd, name in ((64, "near"), (128, "orbit")):
        m, p = model(N, dd, pmode)
        src = source(g, name, dd)
        out = N.render_hierarchical(m, ro, rd, 2.0, 6.0, S, Ni, dino=src)
        assert out["z_vals"].shape == (H * W, S + Ni) and torch.all(out["z_vals"][:, 1:] >= out["z_vals"][:, :-1])
        coarse = O.render_rays(p, "v3", ro, rd, 2.0, 6.0, S, dino=src)
        assert maxdiff(out["coarse"]["rgb"], coarse["rgb"]) <= TOL and maxdiff(out["coarse"]["weights"], coarse["weights"]) <= TOL
        fine = O.render_rays(p, "v3", ro, rd, 2.0, 6.0, S + Ni, dino=src, z_in=out["z_vals"].cpu())
        for k in ("rgb", "depth", "weights"):
            assert maxdiff(out[k], fine[k]) <= TOL, (dd, name, k, maxdiff(out[k], fine[k]))


# ------------------------------------------------------------------ the 16-bit modes at dino_dim 128 (render_v3w)
def test_128d_16bit_modes_cross_view_and_forward(N, g, golden):
    """multiscale.yaml's width in the throughput modes: f16 (the packed DinoHeld hold, nets.hpp) and bf16 (the build that spills
    into scratch), through the cross-view render against the reference's frames and through m(pos, dirs, dino) against
    mlp_v3_d128.npz.  Bounds: the measured error (tests/gpu_error_report.py --dino-views, MI355X) with the margin of the
    neighbouring tests; bf16 carries no 1e-4 claim: finite, in range, a PSNR floor."""
    H, W, S, f, c2w, ro, rd = frame(g)
    m, _ = model(N, 128, "f16")
    for name in POSES:
        key = f"{name}_d128_plain"
        out = N.render_rays(m, ro, rd, 2.0, 6.0, S, dino=source(g, name, 128), mma_mode="f16")
        # measured f16: rgb 3.5e-4 / 3.9e-4, depth 5.0e-4 / 6.4e-4, 80.0 / 79.8 dB (orbit / near)
        assert maxdiff(out["rgb"], g[key + "_rgb"]) <= 1e-3 and maxdiff(out["depth"], g[key + "_depth"]) <= 2e-3, name
        assert O.psnr(out["rgb"].cpu(), T(g[key + "_rgb"])) > 76, name
        out = N.render_rays(m, ro, rd, 2.0, 6.0, S, dino=source(g, name, 128), mma_mode="bf16")
        assert torch.isfinite(out["rgb"]).all() and torch.isfinite(out["depth"]).all()
        assert float(out["rgb"].min()) >= 0 and float(out["rgb"].max()) <= 1 + 1e-5
        # measured bf16: 58.3 / 57.9 dB (max rgb error 4.0e-3 / 4.5e-3)
        assert O.psnr(out["rgb"].cpu(), T(g[key + "_rgb"])) > 54, name
    gm = golden("mlp_v3_d128")
    for mode, tol in (("f16", 3e-3), ("bf16", 4e-2)):           # measured rgb 1.25e-3 / 1.45e-2 (density 7.7e-4 / 8.0e-3)
        m.mma_mode = mode
        with torch.no_grad():
            rgb, dens = m(T(gm["pos"]), T(gm["dirs"]), T(gm["dino"]))
        assert torch.isfinite(rgb).all() and torch.isfinite(dens).all()
        assert maxdiff(rgb, gm["rgb"]) <= tol and maxdiff(dens, gm["density"]) <= tol, (mode, maxdiff(rgb, gm["rgb"]))


# ------------------------------------------------------------------ invariances with a gather that varies along the ray
@pytest.mark.parametrize("mode", ["f16", "f16x3"])
@pytest.mark.parametrize("dd", WIDTHS)
def test_cross_view_every_samples_per_pass_split_gives_the_same_bits(N, g, dd, mode, monkeypatch):
    """As test_gpu_parity.py's V2 test: every pinned samples-per-pass split (env NRF_SPW, read per launch) reproduces the SPW = 1
    march bit for bit -- here with the samples of one ray gathering from different texels, so a column mix-up shows."""
    c2w = T(O.LEGO_LIKE_C2W)
    m, _ = model(N, dd, mode, "solid")
    H, W, S = 100, 100, 32
    monkeypatch.setenv("NRF_SPW", "0")
    ref = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, dino=source(g, "orbit", dd))
    ro, rd = N.get_rays(37, 29, O.focal_for(29), c2w)                  # 1073 rays: ragged tiles at every split
    ref2 = N.render_rays(m, ro, rd, 2.0, 6.0, 21, perturb=True, seed=5, return_z=True, dino=source(g, "near", dd))
    for l in range(1, 7):
        monkeypatch.setenv("NRF_SPW", str(l))
        got = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, dino=source(g, "orbit", dd))
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), l
        got2 = N.render_rays(m, ro, rd, 2.0, 6.0, 21, perturb=True, seed=5, return_z=True, dino=source(g, "near", dd))
        for k in ("rgb", "depth", "weights", "z_vals"):
            assert torch.equal(got2[k], ref2[k]), (l, k)
    monkeypatch.delenv("NRF_SPW")
    auto = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, dino=source(g, "orbit", dd))
    assert torch.equal(auto[0], ref[0]) and torch.equal(auto[1], ref[1])


@pytest.mark.parametrize("mode", ["f16", "f16x3"])
def test_cross_view_random_launch_cuts_never_change_a_bit(N, g, mode):
    """A launch vs the same rays cut at a random place, tile and ray-queue kernels, both widths and both source views, with jitter."""
    rng = np.random.RandomState(13 if mode == "f16" else 17)
    c2w = T(O.LEGO_LIKE_C2W)
    models = {dd: model(N, dd, mode, "solid")[0] for dd in WIDTHS}
    for it in range(8):
        dd, name = WIDTHS[it % 2], POSES[(it // 2) % 2]
        Hh, Ww = int(rng.randint(2, 60)), int(rng.randint(2, 60))
        S = int(rng.choice([3, 8, 21, 32, 48, 64]))
        eps = 1e-30 if it % 4 >= 2 else 0.0
        ro, rd = N.get_rays(Hh, Ww, O.focal_for(Ww), c2w)
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        Rr = ro.shape[0]
        tr = torch.from_numpy(rng.rand(Rr, S).astype(np.float32)).cuda()
        cut = int(rng.randint(1, Rr))
        kw = dict(ert_eps=eps, dino=source(g, name, dd), return_z=True)
        whole = N.render_rays(models[dd], ro, rd, 2.0, 6.0, S, t_rand=tr, **kw)
        a = N.render_rays(models[dd], ro[:cut], rd[:cut], 2.0, 6.0, S, t_rand=tr[:cut], **kw)
        b = N.render_rays(models[dd], ro[cut:], rd[cut:], 2.0, 6.0, S, t_rand=tr[cut:], **kw)
        for k in ("rgb", "depth", "weights", "z_vals"):
            assert torch.equal(whole[k], torch.cat([a[k], b[k]])), (it, dd, name, Hh, Ww, S, eps, cut, k)
        assert torch.isfinite(whole["rgb"]).all()


@pytest.mark.parametrize("dd", WIDTHS)
def test_cross_view_ray_queue_kernel_matches_tile_kernel(N, g, dd):
    """ert_eps > 0 selects the ray-queue kernel; with a vanishing eps it must reproduce the tile kernel in every mode, with ragged ray
    counts, explicit jitter, the counter RNG and the in-kernel camera."""
    c2w = T(O.LEGO_LIKE_C2W)
    for mode in ("bf16", "f16", "f32", "f16x3"):
        m, _ = model(N, dd, mode, "solid")
        for name in POSES:
            src = source(g, name, dd)
            for (H, W, S) in ((37, 53, 16), (8, 9, 40)):
                ro, rd = N.get_rays(H, W, O.focal_for(W), c2w)
                a = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, dino=src)
                b = N.render_rays(m, ro, rd, 2.0, 6.0, S, return_z=True, ert_eps=1e-30, dino=src)
                for k in ("rgb", "depth", "weights", "z_vals"):
                    assert maxdiff(a[k], b[k]) <= 1e-30, (mode, name, H, W, S, k)
                cam = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, ert_eps=1e-30, dino=src)
                assert maxdiff(cam[0], a["rgb"]) <= 1e-30, (mode, name, H, W, S)
            H, W, S = 12, 16, 24
            ro, rd = N.get_rays(H, W, O.focal_for(W), c2w)
            tr = torch.from_numpy(O.uniform01(5, H * W * S).reshape(H * W, S))
            a = N.render_rays(m, ro, rd, 2.0, 6.0, S, t_rand=tr, dino=src)
            b = N.render_rays(m, ro, rd, 2.0, 6.0, S, t_rand=tr, ert_eps=1e-30, dino=src)
            assert maxdiff(a["rgb"], b["rgb"]) <= 1e-30 and maxdiff(a["weights"], b["weights"]) <= 1e-30, (mode, name)
            a = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, perturb=True, seed=3, dino=src)
            b = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, perturb=True, seed=3, ert_eps=1e-30, dino=src)
            assert maxdiff(a[0], b[0]) <= 1e-30, (mode, name)


@pytest.mark.parametrize("dd", WIDTHS)
def test_evaluate_views_conditioned_on_view_0(N, g, dd):
    """The reference's evaluate(): three test poses rendered in one batch, every one of them on training view 0's map (the 'orbit'
    view).  evaluate_views and a two-rank tile split equal per-view render_rays of explicit rays bit for bit, and the oracle at 1e-4
    (split-f16 mode)."""
    from nerf_few_shot_limitations_amd import tiles
    H, W, S, f, c2w, _, _ = frame(g)
    a = np.radians(-25.0)
    rz = torch.tensor([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32)
    poses = torch.stack([c2w, c2w.clone(), rz @ c2w])
    poses[1, 0, 3] += 0.3
    poses[1, 2, 3] -= 0.2
    src = source(g, "orbit", dd)
    m, p = model(N, dd, "f16x3")
    res = N.evaluate_views(m, poses, H, W, f, 2.0, 6.0, S, dino=src)
    assert res["images"].shape == (3, H, W, 3)
    for v in range(3):
        ro, rd = O.get_rays(H, W, f, poses[v])
        ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
        one = N.render_rays(m, ro, rd, 2.0, 6.0, S, dino=src)
        assert torch.equal(res["images"][v].reshape(-1, 3), one["rgb"]) and torch.equal(res["depth"][v].reshape(-1), one["depth"]), v
        ref = O.render_rays(p, "v3", ro, rd, 2.0, 6.0, S, dino=src)
        assert maxdiff(one["rgb"], ref["rgb"]) <= TOL and maxdiff(one["depth"], ref["depth"]) <= TOL, v
        for rank in (0, 1):
            job = tiles.TileJob(m, H, W, f, poses, 2.0, 6.0, S, rank, 2, 2 * W, dino=src)
            job.launch()
            ids = tiles.local_ray_ids(rank, 2, H * W, 2 * W)[: job.n_real * 2 * W].cuda()
            got = job.buf[v, : job.n_real * 2 * W]
            assert torch.equal(got[:, :3], one["rgb"][ids]) and torch.equal(got[:, 3], one["depth"][ids]), (v, rank)


@pytest.mark.parametrize("dd", WIDTHS)
def test_cross_view_per_ray_termination_bound(N, g, dd):
    """Each ray stops at its own T < eps: the frame differs from the full march by < eps (rgb) / eps * far (depth)."""
    c2w = T(O.LEGO_LIKE_C2W)
    H = W = 48
    S = 64
    m, _ = model(N, dd, "bf16", "smooth")
    ro, rd = N.get_rays(H, W, O.focal_for(W), c2w)
    for name in POSES:
        src = source(g, name, dd)
        full = N.render_rays(m, ro, rd, 2.0, 6.0, S, dino=src)
        # rays whose transmittance falls below 1e-2 before their last sample (measured: d64 0.51 / 0.85, d128 1.0 of the frame)
        assert float((full["weights"][:, :-1].sum(-1) > 1 - 1e-2).double().mean()) > 0.3, name
        for eps in (1e-2, 1e-4):
            ert = N.render_camera(m, H, W, O.focal_for(W), c2w, 2.0, 6.0, S, ert_eps=eps, dino=src)
            assert maxdiff(ert[0], full["rgb"]) <= eps * 1.01 and maxdiff(ert[1], full["depth"]) <= eps * 6.0 * 1.01, (name, eps)


# ------------------------------------------------------------------ non-finite texels
@pytest.mark.parametrize("mode", ["f16", "f32"])
@pytest.mark.parametrize("dd", WIDTHS)
def test_non_finite_texels_reach_only_the_samples_that_tap_them(N, g, dd, mode):
    """grid_sample's zeros padding: a tap outside the map contributes exactly 0 whatever the map holds.  With NaN at texel (0, 0),
    +Inf at (Hp-1, Wp-1) and NaN at an interior texel, every ray none of whose samples has an ON-MAP tap on a bad texel renders
    finite and bit-identical to the render with the clean map -- rays with off-map taps included -- in the tile and ray-queue
    kernels.  Then the staged fetch against the reference's, NaN positions included."""
    H, W, S, f, c2w, ro, rd = frame(g)
    m, _ = model(N, dd, mode)
    bad_map, bad = poisoned(g, dd)
    for name in POSES:
        src = source(g, name, dd)
        for eps in (0.0, 1e-30):
            clean = N.render_rays(m, ro, rd, 2.0, 6.0, S, ert_eps=eps, dino=src, return_z=True)
            got = N.render_rays(m, ro, rd, 2.0, 6.0, S, ert_eps=eps, dino=dict(src, features=bad_map), return_z=True)
            n_on, _, _, gx, gy = census(src, kernel_points(ro, rd, clean["z_vals"]))
            # a sample has an on-map tap on texel (y, x) iff |gx - x| < 1 and |gy - y| < 1; the margin absorbs the last ulp of the
            # projection, which the kernel and the oracle may order differently
            touch = torch.zeros_like(gx, dtype=torch.bool)
            for y, x in bad:
                touch |= ((gx - x).abs() < 1 + 1e-3) & ((gy - y).abs() < 1 + 1e-3)
            keep = ~touch.reshape(-1, S).any(1)
            off_map = (n_on < 4).reshape(-1, S).any(1)
            assert int(keep.sum()) >= 0.3 * keep.numel() and int((keep & off_map).sum()) >= 0.2 * keep.numel(), (name, int(keep.sum()))
            keep = keep.nonzero().flatten().cuda()
            for k in ("rgb", "depth", "weights", "z_vals"):
                assert torch.isfinite(got[k][keep]).all(), (name, eps, k)
                assert torch.equal(got[k][keep], clean[k][keep]), (name, eps, k)
    if dd == 64:
        want = g["fetch_poisoned"]
        feats = N.sample_features_at_points(bad_map.cuda(), T(g["fetch_xy"]).cuda()).cpu().double().numpy()
        assert np.array_equal(np.isnan(feats), np.isnan(want)) and np.array_equal(np.isposinf(feats), np.isposinf(want))
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(feats), fin) and np.max(np.abs(feats[fin] - want[fin])) <= 1e-5
