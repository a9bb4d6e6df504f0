"""The patch-based depth-smoothness term (RegNeRF) of the fused training step, without a GPU: the kernel's dL/d depth stencil replayed
in fp32 against float64 autograd of the definition of `smooth`; the exported entries and their refusals; FusedStep's keywords and
refusals; train_cli's flags; the patch and pose samplers of ray_sampler; the new unit's resource census
(tests/golden/kernel_resources_patch_reg.json)."""
import argparse
import ctypes as C
import inspect
import json
import math
import os

import pytest
import torch

from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def smooth_of(depth):
    """`smooth` of (N_p, P, P) depths by its definition (RegNeRF's compute_tv_norm(...).mean()), in depth's dtype."""
    a = depth[:, :-1, :-1] - depth[:, :-1, 1:]
    b = depth[:, :-1, :-1] - depth[:, 1:, :-1]
    return (a * a + b * b).mean()


def stencil_gd(depth, weight):
    """dL/d depth of every patch ray in depth's dtype, in the kernel's operation order: t = (c - right) + (c - below) at an anchor,
    then - (left - c) where the left neighbour is an anchor, then - (above - c) where the upper one is; gd = scale * t with the
    scale formed once on the host as 2 w / (N_p (P-1)^2).  Returns (gd, per-patch DS in anchor order)."""
    n, P, _ = depth.shape
    dt = depth.dtype
    scale = torch.tensor(2.0 * weight, dtype=dt) / (torch.tensor(float(n), dtype=dt) * torch.tensor(float((P - 1) * (P - 1)), dtype=dt))
    t = torch.zeros_like(depth)
    c = depth
    t[:, :-1, :-1] = (c[:, :-1, :-1] - c[:, :-1, 1:]) + (c[:, :-1, :-1] - c[:, 1:, :-1])
    t[:, :-1, 1:] = t[:, :-1, 1:] - (c[:, :-1, :-1] - c[:, :-1, 1:])
    t[:, 1:, :-1] = t[:, 1:, :-1] - (c[:, :-1, :-1] - c[:, 1:, :-1])
    a = c[:, :-1, :-1] - c[:, :-1, 1:]
    b = c[:, :-1, :-1] - c[:, 1:, :-1]
    return scale * t, (a * a + b * b).reshape(n, -1).sum(dim=1)


def stencil_bound(depth, weight):
    """(N_p,) the allowance on |gd - float64 gd| of a patch: 32 eps scale max |depth difference of that patch| -- at most four
    subtractions, three additions and two multiplications, each rounded once."""
    n, P, _ = depth.shape
    d = depth.double()
    dmax = torch.maximum((d[:, :, :-1] - d[:, :, 1:]).abs().amax(dim=(1, 2)), (d[:, :-1, :] - d[:, 1:, :]).abs().amax(dim=(1, 2)))
    return 32.0 * EPS * (2.0 * weight / (n * (P - 1) ** 2)) * dmax


@pytest.mark.parametrize("P", [2, 3, 8, 16])
def test_stencil_matches_float64_autograd_of_the_definition(P):
    n, lam = 3, 0.7
    depth = torch.from_numpy(O.uniform01(900 + P, n * P * P).reshape(n, P, P) * 4 + 2).float()
    d64 = depth.double().requires_grad_(True)
    (lam * smooth_of(d64)).backward()
    got, ds = stencil_gd(depth, lam)
    assert got.dtype == torch.float32
    err = (got.double() - d64.grad).abs().amax(dim=(1, 2))
    bound = stencil_bound(depth, lam)
    print(f"P={P} err {err.tolist()} bound {bound.tolist()}")
    assert torch.all(err <= bound) and d64.grad.abs().max() > 0
    ref_ds = stencil_gd(depth.double(), lam)[1]
    assert torch.all((ds.double() - ref_ds).abs() <= 1e-5 * ref_ds)
    # the float64 stencil is the float64 gradient
    assert torch.allclose(stencil_gd(depth.double(), lam)[0], d64.grad, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("P", [2, 3, 8, 16])
def test_a_constant_patch_has_no_gradient_and_no_term(P):
    depth = torch.full((3, P, P), 3.7)
    gd, ds = stencil_gd(depth, 0.7)
    assert torch.all(gd == 0) and torch.all(ds == 0)


# ---------------------------------------------------------------------------------------------
# the library's entries and their refusals
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib as L
    L.lib()
    return L


ENTRIES = ("nrf_composite_patch_loss_backward", "nrf_patch_terms_finish")
EINVAL = -1          # NRF_EINVAL


def test_the_library_exports_both_entries_and_the_abi_stays_5(L):
    for name in ENTRIES:
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    for name in ENTRIES + ("nrf_patch_reg", "depth_smooth_weight", "patch_size", "n_patches"):
        assert name in header
    assert [f for f, _ in L.nrf_patch_reg._fields_] == ["struct_bytes", "depth_smooth_weight", "patch_size", "n_patches"]
    assert C.sizeof(L.nrf_patch_reg) == 16 and L.patch_reg().struct_bytes == 16
    assert L.lib().nrf_abi_version() == 5


def _call(L, patch, S=8, n_rays=40, reg="ok", lo="ok", slot=None, patch_terms=4096):
    """nrf_composite_patch_loss_backward on pointers no launch will ever read: every refusal fires before the device is touched."""
    p = 4096
    lo = L.loss_opts() if lo == "ok" else lo
    reg = L.ray_reg() if reg == "ok" else reg
    return L.lib().nrf_composite_patch_loss_backward(p, 3, p, 1, p, p, n_rays, S, 0, p, C.byref(lo) if lo is not None else None,
                                                     C.byref(reg) if reg is not None else None, slot, p, p, 3, p, 1, p, None, 0, None,
                                                     C.byref(patch) if patch is not None else None, patch_terms, None)


def _finish(L, patch, S=8, n_rays=40, reg="ok", lo="ok"):
    lo = L.loss_opts() if lo == "ok" else lo
    reg = L.ray_reg() if reg == "ok" else reg
    return L.lib().nrf_patch_terms_finish(4096, n_rays, S, C.byref(lo) if lo is not None else None, C.byref(reg) if reg is not None else None,
                                          C.byref(patch) if patch is not None else None, 4096, 8192, None)


@pytest.mark.parametrize("why,kw,S,n_rays", [
    ("negative weight", dict(depth_smooth_weight=-0.1, patch_size=2, n_patches=1), 8, 40),
    ("nan weight", dict(depth_smooth_weight=float("nan"), patch_size=2, n_patches=1), 8, 40),
    ("infinite weight", dict(depth_smooth_weight=float("inf"), patch_size=2, n_patches=1), 8, 40),
    ("P = 1", dict(depth_smooth_weight=0.1, patch_size=1, n_patches=1), 8, 40),
    ("P = 17", dict(depth_smooth_weight=0.1, patch_size=17, n_patches=1), 8, 4000),
    ("negative n_patches", dict(depth_smooth_weight=0.1, patch_size=2, n_patches=-1), 8, 40),
    ("no supervised ray", dict(depth_smooth_weight=0.1, patch_size=2, n_patches=10), 8, 40),
    ("more patch rays than rays", dict(depth_smooth_weight=0.1, patch_size=16, n_patches=3), 8, 40),
    ("S = 0", dict(depth_smooth_weight=0.1, patch_size=2, n_patches=1), 0, 40),
    ("S > 4096", dict(depth_smooth_weight=0.1, patch_size=2, n_patches=1), 4097, 40),
])
def test_refusals_fire_without_a_gpu(L, why, kw, S, n_rays):
    patch = L.patch_reg(**kw)
    assert _call(L, patch, S, n_rays) == EINVAL, why
    assert L.lib().nrf_last_error()
    assert _finish(L, patch, S, n_rays) == EINVAL, why


def test_struct_bytes_null_and_the_parents_refusals(L):
    ok = L.patch_reg(0.1, 2, 1)
    bad = L.patch_reg(0.1, 2, 1)
    bad.struct_bytes = 12
    assert _call(L, bad) == EINVAL and b"struct_bytes" in L.lib().nrf_last_error()
    assert _finish(L, bad) == EINVAL
    assert _call(L, None) == EINVAL and _finish(L, None) == EINVAL
    assert _call(L, ok, patch_terms=None) == EINVAL
    # the parent's own: the ray regularisers' struct, the loss options, the slot's alignment, the sizes
    assert _call(L, ok, reg=None) == EINVAL and _finish(L, ok, reg=None) == EINVAL
    assert _call(L, ok, reg=L.ray_reg(dist_weight=1.0, dist_inv_span=0.0)) == EINVAL
    assert _call(L, ok, reg=L.ray_reg(occ_weight=1.0, occ_samples=0)) == EINVAL
    assert _call(L, ok, lo=None) == EINVAL and _finish(L, ok, lo=None) == EINVAL
    assert _call(L, ok, lo=L.loss_opts(rgb_weight=-1.0)) == EINVAL and _finish(L, ok, lo=L.loss_opts(rgb_weight=-1.0)) == EINVAL
    assert _call(L, ok, slot=4098) == EINVAL and b"aligned" in L.lib().nrf_last_error()
    assert _call(L, ok, n_rays=0) == EINVAL and _finish(L, ok, n_rays=0) == EINVAL
    assert L.lib().nrf_patch_terms_finish(None, 40, 8, C.byref(L.loss_opts()), C.byref(L.ray_reg()), C.byref(ok), 4096, 8192, None) == EINVAL
    assert L.lib().nrf_patch_terms_finish(4096, 40, 8, C.byref(L.loss_opts()), C.byref(L.ray_reg()), C.byref(ok), None, 8192, None) == EINVAL


# ---------------------------------------------------------------------------------------------
# FusedStep and train_cli
# ---------------------------------------------------------------------------------------------
def _model():
    import nerf_few_shot_limitations_amd as N
    return N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2)


def test_fused_step_takes_the_keywords_and_refuses_bad_ones():
    from nerf_few_shot_limitations_amd.training import FusedStep
    p = inspect.signature(FusedStep.__init__).parameters
    assert [p[k].default for k in ("depth_smooth_weight", "patch_size")] == [0.0, 8]
    for fn in (FusedStep.__call__, FusedStep.step_rays):
        assert inspect.signature(fn).parameters["n_patches"].default == 0
    m = _model()
    plain = FusedStep(m)
    assert not plain.patch_reg and not plain.ray_reg and plain.last_patch_depth is None
    s = FusedStep(m, depth_smooth_weight=0.1, patch_size=4)
    assert s.patch_reg and not s.ray_reg and (s.depth_smooth_weight, s.patch_size) == (0.1, 4)
    for bad in (dict(depth_smooth_weight=-1e-3), dict(depth_smooth_weight=float("nan")), dict(depth_smooth_weight=float("inf")),
                dict(depth_smooth_weight=0.1, patch_size=1), dict(depth_smooth_weight=0.1, patch_size=17), dict(patch_size=0),
                dict(depth_smooth_weight=0.1, patch_size=2.5)):
        with pytest.raises(ValueError):
            FusedStep(m, **bad)


def test_step_view_and_the_hierarchical_steps_refuse_the_term():
    from nerf_few_shot_limitations_amd.training import FusedStep
    s = FusedStep(_model(), depth_smooth_weight=0.1)
    o = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="depth_smooth_weight"):
        s.step_view(None, None, 4, 4, 1.0, None, 2.0, 6.0, 8)
    with pytest.raises(ValueError, match="depth_smooth_weight"):
        s.step_rays_hierarchical(o, o, o, 2.0, 6.0, 8, 4)
    with pytest.raises(ValueError, match="depth_smooth_weight"):
        s.step_view_hierarchical(None, None, 4, 4, 1.0, None, 2.0, 6.0, 8, 4)


def test_patch_counts_are_checked_on_the_host():
    from nerf_few_shot_limitations_amd.training import FusedStep
    plain, s = FusedStep(_model()), FusedStep(_model(), depth_smooth_weight=0.1, patch_size=2)
    with pytest.raises(ValueError, match="depth_smooth_weight"):
        plain._patch_check(40, 1)
    assert plain._patch_check(40, 0) == 40 and s._patch_check(40, 0) == 40 and s._patch_check(40, 9) == 4
    for bad in (-1, 10, 11):
        with pytest.raises(ValueError):
            s._patch_check(40, bad)


def test_train_cli_flags_and_refusals():
    from nerf_few_shot_limitations_amd import train_cli
    ns = lambda **kw: argparse.Namespace(**{**dict(depth_smooth_weight=0.0, patch_size=8, patches_per_step=16, patch_stride=1, n_importance=0,
                                                   fused_inputs=False, occupancy_res=0, occupancy_per_view=False, train_extractor=False), **kw})
    err = train_cli.patch_reg_args_error
    assert err(ns()) is None and err(argparse.Namespace()) is None
    assert err(ns(depth_smooth_weight=0.1)) is None and err(ns(depth_smooth_weight=0.1, patch_size=4, patches_per_step=3, patch_stride=2)) is None
    assert "--n-importance" in err(ns(depth_smooth_weight=0.1, n_importance=8))
    assert "--fused-inputs" in err(ns(depth_smooth_weight=0.1, fused_inputs=True))
    assert "--occupancy" in err(ns(depth_smooth_weight=0.1, occupancy_res=64))
    assert "--occupancy" in err(ns(depth_smooth_weight=0.1, occupancy_warmup=4))
    assert "--occupancy" in err(ns(depth_smooth_weight=0.1, occupancy_per_view=True))
    assert "--train-extractor" in err(ns(depth_smooth_weight=0.1, train_extractor=True))
    assert err(ns(depth_smooth_weight=-1.0)) is not None and err(ns(depth_smooth_weight=float("nan"))) is not None
    assert "--patch-size" in err(ns(depth_smooth_weight=0.1, patch_size=1)) and "--patch-size" in err(ns(depth_smooth_weight=0.1, patch_size=17))
    assert "--patches-per-step" in err(ns(depth_smooth_weight=0.1, patches_per_step=0))
    assert "--patch-stride" in err(ns(depth_smooth_weight=0.1, patch_stride=0))
    assert train_cli.patch_reg_options(ns()) == {}
    assert train_cli.patch_reg_options(ns(depth_smooth_weight=0.1, patch_size=4)) == dict(depth_smooth_weight=0.1, patch_size=4)
    # the command refuses before it reads a config or a data set
    for flag, more in (("--n-importance", ["--n-importance", "8"]), ("--fused-inputs", ["--fused-inputs"]),
                       ("--occupancy", ["--occupancy-res", "64"]), ("--occupancy", ["--occupancy-warmup", "4"]),
                       ("--train-extractor", ["--train-extractor"])):
        with pytest.raises(SystemExit, match=flag):
            train_cli.main(["--config", "/nonexistent.yaml", "--data", "/nonexistent", "--depth-smooth-weight", "0.1", *more])
    doc = " ".join(train_cli.__doc__.split())
    for word in ("--depth-smooth-weight W", "--patch-size P", "--patches-per-step N", "--patch-stride K", "RegNeRF", "nrf_patch_reg"):
        assert word in doc, word


# ---------------------------------------------------------------------------------------------
# the samplers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,P,n,stride", [(20, 30, 8, 5, 1), (20, 30, 4, 7, 3), (16, 16, 16, 3, 1), (9, 40, 2, 4, 7), (31, 31, 16, 2, 2)])
def test_patch_pixels_are_in_image_windows_in_row_major_order(H, W, P, n, stride):
    from nerf_few_shot_limitations_amd.ray_sampler import patch_pixels
    g = torch.Generator().manual_seed(5)
    ids = patch_pixels(H, W, P, n, generator=g, stride=stride)
    assert ids.dtype == torch.int64 and ids.shape == (n * P * P,)
    assert int(ids.min()) >= 0 and int(ids.max()) < H * W
    y, x = (ids // W).reshape(n, P, P), (ids % W).reshape(n, P, P)
    k = torch.arange(P) * stride
    assert torch.equal(y, (y[:, :1, :1] + k[None, :, None]).expand(n, P, P)) and torch.equal(x, (x[:, :1, :1] + k[None, None, :]).expand(n, P, P))
    assert int(y.max()) < H and int(x.max()) < W
    again = patch_pixels(H, W, P, n, generator=torch.Generator().manual_seed(5), stride=stride)
    other = patch_pixels(H, W, P, 64, generator=torch.Generator().manual_seed(6), stride=stride)
    assert torch.equal(ids, again)
    if (P - 1) * stride + 1 < min(H, W):
        assert len({int(v) for v in other.reshape(64, -1)[:, 0]}) > 1            # the windows move
    with pytest.raises(ValueError):
        patch_pixels(8, 8, 8, 1, stride=2)
    with pytest.raises(ValueError):
        patch_pixels(8, 8, 1, 1)


def _train_poses(V=5, seed=3):
    """Cameras on a sphere of radius about 4 in the upper half space, looking at the origin (the blender scenes' layout)."""
    g = torch.Generator().manual_seed(seed)
    th, ph = torch.rand(V, generator=g) * 2.0 + 0.3, torch.rand(V, generator=g) * 0.8 + 0.3
    r = 4.0 + 0.2 * torch.rand(V, generator=g)
    c = torch.stack([r * torch.cos(th) * torch.cos(ph), r * torch.sin(th) * torch.cos(ph), r * torch.sin(ph)], dim=1)
    z = c / c.norm(dim=1, keepdim=True)
    x = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]).expand(V, 3), z)
    x = x / x.norm(dim=1, keepdim=True)
    y = torch.linalg.cross(z, x)
    out = torch.eye(4).repeat(V, 1, 1)
    out[:, :3, 0], out[:, :3, 1], out[:, :3, 2], out[:, :3, 3] = x, y, z, c
    return out


@pytest.mark.parametrize("jitter", [0.0, 0.125])
def test_sampled_patch_poses_are_cameras_at_the_training_radius_looking_at_the_focus(jitter):
    from nerf_few_shot_limitations_amd.ray_sampler import sample_patch_poses
    tp = _train_poses()
    n = 64
    poses = sample_patch_poses(tp, n, generator=torch.Generator().manual_seed(11), focus_jitter=jitter)
    assert poses.shape == (n, 4, 4) and poses.dtype == torch.float32
    assert torch.equal(poses, sample_patch_poses(tp, n, generator=torch.Generator().manual_seed(11), focus_jitter=jitter))
    R, c = poses[:, :3, :3].double(), poses[:, :3, 3].double()
    assert (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6
    assert (torch.linalg.det(R) - 1.0).abs().max() < 1e-6
    assert torch.equal(poses[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(n, 4))
    # at the training cameras' mean radius, and in a direction the bounding box of their positions subtends: some s > 0 with s c in the box
    pos = tp[:, :3, 3].double()
    assert (c.norm(dim=1) - pos.norm(dim=1).mean()).abs().max() < 1e-5
    lo, hi = pos.amin(dim=0), pos.amax(dim=0)
    s_lo, s_hi = torch.zeros(n, dtype=torch.float64), torch.full((n,), float("inf"), dtype=torch.float64)
    for k in range(3):
        a, b = lo[k] / c[:, k], hi[k] / c[:, k]
        s_lo, s_hi = torch.maximum(s_lo, torch.minimum(a, b)), torch.minimum(s_hi, torch.maximum(a, b))
    assert torch.all(s_lo <= s_hi * (1 + 1e-6))
    assert c.std(dim=0).max() > 0.05                                           # they are not one pose
    # the up vector: the camera's y axis leans towards the mean training up
    up = tp[:, :3, 1].double().mean(dim=0)
    assert torch.all(R[:, :, 1] @ up > 0)
    # the centre ray of get_rays' formula -- R (0, 0, -1) at pixel (W/2, H/2) -- points at the focus
    centre = -R[:, :, 2]
    to_origin = -c / c.norm(dim=1, keepdim=True)
    # (atan2 of cross and dot: acos cannot resolve angles below 3e-4 in numbers that were rounded to float32)
    ang = torch.atan2(torch.linalg.cross(centre, to_origin).norm(dim=1), (centre * to_origin).sum(dim=1))
    if jitter == 0.0:
        assert ang.max() < 1e-5
    else:
        # the focus is N(0, jitter^2) per axis: its offset seen from the camera is below 6 sigma sqrt(3) / radius
        assert 1e-4 < ang.max() < 6.0 * jitter * math.sqrt(3.0) / 3.5
    with pytest.raises(ValueError):
        sample_patch_poses(torch.zeros(4, 4), 2)


def test_patch_rays_follow_get_rays_formula_on_the_cpu():
    """One patch per pose, the batch layout, get_rays' arithmetic written out (the GPU test holds it to the kernel's rays)."""
    from nerf_few_shot_limitations_amd.ray_sampler import patch_pixels, patch_rays, sample_patch_poses
    H, W, focal, P, n = 20, 30, 25.0, 4, 3
    poses = sample_patch_poses(_train_poses(), n, generator=torch.Generator().manual_seed(2))
    o, d = patch_rays(H, W, focal, poses, P, generator=torch.Generator().manual_seed(9), stride=2)
    ids = patch_pixels(H, W, P, n, generator=torch.Generator().manual_seed(9), stride=2).reshape(n, P * P)
    assert o.shape == d.shape == (n * P * P, 3)
    for p in range(n):
        x, y = (ids[p] % W).float(), (ids[p] // W).float()
        cam = torch.stack([(x - W * 0.5) / focal, -(y - H * 0.5) / focal, -torch.ones_like(x)], dim=-1)
        want = cam @ poses[p, :3, :3].t()
        assert (d[p * P * P:(p + 1) * P * P] - want).abs().max() < 1e-6
        assert torch.equal(o[p * P * P:(p + 1) * P * P], poses[p, :3, 3].expand(P * P, 3))


# ---------------------------------------------------------------------------------------------
# the new unit's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from nerf_few_shot_limitations_amd import build as B
    sub = os.path.join(B.OBJ, B.PATCH_REG_DIR)
    if not os.path.isdir(sub) or not any(f.endswith(".o.remarks") for f in os.listdir(sub)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B


NEW = ("patch_loss_backward_kernel<false, false>", "patch_loss_backward_kernel<false, true>", "patch_loss_backward_kernel<true, false>",
       "patch_loss_backward_kernel<true, true>", "patch_terms_finish_kernel")


def test_new_kernels_match_their_census_and_spill_nothing(B):
    res = B.kernel_resources(os.path.join(B.OBJ, B.PATCH_REG_DIR))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_patch_reg.json")))
    fields = gold["fields"]
    assert set(res) == set(gold["kernels"]) and len(res) == len(NEW), sorted(res)
    for kernel in NEW:
        (name, r), = [(k, v) for k, v in res.items() if "::" + kernel + "(" in k]
        print(kernel, r)
        assert r["tu"] == "patch_reg"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["agprs"] == 0, (name, r)
        assert [r.get(f, 0) for f in fields] == gold["kernels"][name], (name, dict(zip(fields, gold["kernels"][name])), r)


def test_the_unit_stays_out_of_the_main_census_and_the_pinned_tables(B):
    main = B.kernel_resources()
    assert not any(k.startswith("patch_reg:") or "patch_loss_backward_kernel" in k or "patch_terms_finish_kernel" in k for k in main)
    for table in (B.SOURCES, B.SUBDIR_SOURCES, B.RAY_REG_SOURCES, B.FREQ_MASK_SOURCES):
        assert not any(src == "patch_reg.hip" for src, *_ in table)
    assert [(src, name, sub) for src, name, _, sub in B.PATCH_REG_SOURCES] == [("patch_reg.hip", "patch_reg", B.PATCH_REG_DIR)]
    ray_reg = B.kernel_resources(os.path.join(B.OBJ, B.RAY_REG_DIR))
    assert not any("patch_" in k for k in ray_reg)
