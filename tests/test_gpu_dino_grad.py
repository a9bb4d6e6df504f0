"""GPU tests of the gradient with respect to the DINO features and feature maps (nrf_mlp_backward_dino: csrc/
train_dino_grad_impl.hpp; nrf_project_fetch_backward / nrf_sample_features_backward: csrc/staged_kernels.hip) and of the opt-in
Python surface on top of them (NeRFMLP(dino_grad=True), sample_features_at_points(feature_grad=True), render_rays_train with a
live map, FusedStep(d_dino_out=))."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

MARGIN = 2e-5          # as tests/test_gpu_training.py: samples with a ReLU on its threshold get no incoming gradient
FOCAL = 40.0
POSE = [[1.0, 0.0, 0.0, 0.2], [0.0, 1.0, 0.0, -0.1], [0.0, 0.0, 1.0, -3.0], [0.0, 0.0, 0.0, 1.0]]      # looks down +z from z = -3


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def L(N):
    from nerf_few_shot_limitations_amd import _lib
    return _lib


def make_v3(N, mode, scene="fog", n_layers=8, dino_dim=64, seed=2, dino_grad=True):
    m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=n_layers, use_dino=True, dino_dim=dino_dim, mma_mode=mode,
                  dino_grad=dino_grad)
    p = O.make_weights("v3", seed, scene, n_layers=n_layers, dino_dim=dino_dim)
    m.load_state_dict(p, strict=False)
    return m.cuda().train(), p


def v3_inputs(n, dino_dim=64, seed=25):
    pos = torch.from_numpy(O.uniform01(seed, n * 3).reshape(n, 3) * 4 - 2).float()
    dirs = torch.from_numpy(O.uniform01(seed + 1, n * 3).reshape(n, 3) - 0.5).float()
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    g_rgb = torch.from_numpy(O.uniform01(seed + 2, n * 3).reshape(n, 3) - 0.5).float()
    g_den = torch.from_numpy(O.uniform01(seed + 3, n).reshape(n, 1) - 0.5).float()
    dino = torch.from_numpy(O.uniform01(seed + 9, n * dino_dim).reshape(n, dino_dim) * 2 - 1).float()
    return pos, dirs, dino, g_rgb, g_den


def rel_to_max(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cosine(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-300))


def d_dino_of(model, pos, dirs, dino, g_rgb, g_den):
    """dL/d dino through NeRFMLP.forward for L = <rgb, g_rgb> + <density, g_den>, and the parameter gradients."""
    model.zero_grad(set_to_none=True)
    f = dino.cuda().requires_grad_(True)
    rgb, den = model(pos.cuda(), dirs.cuda(), f)
    ((rgb * g_rgb.cuda()).sum() + (den * g_den.cuda()).sum()).backward()
    return f.grad.detach().clone(), {k: q.grad.detach().clone() for k, q in model.named_parameters() if q.grad is not None}


# ---------------------------------------------------------------------------------------------
# the raw fetch adjoints
# ---------------------------------------------------------------------------------------------
def points_2d(n, seed, off_map=0.3):
    """normalised image points, a share of them outside [-1, 1] (zeros padding), some exactly on the border"""
    xy = torch.from_numpy(O.uniform01(seed, n * 2).reshape(n, 2)).float() * 2 - 1
    k = int(n * off_map)
    xy[:k] = xy[:k] * 1.6
    if n > 8:
        xy[-1] = torch.tensor([1.0, -1.0]); xy[-2] = torch.tensor([-1.0, 0.3])
    return xy


def points_3d(n, seed):
    """world points around the origin: most in front of POSE's camera, some behind it (z < -3) and some far off axis"""
    p = torch.from_numpy(O.uniform01(seed, n * 3).reshape(n, 3)).float() * 4 - 2
    p[: n // 10, 2] -= 4.0
    p[n // 10: n // 5, 0] *= 6.0
    return p


def dino_struct(L, Hp, Wp, Cc, features=None, H=128, W=128, focal=FOCAL):
    inv = torch.inverse(torch.tensor(POSE))
    return L.nrf_dino(None if features is None else features.data_ptr(), Hp, Wp, Cc, (C.c_float * 16)(*inv.reshape(-1).tolist()), focal, H, W)


def fetch(L, fmap, pts):
    n, (_, Hp, Wp, Cc) = pts.shape[0], fmap.shape
    out = torch.empty((n, Cc), dtype=torch.float32, device="cuda")
    if pts.shape[1] == 2:
        L.check(L.lib().nrf_sample_features(L.ptr(fmap), Hp, Wp, Cc, L.ptr(pts), n, L.ptr(out), L.stream_ptr()))
    else:
        d = dino_struct(L, Hp, Wp, Cc, fmap)
        L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(pts), n, L.ptr(out), None, L.stream_ptr()))
    return out


def fetch_T(L, shape, pts, g, d_map=None, accumulate=0):
    _, Hp, Wp, Cc = shape
    n = pts.shape[0]
    nbytes = L.lib().nrf_fetch_backward_workspace_bytes(Hp, Wp, Cc, n)
    assert nbytes >= Hp * Wp * Cc * 4
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    if d_map is None:
        d_map = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")        # accumulate = 0 must overwrite
    if pts.shape[1] == 2:
        L.check(L.lib().nrf_sample_features_backward(Hp, Wp, Cc, L.ptr(pts), n, L.ptr(g), L.ptr(d_map), accumulate, L.ptr(ws), nbytes, L.stream_ptr()))
    else:
        d = dino_struct(L, Hp, Wp, Cc)
        L.check(L.lib().nrf_project_fetch_backward(C.byref(d), L.ptr(pts), n, L.ptr(g), L.ptr(d_map), accumulate, L.ptr(ws), nbytes, L.stream_ptr()))
    return d_map


SIZES = [(9, 9, 64), (9, 9, 128), (14, 22, 64), (37, 37, 128)]      # the reference's maps, a non-square one, one larger than LDS


@pytest.mark.parametrize("kind", ["points2d", "world"])
@pytest.mark.parametrize("Hp,Wp,Cc", SIZES)
def test_fetch_backward_is_the_adjoint_of_the_fetch(L, Hp, Wp, Cc, kind):
    """<fetch(m), g> = <m, fetch^T(g)> with the EXISTING forward kernels, and element-wise against autograd through the oracle.
    Bound of the identity: every product is one rounding, a texel element's sum runs over at most 256 additions inside a slab
    (64 samples x 4 taps) and 1024 slabs: (256 + 1024) * 2^-24 = 7.7e-5 of the sum of the terms' magnitudes -> 1e-4."""
    n = 5000 + 37                                                # not a multiple of any slab size
    pts = (points_2d(n, 61) if kind == "points2d" else points_3d(n, 62)).cuda()
    m = torch.from_numpy(O.uniform01(63, Hp * Wp * Cc).reshape(1, Hp, Wp, Cc) * 2 - 1).float().cuda()
    g = torch.from_numpy(O.uniform01(64, n * Cc).reshape(n, Cc) - 0.5).float().cuda()
    f = fetch(L, m, pts)
    on_map = float((f.abs().sum(-1) > 0).float().mean())
    assert 0.3 < on_map < 0.97, on_map                           # both the taps and the zeros padding are exercised
    d_map = fetch_T(L, m.shape, pts, g)
    assert torch.isfinite(d_map).all()
    lhs = float((f.double() * g.double()).sum())
    rhs = float((m.double() * d_map.double()).sum())
    scale = float((fetch(L, m.abs(), pts).double() * g.abs().double()).sum())
    print(f"adjoint {Hp}x{Wp}x{Cc} {kind}: lhs {lhs:.9g} rhs {rhs:.9g} |diff|/scale {abs(lhs - rhs) / scale:.3g}")
    assert abs(lhs - rhs) <= 1e-4 * scale
    # element-wise: autograd through the oracle's tap-by-tap fetch on the CPU
    mm = m.cpu().clone().requires_grad_(True)
    xy = pts.cpu() if kind == "points2d" else O.project_points_to_image(pts.cpu(), torch.tensor(POSE), FOCAL, 128, 128)[0]
    (O.sample_features_at_points(mm, xy) * g.cpu()).sum().backward()
    err = rel_to_max(d_map, mm.grad)
    print(f"  d_map vs oracle autograd: {err:.3g} of max")
    assert err <= 2e-4
    # accumulate = 1 adds exactly that result onto what d_map holds
    base = torch.from_numpy(O.uniform01(65, Hp * Wp * Cc).reshape(1, Hp, Wp, Cc)).float().cuda()
    acc = fetch_T(L, m.shape, pts, g, d_map=base.clone(), accumulate=1)
    assert torch.equal(acc, base + d_map)


def test_fetch_backward_off_map_points_leave_an_exactly_zero_gradient(L):
    n = 700
    xy = (torch.from_numpy(O.uniform01(66, n * 2).reshape(n, 2)).float() + 1.5).cuda()            # all beyond the border texels' reach
    g = torch.ones((n, 64), dtype=torch.float32, device="cuda")
    assert not fetch_T(L, (1, 9, 9, 64), xy, g).any()
    behind = torch.tensor([[0.0, 0.0, -50.0]] * 40).cuda() + torch.from_numpy(O.uniform01(67, 120).reshape(40, 3)).float().cuda() * 40 - 20
    d = fetch_T(L, (1, 9, 9, 64), behind, g[:40].contiguous())
    assert torch.equal(d, fetch_T(L, (1, 9, 9, 64), behind, g[:40].contiguous())) and torch.isfinite(d).all()
    # n == 0: accumulate = 0 clears, accumulate = 1 leaves the map alone
    none = torch.empty((0, 2), device="cuda")
    assert not fetch_T(L, (1, 9, 9, 64), none, torch.empty((0, 64), device="cuda")).any()
    keep = torch.ones((1, 9, 9, 64), device="cuda")
    assert torch.equal(fetch_T(L, (1, 9, 9, 64), none, torch.empty((0, 64), device="cuda"), d_map=keep.clone(), accumulate=1), keep)


@pytest.mark.parametrize("Hp,Wp,Cc", [(9, 9, 64), (37, 37, 128), (5, 7, 3), (2, 2, 300)])
def test_fetch_backward_is_bit_reproducible_and_takes_any_size(L, Hp, Wp, Cc):
    n = 20011
    pts = points_3d(n, 71).cuda()
    g = torch.from_numpy(O.uniform01(72, n * Cc).reshape(n, Cc) - 0.5).float().cuda()
    a = fetch_T(L, (1, Hp, Wp, Cc), pts, g)
    b = fetch_T(L, (1, Hp, Wp, Cc), pts, g)
    assert torch.equal(a, b) and a.abs().max() > 0
    m = torch.from_numpy(O.uniform01(73, Hp * Wp * Cc).reshape(1, Hp, Wp, Cc)).float().cuda()
    lhs, rhs = float((fetch(L, m, pts).double() * g.double()).sum()), float((m.double() * a.double()).sum())
    scale = float((fetch(L, m, pts).double() * g.abs().double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("n", [1, 31, 33])
def test_fetch_backward_tiny_batches(L, n):
    xy = points_2d(n, 74, off_map=0.0).cuda() * 0.9
    g = torch.from_numpy(O.uniform01(75, n * 64).reshape(n, 64) - 0.5).float().cuda()
    mm = torch.zeros((1, 9, 9, 64), requires_grad=True)
    (O.sample_features_at_points(mm, xy.cpu()) * g.cpu()).sum().backward()
    assert rel_to_max(fetch_T(L, (1, 9, 9, 64), xy, g), mm.grad) <= 2e-4


def test_fetch_backward_nan_stays_in_the_texels_its_taps_touch(L):
    n, Hp, Wp, Cc = 999, 9, 9, 64
    xy = (points_2d(n, 76, off_map=0.0) * 0.8).cuda()
    g = torch.from_numpy(O.uniform01(77, n * Cc).reshape(n, Cc) - 0.5).float().cuda()
    for j, bad in ((123, float("nan")), (777, float("inf"))):
        gg = g.clone()
        gg[j] = bad
        d = fetch_T(L, (1, Hp, Wp, Cc), xy, gg)[0]
        gx = ((xy[j, 0].item() + 1) * Wp - 1) / 2
        gy = ((xy[j, 1].item() + 1) * Hp - 1) / 2
        taps = {(int(np.floor(gy)) + dy, int(np.floor(gx)) + dx) for dy in (0, 1) for dx in (0, 1)}
        hit = {(int(y), int(x)) for y, x in (~torch.isfinite(d).all(-1)).nonzero().tolist()}
        assert hit and hit <= taps, (hit, taps)
        clean = fetch_T(L, (1, Hp, Wp, Cc), xy, g)[0]
        ok = torch.isfinite(d).all(-1)
        assert torch.equal(d[ok], clean[ok])                     # every other texel: the very same additions


# ---------------------------------------------------------------------------------------------
# dino_grad_kernel through NeRFMLP.forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_layers,dino_dim", [(1000, 8, 64), (300, 8, 128), (1, 3, 64), (31, 3, 64), (33, 3, 128), (4096 + 17, 2, 64)])
def test_feature_gradient_fp32_mode_matches_autograd(N, n, n_layers, dino_dim):
    """fp32 mode against torch autograd through the oracle network, to the bar the parameter gradients of the same chain are held
    to (tests/test_gpu_training.py: 2e-4 of the largest element); the parameter gradients of the same backward are checked too."""
    model, p = make_v3(N, "f32", scene="solid", n_layers=n_layers, dino_dim=dino_dim)
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n, dino_dim)
    keep = (O.relu_margin(p, "v3", pos, dirs, dino) > MARGIN)[:, None]
    g_rgb, g_den = g_rgb * keep, g_den * keep
    d_dino, grads = d_dino_of(model, pos, dirs, dino, g_rgb, g_den)
    pp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    f = dino.clone().requires_grad_(True)
    o_rgb, o_den = O.mlp_v3(pp, pos, dirs, f)
    ((o_rgb * g_rgb).sum() + (o_den * g_den).sum()).backward()
    if f.grad.abs().max() == 0:
        assert not d_dino.any()
        return
    err = rel_to_max(d_dino, f.grad)
    print(f"d_dino n={n} C={dino_dim}: {err:.3g} of max {float(f.grad.abs().max()):.3g}")
    assert err <= 2e-4
    for name, q in grads.items():
        if name in pp:
            assert rel_to_max(q, pp[name].grad) < 2e-4, name


@pytest.mark.parametrize("mode,cos_min", [("bf16", 0.97), ("f16", 0.995)])
@pytest.mark.parametrize("dino_dim", [64, 128])
def test_feature_and_map_gradients_16bit_modes_vs_fp32_mode(N, L, mode, cos_min, dino_dim):
    """The 16-bit modes against the fp32-mode result of the same inputs, at the project's bars for 16-bit gradients
    (test_v2_gradients_16bit_modes_vs_fp32_autograd: 0.97 bf16, 0.995 f16), for d_feats and for the d_map scattered from it."""
    n = 3000
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n, dino_dim, seed=35)
    xy = points_2d(n, 36).cuda()
    out = {}
    for md in ("f32", mode):
        model, _ = make_v3(N, md, dino_dim=dino_dim)
        d_dino, _ = d_dino_of(model, pos, dirs, dino, g_rgb, g_den)
        out[md] = (d_dino, fetch_T(L, (1, 9, 9, dino_dim), xy, d_dino))
    c_f, c_m = cosine(out[mode][0], out["f32"][0]), cosine(out[mode][1], out["f32"][1])
    print(f"{mode} C={dino_dim}: cosine d_feats {c_f:.5f}  d_map {c_m:.5f}")
    assert c_f > cos_min and c_m > cos_min, (c_f, c_m)


@pytest.mark.parametrize("mode,n", [("f32", 3000), ("bf16", 3000), ("bf16", 40000)])      # 40000 samples: the 8-wave chain geometry
def test_feature_gradient_is_bit_reproducible_in_every_geometry(N, mode, n):
    model, _ = make_v3(N, mode, n_layers=3)
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n, 64, seed=45)
    a, ga = d_dino_of(model, pos, dirs, dino, g_rgb, g_den)
    b, gb = d_dino_of(model, pos, dirs, dino, g_rgb, g_den)
    assert torch.equal(a, b) and a.abs().max() > 0 and torch.isfinite(a).all()
    if n == 40000:                                               # and it is the same function as the 4-wave geometry's
        ref_model, _ = make_v3(N, "f32", n_layers=3)
        r, _ = d_dino_of(ref_model, pos, dirs, dino, g_rgb, g_den)
        assert cosine(a, r) > 0.97
        head, _ = d_dino_of(model, pos[:3000], dirs[:3000], dino[:3000], g_rgb[:3000], g_den[:3000])
        assert torch.equal(head, a[:3000])                       # a sample's gradient does not depend on the batch around it


def test_parameter_gradients_do_not_depend_on_the_switch(N):
    pos, dirs, dino, g_rgb, g_den = v3_inputs(2000, 64, seed=55)
    on, _ = make_v3(N, "bf16", n_layers=3, dino_grad=True)
    off, _ = make_v3(N, "bf16", n_layers=3, dino_grad=False)
    _, g_on = d_dino_of(on, pos, dirs, dino, g_rgb, g_den)
    rgb, den = off(pos.cuda(), dirs.cuda(), dino.cuda())
    ((rgb * g_rgb.cuda()).sum() + (den * g_den.cuda()).sum()).backward()
    for name, q in off.named_parameters():
        assert torch.equal(q.grad, g_on[name]), name
    with pytest.raises(NotImplementedError, match="dino_grad"):
        off(pos.cuda(), dirs.cuda(), dino.cuda().requires_grad_(True))
    # features that do not require grad: no extra launch, no gradient
    f = dino.cuda()
    on.zero_grad(set_to_none=True)
    rgb, den = on(pos.cuda(), dirs.cuda(), f)
    rgb.sum().backward()
    assert f.grad is None


# ---------------------------------------------------------------------------------------------
# the three routes to d_map
# ---------------------------------------------------------------------------------------------
def ray_batch(R, S, seed=81):
    o = torch.tensor(POSE)[:3, 3].expand(R, 3).contiguous()
    d = torch.from_numpy(O.uniform01(seed, R * 3).reshape(R, 3)).float() - 0.5
    d[:, 2] = 1.0
    z = torch.sort(torch.from_numpy(O.uniform01(seed + 1, R * S).reshape(R, S) * 4 + 1).float(), dim=-1).values
    tgt = torch.from_numpy(O.uniform01(seed + 2, R * 3).reshape(R, 3)).float()
    return o.cuda(), d.cuda(), z.cuda(), tgt.cuda()


@pytest.mark.parametrize("dino_dim", [64, 128])
def test_three_routes_give_the_same_map_gradient(N, L, dino_dim):
    """autograd through NeRFMLP(dino_grad=True).forward behind sample_features_at_points(feature_grad=True), render_rays_train with
    a live map, and FusedStep(d_dino_out=) + project_fetch_backward: same kernels, same d_map (1e-5 of its largest element, the
    relative bar test_fused_step_equals_autograd_route holds the routes' losses to)."""
    from nerf_few_shot_limitations_amd import dino_features as DF
    from nerf_few_shot_limitations_amd.training import FusedStep, project_fetch_backward, render_rays_train
    R, S = 96, 16
    o, d, z, tgt = ray_batch(R, S)
    fmap = torch.from_numpy(O.uniform01(84, 81 * dino_dim).reshape(1, 9, 9, dino_dim) * 2 - 1).float().cuda()
    cam = dict(pose=torch.tensor(POSE), focal=FOCAL, H=128, W=128)
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    dirs = d[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    seed = 4 if dino_dim == 128 else 2
    vr = N.VolumeRenderer()

    a, _ = make_v3(N, "f32", scene="solid", dino_dim=dino_dim, seed=seed, n_layers=3)
    ma = fmap.clone().requires_grad_(True)
    xy = DF.project_points_to_image(pts, cam["pose"], cam["focal"], cam["H"], cam["W"])[0]
    feats = DF.sample_features_at_points(ma, xy, feature_grad=True)
    assert feats.requires_grad and float((feats.detach().abs().sum(-1) > 0).float().mean()) > 0.5
    rgb, den = a(pts, dirs, feats)
    loss_a = torch.nn.functional.mse_loss(vr(rgb.view(R, S, 3), den.view(R, S, 1), z, d)[0], tgt)
    loss_a.backward()

    b, _ = make_v3(N, "f32", scene="solid", dino_dim=dino_dim, seed=seed, n_layers=3)
    mb = fmap.clone().requires_grad_(True)
    out = render_rays_train(b, o, d, 1.0, 5.0, S, z_in=z, dino=dict(features=mb, **cam))
    loss_b = torch.nn.functional.mse_loss(out["rgb"], tgt)
    loss_b.backward()

    c, _ = make_v3(N, "f32", scene="solid", dino_dim=dino_dim, seed=seed, n_layers=3)
    c2, _ = make_v3(N, "f32", scene="solid", dino_dim=dino_dim, seed=seed, n_layers=3)
    d_feats = torch.full((R * S, dino_dim), float("nan"), device="cuda")
    loss_c = FusedStep(c, lr=5e-4)(pts, z, d, tgt, dirs=dirs, dino=feats.detach(), d_dino_out=d_feats)
    loss_c2 = FusedStep(c2, lr=5e-4)(pts, z, d, tgt, dirs=dirs, dino=feats.detach())
    mc = project_fetch_backward(dict(features=fmap, **cam), pts, d_feats, torch.zeros_like(fmap), accumulate=True)

    top = float(ma.grad.abs().max())
    e_b, e_c = float((mb.grad - ma.grad).abs().max()) / top, float((mc - ma.grad).abs().max()) / top
    print(f"C={dino_dim}: losses {loss_a.item():.8g} {loss_b.item():.8g} {loss_c.item():.8g}; max|d_map| {top:.3g}; route errors {e_b:.3g} {e_c:.3g}")
    assert top > 0 and e_b <= 1e-5 and e_c <= 1e-5
    # the feature adds a launch, it changes none: loss and updated parameters of the fused step are bit-identical with and without
    assert torch.equal(loss_c, loss_c2)
    for (name, p), q in zip(c.named_parameters(), c2.parameters()):
        assert torch.equal(p, q), name
    # ... and so are the parameter gradients of the two autograd routes
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert rel_to_max(p.grad, q.grad) <= 1e-5, name
    # default modules keep refusing a live map
    off, _ = make_v3(N, "f32", scene="solid", dino_dim=dino_dim, seed=seed, n_layers=3, dino_grad=False)
    with pytest.raises(NotImplementedError, match="dino_grad"):
        render_rays_train(off, o, d, 1.0, 5.0, S, z_in=z, dino=dict(features=fmap.clone().requires_grad_(True), **cam))
    with pytest.raises(ValueError):
        FusedStep(off, lr=5e-4)(pts, z, d, tgt, dirs=dirs, dino=feats.detach(), d_dino_out=d_feats)


def test_sample_features_default_is_detached_and_batched_maps_get_their_own_gradient(N):
    from nerf_few_shot_limitations_amd import dino_features as DF
    n = 500
    xy = points_2d(n, 91).cuda()
    m = torch.from_numpy(O.uniform01(92, 2 * 81 * 64).reshape(2, 9, 9, 64)).float().cuda().requires_grad_(True)
    assert not DF.sample_features_at_points(m, xy).requires_grad                      # today's read
    out = DF.sample_features_at_points(m, xy, feature_grad=True)
    assert out.shape == (2, n, 64)
    g = torch.from_numpy(O.uniform01(93, 2 * n * 64).reshape(2, n, 64) - 0.5).float()
    (out * g.cuda()).sum().backward()
    for b in range(2):
        mm = m[b:b + 1].detach().cpu().clone().requires_grad_(True)
        (O.sample_features_at_points(mm, xy.cpu()) * g[b]).sum().backward()
        assert rel_to_max(m.grad[b], mm.grad[0]) <= 2e-4
    from nerf_few_shot_limitations_amd import dino_feature_model as M
    assert M.SpatialDINOFeatures.feature_grad is False and M.MultiScaleDINOFeatures.feature_grad is False


# ---------------------------------------------------------------------------------------------
# golden: loss.backward() of the reference's own modules with a feature map that requires grad
# (tests/golden/make_golden_dino_grad.py)
# ---------------------------------------------------------------------------------------------
def thin(t):
    return t[::8] if t.ndim == 2 and t.numel() > 20000 else t


def test_map_gradient_matches_reference_golden(N, golden):
    """fp32 mode against the reference's project_points_to_image -> sample_features_at_points (F.grid_sample) -> NeRFWithDINO ->
    VolumeRenderer -> mse_loss -> backward(): loss to 1e-5 relative, d_feats and d_map to 2e-4 of the reference's largest element
    -- the bar test_v3_backward_matches_reference_golden holds the parameter gradients to -- and the stored parameter gradients
    to the same bar (the new route leaves them alone)."""
    from nerf_few_shot_limitations_amd import dino_features as DF
    g = golden("dino_grads")
    R, S = g["z"].shape
    model = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=3, use_dino=True, dino_dim=64, mma_mode="f32", dino_grad=True)
    model.load_state_dict(O.make_weights("v3", 1, "solid", n_layers=3), strict=False)
    model = model.cuda().train()
    fmap = torch.from_numpy(g["fmap"]).cuda().requires_grad_(True)
    pts = torch.from_numpy(g["pts"]).reshape(-1, 3).cuda()
    xy = DF.project_points_to_image(pts, torch.from_numpy(g["pose"]), float(g["focal"]), int(g["H"]), int(g["W"]))[0]
    feats = DF.sample_features_at_points(fmap, xy, feature_grad=True)
    feats.retain_grad()
    rgb, den = model(pts, torch.from_numpy(g["dirs"]).reshape(-1, 3).cuda(), feats)
    rgb_map = N.VolumeRenderer()(rgb.reshape(R, S, 3), den.reshape(R, S, 1), torch.from_numpy(g["z"]).cuda(), torch.from_numpy(g["rays_d"]).cuda())[0]
    loss = torch.nn.functional.mse_loss(rgb_map, torch.from_numpy(g["target"]).cuda())
    loss.backward()
    e_loss = abs(loss.item() - float(g["loss"])) / float(g["loss"])
    e_feats = np.abs(feats.grad.cpu().numpy() - g["d_feats"]).max() / np.abs(g["d_feats"]).max()
    e_map = np.abs(fmap.grad.cpu().numpy() - g["d_map"]).max() / np.abs(g["d_map"]).max()
    print(f"golden: loss {e_loss:.3g} rel, d_feats {e_feats:.3g}, d_map {e_map:.3g} of the reference's largest element")
    assert e_loss < 1e-5 and e_feats <= 2e-4 and e_map <= 2e-4
    checked = 0
    for name, q in model.named_parameters():
        if "grad_" + name in g:
            ref = g["grad_" + name]
            assert np.abs(thin(q.grad).cpu().numpy() - ref).max() <= 2e-4 * np.abs(ref).max(), name
            checked += 1
    assert checked == 13 + 5                                     # every bias, five weights


# ---------------------------------------------------------------------------------------------
# it trains: train_cli's --train-extractor loop on a tiny random-init extractor
# ---------------------------------------------------------------------------------------------
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, image_size=56, patch_size=14)
TRAIN_CFG = {"training": {"batch_size": 196, "progressive_schedule": {"epochs_0_50": [28, 28, 16], "epochs_50_100": [28, 28, 16],
                                                                      "epochs_100_plus": [28, 28, 16]}}}


def _synthetic_scene(root, size, n_train):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "synthetic_scene.py")
    spec = importlib.util.spec_from_file_location("synthetic_scene", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.write_scene(root, size=size, n_train=n_train, n_test=1)


def _extractor_run(N, root, train_extractor, epochs=10):
    import warnings
    from nerf_few_shot_limitations_amd import config, dino_feature_model as F, train_cli
    from nerf_few_shot_limitations_amd.training import FusedStep
    dev = torch.device("cuda")
    images, poses, (H, W, focal) = N.load_blender_data(root, "train", img_size=56)
    images = [im.permute(1, 2, 0).float().to(dev) for im in images]
    poses = [p.float() for p in poses]
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ext = F.SpatialDINOFeatures(None, use_lora=True, lora_rank=4, lora_alpha=8, image_size=56, pos_embed_dim=8, config=TINY).to(dev)
    stack = torch.stack(images)[..., :3]
    maps0 = config.precompute_dino_features(ext, stack).float()
    model, _ = make_v3(N, "f32", scene="fog", dino_grad=train_extractor)
    step = FusedStep(model, lr=1e-3)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    tr = train_cli.ExtractorTrainer(ext, stack, lr=2e-3, weight_decay=0.0) if train_extractor else None
    before = {n: p.detach().clone() for n, p in ext.named_parameters()}
    losses = [train_cli.train_epoch(step, TRAIN_CFG, e, images, poses, H, W, focal, 2.0, 6.0, gen, maps0, extractor=tr)[0] for e in range(epochs)]
    maps1 = config.precompute_dino_features(ext, stack).float()
    return losses, ext, before, maps0, maps1, tr


def test_train_extractor_loop_trains_the_lora_matrices(N, tmp_path):
    """A few dozen steps of train_cli's loop (train_epoch with an ExtractorTrainer) on two views of the synthetic scene: every
    lora_B leaves zero, the views' maps move, nothing else of the extractor does, the losses are finite and the last epoch's is
    below the first's.  The frozen-extractor run of the same seed is printed next to it, not asserted."""
    root = str(tmp_path / "scene")
    _synthetic_scene(root, 56, 2)
    losses, ext, before, maps0, maps1, tr = _extractor_run(N, root, True)
    frozen = _extractor_run(N, root, False)[0]
    print("epoch losses, extractor trained:", [round(x, 6) for x in losses])
    print("epoch losses, extractor frozen :", [round(x, 6) for x in frozen])
    assert tr.steps == 2 * len(losses)                          # one extractor step per view and epoch
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    for n, p in ext.named_parameters():
        if "lora_B" in n:
            assert p.detach().abs().max() > 0, n
        if "lora" not in n:
            assert torch.equal(p.detach(), before[n]), n
    assert not torch.equal(maps0, maps1) and torch.isfinite(maps1).all()
