"""The training forward that takes rays (nrf_mlp_forward_train_rays, FusedStep.step_rays / step_view, train_cli --fused-inputs)
against the staged route it stands in for: sample_points_along_rays + expanded directions + project/fetch + encodings in front
of nrf_mlp_forward_train*.

What is derivable is held to the bit: depths, points and directions come from the same explicitly rounded device functions as
the staged kernels', and the V2 kernel differs from its staged sibling only in where its six input floats come from.  V3's
fetch is a different kernel (staged_kernels.hip:project_fetch_kernel vs the renderer's nets.hpp:dino_taps / DinoRaw), but both
run the same rounded multiply-adds in the same tap order (the build compiles with -ffp-contract=off), so V3 is held to the bit
too: here on the outputs and on the parameters after every one of five steps, and slot by slot, plane by plane in
tests/test_gpu_train_rays_link.py.  V1's staged route takes an encoding from torch where the kernel runs nets.hpp:encode3, so
against THAT staged input V1 keeps the bounds the existing tests hold the staged route itself to (section 3 below); the bit-level
tie of V1 -- the staged chain on the ray route's own saved encoding, and that encoding against the float64 one -- is
tests/test_gpu_train_rays_link.py, section 2."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_dino_grad import thin                    # tests/golden/dino_grads.npz stores every 8th row of the large matrices
from tests.test_gpu_training import _CFG, _write_scene, cosine, make_model, make_v2, make_v3, named_grads, rel_to_max

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
CANARY = -777.25
# (R, S): every S of the reference's schedules, R*S on both sides of the 4/8-wave switch (32768 samples on 256 CUs), never a
# multiple of 256 -- the last workgroup tile is padded
SHAPES = [(1000, 1), (40001, 1), (333, 8), (4100, 8), (100, 32), (1031, 32), (77, 48), (700, 48), (50, 64), (515, 64)]


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def u01(seed, *shape):
    return torch.from_numpy(O.uniform01(seed, int(np.prod(shape))).reshape(shape)).float()


def ray_batch(R, seed=50):
    """Rays from around the origin, directions of length 0.5 .. 1.5 (not unit: |d| enters the compositor)."""
    o = (u01(seed, R, 3) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(u01(seed + 1, R, 3) - 0.5, dim=-1) * (0.5 + u01(seed + 2, R, 1))
    return o, d.cuda().contiguous()


def padded(n_floats, pad=64):
    """A buffer with `pad` canary floats behind the n_floats the kernel may write; returns (whole, view of the first n_floats)."""
    whole = torch.full((n_floats + pad,), CANARY, dtype=torch.float32, device="cuda")
    return whole, whole[:n_floats]


def canaries_intact(whole, n_floats):
    return bool((whole[n_floats:] == CANARY).all())


def forward_rays(model, S, o=None, d=None, pixels=None, cam=None, perturb=False, t_rand=None, seed=0, lindisp=False, z_in=None, dino=None,
                 near=NEAR, far=FAR, points=True, buf=None):
    """One nrf_mlp_forward_train_rays through the C ABI.  Returns a dict: z (R,S), pts (R*S,3), d_out (R,3), a / b (the two outputs),
    buf / nbytes / h / mode / n (the context), and `intact` (canaries behind z, pts and d_out)."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts, make_dino
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    h, mode = _train_handle(model, dev)
    R = int(o.shape[0] if o is not None else pixels.shape[0])
    n = R * S
    zw, z = padded(n)
    pw, pts = padded(3 * n)
    dw, d_out = padded(3 * R)
    dn, keep = make_dino(**dino) if dino is not None else (None, None)
    opts = _opts(near, far, S, perturb, t_rand, seed, lindisp, 0.0, False, L.TRAIN_MODE[model.mma_mode], dn, dev, z_in)
    if pixels is not None:
        from nerf_few_shot_limitations_amd.ray_sampler import _c2w12
        rays = L.train_rays(pixels=pixels.data_ptr(), H=cam["H"], W=cam["W"], focal=cam["focal"], c2w=_c2w12(cam["pose"]), z_vals=L.ptr(z),
                            rays_d_out=L.ptr(d_out), points_out=L.ptr(pts) if points else None)
    else:
        rays = L.train_rays(rays_o=L.ptr(o), rays_d=L.ptr(d), z_vals=L.ptr(z), rays_d_out=L.ptr(d_out), points_out=L.ptr(pts) if points else None)
    nbytes = L.lib().nrf_train_context_bytes(h, mode, n)
    assert nbytes >= 0
    if buf is None:
        buf = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
    v1 = model.net == L.NRF_NET_V1
    a = torch.empty((n, 4 if v1 else 3), device=dev)
    b = None if v1 else torch.empty((n, 1), device=dev)
    L.check(L.lib().nrf_mlp_forward_train_rays(h, C.byref(rays), R, C.byref(opts), L.ptr(a), L.ptr(b), C.c_void_p(buf.data_ptr()), nbytes, L.stream_ptr()))
    torch.cuda.synchronize()
    intact = canaries_intact(zw, n) and canaries_intact(pw, 3 * n) and canaries_intact(dw, 3 * R)
    return dict(z=z.view(R, S), pts=pts.view(n, 3), d_out=d_out.view(R, 3), a=a, b=b, buf=buf, nbytes=nbytes, h=h, mode=mode, n=n, intact=intact)


def backward_v2(model, f, g_rgb, g_den):
    from nerf_few_shot_limitations_amd import _lib as L
    grad = torch.zeros(model.flat_params().flat.numel(), device="cuda")
    L.check(L.lib().nrf_mlp_backward(f["h"], f["mode"], L.ptr(f["a"]), L.ptr(f["b"]), L.ptr(g_rgb), L.ptr(g_den), f["n"], C.c_void_p(f["buf"].data_ptr()),
                                     f["nbytes"], L.ptr(grad), L.stream_ptr()))
    torch.cuda.synchronize()
    return grad


def staged_v2(model, pts, dirs, g_rgb, g_den, dino=None):
    """nrf_mlp_forward_train + nrf_mlp_backward on staged inputs: rgb, density, flat gradient."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    h, mode = _train_handle(model, dev)
    n = pts.shape[0]
    nbytes = L.lib().nrf_train_context_bytes(h, mode, n)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    rgb, den = torch.empty((n, 3), device=dev), torch.empty((n, 1), device=dev)
    ctx = C.c_void_p(buf.data_ptr())
    L.check(L.lib().nrf_mlp_forward_train(h, mode, L.ptr(pts), L.ptr(dirs), L.ptr(dino), n, L.ptr(rgb), L.ptr(den), ctx, nbytes, L.stream_ptr()))
    grad = torch.zeros(model.flat_params().flat.numel(), device=dev)
    L.check(L.lib().nrf_mlp_backward(h, mode, L.ptr(rgb), L.ptr(den), L.ptr(g_rgb), L.ptr(g_den), n, ctx, nbytes, L.ptr(grad), L.stream_ptr()))
    torch.cuda.synchronize()
    return rgb, den, grad


def expand_dirs(d, S):
    return d[:, None, :].expand(d.shape[0], S, 3).reshape(-1, 3).contiguous()


# ---------------------------------------------------------------------------------------------
# 1. depths and points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", SHAPES)
def test_depths_and_points_are_the_staged_samplers(N, R, S):
    model, _ = make_v2(N, "bf16")
    o, d = ray_batch(R)
    tr = u01(60, R, S).cuda()
    z_explicit = torch.sort(u01(61, R, S) * 4 + 2, dim=-1).values.cuda()
    cases = {"plain": dict(perturb=False), "seed": dict(perturb=True, seed=12345 + R), "t_rand": dict(perturb=True, t_rand=tr),
             "lindisp": dict(perturb=False, lindisp=True), "lindisp+seed": dict(perturb=True, lindisp=True, seed=99)}
    for name, kw in cases.items():
        f = forward_rays(model, S, o, d, **kw)
        pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=kw["perturb"], lindisp=kw.get("lindisp", False), t_rand=kw.get("t_rand"),
                                            seed=kw.get("seed"))
        assert torch.equal(f["z"], z), (name, R, S)
        assert torch.equal(f["pts"], pts.reshape(-1, 3)), (name, R, S)
        assert torch.equal(f["d_out"], d) and f["intact"], (name, R, S)
    f = forward_rays(model, S, o, d, z_in=z_explicit)
    assert torch.equal(f["z"], z_explicit) and f["intact"]
    assert torch.equal(f["pts"], (o[:, None, :] + d[:, None, :] * z_explicit[..., None]).reshape(-1, 3))      # ray_utils.py:82: product, then sum


@pytest.mark.parametrize("R,S", [(100, 32), (1031, 32), (515, 64)])
def test_pixel_mode_casts_get_rays_rays(N, R, S):
    model, _ = make_v2(N, "bf16")
    H, W = 40, 56
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    ro, rd = N.get_rays(H, W, focal, pose)
    g = torch.Generator().manual_seed(R)
    pix = torch.randint(0, H * W, (R,), generator=g, dtype=torch.int64).cuda()          # with repeats: the jitter is keyed by the row
    o, d = ro.reshape(-1, 3)[pix].contiguous(), rd.reshape(-1, 3)[pix].contiguous()
    f = forward_rays(model, S, pixels=pix, cam=dict(H=H, W=W, focal=focal, pose=pose), perturb=True, seed=7)
    pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=7)
    assert torch.equal(f["d_out"], d) and torch.equal(f["z"], z) and torch.equal(f["pts"], pts.reshape(-1, 3)) and f["intact"]
    r = forward_rays(model, S, o, d, perturb=True, seed=7)
    assert torch.equal(r["a"], f["a"]) and torch.equal(r["b"], f["b"])


# ---------------------------------------------------------------------------------------------
# 2. V2 is the staged route, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(100, 32), (1031, 32)], ids=["4waves", "8waves"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_v2_forward_and_gradient_equal_the_staged_route(N, mode, R, S):
    model, _ = make_v2(N, mode)
    o, d = ray_batch(R, seed=70)
    n = R * S
    g_rgb, g_den = (u01(71, n, 3) - 0.5).cuda(), (u01(72, n, 1) - 0.5).cuda()
    f = forward_rays(model, S, o, d, perturb=True, seed=4242)
    grad = backward_v2(model, f, g_rgb, g_den)
    pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=4242)
    rgb, den, ref = staged_v2(model, pts.reshape(-1, 3), expand_dirs(d, S), g_rgb, g_den)
    assert torch.equal(f["a"], rgb) and torch.equal(f["b"], den)
    assert torch.equal(grad, ref) and float(ref.abs().max()) > 0
    assert f["intact"]


def _step_pair(N, mode, **step_kw):
    from nerf_few_shot_limitations_amd.training import FusedStep
    a, _ = make_v2(N, mode, scene="solid")
    b, _ = make_v2(N, mode, scene="solid")
    return FusedStep(a, **step_kw), FusedStep(b, **step_kw)


@pytest.mark.parametrize("recipe", ["plain", "multiscale"])
def test_five_step_rays_steps_equal_five_staged_steps(N, recipe):
    kw = dict(lr=5e-4, weight_decay=1e-6)
    if recipe == "multiscale":
        kw.update(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True, seed=31)
    sa, sb = _step_pair(N, "bf16", **kw)
    R, S = 160, 32
    o, d = ray_batch(R, seed=80)
    tgt = u01(83, R, 3).cuda()
    for i in range(5):
        pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=1000 + i)
        la = sa(pts.reshape(-1, 3), z, d, tgt, dirs=expand_dirs(d, S))
        lb = sb.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=1000 + i)
        assert torch.equal(la, lb), i
        assert torch.equal(sb.last_z, z)
        for k in sa.last_losses:
            assert torch.equal(sa.last_losses[k], sb.last_losses[k]), (i, k)
        if recipe == "multiscale":
            assert torch.equal(sa.last_grad_norm, sb.last_grad_norm)
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)
    assert sa.opt.step_count == sb.opt.step_count == 5


def test_step_view_equals_step_rays_on_the_gathered_rays(N):
    sa, sb = _step_pair(N, "bf16", lr=5e-4)
    H, W, R, S = 24, 24, 200, 16
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    image = u01(90, H, W, 3).cuda()
    ro, rd = N.get_rays(H, W, focal, pose)
    for i in range(3):
        pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(i))[:R].cuda()
        la = sa.step_rays(ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix], image.reshape(-1, 3)[pix], NEAR, FAR, S, seed=5 + i)
        lb = sb.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, seed=5 + i)
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z)
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)


# ---------------------------------------------------------------------------------------------
# 3. V1: the kernel encodes (nets.hpp:encode3) where the staged route reads torch's PositionalEncoding
# ---------------------------------------------------------------------------------------------
def test_v1_f32_step_matches_the_staged_route(N):
    """Loss within 1e-5 relative, every parameter gradient within 2e-4 of the staged route's largest element: the bounds
    tests/test_gpu_training.py holds the f32 mode to."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    a, _ = make_model(N, "f32", scene="solid")
    b, _ = make_model(N, "f32", scene="solid")
    sa, sb = FusedStep(a, lr=5e-4), FusedStep(b, lr=5e-4)
    R, S = 150, 32
    o, d = ray_batch(R, seed=100)
    tgt = u01(103, R, 3).cuda()
    pts, z = N.sample_points_along_rays(o, d, 0.5, 2.0, S, perturb=True, seed=3)
    x = O.positional_encoding(pts.reshape(-1, 3).cpu(), 10).cuda()
    la = sa(x, z, d, tgt)
    lb = sb.step_rays(o, d, tgt, 0.5, 2.0, S, perturb=True, seed=3)
    e_loss = abs(la.item() - lb.item()) / abs(la.item())
    worst = max((rel_to_max(gb, ga), name) for (name, ga), gb in zip(named_grads(a, sa.grad).items(), named_grads(b, sb.grad).values()))
    print(f"V1 f32: loss {la.item():.6g} vs {lb.item():.6g} ({e_loss:.3g} rel), worst gradient {worst[0]:.3g} of max ({worst[1]})")
    assert e_loss < 1e-5
    assert worst[0] < 2e-4, worst


@pytest.mark.parametrize("mode,cos_min,R,S", [("bf16", 0.97, 125, 24), ("f16", 0.995, 125, 24), ("bf16", 0.97, 1250, 32)])
def test_v1_16bit_gradients_vs_fp32_autograd(N, mode, cos_min, R, S):
    """The thresholds of test_gradients_16bit_modes_vs_fp32_autograd, on the positions the kernel derived (points_out)."""
    from nerf_few_shot_limitations_amd import _lib as L
    model, p = make_model(N, mode)
    o, d = ray_batch(R, seed=110)
    n = R * S
    f = forward_rays(model, S, o, d, perturb=True, seed=9, near=0.5, far=2.0)
    g = (u01(111, n, 4) - 0.5).cuda()
    grad = torch.zeros(model.flat_params().flat.numel(), device="cuda")
    L.check(L.lib().nrf_mlp_backward_v1(f["h"], f["mode"], L.ptr(f["a"]), L.ptr(g), n, C.c_void_p(f["buf"].data_ptr()), f["nbytes"], L.ptr(grad),
                                        L.stream_ptr()))
    torch.cuda.synchronize()
    pp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    (O.mlp_v1(pp, O.positional_encoding(f["pts"].cpu(), 10)) * g.cpu()).sum().backward()
    for name, gv in named_grads(model, grad).items():
        if name.endswith("weight"):
            c = cosine(gv, pp[name].grad)
            print(mode, n, name, round(c, 5))
            assert c > cos_min, (name, c)


# ---------------------------------------------------------------------------------------------
# 4. V3
# ---------------------------------------------------------------------------------------------
def test_v3_f32_step_matches_the_reference_golden(N, golden):
    """tests/golden/dino_grads.npz (the reference's own loss.backward()) through step_rays with explicit depths: the bounds of
    test_map_gradient_matches_reference_golden."""
    from nerf_few_shot_limitations_amd.training import FusedStep, project_fetch_backward
    g = golden("dino_grads")
    R, S = g["z"].shape
    model = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=3, use_dino=True, dino_dim=64, mma_mode="f32", dino_grad=True)
    model.load_state_dict(O.make_weights("v3", 1, "solid", n_layers=3), strict=False)
    model = model.cuda().train()
    t = lambda k: torch.from_numpy(g[k]).cuda()
    fmap = t("fmap")
    cam = dict(features=fmap, pose=torch.from_numpy(g["pose"]), focal=float(g["focal"]), H=int(g["H"]), W=int(g["W"]))
    step = FusedStep(model, lr=1e-4)
    d_feats = torch.empty((R * S, 64), device="cuda")
    pts = torch.empty((R * S, 3), device="cuda")
    loss = step.step_rays(t("rays_o"), t("rays_d"), t("target"), NEAR, FAR, S, perturb=False, z_in=t("z"), dino=cam, d_dino_out=d_feats, points_out=pts)
    names = {id(q): name for name, q in model.named_parameters()}
    order = [names[id(q)] for q in model.flat_params().params()]
    assert torch.equal(step.last_z, t("z"))
    e_pts = float((pts.cpu() - torch.from_numpy(g["pts"]).reshape(-1, 3)).abs().max())
    e_loss = abs(loss.item() - float(g["loss"])) / float(g["loss"])
    e_pred = float((step.pred.cpu() - torch.from_numpy(g["pred"])).abs().max())
    d_map = project_fetch_backward(cam, pts, d_feats, torch.zeros_like(fmap), accumulate=False)
    e_feats = np.abs(d_feats.cpu().numpy() - g["d_feats"]).max() / np.abs(g["d_feats"]).max()
    e_map = np.abs(d_map.cpu().numpy() - g["d_map"]).max() / np.abs(g["d_map"]).max()
    print(f"golden via step_rays: pts {e_pts:.3g} abs, loss {e_loss:.3g} rel, pred {e_pred:.3g} abs, d_feats {e_feats:.3g}, d_map {e_map:.3g} of max")
    assert e_pts == 0.0
    assert e_loss < 1e-5 and e_pred < 1e-4
    assert e_feats <= 2e-4 and e_map <= 2e-4
    checked = 0
    for name, gv in zip(order, model.flat_params().views(step.grad)):
        if "grad_" + name in g:
            ref = g["grad_" + name]
            err = np.abs(thin(gv).cpu().numpy() - ref).max() / np.abs(ref).max()
            assert err <= 2e-4, (name, err)
            checked += 1
    assert checked == 13 + 5                                     # every bias, five weights


def _v3_scene(dino_dim, R, S):
    """Rays of a 32 x 32 view of the lego-like camera and a feature map seen from a camera beside it: most samples project
    into the map."""
    import nerf_few_shot_limitations_amd as N
    H = W = 32
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    ro, rd = N.get_rays(H, W, focal, pose)
    pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))[:R].cuda()
    src = O.LEGO_LIKE_C2W.copy()
    src[0, 3] += 0.3
    fmap = (u01(120, 1, 9, 9, dino_dim) * 2 - 1).cuda()
    cam = dict(features=fmap, pose=torch.from_numpy(src), focal=focal, H=H, W=W)
    return ro.reshape(-1, 3)[pix].contiguous(), rd.reshape(-1, 3)[pix].contiguous(), cam


@pytest.mark.parametrize("dino_dim", [64, 128])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_v3_16bit_five_steps_follow_the_staged_route(N, mode, dino_dim):
    """Losses to rtol 2e-3 (test_fused_step_equals_autograd_route's bound for the 16-bit modes), the last below the first; the
    parameters of the two routes bit-equal after every step."""
    from nerf_few_shot_limitations_amd import train_cli
    from nerf_few_shot_limitations_amd.renderer import make_dino
    from nerf_few_shot_limitations_amd.training import FusedStep
    seed = 4 if dino_dim == 128 else 2                            # as test_fused_step_equals_autograd_route picks them
    a, _ = make_v3(N, mode, scene="solid", dino_dim=dino_dim, seed=seed)
    b, _ = make_v3(N, mode, scene="solid", dino_dim=dino_dim, seed=seed)
    sa, sb = FusedStep(a, lr=5e-4, weight_decay=1e-6), FusedStep(b, lr=5e-4, weight_decay=1e-6)
    R, S = 160, 32
    o, d, cam = _v3_scene(dino_dim, R, S)
    tgt = u01(123, R, 3).cuda()
    dstruct = make_dino(**cam)
    la, lb, equal = [], [], True
    for i in range(5):
        pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=50 + i)
        feats = train_cli.fetch_features(dstruct, pts.reshape(-1, 3))
        if i == 0:
            assert float((feats.abs().sum(-1) > 0).float().mean()) > 0.5          # the scene does feed the feature branch
        la.append(sa(pts.reshape(-1, 3), z, d, tgt, dirs=expand_dirs(d, S), dino=feats).item())
        lb.append(sb.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=50 + i, dino=cam).item())
        same = torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)
        assert same, f"the parameters of the two routes differ after step {i}: staged losses {la}, rays {lb}"
        equal = equal and same
    print(f"V3 {mode} dino_dim {dino_dim}: staged {la} rays {lb} bit-equal parameters after every step: {equal}")
    assert np.allclose(la, lb, rtol=2e-3, atol=1e-7), (la, lb)
    assert lb[-1] < lb[0]


def test_v3_forward_against_the_staged_fetch_is_reported(N):
    """f32 mode, one forward: rgb / density of the in-kernel gather are torch.equal to the staged fetch + forward (the distance is
    still printed, and the 1e-4 the golden test above holds `pred` to, on rgb, still asserted)."""
    from nerf_few_shot_limitations_amd import train_cli
    from nerf_few_shot_limitations_amd.renderer import make_dino
    model, _ = make_v3(N, "f32", scene="solid")
    R, S = 160, 32
    o, d, cam = _v3_scene(64, R, S)
    f = forward_rays(model, S, o, d, perturb=True, seed=1, dino=cam)
    feats = train_cli.fetch_features(make_dino(**cam), f["pts"])
    g_rgb, g_den = torch.zeros((R * S, 3), device="cuda"), torch.zeros((R * S, 1), device="cuda")
    rgb, den, _ = staged_v2(model, f["pts"], expand_dirs(d, S), g_rgb, g_den, dino=feats)
    print(f"V3 f32 forward, rays vs staged: rgb max abs {float((rgb - f['a']).abs().max()):.3g}, density rel {rel_to_max(f['b'], den):.3g}, "
          f"bit-equal: {torch.equal(rgb, f['a']) and torch.equal(den, f['b'])}")
    assert float((rgb - f["a"]).abs().max()) < 1e-4 and f["intact"]
    assert torch.equal(rgb, f["a"]) and torch.equal(den, f["b"])


# ---------------------------------------------------------------------------------------------
# 5. edges and the refusals that read the model
# ---------------------------------------------------------------------------------------------
def test_empty_batch_and_single_sample(N):
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts
    from nerf_few_shot_limitations_amd.training import _train_handle
    model, _ = make_v2(N, "bf16")
    h, mode = _train_handle(model, torch.device("cuda", 0))
    opts = _opts(NEAR, FAR, 8, False, None, 0, False, 0.0, False, "bf16", None, torch.device("cuda", 0))
    rays = L.train_rays(rays_o=0x1000, rays_d=0x2000, z_vals=0x3000)
    assert L.lib().nrf_mlp_forward_train_rays(h, C.byref(rays), 0, C.byref(opts), None, None, None, 0, L.stream_ptr()) == 0      # R = 0: nothing launched
    o, d = ray_batch(1)
    f = forward_rays(model, 1, o, d)                                                                                             # R * S = 1
    pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, 1, perturb=False)
    assert torch.equal(f["z"], z) and torch.equal(f["pts"], pts.reshape(-1, 3)) and f["intact"]
    rgb, den, _ = staged_v2(model, pts.reshape(-1, 3), d, torch.zeros(1, 3, device="cuda"), torch.zeros(1, 1, device="cuda"))
    assert torch.equal(f["a"], rgb) and torch.equal(f["b"], den)


@pytest.mark.parametrize("net", ["v1", "v2", "v3"])
def test_padded_last_tile_writes_nothing_outside_and_repeats(N, net):
    """R * S = 259 * 5 = 1295: five whole 256-sample groups and a sixth with 15 real samples.  Canaries behind z_vals,
    points_out and rays_d_out stay; two identical calls leave identical outputs and gradients."""
    from nerf_few_shot_limitations_amd import _lib as L
    model = {"v1": make_model, "v2": make_v2, "v3": make_v3}[net](N, "bf16")[0]
    R, S = 259, 5
    if net == "v3":
        o, d, cam = _v3_scene(64, R, S)
    else:
        (o, d), cam = ray_batch(R, seed=130), None
    n = R * S
    outs = []
    for _ in range(2):
        f = forward_rays(model, S, o, d, perturb=True, seed=77, dino=cam)
        assert f["intact"]
        if net == "v1":
            g = (u01(131, n, 4) - 0.5).cuda()
            grad = torch.zeros(model.flat_params().flat.numel(), device="cuda")
            L.check(L.lib().nrf_mlp_backward_v1(f["h"], f["mode"], L.ptr(f["a"]), L.ptr(g), n, C.c_void_p(f["buf"].data_ptr()), f["nbytes"],
                                                L.ptr(grad), L.stream_ptr()))
            torch.cuda.synchronize()
        else:
            grad = backward_v2(model, f, (u01(131, n, 3) - 0.5).cuda(), (u01(132, n, 1) - 0.5).cuda())
        assert torch.isfinite(f["a"]).all() and torch.isfinite(grad).all() and float(grad.abs().max()) > 0
        outs.append((f["a"], f["b"], grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    if net != "v1":
        assert torch.equal(outs[0][1], outs[1][1])


def test_refusals_that_read_the_model(N):
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts, make_dino
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    lib = L.lib()
    R, S = 8, 4
    o, d = ray_batch(R)
    z = torch.empty(R, S, device=dev)
    a, b = torch.empty(R * S, 3, device=dev), torch.empty(R * S, 1, device=dev)
    rays = L.train_rays(rays_o=L.ptr(o), rays_d=L.ptr(d), z_vals=L.ptr(z))

    def call(h, opts, out_b, nbytes, buf):
        return lib.nrf_mlp_forward_train_rays(h, C.byref(rays), R, C.byref(opts), L.ptr(a), out_b, C.c_void_p(buf.data_ptr()), nbytes, L.stream_ptr())

    v3, _ = make_v3(N, "bf16")
    h, mode = _train_handle(v3, dev)
    nbytes = lib.nrf_train_context_bytes(h, mode, R * S)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert call(h, _opts(NEAR, FAR, S, False, None, 0, False, 0.0, False, "bf16", None, dev), L.ptr(b), nbytes, buf) == -1
    assert b"dino" in lib.nrf_last_error()
    wide, keep = make_dino(features=torch.zeros(1, 4, 4, 128, device=dev), pose=torch.eye(4), focal=10.0, H=8, W=8)
    assert call(h, _opts(NEAR, FAR, S, False, None, 0, False, 0.0, False, "bf16", wide, dev), L.ptr(b), nbytes, buf) == -1
    assert b"dino_dim" in lib.nrf_last_error()
    good, keep2 = make_dino(features=torch.zeros(1, 4, 4, 64, device=dev), pose=torch.eye(4), focal=10.0, H=8, W=8)
    ok = _opts(NEAR, FAR, S, False, None, 0, False, 0.0, False, "bf16", good, dev)
    assert call(h, ok, L.ptr(b), nbytes - 1, buf) == -1 and b"context" in lib.nrf_last_error()
    assert call(h, ok, None, nbytes, buf) == -1                                                     # V3 writes two outputs
    assert call(h, ok, L.ptr(b), nbytes, buf) == 0
    v1, _ = make_model(N, "bf16")
    h1, _ = _train_handle(v1, dev)
    n1 = lib.nrf_train_context_bytes(h1, mode, R * S)
    buf1 = torch.empty(n1, dtype=torch.uint8, device=dev)
    a4 = torch.empty(R * S, 4, device=dev)
    o1 = _opts(NEAR, FAR, S, False, None, 0, False, 0.0, False, "bf16", None, dev)
    assert lib.nrf_mlp_forward_train_rays(h1, C.byref(rays), R, C.byref(o1), L.ptr(a4), L.ptr(b), C.c_void_p(buf1.data_ptr()), n1, L.stream_ptr()) == -1
    assert b"out_b must be NULL" in lib.nrf_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 6. the command
# ---------------------------------------------------------------------------------------------
def test_train_epoch_fused_inputs_equals_the_default_route(N, tmp_path):
    from nerf_few_shot_limitations_amd import load_config, train_cli
    from nerf_few_shot_limitations_amd.training import FusedStep
    root = str(tmp_path / "scene")
    _write_scene(root)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(_CFG.format(dino="false", pf=10))
    cfg = load_config(str(cfg_path))
    dev = torch.device("cuda", 0)
    images, poses, (H, W, focal) = N.load_blender_data(root, "train", img_size=16)
    images = [im.permute(1, 2, 0).float().to(dev) for im in images]
    poses = [p.float() for p in poses]
    results = []
    for fused in (False, True):
        model, _ = make_v2(N, "bf16")
        step = FusedStep(model, lr=2e-3, weight_decay=1e-6)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        out = [train_cli.train_epoch(step, cfg, e, images, poses, H, W, focal, 2.0, 6.0, gen, fused_inputs=fused) for e in (0, 1)]
        results.append((out, model.flat_params().flat.clone()))
    (la, pa), (lb, pb) = results
    assert la == lb and la[0][1] == 2 * 16 * 16 * 8                      # (mean loss, ray-samples) of both epochs
    assert torch.equal(pa, pb)


def test_train_cli_fused_inputs_with_a_trained_extractor(N, tmp_path):
    from nerf_few_shot_limitations_amd import train_cli
    root = str(tmp_path / "scene")
    _write_scene(root)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino="true", pf=12))
    p = dict(O.make_weights("v3", 2, "fog"))
    p["pos_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 11, 12)
    p["dir_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 3, 4)
    torch.save({"epoch": 0, "nerf_model_state_dict": p}, str(tmp_path / "init.pth"))
    log = train_cli.main(["--config", str(cfg), "--data", root, "--out", str(tmp_path / "run"), "--mode", "f32", "--epochs", "4",
                          "--checkpoint", str(tmp_path / "init.pth"), "--dino-random-init", "--train-extractor", "--fused-inputs"])
    losses = [r["loss"] for r in log]
    print("--fused-inputs --train-extractor epoch losses:", losses)
    assert len(losses) == 4 and all(np.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
