"""The ray route under an occupancy grid (nrf_mlp_forward_train_rays_indexed, FusedStep.step_rays / step_view with
grid_inputs="rays", train_cli --occupancy-per-view) against what it stands in for.

The indexed forward derives row j as nrf_mlp_forward_train_rays derives row index[j], so its outputs are held to the bit against
that kernel's rows and (V2, V3) against the staged forward on the compacted points; an all-ones grid makes the whole step the plain
ray step, a random grid makes it (V2, V3) the staged step under the same grid -- parameters torch.equal.  V1's staged route takes an
encoding from nrf_encode where the kernel runs its own, so V1 is held to the ray route's dense rows to the bit and its flat gradient
to the dense masked step under rel_to_max < 2e-5, the bar test_step_equals_the_dense_masked_step holds the same re-cut sum to."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_dino_grad import make_v3 as make_v3_grad
from tests.test_gpu_train_occupancy import compact, full_grid, grid_of, staged_forward
from tests.test_gpu_train_rays import CANARY, FAR, NEAR, _v3_scene, canaries_intact, expand_dirs, forward_rays, padded, ray_batch, u01
from tests.test_gpu_training import _CFG, _write_scene, make_model, make_v2, make_v3, rel_to_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def make_net(N, net, mode, scene="fog"):
    """net: v1, v2, v3 (dino_dim 64) or v3w (128); the dino_dim 128 weights with the seed test_fused_step_equals_autograd_route picks."""
    if net == "v3w":
        return make_v3(N, mode, scene=scene, dino_dim=128, seed=4)[0]
    return {"v1": make_model, "v2": make_v2, "v3": make_v3}[net](N, mode, scene=scene)[0]


# the fields of the step tests: "solid" for V1 / V2; the V3 "solid" weights are empty along _v3_scene's rays (no density above 0, so no
# gradient at all -- the oracle on the CPU shows it), the thin medium is not
STEP_SCENE = {"v1": "solid", "v2": "solid", "v3": "fog"}


def pixel_scene(dino_dim, R):
    """_v3_scene with its pixel ids: (pixels, camera of the pixels, gathered o, d, the source view)."""
    import nerf_few_shot_limitations_amd as N
    H = W = 32
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))[:R].cuda()
    o, d, cam = _v3_scene(dino_dim, R, 1)
    return pix, dict(H=H, W=W, focal=focal, pose=pose), o, d, cam


def forward_indexed(model, S, index, z, o=None, d=None, pixels=None, cam=None, dino=None, n_rows=None):
    """One nrf_mlp_forward_train_rays_indexed through the C ABI on the rows `index` (int32, device) of the (R,S) batch whose depths are
    `z`.  Canaries stand behind every output and in the whole of points_out, which the call must not write; z_vals and rays_d_out are
    compared with what went in."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts, make_dino
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    h, mode = _train_handle(model, dev)
    R = int(o.shape[0] if o is not None else pixels.shape[0])
    n, M = R * S, int(index.numel() if n_rows is None else n_rows)
    zw, zb = padded(n)
    zb.copy_(z.reshape(-1))
    dw, d_out = padded(3 * R)
    d_out.copy_((u01(7, 3 * R) + 5.0).cuda())                    # the call reads the directions from the ray source, never from here
    d_before = dw.clone()
    pw, pts = padded(3 * n)
    dn, keep = make_dino(**dino) if dino is not None else (None, None)
    opts = _opts(NEAR, FAR, S, False, None, 0, False, 0.0, False, L.TRAIN_MODE[model.mma_mode], dn, dev, None)
    if pixels is not None:
        from nerf_few_shot_limitations_amd.ray_sampler import _c2w12
        rays = L.train_rays(pixels=pixels.data_ptr(), H=cam["H"], W=cam["W"], focal=cam["focal"], c2w=_c2w12(cam["pose"]), z_vals=L.ptr(zb),
                            rays_d_out=L.ptr(d_out), points_out=L.ptr(pts))
    else:
        rays = L.train_rays(rays_o=L.ptr(o), rays_d=L.ptr(d), z_vals=L.ptr(zb), rays_d_out=L.ptr(d_out), points_out=L.ptr(pts))
    nbytes = L.lib().nrf_train_context_bytes(h, mode, M)
    assert nbytes >= 0
    buf = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
    v1 = model.net == L.NRF_NET_V1
    aw, a = padded(M * (4 if v1 else 3))
    bw, b = (None, None) if v1 else padded(M)
    idx = index.to(device=dev, dtype=torch.int32).contiguous()
    L.check(L.lib().nrf_mlp_forward_train_rays_indexed(h, C.byref(rays), R, C.byref(opts), idx.data_ptr(), M, L.ptr(a), L.ptr(b),
                                                       C.c_void_p(buf.data_ptr()), nbytes, L.stream_ptr()))
    torch.cuda.synchronize()
    del keep
    intact = (canaries_intact(aw, a.numel()) and (v1 or canaries_intact(bw, M)) and bool((pw == CANARY).all())
              and torch.equal(zw[:n].view(torch.int32), z.reshape(-1).view(torch.int32)) and canaries_intact(zw, n)
              and torch.equal(dw.view(torch.int32), d_before.view(torch.int32)))
    return dict(a=a.view(M, -1), b=None if v1 else b.view(M, 1), buf=buf, nbytes=nbytes, h=h, mode=mode, n=M, intact=intact)


# ---------------------------------------------------------------------------------------------
# 1. rows
# ---------------------------------------------------------------------------------------------
ROWS = (1, 31, 32, 33, 255, 256, 257)


def chosen_depths(R, S, M):
    """test_compacted_forward_rows_are_the_dense_forward_rows' depths: M chosen samples 3.5 .. 4.5 in front of the camera (inside the
    box), the others far outside it."""
    chosen = torch.zeros(R * S, dtype=torch.bool)
    chosen[torch.randperm(R * S, generator=torch.Generator().manual_seed(M))[:M]] = True
    z = torch.where(chosen.reshape(R, S), 3.5 + u01(140, R, S), 40.0 + u01(141, R, S)).cuda().contiguous()
    return chosen, z


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("net", ["v1", "v2", "v3", "v3w"])
def test_indexed_rows_are_the_ray_forwards_rows(N, net, mode):
    """R * S = 9 * 32 = 288 samples; M = 1, 31, 32, 33 (around one wave's tile) and 255, 256, 257 (around a 256-sample group)."""
    model = make_net(N, net, mode)
    R, S = 9, 32
    o, d, cam = _v3_scene(128 if net == "v3w" else 64, R, S)
    dino = cam if net in ("v3", "v3w") else None
    grid = grid_of("ones", outside=1)
    for M in ROWS:
        chosen, z = chosen_depths(R, S, M)
        c = compact(grid, S, o, d, z_in=z)
        assert c["M"] == M and c["intact"] and np.array_equal(c["index"].cpu().numpy(), np.nonzero(chosen.numpy())[0])
        dense = forward_rays(model, S, o, d, z_in=z, dino=dino)
        assert dense["intact"] and torch.equal(dense["z"], z)
        f = forward_indexed(model, S, c["index"], c["z"], o, d, dino=dino)
        assert f["intact"], (net, mode, M)
        rows = c["index"].long()
        assert torch.equal(f["a"], dense["a"][rows]) and torch.isfinite(f["a"]).all(), (net, mode, M)
        if net != "v1":
            assert torch.equal(f["b"], dense["b"][rows]), (net, mode, M)
            comp = staged_forward(model, c["pos"].contiguous(), c["dirs"].contiguous(), cam)          # the staged compacted forward, bit for bit
            assert torch.equal(f["a"], comp["outs"][0]) and torch.equal(f["b"], comp["outs"][1]), (net, mode, M)


@pytest.mark.parametrize("net", ["v1", "v3"])
def test_indexed_rows_from_pixel_ids(N, net):
    model = make_net(N, net, "bf16")
    R, S = 9, 32
    pix, view, o, d, cam = pixel_scene(64, R)
    dino = cam if net == "v3" else None
    grid = grid_of("ones", outside=1)
    for M in (33, 257):
        chosen, z = chosen_depths(R, S, M)
        c = compact(grid, S, pixels=pix, cam=view, z_in=z)
        assert c["M"] == M and c["intact"]
        dense = forward_rays(model, S, pixels=pix, cam=view, z_in=z, dino=dino)
        by_rays = forward_rays(model, S, o, d, z_in=z, dino=dino)
        f = forward_indexed(model, S, c["index"], c["z"], pixels=pix, cam=view, dino=dino)
        assert f["intact"] and dense["intact"]
        rows = c["index"].long()
        assert torch.equal(f["a"], dense["a"][rows]) and torch.equal(f["a"], by_rays["a"][rows]), (net, M)
        if net != "v1":
            assert torch.equal(f["b"], dense["b"][rows])


@pytest.mark.parametrize("above", [False, True], ids=["at_the_switch", "above_it"])
def test_all_rows_at_and_above_the_geometry_switch(N, above):
    """dispatch_chain takes 4 waves per workgroup up to 128 rows per CU and 8 above (32 768 / 40 960 rows on 256 CUs): all rows of an
    all-ones grid at both, against the plain ray forward."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    S = 32
    R = (5 if above else 4) * cu
    model = make_net(N, "v3", "bf16")
    H = W = 64
    focal = O.focal_for(W)
    ro, rd = N.get_rays(H, W, focal, torch.from_numpy(O.LEGO_LIKE_C2W))
    pick = torch.randint(0, H * W, (R,), generator=torch.Generator().manual_seed(11)).cuda()
    o, d = ro.reshape(-1, 3)[pick].contiguous(), rd.reshape(-1, 3)[pick].contiguous()
    cam = _v3_scene(64, 1, 1)[2]
    dense = forward_rays(model, S, o, d, perturb=True, seed=21, dino=cam, points=False)
    index = torch.arange(R * S, dtype=torch.int32, device="cuda")
    f = forward_indexed(model, S, index, dense["z"].clone(), o, d, dino=cam)
    assert f["intact"] and f["n"] == R * S == (160 if above else 128) * cu
    assert torch.equal(f["a"], dense["a"]) and torch.equal(f["b"], dense["b"]) and torch.isfinite(f["a"]).all()


def test_context_too_small_and_no_rows(N):
    """The refusals that read the model (the others: tests/test_train_occupancy_rays_host.py), and n_rows == 0."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    lib = L.lib()
    R, S, M = 8, 4, 20
    o, d = ray_batch(R)
    z = torch.full((R, S), 3.0, device=dev)
    a, b = torch.empty(M, 3, device=dev), torch.empty(M, 1, device=dev)
    index = torch.arange(M, dtype=torch.int32, device=dev)
    rays = L.train_rays(rays_o=L.ptr(o), rays_d=L.ptr(d), z_vals=L.ptr(z))
    model, _ = make_v2(N, "bf16")
    h, mode = _train_handle(model, dev)
    opts = _opts(NEAR, FAR, S, False, None, 0, False, 0.0, False, "bf16", None, dev)
    nbytes = lib.nrf_train_context_bytes(h, mode, M)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call = lambda rows, nb, out_b=L.ptr(b): lib.nrf_mlp_forward_train_rays_indexed(h, C.byref(rays), R, C.byref(opts), index.data_ptr(), rows, L.ptr(a), out_b,
                                                                                  C.c_void_p(buf.data_ptr()), nb, L.stream_ptr())
    assert call(M, nbytes - 1) == -1 and b"context" in lib.nrf_last_error()
    assert call(M, nbytes, None) == -1                                             # V2 writes two outputs
    assert call(0, 0) == 0                                                         # no rows: nothing launched
    assert call(M, nbytes) == 0
    v1, _ = make_model(N, "bf16")
    h1, _ = _train_handle(v1, dev)
    a4 = torch.empty(M, 4, device=dev)
    assert lib.nrf_mlp_forward_train_rays_indexed(h1, C.byref(rays), R, C.byref(opts), index.data_ptr(), M, L.ptr(a4), L.ptr(b), C.c_void_p(buf.data_ptr()),
                                                  1 << 30, L.stream_ptr()) == -1
    assert b"out_b must be NULL" in lib.nrf_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 2. the all-ones grid: the plain ray step
# ---------------------------------------------------------------------------------------------
def step_kw(recipe):
    kw = dict(lr=5e-4, weight_decay=1e-6)
    if recipe == "multiscale":
        kw.update(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True, seed=31)
    return kw


def same_state(sa, sb):
    return (torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat) and torch.equal(sa.opt.exp_avg, sb.opt.exp_avg)
            and torch.equal(sa.opt.exp_avg_sq, sb.opt.exp_avg_sq) and sa.opt.step_count == sb.opt.step_count)


@pytest.mark.parametrize("recipe", ["plain", "multiscale"])
@pytest.mark.parametrize("net", ["v1", "v2", "v3"])
def test_three_steps_under_an_all_ones_grid_are_the_plain_ray_steps(N, net, recipe):
    from nerf_few_shot_limitations_amd.training import FusedStep
    sa, sb = (FusedStep(make_net(N, net, "bf16", STEP_SCENE[net]), **step_kw(recipe)) for _ in range(2))
    R, S = 37, 33
    o, d, cam = _v3_scene(64, R, S)
    dino = dict(dino=cam) if net == "v3" else {}
    tgt = u01(161, R, 3).cuda()
    grid = full_grid()
    for i in range(3):
        la = sa.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=70 + i, **dino)
        lb = sb.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=70 + i, occupancy=grid, grid_inputs="rays", **dino)
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z) and sb.last_count == R * S, (net, recipe, i)
        for k in sa.last_losses:
            assert torch.equal(sa.last_losses[k], sb.last_losses[k]), (i, k)
        assert float(sb.grad.abs().max()) > 0, (net, recipe, i)                   # the steps do move the parameters
    assert same_state(sa, sb) and sa.opt.step_count == 3 and sa.last_count is None


@pytest.mark.parametrize("net", ["v1", "v2", "v3"])
def test_step_view_under_an_all_ones_grid_is_the_plain_step_view(N, net):
    from nerf_few_shot_limitations_amd.training import FusedStep
    sa, sb = (FusedStep(make_net(N, net, "bf16", STEP_SCENE[net]), lr=5e-4) for _ in range(2))
    H, W, R, S = 24, 24, 100, 16
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    image = u01(162, H, W, 3).cuda()
    dino = dict(dino=_v3_scene(64, 1, 1)[2]) if net == "v3" else {}
    for i in range(3):
        pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(i))[:R].cuda()
        la = sa.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, seed=5 + i, **dino)
        lb = sb.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, seed=5 + i, occupancy=full_grid(), grid_inputs="rays", **dino)
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z) and sb.last_count == R * S, (net, i)
    assert same_state(sa, sb)


def test_grid_inputs_is_refused_without_a_grid(N):
    from nerf_few_shot_limitations_amd.training import FusedStep
    step = FusedStep(make_net(N, "v2", "bf16"), lr=1e-3)
    o, d = ray_batch(8)
    tgt = u01(172, 8, 3).cuda()
    with pytest.raises(ValueError, match="occupancy="):
        step.step_rays(o, d, tgt, NEAR, FAR, 4, grid_inputs="rays")
    with pytest.raises(ValueError, match="staged"):
        step.step_rays(o, d, tgt, NEAR, FAR, 4, occupancy=full_grid(), grid_inputs="points")
    assert step.opt.step_count == 0


# ---------------------------------------------------------------------------------------------
# 3. a random grid
# ---------------------------------------------------------------------------------------------
R3, S3 = 50, 33


def random_grid():
    return grid_of("random", outside=1, seed=151, box=(-6.0, 6.0))


@pytest.mark.parametrize("net", ["v2", "v3"])
def test_three_steps_under_a_random_grid_are_the_staged_route_steps(N, net):
    from nerf_few_shot_limitations_amd.training import FusedStep
    sa, sb = (FusedStep(make_net(N, net, "bf16", STEP_SCENE[net]), lr=5e-4, weight_decay=1e-6) for _ in range(2))
    o, d, cam = _v3_scene(64, R3, S3)
    dino = dict(dino=cam) if net == "v3" else {}
    tgt = u01(153, R3, 3).cuda()
    grid = random_grid()
    for i in range(3):
        la = sa.step_rays(o, d, tgt, NEAR, FAR, S3, perturb=True, seed=152 + i, occupancy=grid, **dino)
        lb = sb.step_rays(o, d, tgt, NEAR, FAR, S3, perturb=True, seed=152 + i, occupancy=grid, grid_inputs="rays", **dino)
        assert sa.last_count == sb.last_count and 0.2 < sb.last_count / (R3 * S3) < 0.8, (i, sb.last_count)
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z), (net, i)
        assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat), (net, i)
        assert float(sb.grad.abs().max()) > 0 and bool(torch.isfinite(sb.grad).all()), (net, i)      # the steps do move the parameters
    assert same_state(sa, sb)


def test_v1_step_under_a_random_grid_against_the_dense_ray_route(N):
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import FusedStep
    lib = L.lib()
    model, twin = make_net(N, "v1", "bf16", "solid"), make_net(N, "v1", "bf16", "solid")
    R, S, n = R3, S3, R3 * S3
    o, d = ray_batch(R, seed=150)
    tgt = u01(153, R, 3).cuda()
    grid = random_grid()
    c = compact(grid, S, o, d, perturb=True, seed=152, directions=False)
    M, index, z = c["M"], c["index"].long(), c["z"].contiguous()
    assert 0.2 < M / n < 0.8
    # the dense ray-route forward (the twin holds the parameters the step starts from), its rows gathered through the indexed compositor
    dense = forward_rays(twin, S, o, d, perturb=True, seed=152)
    assert torch.equal(dense["z"], z)
    rows = dense["a"][index].contiguous()
    lo = L.loss_opts(0.7)
    st = L.stream_ptr()
    d_rows = torch.full((M, 4), CANARY, device="cuda")
    pred, terms = torch.empty((R, 3), device="cuda"), torch.zeros((3, R), device="cuda")
    L.check(lib.nrf_composite_loss_backward_indexed(L.ptr(rows), 4, C.c_void_p(rows.data_ptr() + 12), 4, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo),
                                                    c["slot"].data_ptr(), L.ptr(pred), L.ptr(d_rows), 4, C.c_void_p(d_rows.data_ptr() + 12), 4, L.ptr(terms),
                                                    None, 0, st))
    # the dense masked step: skipped samples composited as colour 0 / density -inf, the V1 dZ chain over all n rows
    skipped = torch.ones(n, dtype=torch.bool, device="cuda")
    skipped[index] = False
    masked = dense["a"].clone()
    masked[skipped, :3] = 0.0
    masked[skipped, 3] = float("-inf")
    g = torch.full((n, 4), CANARY, device="cuda")
    pred_d, terms_d = torch.empty((R, 3), device="cuda"), torch.zeros((3, R), device="cuda")
    L.check(lib.nrf_composite_loss_backward(L.ptr(masked), 4, C.c_void_p(masked.data_ptr() + 12), 4, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo),
                                            L.ptr(pred_d), L.ptr(g), 4, C.c_void_p(g.data_ptr() + 12), 4, L.ptr(terms_d), None, 0, st))
    grad_d = torch.zeros(twin.flat_params().flat.numel(), device="cuda")
    L.check(lib.nrf_mlp_backward_v1(dense["h"], dense["mode"], L.ptr(masked), L.ptr(g), n, C.c_void_p(dense["buf"].data_ptr()), dense["nbytes"],
                                    L.ptr(grad_d), st))
    torch.cuda.synchronize()
    assert bool((g[skipped] == 0).all())                                          # a skipped sample passes no gradient
    # the step
    step = FusedStep(model, lr=5e-4, rgb_weight=0.7)
    step.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=152, occupancy=grid, grid_inputs="rays")
    bits = lambda t: t.contiguous().view(torch.int32)
    assert step.last_count == M and torch.equal(step.last_z, z)
    assert torch.equal(bits(step.out4[:M]), bits(rows))                           # the step's outputs: the dense rows
    assert torch.equal(bits(step.d_out4[:M]), bits(d_rows)) and torch.equal(bits(step.d_out4[:M]), bits(g[index]))
    assert torch.equal(bits(step.pred), bits(pred)) and torch.equal(bits(pred), bits(pred_d))
    assert float(grad_d.abs().max()) > 0 and bool(torch.isfinite(grad_d).all())
    err = rel_to_max(step.grad, grad_d)
    print(f"V1 ray route under a grid vs dense masked step: M / (R S) = {M / n:.3f}, flat gradient rel_to_max {err:.3g}")
    assert err < 2e-5


# ---------------------------------------------------------------------------------------------
# 4. per-sample gradients under the grid
# ---------------------------------------------------------------------------------------------
def fetch_adjoint_orders(cam, pts, g):
    """The adjoint of the bilinear fetch at `pts` applied to `g`, on the CPU: contributions formed in float64 (the oracle's projection
    and taps), summed per texel in float64 and in float32 in two orders -- row by row, and in 16 slabs of rows added up afterwards.
    Returns the largest distance of either fp32 order from the float64 sum, relative to that sum's largest element."""
    fm = cam["features"]
    Hp, Wp, Cc = (int(v) for v in fm.shape[1:])
    p64 = pts.cpu().double()
    pc = torch.cat([p64, torch.ones_like(p64[:, :1])], -1) @ torch.inverse(torch.as_tensor(cam["pose"]).double()).T      # oracle: project_points_to_image
    xn = (pc[:, 0] / (pc[:, 2] + 1e-8) * float(cam["focal"]) + cam["W"] / 2) / cam["W"] * 2 - 1
    yn = (pc[:, 1] / (pc[:, 2] + 1e-8) * float(cam["focal"]) + cam["H"] / 2) / cam["H"] * 2 - 1
    gx, gy = ((xn + 1) * Wp - 1) / 2, ((yn + 1) * Hp - 1) / 2                                                            # oracle: sample_features_at_points
    x0, y0 = torch.floor(gx), torch.floor(gy)
    g64 = g.cpu().double()
    texel, contrib = [], []
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            w = ((gx - x0) if dx else (x0 + 1 - gx)) * ((gy - y0) if dy else (y0 + 1 - gy))
            ok = (xi >= 0) & (xi <= Wp - 1) & (yi >= 0) & (yi <= Hp - 1)              # (no Z > 0 mask: nets.hpp dino_taps has none)
            texel.append(torch.where(ok, yi * Wp + xi, torch.full_like(xi, -1)).long())
            contrib.append(g64 * w[:, None])
    texel, contrib = torch.stack(texel, 1).reshape(-1).numpy(), torch.stack(contrib, 1).reshape(-1, Cc).numpy()      # row-major: a row's four taps together
    ref = np.zeros((Hp * Wp, Cc))
    seq, slabs = np.zeros((Hp * Wp, Cc), np.float32), np.zeros((Hp * Wp, Cc), np.float32)
    bounds = np.linspace(0, texel.size, 17).astype(np.int64)
    for t in range(Hp * Wp):
        mine = np.nonzero(texel == t)[0]
        if mine.size == 0:
            continue
        c = contrib[mine]
        ref[t] = c.sum(0)
        c32 = c.astype(np.float32)
        seq[t] = np.cumsum(c32, 0, dtype=np.float32)[-1]
        part = [np.cumsum(c32[(mine >= a) & (mine < b)], 0, dtype=np.float32)[-1] for a, b in zip(bounds[:-1], bounds[1:]) if ((mine >= a) & (mine < b)).any()]
        slabs[t] = np.cumsum(np.stack(part), 0, dtype=np.float32)[-1]
    top = np.abs(ref).max()
    assert top > 0
    return max(np.abs(seq - ref).max(), np.abs(slabs - ref).max()) / top


@pytest.mark.parametrize("dino_dim", [64, 128])
def test_per_sample_gradients_on_the_compacted_rows(N, dino_dim):
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import FusedStep, project_fetch_backward
    lib = L.lib()
    seed = 4 if dino_dim == 128 else 2
    model, twin = (make_v3_grad(N, "bf16", scene=STEP_SCENE["v3"], dino_dim=dino_dim, seed=seed)[0] for _ in range(2))
    R, S, n = R3, S3, R3 * S3
    o, d, cam = _v3_scene(dino_dim, R, S)
    tgt = u01(153, R, 3).cuda()
    grid = random_grid()
    c = compact(grid, S, o, d, perturb=True, seed=152)
    M, index, z = c["M"], c["index"].long(), c["z"].contiguous()
    assert 0.2 < M / n < 0.8
    # the dense masked step on the twin, assembled from the entry points: d_dino of all n rows
    dense = forward_rays(twin, S, o, d, perturb=True, seed=152, dino=cam)
    skipped = torch.ones(n, dtype=torch.bool, device="cuda")
    skipped[index] = False
    rgb_m, den_m = dense["a"].clone(), dense["b"].clone()
    rgb_m[skipped] = 0.0
    den_m[skipped] = float("-inf")
    g_rgb, g_den = torch.empty((n, 3), device="cuda"), torch.empty((n, 1), device="cuda")
    pred_d, terms_d = torch.empty((R, 3), device="cuda"), torch.zeros((3, R), device="cuda")
    lo = L.loss_opts(1.0)
    st = L.stream_ptr()
    L.check(lib.nrf_composite_loss_backward(L.ptr(rgb_m), 3, L.ptr(den_m), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo), L.ptr(pred_d),
                                            L.ptr(g_rgb), 3, L.ptr(g_den), 1, L.ptr(terms_d), None, 0, st))
    grad_d = torch.zeros(twin.flat_params().flat.numel(), device="cuda")
    ctx = C.c_void_p(dense["buf"].data_ptr())
    L.check(lib.nrf_mlp_backward(dense["h"], dense["mode"], L.ptr(rgb_m), L.ptr(den_m), L.ptr(g_rgb), L.ptr(g_den), n, ctx, dense["nbytes"], L.ptr(grad_d), st))
    dd_dense = torch.empty((n, dino_dim), device="cuda")
    L.check(lib.nrf_mlp_backward_dino(dense["h"], dense["mode"], n, ctx, dense["nbytes"], L.ptr(dd_dense), st))
    torch.cuda.synchronize()
    print(f"dense masked step, dino_dim {dino_dim}: M / (R S) {M / n:.3f}, kept rows with density > 0 {float((den_m[index] > 0).float().mean()):.3f}, "
          f"max |g_rgb| {float(g_rgb.abs().max()):.3g}, max |g_den| {float(g_den.abs().max()):.3g}, max |flat gradient| {float(grad_d.abs().max()):.3g}, "
          f"max |d_dino| {float(dd_dense.abs().max()):.3g}, loss terms {float(terms_d[0].sum()):.3g}")
    assert float(grad_d.abs().max()) > 0 and bool(torch.isfinite(grad_d).all())
    assert bool((dd_dense[skipped] == 0).all()) and float(dd_dense.abs().max()) > 0      # a skipped row's dZ is zero: so is its d_dino
    # the step under the grid hands out the M rows
    dw, dd = padded(n * dino_dim)
    pw, pp = padded(n * 3)
    dd, pp = dd.view(n, dino_dim), pp.view(n, 3)
    step = FusedStep(model, lr=5e-4)
    step.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=152, dino=cam, occupancy=grid, grid_inputs="rays", d_dino_out=dd, points_out=pp)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert step.last_count == M
    assert torch.equal(bits(dd[:M]), bits(dd_dense[index])), dino_dim
    assert torch.equal(bits(pp[:M]), bits(c["pos"])) and torch.equal(bits(pp[:M]), bits(dense["pts"][index]))
    assert bool((dd[M:] == CANARY).all()) and bool((pp[M:] == CANARY).all())      # rows >= M are not written
    assert canaries_intact(dw, n * dino_dim) and canaries_intact(pw, n * 3)
    # the map's gradient: M rows against all R * S rows whose skipped rows are zero -- another cut of the same fp32 sum.  First, on the
    # CPU: two fp32 orders of this very sum stay within half the bound of its float64 value
    order = fetch_adjoint_orders(cam, dense["pts"], dd_dense)
    print(f"fetch adjoint, dino_dim {dino_dim}: fp32 summation orders vs float64 on the CPU {order:.3g} of max")
    assert order < 1e-5
    fmap = cam["features"]
    map_rows = project_fetch_backward(cam, pp[:M].contiguous(), dd[:M].contiguous(), torch.zeros_like(fmap), accumulate=False)
    map_all = project_fetch_backward(cam, dense["pts"], dd_dense, torch.zeros_like(fmap), accumulate=False)
    torch.cuda.synchronize()
    err = rel_to_max(map_rows, map_all)
    print(f"d_map from the {M} compacted rows vs from all {n} rows: rel_to_max {err:.3g}")
    assert float(map_all.abs().max()) > 0 and err < 2e-5
    # the default route keeps refusing the combination
    with pytest.raises(ValueError, match="d_dino_out / points_out"):
        step.step_rays(o, d, tgt, NEAR, FAR, S, dino=cam, occupancy=grid, d_dino_out=dd)


def test_a_step_that_keeps_no_sample_writes_neither_buffer(N):
    from nerf_few_shot_limitations_amd.training import FusedStep
    model = make_v3_grad(N, "bf16", scene=STEP_SCENE["v3"])[0]
    step = FusedStep(model, lr=1e-3)
    before = model.flat_params().ensure().clone()
    R, S = 37, 5
    o, d, cam = _v3_scene(64, R, S)
    tgt = u01(171, R, 3).cuda()
    dw, dd = padded(R * S * 64)
    pw, pp = padded(R * S * 3)
    loss = step.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=1, dino=cam, occupancy=grid_of("zeros", outside=1), grid_inputs="rays",
                          d_dino_out=dd.view(R * S, 64), points_out=pp.view(R * S, 3))
    assert step.last_count == 0 and step.opt.step_count == 1 and torch.isfinite(loss)
    assert bool((dw == CANARY).all()) and bool((pw == CANARY).all())
    assert torch.equal(step.pred, torch.zeros((R, 3), device="cuda")) and bool((step.grad == 0).all())
    assert torch.equal(model.flat_params().flat, before)


# ---------------------------------------------------------------------------------------------
# 5. the trainer
# ---------------------------------------------------------------------------------------------
def _cli_setup(tmp_path):
    root = str(tmp_path / "scene")
    _write_scene(root)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino="true", pf=12))
    p = dict(O.make_weights("v3", 2, "fog"))
    p["pos_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 11, 12)
    p["dir_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 3, 4)
    torch.save({"epoch": 0, "nerf_model_state_dict": p}, str(tmp_path / "init.pth"))
    return ["--config", str(cfg), "--data", root, "--mode", "bf16", "--dino-random-init"]


GRID_FLAGS = ["--occupancy-res", "32", "--occupancy-per-view", "--occupancy-warmup", "2", "--occupancy-refresh-every", "2", "--max-batches", "6",
              "--occupancy-box", "-2.5", "2.5"]


@pytest.mark.parametrize("extractor", [False, True], ids=["maps", "train_extractor"])
def test_train_cli_per_view_grids(N, tmp_path, monkeypatch, extractor):
    """Two epochs of the 16-pixel set: 2 views x 2 batches per epoch, so every view's grid takes 4 steps -- 2 of warm-up -- and 2
    refreshes; the checkpoint carries the grids and a resumed run starts from them, bit for bit."""
    from nerf_few_shot_limitations_amd import train_cli
    common = _cli_setup(tmp_path) + (["--train-extractor"] if extractor else [])
    seen = []
    epoch = train_cli.train_epoch

    def spy(step, *a, **kw):
        occ, ext = kw["occupancy"], kw.get("extractor")
        if not seen:
            seen.append(dict(state=occ.state_dict(), occ=occ, ext=ext, lora=None if ext is None else [q.detach().clone() for q in ext.params]))
        return epoch(step, *a, **kw)

    monkeypatch.setattr(train_cli, "train_epoch", spy)
    log = train_cli.main(common + GRID_FLAGS + ["--out", str(tmp_path / "run"), "--epochs", "2", "--checkpoint", str(tmp_path / "init.pth")])
    losses = [r["loss"] for r in log]
    print("--occupancy-per-view epoch losses:", losses, "occupied", [r["occupied_fraction"] for r in log])
    assert len(losses) == 2 and all(np.isfinite(x) for x in losses) and all(0.0 <= r["occupied_fraction"] <= 1.0 for r in log)
    first = seen[0]
    occ = first["occ"]
    assert isinstance(occ, train_cli.PerViewOccupancy) and len(occ.views) == 2                    # one grid per view
    assert all(s["steps"] == 0 and s["ema"] is None for s in first["state"]["views"])             # ... fresh at the start of the run
    for s in occ.views:
        assert s.steps == 4 and s.grid._refreshes == 2 and s.grid.ema is not None and s.current() is s.grid
    ckpt = torch.load(str(tmp_path / "run" / "best_tiny.pth"), map_location="cpu", weights_only=True)
    saved = ckpt["occupancy_per_view_state"]
    for s, sd in zip(occ.views, saved["views"]):
        assert torch.equal(s.grid.bits.cpu(), sd["bits"]) and torch.equal(s.grid.ema.cpu(), sd["ema"])
        assert (sd["cursor"], sd["refreshes"], sd["steps"]) == (s.grid._cursor, 2, 4)
    if extractor:
        assert any(not torch.equal(q.detach(), q0) for q, q0 in zip(first["ext"].params, first["lora"]))       # a LoRA parameter has changed
        assert "dino_model_state_dict" in ckpt
    # a second run resumes the grids
    seen.clear()
    log2 = train_cli.main(common + GRID_FLAGS + ["--out", str(tmp_path / "again"), "--epochs", "3", "--checkpoint", str(tmp_path / "run" / "best_tiny.pth")])
    assert len(log2) == 1 and np.isfinite(log2[0]["loss"])                                        # epoch 3 alone
    for got, sd in zip(seen[0]["state"]["views"], saved["views"]):
        assert torch.equal(got["bits"], sd["bits"]) and torch.equal(got["ema"], sd["ema"])
        assert (got["cursor"], got["refreshes"], got["steps"]) == (sd["cursor"], sd["refreshes"], sd["steps"])
    assert all(s.steps == 6 for s in seen[0]["occ"].views)                                        # no second warm-up: the counters went on


def test_train_cli_without_the_flag_keeps_refusing_use_dino(N, tmp_path):
    from nerf_few_shot_limitations_amd import train_cli
    common = _cli_setup(tmp_path)
    with pytest.raises(SystemExit) as e:
        train_cli.main(common + ["--occupancy-res", "32", "--out", str(tmp_path / "run"), "--epochs", "1"])
    assert "use_dino: true" in str(e.value) and "ONE source view" in str(e.value)


# ---------------------------------------------------------------------------------------------
# 6. sixty V3 steps under a grid that follows the field
# ---------------------------------------------------------------------------------------------
def test_sixty_v3_steps_with_a_refresh_every_ten_reduce_the_loss(N):
    """test_sixty_steps_with_a_refresh_every_ten_reduce_the_loss with the V3 network on the ray route: the loss on a fixed batch falls
    below 0.7 of where it started, under a grid of the source view that is refreshed from the field every 10 steps.  The threshold is
    put at the median over the cells the view's own SAMPLES fall into, not over all cells as there: a V3 field's density follows the
    source view's map, most cells of the box lie beside that map, and a grid-wide median separates the two kinds of cell and leaves
    the view's samples where they were (measured: 1.5 % of them skipped)."""
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    from nerf_few_shot_limitations_amd.training import FusedStep
    dev = torch.device("cuda", 0)
    model = make_net(N, "v3", "bf16")
    step = FusedStep(model, lr=1e-3)
    H = W = 24
    S = 32
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    cam = _v3_scene(64, 1, 1)[2]
    yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
    image = torch.stack([xx, yy, 0.5 * torch.ones_like(xx)], -1).cuda().contiguous()
    pix = torch.arange(H * W, dtype=torch.int64, device=dev)
    grid = OccupancyGrid.full(32, -2.5, 2.5, device=dev)
    ro, rd = N.get_rays(H, W, focal, pose)
    ro, rd = ro.reshape(-1, 1, 3).to(dev), rd.reshape(-1, 1, 3).to(dev)
    losses, counts, threshold = [], [], None
    for i in range(60):
        losses.append(step.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, perturb=True, seed=900 + i, dino=cam, occupancy=grid,
                                     grid_inputs="rays").item())
        counts.append(step.last_count)
        if (i + 1) % 10 == 0:
            if threshold is None:
                # the first probe of the whole grid; the threshold: the median value over the cells of the last step's samples, so that the
                # run does train with about half of its samples skipped and the later refreshes have cells to bring back or drop
                grid.refresh(model, decay=0.95, threshold=0.0, samples_per_cell=2, dino=cam)
                t = (ro + rd * step.last_z[..., None] + 2.5) * (32 / 5.0)
                inside = ((t >= 0) & (t < 32)).all(-1)
                i = t.floor().long().clamp(0, 31)
                cell = (i[..., 2] * 32 + i[..., 1]) * 32 + i[..., 0]
                assert float(inside.float().mean()) > 0.9                         # the view's samples do lie in the box
                threshold = float(grid.ema[cell[inside]].median())
            grid.refresh(model, decay=0.95, threshold=threshold, samples_per_cell=2, cells=grid.n_cells // 2, dino=cam)
    print(f"60 V3 steps under a refreshed grid: loss {losses[0]:.4g} -> {losses[-1]:.4g}, M / (R S) {counts[0] / (H * W * S):.3f} -> "
          f"{counts[-1] / (H * W * S):.3f}, occupied cells {grid.occupied_fraction:.3f}")
    assert all(np.isfinite(losses)) and counts[0] == H * W * S
    assert min(counts) < 0.9 * H * W * S                                          # the grid did skip samples on the way
    assert losses[-1] < 0.7 * losses[0], losses
