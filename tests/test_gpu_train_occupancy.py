"""Training under an occupancy grid (nrf_occupancy_compact_rays, nrf_composite_loss_backward_indexed, FusedStep.step_rays /
step_view with occupancy=, OccupancyGrid.full / refresh) against what it stands in for.

A step under a grid is the plain step with every sample in an empty cell composited as colour 0 and effective density -inf, so
everything derivable is held to the bit: the compaction against a float32 numpy replay of the cell rule and against the staged
samplers, the network's rows against the dense staged forward, the compositor's outputs against the dense masked step, the
all-ones grid against the plain step.  Only the flat gradient is a sum over a re-cut batch: rel_to_max < 2e-5, the figure
test_gradient_is_additive_over_the_batch_at_scale holds the same cause to (fp32 summation order)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_train_rays import CANARY, NEAR, FAR, _v3_scene, expand_dirs, ray_batch, u01
from tests.test_gpu_training import MARGIN, make_model, make_v2, make_v3, rel_to_max

pytestmark = pytest.mark.gpu

BOX = (-3.0, 3.0)                 # ray_batch's samples lie 1 .. 9 from the origin: the rays partly leave it
RES = (32, 8, 8)


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def grid_of(kind, outside=0, res=RES, box=BOX, seed=7):
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    rx, ry, rz = res
    if kind == "ones":
        mask = torch.ones(rz, ry, rx, dtype=torch.bool)
    elif kind == "zeros":
        mask = torch.zeros(rz, ry, rx, dtype=torch.bool)
    else:
        mask = u01(seed, rz, ry, rx) < 0.5
    return OccupancyGrid.from_mask(mask, box[0], box[1], outside=outside).to(torch.device("cuda", 0))


def keep_replay(grid, o, d, z):
    """The cell rule of nerfhip.h (nrf_occupancy) in float32 numpy, one rounded operation at a time: (R,S) bool, True = evaluated."""
    o, d, z = (t.detach().cpu().numpy().astype(np.float32) for t in (o, d, z))
    with np.errstate(all="ignore"):
        p = o[:, None, :] + d[:, None, :] * z[:, :, None]                       # one rounded product, one rounded sum
        lo, scale, res = np.asarray(grid.lo, np.float32), np.asarray(grid.scale, np.float32), np.asarray(grid.res, np.float32)
        t = (p - lo) * scale
        inside = ((t >= 0) & (t < res)).all(-1)                                 # a NaN is not inside
        finite = (np.abs(p) < np.inf).all(-1)
        i = np.floor(np.where(inside[..., None], t, 0)).astype(np.int64)
    idx = (i[..., 2] * grid.res[1] + i[..., 1]) * grid.res[0] + i[..., 0]
    bit = grid.to_mask().cpu().numpy().reshape(-1)[idx]
    return np.where(inside, bit, ~(bool(grid.outside) & finite)), p


def compact(grid, S, o=None, d=None, pixels=None, cam=None, perturb=False, t_rand=None, seed=0, lindisp=False, z_in=None, near=NEAR, far=FAR,
            directions=True):
    """One nrf_occupancy_compact_rays through the C ABI, every output with canaries behind it (and, for the compacted outputs, in
    the rows >= M, which the call must not write)."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.renderer import _opts
    dev = torch.device("cuda", 0)
    R = int(o.shape[0] if o is not None else pixels.shape[0])
    n, pad = R * S, 64
    f = lambda k: torch.full((k + pad,), CANARY, dtype=torch.float32, device=dev)
    i32 = lambda k: torch.full((k + pad,), -777, dtype=torch.int32, device=dev)
    z, d_out, pos, dirs, index, slot = f(n), f(3 * R), f(3 * n), f(3 * n), i32(n), i32(n)
    count = torch.full((2,), -777, dtype=torch.int64, device=dev)
    wsb = int(L.lib().nrf_occupancy_compact_workspace_bytes(R))
    ws = torch.zeros(wsb + 64, dtype=torch.uint8, device=dev)
    ws[wsb:] = 0x5A
    opts = _opts(near, far, S, perturb, t_rand, seed, lindisp, 0.0, False, "bf16", None, dev, z_in)
    if pixels is not None:
        from nerf_few_shot_limitations_amd.ray_sampler import _c2w12
        rays = L.train_rays(pixels=pixels.data_ptr(), H=cam["H"], W=cam["W"], focal=cam["focal"], c2w=_c2w12(cam["pose"]), z_vals=z.data_ptr(),
                            rays_d_out=d_out.data_ptr())
    else:
        rays = L.train_rays(rays_o=L.ptr(o), rays_d=L.ptr(d), z_vals=z.data_ptr(), rays_d_out=d_out.data_ptr())
    occ, keep = grid.struct(dev)
    cp = L.compact(n, index.data_ptr(), slot.data_ptr(), pos.data_ptr(), dirs.data_ptr() if directions else None, count.data_ptr(), ws.data_ptr(), wsb)
    L.check(L.lib().nrf_occupancy_compact_rays(C.byref(rays), R, C.byref(opts), C.byref(occ), C.byref(cp), L.stream_ptr()))
    torch.cuda.synchronize()
    M = int(count[0])
    intact = (bool((z[n:] == CANARY).all()) and bool((pos[3 * M:] == CANARY).all()) and bool((index[M:] == -777).all())
              and bool((slot[n:] == -777).all()) and int(count[1]) == -777 and bool((ws[wsb:] == 0x5A).all())
              and bool((dirs[3 * M if directions else 0:] == CANARY).all())
              and bool((d_out[3 * R:] == CANARY).all()))
    return dict(M=M, z=z[:n].view(R, S), d_out=d_out[:3 * R].view(R, 3), pos=pos[:3 * M].view(M, 3), dirs=dirs[:3 * M].view(M, 3), index=index[:M],
                slot=slot[:n], intact=intact, raw=(z, pos, dirs, index, slot, count))


def same_bits(a, b):
    """Equal bit for bit, a NaN matching any NaN (the payload a NaN origin leaves in o + d * z is the adder's business)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


def tbits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check_compaction(c, grid, o, d, z_expected, name):
    R, S = z_expected.shape
    assert c["intact"], name
    assert torch.equal(tbits(c["d_out"]), tbits(d)), name                         # (written in ray mode too when a buffer is given)
    assert torch.equal(c["z"], z_expected), name                                  # the staged sampler's depths, to the bit
    keep, p = keep_replay(grid, o, d, c["z"])
    want = np.nonzero(keep.reshape(-1))[0]
    assert c["M"] == want.size, (name, c["M"], want.size)
    index = c["index"].cpu().numpy()
    assert np.array_equal(index, want), name                                      # strictly ascending flat ids
    assert c["M"] < 2 or bool((np.diff(index) > 0).all())
    slot = np.full(R * S, -1, np.int64)
    slot[want] = np.arange(want.size)
    assert np.array_equal(c["slot"].cpu().numpy(), slot), name                    # the inverse map, -1 elsewhere
    assert same_bits(c["pos"].cpu().numpy(), p.reshape(-1, 3)[want]), name        # o + d * z, bit for bit
    assert same_bits(c["dirs"].cpu().numpy(), d.cpu().numpy()[want // S]), name
    return keep


# ---------------------------------------------------------------------------------------------
# 1. compaction
# ---------------------------------------------------------------------------------------------
def odd_rays(R, seed=50):
    """ray_batch with one ray from an infinite and one from a NaN origin: always evaluated."""
    o, d = ray_batch(R, seed)
    o = o.clone()
    o[5, 0] = float("inf")
    o[6, 1] = float("nan")
    return o, d


@pytest.mark.parametrize("S", [1, 5, 64, 65, 130])
def test_compaction_is_the_cell_rule_on_the_staged_samplers_points(N, S):
    R = 37
    o, d = odd_rays(R)
    tr = u01(60, R, S).cuda()
    z_explicit = torch.sort(u01(61, R, S) * 4 + 2, dim=-1).values.cuda()
    cases = {"plain": dict(perturb=False), "seed": dict(perturb=True, seed=12345 + S), "t_rand": dict(perturb=True, t_rand=tr),
             "lindisp+seed": dict(perturb=True, lindisp=True, seed=99)}
    evaluated = set()
    for kind in ("ones", "zeros", "random"):
        for outside in (0, 1):
            grid = grid_of(kind, outside)
            for name, kw in cases.items():
                _, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=kw["perturb"], lindisp=kw.get("lindisp", False), t_rand=kw.get("t_rand"),
                                                  seed=kw.get("seed"))
                c = compact(grid, S, o, d, **kw)
                keep = check_compaction(c, grid, o, d, z, (kind, outside, name, S))
                assert keep[5].all() and keep[6].all()                            # the non-finite origins
                if kind == "ones" and outside == 0:
                    assert c["M"] == R * S and torch.equal(c["index"], torch.arange(R * S, dtype=torch.int32, device="cuda"))
                if kind == "zeros" and outside == 1:
                    assert c["M"] == 2 * S                                        # nothing but the two non-finite rays
                evaluated.add(c["M"])
                again = compact(grid, S, o, d, **kw)                               # two runs give the same bits
                assert all(torch.equal(tbits(a), tbits(b)) for a, b in zip(c["raw"], again["raw"]))
            c = compact(grid, S, o, d, z_in=z_explicit)
            check_compaction(c, grid, o, d, z_explicit, (kind, outside, "z_in", S))
    assert len(evaluated) >= 3                                                    # the cases do differ in what they keep
    # V1 passes no directions buffer: everything else is the same bits
    grid = grid_of("random", 1)
    a, b = compact(grid, S, o, d, perturb=True, seed=5), compact(grid, S, o, d, perturb=True, seed=5, directions=False)
    assert b["intact"] and a["M"] == b["M"] and torch.equal(tbits(a["pos"]), tbits(b["pos"])) and torch.equal(a["index"], b["index"])
    assert torch.equal(a["slot"], b["slot"])


def test_all_zero_grid_keeps_nothing(N):
    o, d = ray_batch(37)
    c = compact(grid_of("zeros", 1), 64, o, d, perturb=True, seed=3)
    assert c["M"] == 0 and c["intact"] and bool((c["slot"] == -1).all())


@pytest.mark.parametrize("S", [5, 65])
def test_pixel_mode_is_ray_mode_on_the_gathered_rays(N, S):
    H, W, R = 40, 56, 37
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    ro, rd = N.get_rays(H, W, focal, pose)
    pix = torch.randint(0, H * W, (R,), generator=torch.Generator().manual_seed(S), dtype=torch.int64).cuda()       # with repeats: the jitter is keyed by the row
    o, d = ro.reshape(-1, 3)[pix].contiguous(), rd.reshape(-1, 3)[pix].contiguous()
    grid = grid_of("random", 1, box=(-1.5, 1.5))
    a = compact(grid, S, pixels=pix, cam=dict(H=H, W=W, focal=focal, pose=pose), perturb=True, seed=7)
    b = compact(grid, S, o, d, perturb=True, seed=7)
    _, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=7)
    check_compaction(a, grid, o, d, z, ("pixels", S))
    assert torch.equal(a["d_out"], d) and torch.equal(b["d_out"], d)              # nrf_get_rays' directions
    assert 0 < a["M"] < R * S
    for k in ("z", "pos", "dirs", "index", "slot"):
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------
# 2. the network's rows
# ---------------------------------------------------------------------------------------------
def staged_forward(model, pts, dirs, cam):
    """The staged saving forward of any family on n points: V1 nrf_encode in front, V3 nrf_project_fetch.  Returns the outputs, the
    context and what the backward needs."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd import train_cli
    from nerf_few_shot_limitations_amd.renderer import make_dino
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    lib = L.lib()
    h, mode = _train_handle(model, dev)
    n = pts.shape[0]
    nbytes = lib.nrf_train_context_bytes(h, mode, n)
    buf = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device=dev)
    ctx = C.c_void_p(buf.data_ptr())
    if model.net == L.NRF_NET_V1:
        enc = torch.empty((n, 3 * (2 * model.pos_freq + 1)), device=dev)
        L.check(lib.nrf_encode(L.ptr(pts), n, 3, model.pos_freq, 1, None, L.ptr(enc), L.stream_ptr()))
        out = torch.empty((n, 4), device=dev)
        L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(enc), n, L.ptr(out), ctx, nbytes, L.stream_ptr()))
        outs = (out,)
    else:
        feats = train_cli.fetch_features(make_dino(**cam), pts) if model.net == L.NRF_NET_V3 else None
        rgb, den = torch.empty((n, 3), device=dev), torch.empty((n, 1), device=dev)
        L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(pts), L.ptr(dirs), L.ptr(feats), n, L.ptr(rgb), L.ptr(den), ctx, nbytes, L.stream_ptr()))
        outs = (rgb, den)
    torch.cuda.synchronize()
    return dict(outs=outs, buf=buf, nbytes=nbytes, h=h, mode=mode, n=n)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("net", ["v1", "v2", "v3"])
def test_compacted_forward_rows_are_the_dense_forward_rows(N, net, mode):
    """R * S = 9 * 32 = 288 samples of a 32 x 32 view; explicit depths put a chosen set of M of them inside the box (3.5 .. 4.5 in
    front of the camera: around the origin) and the others far outside (40 ..), the grid is all ones with outside = skip.  M = 1,
    255, 256, 257: one row, one short of a 256-sample group, a whole group, one more."""
    model = {"v1": make_model, "v2": make_v2, "v3": make_v3}[net](N, mode)[0]
    R, S = 9, 32
    o, d, cam = _v3_scene(64, R, S)
    grid = grid_of("ones", outside=1)
    dense = None
    for M in (1, 255, 256, 257):
        chosen = torch.zeros(R * S, dtype=torch.bool)
        chosen[torch.randperm(R * S, generator=torch.Generator().manual_seed(M))[:M]] = True
        z = torch.where(chosen.reshape(R, S), 3.5 + u01(140, R, S), 40.0 + u01(141, R, S)).cuda().contiguous()
        c = compact(grid, S, o, d, z_in=z)
        assert c["M"] == M and c["intact"] and np.array_equal(c["index"].cpu().numpy(), np.nonzero(chosen.numpy())[0])
        pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).contiguous()
        assert torch.equal(c["pos"], pts[c["index"].long()])
        dense = staged_forward(model, pts, expand_dirs(d, S), cam)
        comp = staged_forward(model, c["pos"].contiguous(), c["dirs"].contiguous(), cam)
        for a, b in zip(comp["outs"], dense["outs"]):
            assert torch.equal(a, b[c["index"].long()]), (net, mode, M)
            assert torch.isfinite(a).all()


# ---------------------------------------------------------------------------------------------
# 3. the step against the dense masked step, assembled from the existing entry points
# ---------------------------------------------------------------------------------------------
def _backward(model, f, rgb, den, g_rgb, g_den):
    from nerf_few_shot_limitations_amd import _lib as L
    grad = torch.zeros(model.flat_params().flat.numel(), device="cuda")
    L.check(L.lib().nrf_mlp_backward(f["h"], f["mode"], L.ptr(rgb), L.ptr(den), L.ptr(g_rgb), L.ptr(g_den), f["n"], C.c_void_p(f["buf"].data_ptr()),
                                     f["nbytes"], L.ptr(grad), L.stream_ptr()))
    torch.cuda.synchronize()
    return grad


@pytest.mark.parametrize("recipe", ["mse", "multi"])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_step_equals_the_dense_masked_step(N, mode, recipe):
    from nerf_few_shot_limitations_amd import _lib as L
    lib = L.lib()
    model, _ = make_v2(N, mode, scene="solid")
    R, S = 50, 33
    n = R * S
    o, d = ray_batch(R, seed=150)
    grid = grid_of("random", outside=1, seed=151, box=(-6.0, 6.0))
    c = compact(grid, S, o, d, perturb=True, seed=152)
    M, index, z = c["M"], c["index"].long(), c["z"].contiguous()
    assert 0.2 * n < M < 0.8 * n
    skipped = torch.ones(n, dtype=torch.bool, device="cuda")
    skipped[index] = False
    tgt = u01(153, R, 3).cuda()
    if recipe == "multi":
        noise = (u01(154, R, S) * 4 - 2).cuda().contiguous()
        noise.view(-1)[torch.nonzero(skipped)[:7, 0]] = 1e6                       # large positive draws on skipped samples: they stay empty
        td = (u01(155, R) * 4 + 2).cuda()
        lo = L.loss_opts(1.0, 0.05, 0.1, L.ptr(td), 0.3, L.ptr(noise), 0)
    else:
        lo = L.loss_opts(0.7)
    st = L.stream_ptr()
    zero_n = model.flat_params().ensure().numel()

    # the dense masked step: all R * S points, skipped samples set to colour 0 / density -inf, nothing else zeroed
    pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).contiguous()
    fd = staged_forward(model, pts, expand_dirs(d, S), None)
    rgb_d, den_d = fd["outs"]
    rgb_m, den_m = rgb_d.clone(), den_d.clone()
    rgb_m[skipped] = 0.0
    den_m[skipped] = float("-inf")
    g_rgb_d, g_den_d = torch.full((n, 3), CANARY, device="cuda"), torch.full((n, 1), CANARY, device="cuda")
    pred_d, terms_d = torch.empty((R, 3), device="cuda"), torch.zeros((3, R), device="cuda")
    junk = torch.ones(zero_n, device="cuda")
    L.check(lib.nrf_composite_loss_backward(L.ptr(rgb_m), 3, L.ptr(den_m), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo), L.ptr(pred_d),
                                            L.ptr(g_rgb_d), 3, L.ptr(g_den_d), 1, L.ptr(terms_d), L.ptr(junk), zero_n, st))
    torch.cuda.synchronize()
    assert bool((g_den_d[skipped] == 0).all()) and bool((g_rgb_d[skipped] == 0).all())      # a skipped sample passes no gradient
    grad_d = _backward(model, fd, rgb_m, den_m, g_rgb_d, g_den_d)

    # the step under the grid: M rows
    fc = staged_forward(model, c["pos"].contiguous(), c["dirs"].contiguous(), None)
    rgb_c, den_c = fc["outs"]
    g_rgb_c, g_den_c = torch.full((M + 8, 3), CANARY, device="cuda"), torch.full((M + 8, 1), CANARY, device="cuda")
    pred_c, terms_c = torch.empty((R, 3), device="cuda"), torch.zeros((3, R), device="cuda")
    junk2 = torch.ones(zero_n, device="cuda")
    L.check(lib.nrf_composite_loss_backward_indexed(L.ptr(rgb_c), 3, L.ptr(den_c), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo),
                                                    c["slot"].data_ptr(), L.ptr(pred_c), L.ptr(g_rgb_c), 3, L.ptr(g_den_c), 1, L.ptr(terms_c),
                                                    L.ptr(junk2), zero_n, st))
    torch.cuda.synchronize()
    assert bool((junk2 == 0).all()) and bool((g_rgb_c[M:] == CANARY).all()) and bool((g_den_c[M:] == CANARY).all())
    grad_c = _backward(model, fc, rgb_c, den_c, g_rgb_c[:M].contiguous(), g_den_c[:M].contiguous())

    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(pred_c), bits(pred_d))
    rows = 3 if recipe == "multi" else 1
    assert torch.equal(bits(terms_c[:rows]), bits(terms_d[:rows]))
    assert torch.equal(bits(g_rgb_c[:M]), bits(g_rgb_d[index])) and torch.equal(bits(g_den_c[:M]), bits(g_den_d[index]))
    assert float(g_den_d.abs().max()) > 0 and float(grad_d.abs().max()) > 0 and bool(torch.isfinite(grad_d).all())
    err = rel_to_max(grad_c, grad_d)
    print(f"step vs dense masked step, {mode} {recipe}: M / (R S) = {M / n:.3f}, flat gradient rel_to_max {err:.3g}")
    assert err < 2e-5
    if recipe == "mse":                                                           # every option off: the mse kernel's bits
        g3, g1 = torch.empty((n, 3), device="cuda"), torch.empty((n, 1), device="cuda")
        pred_m, rl = torch.empty((R, 3), device="cuda"), torch.empty((R,), device="cuda")
        L.check(lib.nrf_composite_mse_backward(L.ptr(rgb_m), 3, L.ptr(den_m), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), 0.7, L.ptr(pred_m), L.ptr(g3), 3,
                                               L.ptr(g1), 1, L.ptr(rl), None, 0, st))
        torch.cuda.synchronize()
        assert torch.equal(bits(pred_m), bits(pred_c)) and torch.equal(bits(rl), bits(terms_c[0]))
        assert torch.equal(bits(g3[index]), bits(g_rgb_c[:M])) and torch.equal(bits(g1[index]), bits(g_den_c[:M]))


# ---------------------------------------------------------------------------------------------
# 4. FusedStep: the all-ones grid, the empty grid, fp32 against autograd
# ---------------------------------------------------------------------------------------------
def full_grid(outside=0):
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    return OccupancyGrid.full(RES, BOX[0], BOX[1], outside=outside, device=torch.device("cuda", 0))


@pytest.mark.parametrize("recipe", ["plain", "multiscale"])
def test_three_v2_steps_under_an_all_ones_grid_are_the_plain_steps(N, recipe):
    from nerf_few_shot_limitations_amd.training import FusedStep
    kw = dict(lr=5e-4, weight_decay=1e-6)
    if recipe == "multiscale":
        kw.update(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True, seed=31)
    sa, sb = FusedStep(make_v2(N, "bf16", scene="solid")[0], **kw), FusedStep(make_v2(N, "bf16", scene="solid")[0], **kw)
    R, S = 37, 65
    o, d = ray_batch(R, seed=160)
    tgt = u01(161, R, 3).cuda()
    grid = full_grid()
    for i in range(3):
        la = sa.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=70 + i)
        lb = sb.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=70 + i, occupancy=grid)
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z) and sb.last_count == R * S, i
        for k in sa.last_losses:
            assert torch.equal(sa.last_losses[k], sb.last_losses[k]), (i, k)
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)
    assert sa.opt.step_count == sb.opt.step_count == 3 and sa.last_count is None


def test_step_view_under_an_all_ones_grid_is_the_plain_step_view(N):
    from nerf_few_shot_limitations_amd.training import FusedStep
    sa, sb = FusedStep(make_v2(N, "bf16", scene="solid")[0], lr=5e-4), FusedStep(make_v2(N, "bf16", scene="solid")[0], lr=5e-4)
    H, W, R, S = 24, 24, 100, 16
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    image = u01(162, H, W, 3).cuda()
    for i in range(2):
        pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(i))[:R].cuda()
        la = sa.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, seed=5 + i)
        lb = sb.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, seed=5 + i, occupancy=full_grid())
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z)
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)


@pytest.mark.parametrize("net", ["v1", "v3"])
def test_three_v1_v3_steps_under_an_all_ones_grid_are_the_staged_steps(N, net):
    """V1 / V3: the plain ray step encodes / gathers inside its kernel, the step under a grid through the staged leaves: bit-equal to
    __call__ on sample_points_along_rays' points with nrf_encode / nrf_project_fetch in front."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd import train_cli
    from nerf_few_shot_limitations_amd.renderer import make_dino
    from nerf_few_shot_limitations_amd.training import FusedStep
    make = make_model if net == "v1" else make_v3
    sa, sb = FusedStep(make(N, "bf16", scene="solid")[0], lr=5e-4, weight_decay=1e-6), FusedStep(make(N, "bf16", scene="solid")[0], lr=5e-4, weight_decay=1e-6)
    R, S = 37, 33
    o, d, cam = _v3_scene(64, R, S)
    tgt = u01(163, R, 3).cuda()
    grid = full_grid()
    for i in range(3):
        pts, z = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=80 + i)
        pts = pts.reshape(-1, 3).contiguous()
        if net == "v1":
            enc = torch.empty((R * S, 63), device="cuda")
            L.check(L.lib().nrf_encode(L.ptr(pts), R * S, 3, 10, 1, None, L.ptr(enc), L.stream_ptr()))
            la = sa(enc, z, d, tgt)
            lb = sb.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=80 + i, occupancy=grid)
        else:
            la = sa(pts, z, d, tgt, dirs=expand_dirs(d, S), dino=train_cli.fetch_features(make_dino(**cam), pts))
            lb = sb.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=80 + i, dino=cam, occupancy=grid)
        assert torch.equal(la, lb) and sb.last_count == R * S, i
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)


@pytest.mark.parametrize("white", [False, True])
def test_a_step_that_keeps_no_sample(N, white):
    from nerf_few_shot_limitations_amd.training import FusedStep
    model, _ = make_v2(N, "bf16", scene="solid")
    step = FusedStep(model, lr=1e-3, rgb_weight=0.5, white_bkgd=white)
    before = model.flat_params().ensure().clone()
    R, S = 37, 5
    o, d = ray_batch(R, seed=170)
    tgt = u01(171, R, 3).cuda()
    loss = step.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=1, occupancy=grid_of("zeros", outside=1))
    bg = 1.0 if white else 0.0
    assert step.last_count == 0 and step.opt.step_count == 1
    assert torch.equal(step.pred, torch.full((R, 3), bg, device="cuda"))          # the prediction is the background
    # (111 squared errors added in fp32, in two different orders: 111 * 2^-24 = 7e-6 at the very worst)
    assert abs(loss.item() - 0.5 * float(((bg - tgt) ** 2).mean())) <= 1e-5 * loss.item()
    assert bool((step.grad == 0).all())                                           # the gradient is zero ...
    assert torch.equal(model.flat_params().flat, before)                          # ... and Adam without decay leaves the parameters
    loss2 = step.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=2, occupancy=full_grid())
    assert step.last_count == R * S and step.opt.step_count == 2 and torch.isfinite(loss2)
    assert not torch.equal(model.flat_params().flat, before)


def test_occupancy_is_refused_where_it_is_not_built(N):
    from nerf_few_shot_limitations_amd.training import FusedStep
    model = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64, mma_mode="bf16", dino_grad=True).cuda().train()
    step = FusedStep(model, lr=1e-3)
    R, S = 8, 4
    o, d, cam = _v3_scene(64, R, S)
    tgt = u01(172, R, 3).cuda()
    with pytest.raises(ValueError, match="d_dino_out / points_out"):
        step.step_rays(o, d, tgt, NEAR, FAR, S, dino=cam, occupancy=full_grid(), d_dino_out=torch.empty(R * S, 64, device="cuda"))
    with pytest.raises(ValueError, match="d_dino_out / points_out"):
        step.step_rays(o, d, tgt, NEAR, FAR, S, dino=cam, occupancy=full_grid(), points_out=torch.empty(R * S, 3, device="cuda"))
    with pytest.raises(TypeError):
        step.step_rays(o, d, tgt, NEAR, FAR, S, dino=cam, occupancy="grid")
    assert step.opt.step_count == 0


@pytest.mark.parametrize("net", ["v1", "v2"])
def test_fp32_step_matches_autograd_of_the_oracle_with_a_masked_density(N, net):
    """Gradients of one f32 step under a random grid against autograd through the oracle's modules with `density * mask`: every
    parameter gradient within 2e-4 of its tensor's largest element, the bound of test_gradients_fp32_mode_match_autograd.  Its ReLU
    margin filter, in the form a step allows (tests/golden/make_golden.py: select_rays): the batch is the first 40 candidate rays
    none of whose EVALUATED samples has a pre-activation within MARGIN of 0 -- a skipped sample carries no gradient on either side."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    model, p = (make_model if net == "v1" else make_v2)(N, "f32", scene="solid")
    S, R = 16, 40
    oc, dc = ray_batch(160, seed=180)
    grid = grid_of("random", outside=1, seed=181, box=(-6.0, 6.0))
    z = torch.from_numpy(np.asarray(O.z_steps(NEAR, FAR, S), np.float32))[None, :].expand(160, S).contiguous()
    keep_all, _ = keep_replay(grid, oc, dc, z)
    pf = (oc.cpu()[:, None, :] + dc.cpu()[:, None, :] * z[..., None]).reshape(-1, 3)
    df = dc.cpu()[:, None, :].expand(160, S, 3).reshape(-1, 3)
    margin = O.relu_margin(p, "v1", O.positional_encoding(pf, 10)) if net == "v1" else O.relu_margin(p, "v2", pf, df)
    clean = ((margin.reshape(160, S) > MARGIN) | ~torch.from_numpy(keep_all)).all(-1)
    rays = torch.nonzero(clean)[:R, 0]
    assert rays.numel() == R, int(clean.sum())
    o, d, z = oc[rays.cuda()].contiguous(), dc[rays.cuda()].contiguous(), z[rays].contiguous()
    tgt = u01(182, R, 3)
    step = FusedStep(model, lr=1e-5)
    loss = step.step_rays(o, d, tgt.cuda(), NEAR, FAR, S, perturb=False, z_in=z.cuda(), occupancy=grid)
    keep = torch.from_numpy(keep_all[rays.numpy()])
    assert step.last_count == int(keep.sum()) and 0.2 * R * S < step.last_count < 0.8 * R * S
    pp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    pf = (o.cpu()[:, None, :] + d.cpu()[:, None, :] * z[..., None]).reshape(-1, 3)
    df = d.cpu()[:, None, :].expand(R, S, 3).reshape(-1, 3)
    if net == "v1":
        o4 = O.mlp_v1(pp, O.positional_encoding(pf, 10))
        rgb, den = o4[:, :3], o4[:, 3:4]
    else:
        rgb, den = O.mlp_v2(pp, pf, df)
    den = den * keep.reshape(-1, 1).float()
    c, _, _ = O.volume_render(rgb.reshape(R, S, 3), den.reshape(R, S, 1), z, d.cpu(), False)
    ref = torch.nn.functional.mse_loss(c, tgt)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * ref.item()
    names = {id(q): name for name, q in model.named_parameters()}
    order = [names[id(q)] for q in model.flat_params().params()]
    worst = max((rel_to_max(gv, pp[name].grad), name) for name, gv in zip(order, model.flat_params().views(step.grad)))
    print(f"{net} f32 step under a grid vs autograd: loss {loss.item():.6g} vs {ref.item():.6g}, worst gradient {worst[0]:.3g} of max ({worst[1]})")
    assert worst[0] < 2e-4, worst


# ---------------------------------------------------------------------------------------------
# 5. a grid that follows the field
# ---------------------------------------------------------------------------------------------
def test_refresh_probes_a_slab_round_robin(N):
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    dev = torch.device("cuda", 0)
    model, _ = make_v2(N, "bf16", scene="fog")
    res, lo, hi = (32, 4, 4), -1.5, 1.5
    grid = OccupancyGrid.full(res, lo, hi, device=dev)
    n_cells, cells, k, decay = 512, 160, 3, 0.9                                   # slabs of 160, 160, 160 and the cut one of 32
    probe = lambda first, n, seed: OccupancyGrid._density(model.eval(), OccupancyGrid.cell_points(res, lo, hi, first, n, k, seed, dev).reshape(-1, 3).contiguous(),
                                                          None).reshape(n, k).max(dim=1).values
    with torch.no_grad():
        threshold = float(probe(0, 160, 100).median())                           # a threshold that splits the first slab
    model.train()
    ema = torch.zeros(n_cells, device=dev)
    mask = torch.ones(n_cells, dtype=torch.bool, device=dev)
    visited = torch.zeros(n_cells, dtype=torch.int64)
    for call in range(9):                                                        # two periods and one call
        first, n = grid.refresh(model, decay=decay, threshold=threshold, samples_per_cell=k, cells=cells, seed=100 + call)
        assert (first, n) == ((call % 4) * 160, 160 if call % 4 < 3 else 32)
        assert model.training                                                     # left as it was found
        with torch.no_grad():
            want = torch.maximum(ema[first:first + n] * decay, probe(first, n, 100 + call))
        model.train()
        ema[first:first + n] = want
        mask[first:first + n] = want > threshold
        assert torch.equal(grid.ema, ema), call                                   # the slab's values; every other cell untouched
        assert torch.equal(grid.to_mask().reshape(-1), mask), call                # bits = value > threshold on the slab, the others as they were
        visited[first:first + n] += 1
        if call in (3, 7):
            assert bool((visited == (call + 1) // 4).all())                       # every cell exactly once per period
    assert 0 < int(mask.sum()) < n_cells
    # a decayed value outlives a probe that no longer finds the cell dense
    g2 = OccupancyGrid.full(res, lo, hi, device=dev)
    g2.ema = torch.full((n_cells,), 1e6, device=dev)
    g2._cursor, g2._refreshes = 0, 0
    g2.refresh(model, decay=0.5, threshold=threshold, samples_per_cell=1)
    assert bool((g2.ema >= 5e5).all()) and g2.occupied_fraction == 1.0
    with pytest.raises(ValueError):
        grid.refresh(model, cells=40)


def test_sixty_steps_with_a_refresh_every_ten_reduce_the_loss(N):
    """A small view trained under a grid that is refreshed from the field every 10 steps: the criterion of
    test_fused_adam_loop_reduces_loss (the loss on a fixed batch falls below 0.7 of where it started)."""
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    from nerf_few_shot_limitations_amd.training import FusedStep
    dev = torch.device("cuda", 0)
    model, _ = make_v2(N, "bf16", scene="fog")
    step = FusedStep(model, lr=1e-3)
    H = W = 24
    S = 32
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
    image = torch.stack([xx, yy, 0.5 * torch.ones_like(xx)], -1).cuda().contiguous()
    pix = torch.arange(H * W, dtype=torch.int64, device=dev)
    grid = OccupancyGrid.full(32, -2.5, 2.5, device=dev)
    losses, counts, threshold = [], [], None
    for i in range(60):
        losses.append(step.step_view(image, pose, H, W, focal, pix, NEAR, FAR, S, perturb=True, seed=900 + i, occupancy=grid).item())
        counts.append(step.last_count)
        if (i + 1) % 10 == 0:
            if threshold is None:
                # the fog field is dense everywhere: the threshold is put at the median of the first probe of the whole grid, so that
                # the run does train with about half of its cells empty and the later refreshes have cells to bring back or drop
                grid.refresh(model, decay=0.95, threshold=0.0, samples_per_cell=2)
                threshold = float(grid.ema.median())
            grid.refresh(model, decay=0.95, threshold=threshold, samples_per_cell=2, cells=grid.n_cells // 2)
    print(f"60 steps under a refreshed grid: loss {losses[0]:.4g} -> {losses[-1]:.4g}, M / (R S) {counts[0] / (H * W * S):.3f} -> "
          f"{counts[-1] / (H * W * S):.3f}, occupied cells {grid.occupied_fraction:.3f}")
    assert all(np.isfinite(losses)) and counts[0] == H * W * S
    assert min(counts) < 0.9 * H * W * S                                          # the grid did skip samples on the way
    assert losses[-1] < 0.7 * losses[0], losses


# ---------------------------------------------------------------------------------------------
# 6. the command
# ---------------------------------------------------------------------------------------------
def test_train_cli_under_a_grid(N, tmp_path):
    """--occupancy-res sends every batch through step_view(occupancy=): with a warm-up longer than the run the grid stays all ones and
    the run is the --fused-inputs run, loss for loss; so is a run whose grid is refreshed but cannot lose a cell; a run whose grid does
    lose cells stays finite, moves, and reports the grid."""
    from tests.test_gpu_training import _CFG, _write_scene
    from nerf_few_shot_limitations_amd import train_cli
    root = str(tmp_path / "scene")
    _write_scene(root)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino="false", pf=10))
    p = dict(O.make_weights("v2", 1, "fog"))
    p["pos_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 9, 10)
    p["dir_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 3, 4)
    torch.save({"epoch": 0, "nerf_model_state_dict": p}, str(tmp_path / "init.pth"))
    common = ["--config", str(cfg), "--data", root, "--mode", "bf16", "--epochs", "4", "--checkpoint", str(tmp_path / "init.pth")]
    plain = train_cli.main(common + ["--out", str(tmp_path / "plain"), "--fused-inputs"])
    ones = train_cli.main(common + ["--out", str(tmp_path / "ones"), "--occupancy-res", "32", "--occupancy-warmup", "1000"])
    assert [r["loss"] for r in ones] == [r["loss"] for r in plain] and [r["psnr"] for r in ones if "psnr" in r] == [r["psnr"] for r in plain if "psnr" in r]
    assert all(r["occupied_fraction"] == 1.0 for r in ones) and all("occupied_fraction" not in r for r in plain)
    # a grid that is refreshed every 2 steps from step 0 on but can lose no cell (the density is a ReLU's output, the threshold below
    # it): the refreshes run the network in eval mode between the steps, the validation renders in f16 follow them at the same
    # parameter version -- and nothing of that may move the run
    kept = train_cli.main(common + ["--out", str(tmp_path / "kept"), "--occupancy-res", "32", "--occupancy-box", "-2.5", "2.5", "--occupancy-warmup", "0",
                                    "--occupancy-refresh-every", "2", "--occupancy-cells-per-refresh", "32768", "--occupancy-threshold", "-1",
                                    "--occupancy-decay", "0.9"])
    assert [r["loss"] for r in kept] == [r["loss"] for r in plain] and all(r["occupied_fraction"] == 1.0 for r in kept)
    assert [r["psnr"] for r in kept if "psnr" in r] == [r["psnr"] for r in plain if "psnr" in r]
    # a grid that does lose cells: the criterion test_train_cli_runs_the_reference_schedule holds a run of this size to -- a dozen
    # noisy steps from a synthetic init need not go down (the plain run above does not), they must stay finite and move
    live = train_cli.main(common + ["--out", str(tmp_path / "live"), "--occupancy-res", "32", "--occupancy-box", "-2.5", "2.5", "--occupancy-warmup", "2",
                                    "--occupancy-refresh-every", "2", "--occupancy-cells-per-refresh", "32768", "--occupancy-threshold", "0.5",
                                    "--occupancy-decay", "0.5"])
    losses = [r["loss"] for r in live]
    print("train_cli: plain epoch losses", [r["loss"] for r in plain], "under a grid that loses cells", losses, "occupied",
          [r["occupied_fraction"] for r in live])
    assert len(losses) == 4 and all(np.isfinite(x) for x in losses) and losses[-1] != losses[0]
    assert all(0.0 <= r["occupied_fraction"] <= 1.0 for r in live)


@pytest.mark.parametrize("under_grid", [True, False])
def test_a_render_in_another_mode_between_a_refresh_and_a_step(N, under_grid):
    """refresh packs the training mode's streams from the stepped parameters; a validation render in another mode at the same
    parameter version must not leave the training mode's backward weights stale (nerf_model.handle packs both in one call)."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    model, _ = make_v2(N, "bf16", scene="solid")
    step = FusedStep(model, lr=5e-4)
    R, S = 37, 8
    o, d = ray_batch(R, seed=190)
    tgt = u01(191, R, 3).cuda()
    grid = full_grid()
    occ = dict(occupancy=grid) if under_grid else {}
    first = step.step_rays(o, d, tgt, NEAR, FAR, S, seed=1, **occ)
    grid.refresh(model, threshold=-1e30)                                           # (every cell stays occupied)
    model.eval()
    with torch.no_grad():
        out = N.render_rays(model, o, d, NEAR, FAR, S, mma_mode="f16")
    model.train()
    second = step.step_rays(o, d, tgt, NEAR, FAR, S, seed=2, **occ)
    assert torch.isfinite(out["rgb"]).all() and torch.isfinite(first) and torch.isfinite(second) and step.opt.step_count == 2
