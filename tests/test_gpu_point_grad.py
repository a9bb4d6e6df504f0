"""GPU tests of the V3 point gradient: fetch_points_backward_kernel (csrc/staged_kernels.hip: nrf_project_fetch_backward_points,
nrf_sample_features_backward_points), input_grad_v3_kernel (csrc/train_input_grad_v3_impl.hpp: nrf_mlp_backward_inputs_v3) and the
opt-in Python surface on top of them -- NeRFMLP(use_dino=True, point_grad=True), project_points_to_image / sample_features_at_points
with point_grad=True, render_rays with rays or depths that require grad, density_normals with a source view.

dL/d point has two paths of very different size: through the positional encoding (0.1 .. 0.6 on the fields used here) and through
the fetched features (2e-4 .. 6e-3).  A test of the sum at 2e-4 of its largest element cannot see a wrong feature path, so that
path is tested on its own, at its own scale.  The bilinear fetch has a kink at every texel edge: the comparisons with autograd
run over the samples more than 1e-3 texel from an edge, and a stated share of the samples has to remain."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_training_host import train_plan
from tests.train_ctx import SavedContext

pytestmark = pytest.mark.gpu

MARGIN = 4e-5          # samples with a ReLU within this of its threshold are masked (their mask is decided by rounding)
EDGE = 1e-3            # texels: samples nearer to a texel edge are left out of the comparisons with autograd
PE, DE = 75, 27
U24 = 2.0 ** -24


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


def u01(seed, *shape):
    return torch.from_numpy(O.uniform01(seed, int(np.prod(shape))).reshape(shape)).float()


def make_v3(N, mode, scene="solid", n_layers=3, dino_dim=64, seed=2, point_grad=True, **kw):
    m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=n_layers, use_dino=True, dino_dim=dino_dim, mma_mode=mode,
                  point_grad=point_grad, **kw)
    p = O.make_weights("v3", seed, scene, n_layers=n_layers, dino_dim=dino_dim)
    m.load_state_dict(p, strict=False)
    return m.cuda().train(), p


def rel_to_max(a, b):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cosine(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def views():
    from tests.conftest import load_golden
    g = load_golden("dino_views")
    return {k: dict(pose=torch.from_numpy(g[k + "_pose"].copy()), focal=float(g[k + "_focal"]), H=int(g[k + "_H"]), W=int(g[k + "_W"]))
            for k in ("orbit", "near")}


def random_map(Hp, Wp, Cc, seed=403):
    return (u01(seed, 1, Hp, Wp, Cc) * 2 - 1).contiguous()


def edge_distance(xy, Hp, Wp):
    gx, gy = ((xy[:, 0] + 1) * Wp - 1) / 2, ((xy[:, 1] + 1) * Hp - 1) / 2
    fx, fy = gx - torch.floor(gx), gy - torch.floor(gy)
    return torch.minimum(torch.minimum(fx, 1 - fx), torch.minimum(fy, 1 - fy))


def any_tap_on_map(xy, Hp, Wp):
    gx, gy = ((xy[:, 0] + 1) * Wp - 1) / 2, ((xy[:, 1] + 1) * Hp - 1) / 2
    x0, y0 = torch.floor(gx), torch.floor(gy)
    return (x0 >= -1) & (x0 <= Wp - 1) & (y0 >= -1) & (y0 <= Hp - 1)


def dino_struct(L, fmap, v):
    inv = torch.inverse(v["pose"])
    return L.nrf_dino(fmap.data_ptr(), int(fmap.shape[1]), int(fmap.shape[2]), int(fmap.shape[3]), (C.c_float * 16)(*inv.reshape(-1).tolist()),
                      v["focal"], v["H"], v["W"])


def fetch_points_T(L, fmap, v, pts, g, out=None):
    """nrf_project_fetch_backward_points (pts (n,3)) / nrf_sample_features_backward_points (pts (n,2)); `out` given: accumulate."""
    n = pts.shape[0]
    if pts.shape[1] == 2:
        res = torch.full((n, 2), float("nan"), device="cuda")
        L.check(L.lib().nrf_sample_features_backward_points(L.ptr(fmap), int(fmap.shape[1]), int(fmap.shape[2]), int(fmap.shape[3]), L.ptr(pts), n,
                                                            L.ptr(g), L.ptr(res), L.stream_ptr()))
        return res
    d = dino_struct(L, fmap, v)
    res = out if out is not None else torch.full((n, 3), float("nan"), device="cuda")          # accumulate = 0 must overwrite
    L.check(L.lib().nrf_project_fetch_backward_points(C.byref(d), L.ptr(pts), n, L.ptr(g), L.ptr(res), int(out is not None), L.stream_ptr()))
    return res


# ---------------------------------------------------------------------------------------------
# fetch_points_backward_kernel alone
# ---------------------------------------------------------------------------------------------
MAPS = [(9, 9, 64), (10, 12, 128), (14, 22, 64), (37, 37, 128)]


@functools.lru_cache(maxsize=None)
def fetch_reference(shape, n, view):
    """Inputs and fp32 autograd through the oracle's projection and tap-by-tap fetch, computed once per case: points u01 * 4 - 2,
    a random map and a random upstream gradient; d_points, d_xy, the projections and the mask of samples off the texel edges."""
    Hp, Wp, Cc = shape
    v = views()[view]
    pts = (u01(411, n, 3) * 4 - 2).contiguous()
    fmap = random_map(Hp, Wp, Cc, seed=412)
    g = (u01(413, n, Cc) - 0.5).contiguous()
    p = pts.clone().requires_grad_(True)
    xy = O.project_points_to_image(p, v["pose"], v["focal"], v["H"], v["W"])[0]
    xy.retain_grad()
    (O.sample_features_at_points(fmap, xy) * g).sum().backward()
    xyd = xy.detach()
    return dict(pts=pts, fmap=fmap, g=g, xy=xyd, d_pts=p.grad, d_xy=xy.grad, keep=edge_distance(xyd, Hp, Wp) > EDGE, on=any_tap_on_map(xyd, Hp, Wp))


@pytest.mark.parametrize("view", ["orbit", "near"])
@pytest.mark.parametrize("n", [1, 33, 257, 4113])
@pytest.mark.parametrize("shape", MAPS)
def test_fetch_adjoint_matches_autograd(L, shape, n, view):
    """d_points (world points) and d_xy (points2d mode) against autograd through the oracle, each within 2e-4 of ITS OWN largest
    element, over the samples more than 1e-3 texel from an edge -- at least 0.9 of them (the share is a property of the inputs: a
    single sample either is or is not); samples with no tap on the map get exactly 0 in every component."""
    r = fetch_reference(shape, n, view)
    v = views()[view]
    fmap, pts, g, xy = r["fmap"].cuda(), r["pts"].cuda(), r["g"].cuda(), r["xy"].cuda().contiguous()
    d_pts = fetch_points_T(L, fmap, v, pts, g).cpu()
    d_xy = fetch_points_T(L, fmap, v, xy, g).cpu()
    keep, on = r["keep"], r["on"]
    share = float(keep.float().mean())
    print(f"\nRECORD fetch adjoint {shape} n {n} {view}: kept {share:.3f}, with a tap on the map {float(on.float().mean()):.3f}")
    if n > 1:
        assert share >= 0.9, share
    assert torch.isfinite(d_pts).all() and torch.isfinite(d_xy).all()
    far = ~on & keep
    assert not d_pts[far].any() and not d_xy[far].any()
    assert not torch.signbit(d_pts[far]).any() and not torch.signbit(d_xy[far]).any()           # +0, not -0
    for name, got, want in (("d_points", d_pts, r["d_pts"]), ("d_xy", d_xy, r["d_xy"])):
        if not keep.any() or want[keep].abs().max() == 0:
            assert not got[keep].any()
            continue
        e = rel_to_max(got[keep], want[keep])
        print(f"RECORD   {name}: {e:.3e} of its largest element {float(want[keep].abs().max()):.3e}")
        assert e <= 2e-4, (name, e)
    # accumulate adds exactly that result onto what d_points holds
    base = u01(414, n, 3).cuda()
    assert torch.equal(fetch_points_T(L, fmap, v, pts, g, out=base.clone()).cpu(), (base + d_pts.cuda()).cpu())


def test_fetch_adjoint_against_the_reference_fixture(L, golden):
    """point_grads.npz: the reference's retained d_feats in, its d_points_feat (autograd through F.grid_sample and the projection) out,
    within 2e-4 of the largest element of d_points_feat."""
    f = golden("point_grads")
    v = dict(pose=torch.from_numpy(f["pose"].copy()), focal=float(f["focal"]), H=int(f["H"]), W=int(f["W"]))
    pts = torch.from_numpy((f["rays_o"][:, None, :] + f["rays_d"][:, None, :] * f["z"][:, :, None]).reshape(-1, 3).astype(np.float32))
    got = fetch_points_T(L, torch.from_numpy(f["fmap"]).cuda(), v, pts.cuda().contiguous(), torch.from_numpy(f["d_feats"]).cuda())
    e = rel_to_max(got, f["d_points_feat"])
    print(f"\nRECORD fixture d_points_feat: {e:.3e} of its largest element {np.abs(f['d_points_feat']).max():.3e}")
    assert e <= 2e-4, e


def test_fetch_adjoint_poisoned_map(L, golden):
    """NaN at texel (0,0), +Inf at the last texel and NaN at one interior texel (the pattern of dino_views.npz): exactly the
    samples that have such a texel among their on-map taps are non-finite, in both modes; every other sample has the bits the
    clean map gives (an off-map tap is selected out, never multiplied by 0)."""
    g = golden("dino_views")
    v = views()["orbit"]
    clean = torch.from_numpy(g["map64"].copy())
    Hp, Wp, Cc = (int(s) for s in clean.shape[1:])
    bad = [tuple(int(q) for q in t) for t in g["bad_texels"]]
    assert bad == [(0, 0), (Hp - 1, Wp - 1), (6, 9)]
    poisoned = clean.clone()
    poisoned[0, 0, 0], poisoned[0, Hp - 1, Wp - 1], poisoned[0, 6, 9] = float("nan"), float("inf"), float("nan")
    xy = torch.from_numpy(g["fetch_xy"].copy()).contiguous()
    n = xy.shape[0]
    up = (u01(421, n, Cc) - 0.5).contiguous()
    # the kernel's own fp32 arithmetic for the cell of every sample
    x32 = xy.numpy()
    gx = ((x32[:, 0] + np.float32(1)) * np.float32(Wp) - np.float32(1)) * np.float32(0.5)
    gy = ((x32[:, 1] + np.float32(1)) * np.float32(Hp) - np.float32(1)) * np.float32(0.5)
    x0, y0 = np.floor(gx).astype(int), np.floor(gy).astype(int)
    hit = np.zeros(n, bool)
    for dy in (0, 1):
        for dx in (0, 1):
            hit |= np.array([(y, x) in bad for y, x in zip(y0 + dy, x0 + dx)])          # a bad texel is on the map by definition
    assert 3 <= hit.sum() < n
    a = fetch_points_T(L, poisoned.cuda(), v, xy.cuda(), up.cuda()).cpu()
    b = fetch_points_T(L, clean.cuda(), v, xy.cuda(), up.cuda()).cpu()
    assert torch.isfinite(b).all()
    assert np.array_equal((~torch.isfinite(a).all(-1)).numpy(), hit)
    assert torch.equal(a[~hit], b[~hit])
    # world points: lift the same image points onto the plane Z = 3 in front of the orbit camera
    pc = torch.stack([(xy[:, 0] + 1) / 2 * v["W"] - v["W"] / 2, (xy[:, 1] + 1) / 2 * v["H"] - v["H"] / 2], -1) / v["focal"] * 3.0
    world = (torch.cat([pc, torch.full((n, 1), 3.0)], -1) @ v["pose"][:3, :3].T + v["pose"][:3, 3]).contiguous()
    xyw = O.project_points_to_image(world, v["pose"], v["focal"], v["H"], v["W"])[0]
    sure = (edge_distance(xyw, Hp, Wp) > EDGE) & (edge_distance(xy, Hp, Wp) > EDGE)      # the lift moves a point by rounding: judge the cells away from the edges
    a3 = fetch_points_T(L, poisoned.cuda(), v, world.cuda(), up.cuda()).cpu()
    b3 = fetch_points_T(L, clean.cuda(), v, world.cuda(), up.cuda()).cpu()
    bad3 = ~torch.isfinite(a3).all(-1)
    assert sure.float().mean() >= 0.4 and hit[sure.numpy()].sum() >= 3      # (half of the fixture's points sit on texel edges on purpose)
    assert np.array_equal(bad3[sure].numpy(), hit[sure.numpy()])
    assert torch.equal(a3[~bad3], b3[~bad3])


@pytest.mark.parametrize("Cc", [3, 66])
def test_fetch_adjoint_takes_any_channel_count_and_alignment(L, Cc):
    """C no multiple of 4 (scalar loads) and a d_feats base that is only 4-byte aligned: the same sums in the same order."""
    n, Hp, Wp = 257, 5, 7
    v = views()["near"]
    pts = (u01(431, n, 3) * 4 - 2).contiguous()
    fmap, g = random_map(Hp, Wp, Cc, seed=432), (u01(433, n, Cc) - 0.5).contiguous()
    p = pts.clone().requires_grad_(True)
    xy = O.project_points_to_image(p, v["pose"], v["focal"], v["H"], v["W"])[0]
    (O.sample_features_at_points(fmap, xy) * g).sum().backward()
    keep = edge_distance(xy.detach(), Hp, Wp) > EDGE
    got = fetch_points_T(L, fmap.cuda(), v, pts.cuda(), g.cuda())
    assert p.grad[keep].abs().max() > 0 and rel_to_max(got.cpu()[keep], p.grad[keep]) <= 2e-4
    if Cc % 4 == 0:
        return
    shifted = torch.empty(n * Cc + 1, device="cuda")[1:]         # 4-byte aligned, not 16
    shifted.copy_(g.cuda().reshape(-1))
    assert torch.equal(fetch_points_T(L, fmap.cuda(), v, pts.cuda(), shifted.view(n, Cc)), got)


def test_fetch_adjoint_misaligned_rows_give_the_same_bits(L):
    """C = 64 through the 16-byte path and, from a base that is only 4-byte aligned, through the scalar path: bit-identical."""
    n, shape = 257, (14, 22, 64)
    r = fetch_reference(shape, n, "orbit")
    v = views()["orbit"]
    fmap, pts, g = r["fmap"].cuda(), r["pts"].cuda(), r["g"].cuda()
    a = fetch_points_T(L, fmap, v, pts, g)
    shifted = torch.empty(n * 64 + 1, device="cuda")[1:]
    shifted.copy_(g.reshape(-1))
    assert torch.equal(fetch_points_T(L, fmap, v, pts, shifted.view(n, 64)), a) and a.abs().max() > 0


# ---------------------------------------------------------------------------------------------
# input_grad_v3_kernel alone: the features are an independent input
# ---------------------------------------------------------------------------------------------
def v3_inputs(n, dino_dim=64, seed=25):
    pos = u01(seed, n, 3) * 4 - 2
    dirs = u01(seed + 1, n, 3) - 0.5
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    return pos, dirs, u01(seed + 9, n, dino_dim) * 2 - 1, u01(seed + 2, n, 3) - 0.5, u01(seed + 3, n, 1) - 0.5


def raw_run(L, model, pos, dirs, dino, g_rgb, g_den, want=("p", "d"), pad=0, feats_too=False):
    """One forward_train / backward / backward_inputs_v3 [/ backward_dino] through the C ABI.  The outputs have `pad` more rows than
    samples and start as NaN.  Returns (return code, {name: tensor}, context buffer)."""
    from nerf_few_shot_limitations_amd import training as TR
    dev = torch.device("cuda", torch.cuda.current_device())
    h, mode = TR._train_handle(model, dev)
    lib, n = L.lib(), pos.shape[0]
    nbytes = lib.nrf_train_context_bytes(h, mode, n)
    assert nbytes >= 0
    buf = torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    grad = torch.zeros_like(model.flat_params().flat)
    cb, st = C.c_void_p(buf.data_ptr()), L.stream_ptr()
    pc, dc, fc = pos.cuda().contiguous(), dirs.cuda().contiguous(), dino.cuda().contiguous()
    rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    den = torch.empty((n, 1), dtype=torch.float32, device=dev)
    gr, gd = g_rgb.cuda().contiguous(), g_den.cuda().contiguous()
    L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(pc), L.ptr(dc), L.ptr(fc), n, L.ptr(rgb), L.ptr(den), cb, nbytes, st))
    L.check(lib.nrf_mlp_backward(h, mode, L.ptr(rgb), L.ptr(den), L.ptr(gr), L.ptr(gd), n, cb, nbytes, L.ptr(grad), st))
    outs = {k: torch.full((n + pad, 3), float("nan"), dtype=torch.float32, device=dev) for k in ("p", "d") if k in want}
    rc = lib.nrf_mlp_backward_inputs_v3(h, mode, n, cb, nbytes, L.ptr(pc), L.ptr(dc), L.ptr(outs.get("p")), L.ptr(outs.get("d")), st)
    if feats_too:
        outs["f"] = torch.empty((n, dino.shape[1]), dtype=torch.float32, device=dev)
        L.check(lib.nrf_mlp_backward_dino(h, mode, n, cb, nbytes, L.ptr(outs["f"]), st))
    torch.cuda.synchronize()
    return rc, outs, buf


def oracle_input_grads(p, pos, dirs, dino, g_rgb, g_den, feats_too=False):
    po, do = pos.clone().requires_grad_(True), dirs.clone().requires_grad_(True)
    fo = dino.clone().requires_grad_(feats_too)
    rgb, den = O.mlp_v3(p, po, do, fo)
    ((rgb * g_rgb).sum() + (den * g_den).sum()).backward()
    return po.grad, do.grad, fo.grad


@pytest.mark.parametrize("dino_dim", [64, 128])
@pytest.mark.parametrize("n_layers", [2, 3, 8])
@pytest.mark.parametrize("n", [1, 33, 4113])
def test_encoding_path_fp32_mode_matches_autograd(N, L, n, n_layers, dino_dim):
    """nrf_mlp_backward_inputs_v3 in fp32 mode against autograd through O.mlp_v3 with respect to positions and directions, the
    features held fixed, over the samples whose ReLU margin exceeds 4e-5: 2e-4 of the largest element."""
    model, p = make_v3(N, "f32", n_layers=n_layers, dino_dim=dino_dim)
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n, dino_dim)
    keep = (O.relu_margin(p, "v3", pos, dirs, dino) > MARGIN)[:, None]
    g_rgb, g_den = g_rgb * keep, g_den * keep
    rc, outs, _ = raw_run(L, model, pos, dirs, dino, g_rgb, g_den)
    assert rc == 0, L.lib().nrf_last_error()
    want_p, want_d, _ = oracle_input_grads(p, pos, dirs, dino, g_rgb, g_den)
    for name, got, want in (("positions", outs["p"], want_p), ("directions", outs["d"], want_d)):
        if want.abs().max() == 0:
            assert not got.any()
            continue
        e = rel_to_max(got, want)
        print(f"\nRECORD f32 v3 n {n} depth {n_layers} C {dino_dim}: d_{name} {e:.3e} of the largest element {float(want.abs().max()):.3e}")
        assert e <= 2e-4, (name, e)
    # NeRFMLP.forward hands out the same bits
    pc, dc = pos.cuda().requires_grad_(True), dirs.cuda().requires_grad_(True)
    rgb, den = model(pc, dc, dino.cuda())
    ((rgb * g_rgb.cuda()).sum() + (den * g_den.cuda()).sum()).backward()
    assert torch.equal(pc.grad, outs["p"]) and torch.equal(dc.grad, outs["d"])


@pytest.mark.parametrize("n", [33, 3000])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_16_bit_products_are_exact_up_to_the_accumulation(N, L, mode, n):
    """The 16-bit kernels against quantize(W0p)^T d1 + w0 quantize(W0p)^T d2 in float64, d1, d2 and the gate decoded from the context
    (tests/train_ctx.py).  Every 16-bit x 16-bit product is exact in the fp32 accumulator, so only the 256-term sums round:
    |err| <= 256 * 2^-24 * (sum_k |w_k d1_k| + |w0| sum_k |w_k d2_k|) per encoded feature (derived, not measured; both passes' terms).
    The kernel has no encoded output, so the products are checked through the adjoint, as for V2: d = sum_u coef_u prod_u with
    coef_u = +-2^f cos|sin(2^f x) or 1, bound sum_u |coef_u| B_u + 40 * 2^-24 * sum_u |coef_u prod_u| (at most 39 fp32 additions, two
    multiplications and a sincosf of <= 2 ulp per term; the argument x * 2^f is exact).  The direction tile likewise, K = 128."""
    depth = 3
    model, p = make_v3(N, mode, n_layers=depth)
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n)
    rc, outs, buf = raw_run(L, model, pos, dirs, dino, g_rgb, g_den)
    assert rc == 0, L.lib().nrf_last_error()
    ctx = SavedContext(train_plan(L, "v3", p, depth, with_planes=True), "v3", depth, mode, n, buf)
    w0 = ctx.gate()[:n, 0].astype(np.float64)

    def product(wname, cols, dz):
        w = O.quantize(p[wname][:, cols], mode).double().numpy()     # (K, F)
        dz = dz.astype(np.float64)                                   # (K, n)
        return w.T @ dz, np.abs(w).T @ np.abs(dz)

    def adjoint(prod, mag, x, Lf, k_terms):
        x32 = x.numpy().astype(np.float32)
        d = np.zeros((x.shape[0], 3))
        bound = np.zeros_like(d)
        for c in range(3):
            terms = [(np.ones(x.shape[0]), c)]
            for f in range(Lf):
                arg = (x32[:, c] * np.float32(2.0 ** f)).astype(np.float64)
                terms += [(2.0 ** f * np.cos(arg), 3 + 6 * f + c), (-(2.0 ** f) * np.sin(arg), 3 + 6 * f + 3 + c)]
            for coef, idx in terms:
                d[:, c] += coef * prod[idx]
                bound[:, c] += np.abs(coef) * k_terms * U24 * mag[idx] + 40 * U24 * np.abs(coef * prod[idx])
        return d, bound

    p1, m1 = product("dino_fusion.fusion.0.weight", slice(0, PE), ctx.slot("dz_fusion0.0")[:, :n])
    p2, m2 = product("dino_fusion.fusion.0.weight", slice(0, PE), ctx.slot("dz_fusion0.1")[:, :n])
    prod, mag = p1 + w0[None, :] * p2, m1 + np.abs(w0)[None, :] * m2
    assert np.abs(p1).max() > 0 and np.abs(p2).max() > 0
    want, bound = adjoint(prod, mag, pos, 12, 256)
    got = outs["p"].cpu().double().numpy()
    print(f"\nRECORD {mode} v3 n {n}: d_positions worst |err| / bound {float((np.abs(got - want) / (bound + 1e-300)).max()):.3f}")
    assert (np.abs(got - want) <= bound).all()
    prod, mag = product("color_mlp.color_layers.0.weight", slice(256, 256 + DE), ctx.slot("dz_c0")[:, :n])
    want, bound = adjoint(prod, mag, dirs, 4, 128)
    got = outs["d"].cpu().double().numpy()
    print(f"RECORD {mode} v3 n {n}: d_directions worst |err| / bound {float((np.abs(got - want) / (bound + 1e-300)).max()):.3f}")
    assert np.abs(want).max() > 0 and (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("mode,cos_min", [("bf16", 0.97), ("f16", 0.995)])
def test_16_bit_encoding_path_end_to_end(N, L, mode, cos_min):
    """d_positions / d_directions of the 16-bit modes against the oracle's fp32 autograd gradient, n = 3000, 8 trunk layers: the
    project's bars for 16-bit gradients (cosine > 0.97 bf16, > 0.995 f16).  The d_feats cosine of the same batch, from the same dZ
    tiles, is printed beside them."""
    n, depth = 3000, 8
    model, p = make_v3(N, mode, scene="fog", n_layers=depth)
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n)
    keep = (O.relu_margin(p, "v3", pos, dirs, dino) > MARGIN)[:, None]
    g_rgb, g_den = g_rgb * keep, g_den * keep
    rc, outs, _ = raw_run(L, model, pos, dirs, dino, g_rgb, g_den, feats_too=True)
    assert rc == 0
    want_p, want_d, want_f = oracle_input_grads(p, pos, dirs, dino, g_rgb, g_den, feats_too=True)
    c_p, c_d, c_f = cosine(outs["p"], want_p), cosine(outs["d"], want_d), cosine(outs["f"], want_f)
    print(f"\nRECORD {mode} v3 n {n} depth {depth}: cosine vs the oracle's fp32 autograd: d_positions {c_p:.5f} d_directions {c_d:.5f} d_feats {c_f:.5f}")
    assert c_p > cos_min and c_d > cos_min, (c_p, c_d, c_f)


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_bit_properties_of_the_two_kernels(N, L, mode):
    """Two runs give the same bits; a sample's rows do not depend on the batch around it (n = 33 inside n = 3000); rows >= n of a
    NaN-filled output stay NaN; one output at a time gives the bits of both together."""
    model, p = make_v3(N, mode)
    big = v3_inputs(3000)
    rc, a, _ = raw_run(L, model, *big, feats_too=True)
    rc2, b, _ = raw_run(L, model, *big, feats_too=True)
    assert rc == 0 and rc2 == 0
    k = 33
    small = tuple(t[:k] for t in big)
    rc, s, _ = raw_run(L, model, *small, pad=37, feats_too=True)
    assert rc == 0
    for name in ("p", "d"):
        assert torch.isfinite(a[name]).all() and a[name].abs().max() > 0, name
        assert torch.equal(a[name], b[name]), name
        assert torch.equal(s[name][:k], a[name][:k]), name
        assert torch.isnan(s[name][k:]).all(), name
        rc, one, _ = raw_run(L, model, *small, want=(name,))
        assert rc == 0 and torch.equal(one[name], s[name][:k]), name
    # the fetch adjoint on the feature gradients of the two batches
    v = views()["orbit"]
    fmap = random_map(14, 22, 64).cuda()
    pts = big[0].cuda().contiguous()
    fa = fetch_points_T(L, fmap, v, pts, a["f"])
    assert torch.equal(fa, fetch_points_T(L, fmap, v, pts, a["f"])) and fa.abs().max() > 0
    assert torch.equal(fetch_points_T(L, fmap, v, pts[:k].contiguous(), a["f"][:k].contiguous()), fa[:k])


# ---------------------------------------------------------------------------------------------
# the whole chain
# ---------------------------------------------------------------------------------------------
def fixture_case(f):
    v = dict(pose=torch.from_numpy(f["pose"].copy()), focal=float(f["focal"]), H=int(f["H"]), W=int(f["W"]))
    t = {k: torch.from_numpy(f[k].copy()) for k in ("rays_o", "rays_d", "z", "target", "fmap")}
    return v, t


def pieces_route(N, model, o, d, z, fmap, v, loss_of, feature_grad=False):
    """The public pieces: points = o + z d (plain torch) -> project_points_to_image -> sample_features_at_points -> NeRFMLP.forward
    -> training.composite(geom_grad=True).  Returns (loss, rgb, depth, points)."""
    from nerf_few_shot_limitations_amd import training as TR
    R, S = z.shape
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    pts.retain_grad()
    xy = N.project_points_to_image(pts, v["pose"], v["focal"], v["H"], v["W"], point_grad=True)[0]
    feats = N.sample_features_at_points(fmap, xy, feature_grad=feature_grad, point_grad=True)
    rgb, den = model(pts, d[:, None, :].expand(R, S, 3).reshape(-1, 3), feats)
    c, dep, _ = TR.composite(torch.cat([rgb, den], -1).reshape(R, S, 4), z, d, False, geom_grad=True)
    return loss_of(c, dep), c, dep, pts


def test_whole_chain_against_the_reference_fixture(N, L, golden):
    """point_grads.npz, fp32 mode: loss within 1e-6 relative; d_rays_o, d_rays_d, d_z and the retained d_points within 2e-4 of the
    largest element, through the public pieces and through render_rays' one node.  Separately the feature-path share of d_points --
    total minus encoding path, both from the staged entry points -- against the reference's d_points_feat at ITS scale."""
    f = golden("point_grads")
    v, t = fixture_case(f)
    model, _ = make_v3(N, "f32", seed=1, n_layers=3)
    o, d, z = (t[k].cuda().requires_grad_(True) for k in ("rays_o", "rays_d", "z"))
    tgt, fmap = t["target"].cuda(), t["fmap"].cuda()
    mse = lambda c, dep: ((c - tgt) ** 2).mean()
    loss, c, _, pts = pieces_route(N, model, o, d, z, fmap, v, mse)
    loss.backward()
    print(f"\nRECORD fixture chain: loss {loss.item():.8e} vs {float(f['loss']):.8e}")
    assert abs(loss.item() - float(f["loss"])) <= 1e-6 * float(f["loss"])
    assert rel_to_max(c, f["pred"]) <= 1e-5
    for name, got in (("d_rays_o", o.grad), ("d_rays_d", d.grad), ("d_z", z.grad), ("d_points", pts.grad)):
        e = rel_to_max(got, f[name])
        print(f"RECORD   pieces {name}: {e:.3e} of the largest element {np.abs(f[name]).max():.3e}")
        assert e <= 2e-4, (name, e)
    o2, d2, z2 = (t[k].cuda().requires_grad_(True) for k in ("rays_o", "rays_d", "z"))
    out = N.render_rays(model, o2, d2, 2.0, 6.0, z.shape[1], perturb=False, z_in=z2, dino=dict(features=fmap, **v))
    mse(out["rgb"], None).backward()
    for name, got in (("d_rays_o", o2.grad), ("d_rays_d", d2.grad), ("d_z", z2.grad)):
        e = rel_to_max(got, f[name])
        print(f"RECORD   one node {name}: {e:.3e}")
        assert e <= 2e-4, (name, e)
    # the feature path on its own: the same upstream gradients through the staged entry points
    R, S = z.shape
    P = pts.detach().contiguous()
    dirs = t["rays_d"][:, None, :].expand(R, S, 3).reshape(-1, 3)
    feats = N.sample_features_at_points(fmap, N.project_points_to_image(P, v["pose"], v["focal"], v["H"], v["W"])[0])
    rgb, den = model(P.clone().requires_grad_(True), dirs.cuda(), feats)
    o4 = torch.cat([rgb, den], -1).detach().reshape(R, S, 4).requires_grad_(True)
    from nerf_few_shot_limitations_amd import training as TR
    mse(TR.composite(o4, z.detach(), d.detach(), False)[0], None).backward()
    g = o4.grad.reshape(-1, 4)
    rc, outs, _ = raw_run(L, model, P.cpu(), dirs, feats.cpu(), g[:, :3].cpu(), g[:, 3:4].cpu(), want=("p",), feats_too=True)
    assert rc == 0
    total = fetch_points_T(L, fmap, v, P, outs["f"], out=outs["p"].clone())
    share = total - outs["p"]
    e = rel_to_max(share, f["d_points_feat"])
    ratio = float(outs["p"].abs().max() / share.abs().max())
    print(f"RECORD   feature-path share: {e:.3e} of its largest element {np.abs(f['d_points_feat']).max():.3e}; encoding path / feature path {ratio:.0f}x")
    assert e <= 2e-4, e                                          # (the fp32 sum it is taken from rounds at 2^-24 * 3.4 / 6.7e-3 = 3e-5 of it)
    assert rel_to_max(total, f["d_points"]) <= 2e-4


def grid_rays(R, first=0):
    """R consecutive rays of the 20 x 20 camera at O.LEGO_LIKE_C2W, from ray `first` on."""
    o, d = O.get_rays(20, 20, O.focal_for(20), torch.from_numpy(O.LEGO_LIKE_C2W.copy()))
    return o.reshape(-1, 3)[first:first + R].contiguous(), d.reshape(-1, 3)[first:first + R].contiguous()


def oracle_chain(p, o, d, z, fmap, v, loss_of):
    """autograd through the oracle, piece by piece; returns (loss, per-ray clean mask: ReLU margins and texel edges)."""
    R, S = z.shape
    pf = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    df = d[:, None, :].expand(R, S, 3).reshape(-1, 3)
    xy = O.project_points_to_image(pf, v["pose"], v["focal"], v["H"], v["W"])[0]
    feats = O.sample_features_at_points(fmap, xy)
    rgb, den = O.mlp_v3(p, pf, df, feats)
    c, dep, _ = O.volume_render(rgb.reshape(R, S, 3), den.reshape(R, S, 1), z, d, False)
    margin = O.relu_margin(p, "v3", pf.detach(), df.detach(), feats.detach()).reshape(R, S)
    edge = edge_distance(xy.detach(), int(fmap.shape[1]), int(fmap.shape[2])).reshape(R, S)
    return loss_of(c, dep), ((margin > MARGIN) & (edge > EDGE)).all(-1)


def test_routes_agree_and_match_autograd(N):
    """Route A: render_rays on a point_grad module with rays that require grad, a live feature map and live parameters -- one node.
    Route B: the same loss through the public pieces.  Ray gradients, parameter gradients and d_map are bit-equal; and (fp32 mode,
    R = 37, S = 16) the ray gradients are within 2e-4 of the largest element of autograd through the oracle over the clean rays (no
    sample within 4e-5 of a ReLU threshold or 1e-3 texel of an edge), at least 0.25 of the rays.  With 16 samples a ray is clean
    less often than with the fixture's 8: the field ('solid', seed 5, 2 trunk layers) and the block of rays (the image's middle
    rows) are the ones for which the oracle alone leaves 0.35 of the rays clean; most other choices leave 0.05 .. 0.24."""
    R, S, near, far = 37, 16, 2.0, 6.0
    model, p = make_v3(N, "f32", seed=5, n_layers=2, dino_grad=True)
    v = views()["orbit"]
    o, d = grid_rays(R, first=180)
    fmap = random_map(14, 22, 64)
    g_rgb, g_depth = u01(441, R, 3) - 0.4, u01(442, R) - 0.3
    loss_of = lambda c, dep, dev="cpu": (c * g_rgb.to(dev)).sum() + (dep * g_depth.to(dev)).sum()
    oa, da, fa = o.cuda().requires_grad_(True), d.cuda().requires_grad_(True), fmap.cuda().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    out = N.render_rays(model, oa, da, near, far, S, perturb=False, dino=dict(features=fa, **v))
    loss_of(out["rgb"], out["depth"], "cuda").backward()
    pa = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
    ob, db, fb = o.cuda().requires_grad_(True), d.cuda().requires_grad_(True), fmap.cuda().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    from nerf_few_shot_limitations_amd import training as TR
    pts, z, dirs = N.sample_points_along_rays(ob, db, near, far, S, perturb=False, ray_grad=True, return_dirs=True)
    xy = N.project_points_to_image(pts.reshape(-1, 3), v["pose"], v["focal"], v["H"], v["W"], point_grad=True)[0]
    feats = N.sample_features_at_points(fb, xy, feature_grad=True, point_grad=True)
    rgb, den = model(pts.reshape(-1, 3), dirs.reshape(-1, 3), feats)
    rgb_b, depth_b, _ = TR.composite(torch.cat([rgb, den], -1).reshape(R, S, 4), z, db, False, geom_grad=True)
    assert torch.equal(rgb_b, out["rgb"]) and torch.equal(depth_b, out["depth"])
    loss_of(rgb_b, depth_b, "cuda").backward()
    assert torch.equal(oa.grad, ob.grad) and torch.equal(da.grad, db.grad)
    assert torch.equal(fa.grad, fb.grad) and fa.grad.abs().max() > 0
    for k, q in model.named_parameters():
        assert torch.equal(q.grad, pa[k]), k
    oo, do = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    zo = O.sample_points_along_rays(oo, do, near, far, S, None)[1]
    loss, clean = oracle_chain(p, oo, do, zo.detach(), fmap, v, loss_of)
    loss.backward()
    assert clean.float().mean() >= 0.25, float(clean.float().mean())
    ro, rd = rel_to_max(oa.grad.cpu()[clean], oo.grad[clean]), rel_to_max(da.grad.cpu()[clean], do.grad[clean])
    print(f"\nRECORD routes v3: clean rays {int(clean.sum())}/{R}, d_rays_o {ro:.3e} d_rays_d {rd:.3e}")
    assert ro <= 2e-4 and rd <= 2e-4


def test_switch_changes_nothing_else(N):
    """point_grad off and on (dino_grad on in both): outputs, parameter gradients, d_feats and d_map are torch.equal."""
    n = 1000
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n)
    v = views()["orbit"]
    res = []
    for switch in (False, True):
        model, _ = make_v3(N, "bf16", seed=1, point_grad=switch, dino_grad=True)       # (seed 1: the density ReLU is open for most samples)
        model.zero_grad(set_to_none=True)
        f = dino.cuda().requires_grad_(True)
        pc, dc = pos.cuda(), dirs.cuda()
        out = model(pc.requires_grad_(True), dc.requires_grad_(True), f) if switch else model(pc, dc, f)
        ((out[0] * g_rgb.cuda()).sum() + (out[1] * g_den.cuda()).sum()).backward()
        grads = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
        # a live map under render_rays with rays that are data
        model.zero_grad(set_to_none=True)
        o, d = grid_rays(24, first=180)                          # (the image's middle rows: the corner rays never reach the orbit view's map)
        fm = random_map(14, 22, 64).cuda().requires_grad_(True)
        r = N.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, 8, perturb=False, dino=dict(features=fm, **v))
        r["rgb"].sum().backward()
        res.append(([o_.detach().clone() for o_ in out] + [r["rgb"].detach().clone()], grads, f.grad.clone(), fm.grad.clone()))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1].keys() == res[1][1].keys()
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3]) and res[0][3].abs().max() > 0


def test_frozen_parameters_still_give_input_gradients_and_keep_no_grad(N):
    model, p = make_v3(N, "f32")
    for q in model.parameters():
        q.requires_grad_(False)
    pos, dirs, dino, g_rgb, g_den = v3_inputs(129)
    keep = (O.relu_margin(p, "v3", pos, dirs, dino) > MARGIN)[:, None]
    g_rgb, g_den = g_rgb * keep, g_den * keep
    pc, dc, fc = pos.cuda().requires_grad_(True), dirs.cuda().requires_grad_(True), dino.cuda().requires_grad_(True)
    rgb, den = model(pc, dc, fc)
    ((rgb * g_rgb.cuda()).sum() + (den * g_den.cuda()).sum()).backward()
    want_p, want_d, want_f = oracle_input_grads(p, pos, dirs, dino, g_rgb, g_den, feats_too=True)
    assert all(q.grad is None for q in model.parameters())
    assert rel_to_max(pc.grad, want_p) <= 2e-4 and rel_to_max(dc.grad, want_d) <= 2e-4 and rel_to_max(fc.grad, want_f) <= 2e-4
    # only the features live: the training kernels still run
    f2 = dino.cuda().requires_grad_(True)
    rgb, den = model(pos.cuda(), dirs.cuda(), f2)
    ((rgb * g_rgb.cuda()).sum() + (den * g_den.cuda()).sum()).backward()
    assert torch.equal(f2.grad, fc.grad)


def test_density_normals_of_a_v3_model(N):
    """(density, -grad sigma / |grad sigma|) with the source view against autograd through the oracle (projection, fetch, network)
    on samples off the ReLU thresholds and the texel edges; no parameter receives a gradient; without the view it is refused."""
    model, p = make_v3(N, "f32", seed=1)                         # (a field whose density ReLU is open for most samples)
    v = views()["near"]
    fmap = random_map(14, 22, 64)
    pos = u01(451, 257, 3) * 4 - 2
    den, nrm = N.density_normals(model, pos.cuda(), dino=dict(features=fmap.cuda(), **v))
    assert all(q.grad is None for q in model.parameters())
    po = pos.clone().requires_grad_(True)
    xy = O.project_points_to_image(po, v["pose"], v["focal"], v["H"], v["W"])[0]
    feats = O.sample_features_at_points(fmap, xy)
    sig = O.mlp_v3(p, po, torch.zeros_like(pos), feats)[1]
    (g,) = torch.autograd.grad(sig.sum(), po)
    keep = (O.relu_margin(p, "v3", pos, torch.zeros_like(pos), feats.detach()) > MARGIN) & (edge_distance(xy.detach(), 14, 22) > EDGE) & \
           (g.norm(dim=-1) > 1e-3 * g.norm(dim=-1).max())
    assert keep.float().mean() > 0.5
    want = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    assert rel_to_max(den, sig) < 1e-4
    assert float((nrm.cpu()[keep] - want[keep]).abs().max()) < 1e-3
    with pytest.raises(ValueError, match="dino="):
        N.density_normals(model, pos.cuda())


def pose_matrix(base, xi):
    """base pose moved by xi[:3] and rotated by the axis-angle xi[3:] (tests/test_gpu_input_grad.py)."""
    z = torch.zeros((), dtype=xi.dtype, device=xi.device)
    K = torch.stack([torch.stack([z, -xi[5], xi[4]]), torch.stack([xi[5], z, -xi[3]]), torch.stack([-xi[4], xi[3], z])])
    top = torch.cat([torch.linalg.matrix_exp(K) @ base[:3, :3], (base[:3, 3] + xi[:3])[:, None]], 1)
    return torch.cat([top, base[3:4]], 0)


def test_pose_recovery_on_v3(N):
    """The loop of tests/test_gpu_input_grad.py::test_pose_recovery on the DINO-conditioned network: a frozen V3 'smooth' field (3
    density layers, f32 mode), source view = the `orbit` view with a 14 x 22 x 64 map from uniform01(403) * 2 - 1, 16x16 rays x 32
    un-jittered samples, near 2, far 6; target = the render at O.LEGO_LIKE_C2W; start = that pose moved by (0.05, -0.03, 0.04) and
    rotated by the axis-angle (0.01, -0.015, 0.012); six pose parameters under Adam(lr=2e-3), 200 steps.  The same loop through the
    oracle on the CPU takes the loss from 2.03e-4 to 2.7e-13 and the translation error from 7.07e-2 to 3.8e-6; required here, as for
    V2: translation error <= 7e-3 and the loss at least 100x down."""
    H = W = 16
    focal = O.focal_for(W)
    model, _ = make_v3(N, "f32", scene="smooth", seed=1, n_layers=3)
    for q in model.parameters():
        q.requires_grad_(False)
    dino = dict(features=random_map(14, 22, 64, seed=403).cuda(), **views()["orbit"])
    base = torch.from_numpy(O.LEGO_LIKE_C2W.copy()).cuda()

    def render(c2w, grad):
        o, d = N.get_rays(H, W, focal, c2w, pose_grad=grad)
        return N.render_rays(model, o.reshape(-1, 3), d.reshape(-1, 3), 2.0, 6.0, 32, perturb=False, dino=dino)["rgb"]
    with torch.no_grad():
        target = render(base, False)
    start = torch.tensor([0.05, -0.03, 0.04, 0.01, -0.015, 0.012], device="cuda")
    xi = torch.zeros(6, device="cuda", requires_grad=True)
    with torch.no_grad():
        moved = pose_matrix(base, start)
    opt = torch.optim.Adam([xi], lr=2e-3)
    first = last = None
    for step in range(200):
        opt.zero_grad()
        loss = ((render(pose_matrix(moved, xi), True) - target) ** 2).mean()
        loss.backward()
        opt.step()
        last = float(loss)
        first = last if first is None else first
    with torch.no_grad():
        t_err = float((pose_matrix(moved, xi)[:3, 3] - base[:3, 3]).norm())
    print(f"\nRECORD V3 pose recovery: loss {first:.3e} -> {last:.3e}, translation error 7.07e-2 -> {t_err:.3e}")
    assert t_err <= 7e-3 and last * 100 <= first


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_without_the_switch_every_input_is_refused_as_before(N):
    from nerf_few_shot_limitations_amd import training as TR
    pos, dirs, dino, _, _ = v3_inputs(8)
    v = views()["orbit"]
    plain, _ = make_v3(N, "f32", n_layers=2, point_grad=False)
    with pytest.raises(NotImplementedError):
        plain(pos.cuda().requires_grad_(True), dirs.cuda(), dino.cuda())
    with pytest.raises(NotImplementedError):
        plain(pos.cuda(), dirs.cuda().requires_grad_(True), dino.cuda())
    with pytest.raises(NotImplementedError):
        plain(pos.cuda(), dirs.cuda(), dino.cuda().requires_grad_(True))
    o, d = grid_rays(4)
    dn = dict(features=random_map(9, 9, 64).cuda(), **v)
    with pytest.raises(NotImplementedError):
        TR.render_rays_train(plain, o.cuda().requires_grad_(True), d.cuda(), 2.0, 6.0, 4, perturb=False, dino=dn)
    with pytest.raises(ValueError):
        N.density_normals(plain, pos.cuda(), dino=dn)
    # the fetch wrappers: points that require grad are data unless asked for
    xy = (u01(461, 8, 2) - 0.5).cuda().requires_grad_(True)
    assert not N.sample_features_at_points(dn["features"], xy).requires_grad
    assert N.sample_features_at_points(dn["features"], xy, point_grad=True).requires_grad
    p3 = pos.cuda().requires_grad_(True)
    assert not N.project_points_to_image(p3, v["pose"], v["focal"], v["H"], v["W"])[0].requires_grad
    # a live map on a point_grad module without dino_grad is still refused
    switched, _ = make_v3(N, "f32", n_layers=2)
    live = dict(dn, features=random_map(9, 9, 64).cuda().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        TR.render_rays_train(switched, o.cuda().requires_grad_(True), d.cuda(), 2.0, 6.0, 4, perturb=False, dino=live)


def test_c_abi_refusals(N, L):
    """Every NRF_EINVAL case of nrf_mlp_backward_inputs_v3, each before any launch; n == 0 succeeds and launches nothing; the V1 / V2
    entry still refuses a V3 handle."""
    from nerf_few_shot_limitations_amd import training as TR
    lib = L.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    n = 33
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n)
    model, _ = make_v3(N, "bf16", n_layers=2)
    rc, outs, buf = raw_run(L, model, pos, dirs, dino, g_rgb, g_den)
    assert rc == 0
    h, mode = TR._train_handle(model, dev)
    nb, cb = buf.numel(), C.c_void_p(buf.data_ptr())
    pc, dc = pos.cuda().contiguous(), dirs.cuda().contiguous()
    op, od = (torch.full((n, 3), float("nan"), device=dev) for _ in range(2))
    call = lambda *a: lib.nrf_mlp_backward_inputs_v3(h, mode, *a, L.stream_ptr())
    assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), None, None) == -1 and b"no output" in lib.nrf_last_error()
    assert call(n, cb, nb, None, L.ptr(dc), L.ptr(op), None) == -1 and b"positions" in lib.nrf_last_error()
    assert call(n, cb, nb, L.ptr(pc), None, None, L.ptr(od)) == -1 and b"directions" in lib.nrf_last_error()
    assert call(n, cb, nb - 1, L.ptr(pc), L.ptr(dc), L.ptr(op), None) == -1 and b"context" in lib.nrf_last_error()
    assert call(n, None, nb, L.ptr(pc), L.ptr(dc), L.ptr(op), None) == -1
    assert call(-1, cb, nb, L.ptr(pc), L.ptr(dc), L.ptr(op), None) == -1
    assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), C.c_void_p(op.data_ptr() + 2), None) == -1 and b"aligned" in lib.nrf_last_error()
    assert lib.nrf_mlp_backward_inputs_v3(h, 3, n, cb, nb, L.ptr(pc), L.ptr(dc), L.ptr(op), None, L.stream_ptr()) == -1
    assert call(0, None, 0, None, None, None, None) == 0
    assert lib.nrf_mlp_backward_inputs(h, mode, n, cb, nb, L.ptr(pc), L.ptr(dc), None, L.ptr(op), None, L.stream_ptr()) == -1
    assert b"projection" in lib.nrf_last_error()
    # stale backward weights: the parameters moved and only the forward side of another mode was re-packed
    with torch.no_grad():
        model.flat_params().flat.mul_(1.0)
    L.check(lib.nrf_model_update_device(h, L.ptr(model.flat_params().flat), 1 << L.MMA_MODES["f32"], L.stream_ptr()))
    assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), L.ptr(op), None) == -1 and b"older than the parameters" in lib.nrf_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(op).all() and torch.isnan(od).all()           # nothing was launched
    # another family
    v2 = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=2, mma_mode="bf16").cuda().train()
    h2, mode2 = TR._train_handle(v2, dev)
    nb2 = lib.nrf_train_context_bytes(h2, mode2, n)
    buf2 = torch.zeros(nb2, dtype=torch.uint8, device=dev)
    assert lib.nrf_mlp_backward_inputs_v3(h2, mode2, n, C.c_void_p(buf2.data_ptr()), nb2, L.ptr(pc), L.ptr(dc), L.ptr(op), None, L.stream_ptr()) == -1
    assert b"V3" in lib.nrf_last_error()
