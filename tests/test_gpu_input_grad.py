"""GPU tests of the input gradient: nrf_mlp_backward_inputs (csrc/train_input_grad_impl.hpp), nrf_composite_backward_geom and
nrf_ray_grad (csrc/staged_kernels.hip), and the opt-in Python surface on top of them -- NeRFMLP(input_grad=True),
training.composite(geom_grad=True), sample_points_along_rays(ray_grad=True), get_rays(pose_grad=True), render_rays with rays that
require grad, density_normals."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_training_host import train_plan
from tests.train_ctx import SavedContext

pytestmark = pytest.mark.gpu

MARGIN = 2e-5          # as tests/test_gpu_training.py: samples with a ReLU on its threshold get no incoming gradient
PE, DE = 63, 27
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


def make(N, variant, mode, scene="fog", n_layers=8, seed=2, input_grad=True):
    if variant == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=n_layers, mma_mode=mode, input_grad=input_grad)
        p = O.make_weights("v1", seed, scene, n_layers=n_layers)
        m.load_state_dict(p)
    else:
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=n_layers, use_dino=False, mma_mode=mode, input_grad=input_grad)
        p = O.make_weights("v2", seed, scene, n_layers=n_layers)
        m.load_state_dict(p, strict=False)
    return m.cuda().train(), p


def u01(seed, *shape):
    return torch.from_numpy(O.uniform01(seed, int(np.prod(shape))).reshape(shape)).float()


def inputs(n, seed=25):
    """pos in [-2,2]^3, unit dirs, upstream gradients in [-0.5,0.5) (tests/test_gpu_dino_grad.py:v3_inputs)."""
    pos = u01(seed, n, 3) * 4 - 2
    dirs = u01(seed + 1, n, 3) - 0.5
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    return pos, dirs, u01(seed + 2, n, 3) - 0.5, u01(seed + 3, n, 1) - 0.5


def rel_to_max(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cosine(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-300))


def keep_mask(p, variant, pos, dirs):
    x = O.positional_encoding(pos, 10) if variant == "v1" else pos
    return (O.relu_margin(p, variant, x, dirs) > MARGIN)[:, None]


def surface_grads(N, model, variant, pos, dirs, g_rgb, g_den):
    """Through NeRFMLP.forward for L = <rgb, g_rgb> + <sigma, g_den>: (outputs, {input: gradient}, {parameter: gradient})."""
    model.zero_grad(set_to_none=True)
    p = pos.cuda().requires_grad_(True)
    ins = {}
    if variant == "v1":
        x = N.PositionalEncoding(10)(pos.cuda()).requires_grad_(True)
        out = model(x, points=p)
        (out * torch.cat([g_rgb, g_den], -1).cuda()).sum().backward()
        ins["x_enc"], outs = x.grad.detach().clone(), (out.detach(),)
    else:
        d = dirs.cuda().requires_grad_(True)
        rgb, den = model(p, d)
        ((rgb * g_rgb.cuda()).sum() + (den * g_den.cuda()).sum()).backward()
        ins["directions"], outs = d.grad.detach().clone(), (rgb.detach(), den.detach())
    ins["positions"] = p.grad.detach().clone()
    return outs, ins, {k: q.grad.detach().clone() for k, q in model.named_parameters() if q.grad is not None}


def oracle_grads(p, variant, pos, dirs, g_rgb, g_den):
    pp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    po = pos.clone().requires_grad_(True)
    ins = {}
    if variant == "v1":
        x = O.positional_encoding(po, 10)
        x.retain_grad()
        (O.mlp_v1(pp, x) * torch.cat([g_rgb, g_den], -1)).sum().backward()
        ins["x_enc"] = x.grad
    else:
        do = dirs.clone().requires_grad_(True)
        rgb, den = O.mlp_v2(pp, po, do)
        ((rgb * g_rgb).sum() + (den * g_den).sum()).backward()
        ins["directions"] = do.grad
    ins["positions"] = po.grad
    return ins, {k: v.grad for k, v in pp.items() if v.grad is not None}


def raw_run(N, L, model, variant, pos, dirs, g_rgb, g_den, want, pad=0):
    """One forward_train / backward / backward_inputs through the C ABI.  `want`: subset of 'x', 'p', 'd'; the outputs have `pad`
    more rows than samples and start as NaN.  Returns (return code, {name: tensor}, context buffer, flat gradient)."""
    from nerf_few_shot_limitations_amd import training as TR
    dev = torch.device("cuda", torch.cuda.current_device())
    h, mode = TR._train_handle(model, dev)
    lib, n = L.lib(), pos.shape[0]
    nbytes = lib.nrf_train_context_bytes(h, mode, n)
    assert nbytes >= 0
    buf = torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    grad = torch.zeros_like(model.flat_params().flat)
    cb, st = C.c_void_p(buf.data_ptr()), L.stream_ptr()
    pc, dc = pos.cuda().contiguous(), dirs.cuda().contiguous()
    if variant == "v1":
        x = N.PositionalEncoding(10)(pc)
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        g = torch.cat([g_rgb, g_den], -1).cuda().contiguous()
        L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(x), n, L.ptr(out), cb, nbytes, st))
        L.check(lib.nrf_mlp_backward_v1(h, mode, L.ptr(out), L.ptr(g), n, cb, nbytes, L.ptr(grad), st))
    else:
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        den = torch.empty((n, 1), dtype=torch.float32, device=dev)
        gr, gd = g_rgb.cuda().contiguous(), g_den.cuda().contiguous()
        L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(pc), L.ptr(dc), None, n, L.ptr(rgb), L.ptr(den), cb, nbytes, st))
        L.check(lib.nrf_mlp_backward(h, mode, L.ptr(rgb), L.ptr(den), L.ptr(gr), L.ptr(gd), n, cb, nbytes, L.ptr(grad), st))
    outs = {k: torch.full((n + pad, w), float("nan"), dtype=torch.float32, device=dev) for k, w in (("x", PE), ("p", 3), ("d", 3)) if k in want}
    rc = lib.nrf_mlp_backward_inputs(h, mode, n, cb, nbytes, L.ptr(pc), L.ptr(dc) if variant == "v2" else None, L.ptr(outs.get("x")),
                                     L.ptr(outs.get("p")), L.ptr(outs.get("d")), st)
    torch.cuda.synchronize()
    return rc, outs, buf, grad


# ---------------------------------------------------------------------------------------------
# input_grad_kernel
# ---------------------------------------------------------------------------------------------
CASES = [(1, 3, "fog"), (31, 2, "solid"), (33, 8, "fog"), (129, 3, "solid"), (4096 + 17, 8, "solid"), (4096 + 17, 2, "fog")]


@pytest.mark.parametrize("n,n_layers,scene", CASES)
@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_input_gradient_fp32_mode_matches_autograd(N, variant, n, n_layers, scene):
    """fp32 mode against torch autograd through the oracle network (O.mlp_v1 on O.positional_encoding; O.mlp_v2), to the bar the
    parameter gradients of the same chain are held to: 2e-4 of the largest element.  (The oracle's own fp32-vs-float64 difference on
    these inputs is <= 1.9e-6 of the maximum, 100x inside the bar.)  The parameter gradients of the same backward are checked too.
    The mask must keep >= 95 % of the samples (a share: asserted where there are enough samples for one, n >= 129)."""
    model, p = make(N, variant, "f32", scene=scene, n_layers=n_layers)
    pos, dirs, g_rgb, g_den = inputs(n)
    keep = keep_mask(p, variant, pos, dirs)
    if n >= 129:
        assert keep.float().mean() >= 0.95, float(keep.float().mean())
    g_rgb, g_den = g_rgb * keep, g_den * keep
    _, got, grads = surface_grads(N, model, variant, pos, dirs, g_rgb, g_den)
    want, pgrads = oracle_grads(p, variant, pos, dirs, g_rgb, g_den)
    for name in want:
        r = rel_to_max(got[name], want[name]) if want[name].abs().max() > 0 else float(got[name].abs().max())
        print(f"\nRECORD f32 {variant} n {n} depth {n_layers} {scene}: d_{name} rel_to_max {r:.3e}")
        assert r <= 2e-4, (name, r)
    for name, g in grads.items():
        if pgrads[name].abs().max() > 0:
            assert rel_to_max(g, pgrads[name]) <= 2e-4, name


def quantize_w(w, mode):
    return O.quantize(w, mode).double().numpy()


@pytest.mark.parametrize("n", [33, 3000])
@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_16_bit_product_is_exact_up_to_the_accumulation(N, L, variant, mode, n):
    """The 16-bit kernels against quantize(W0)^T dZ0 in float64, dZ0 decoded from the context (tests/train_ctx.py).  Every 16-bit x
    16-bit product is exact in the fp32 accumulator, so only the 256-term sum rounds: |err| <= 256 * 2^-24 * sum_k |w_k dz_k| per
    output (derived, not measured).  V1: d_x_enc is the product itself.  V2 has no encoded output, so its products (position tiles and
    the direction tile, K = 128) are checked through the adjoint: d = sum_u coef_u prod_u with coef_u = +-2^f cos|sin(2^f x) or 1, whose
    bound is sum_u |coef_u| B_u (the products' bounds) + 40 * 2^-24 * sum_u |coef_u prod_u| (at most 33 fp32 additions, two
    multiplications and a sincosf of <= 2 ulp per term; the argument x * 2^f is exact)."""
    depth = 3
    model, p = make(N, variant, mode, scene="solid", n_layers=depth)
    pos, dirs, g_rgb, g_den = inputs(n)
    rc, outs, buf, _ = raw_run(N, L, model, variant, pos, dirs, g_rgb, g_den, want=("x", "p") if variant == "v1" else ("p", "d"))
    assert rc == 0, L.lib().nrf_last_error()
    ctx = SavedContext(train_plan(L, variant, p, depth, with_planes=True), variant, depth, mode, n, buf)

    def product(wname, cols, dz):
        w = quantize_w(p[wname][:, cols], mode)                     # (K, F)
        dz = dz.astype(np.float64)                                   # (K, n)
        return w.T @ dz, np.abs(w).T @ np.abs(dz)                    # (F, n) products, and sum |w dz|

    def adjoint(prod, mag, x, Lf, k_terms):
        """float64 adjoint of the encoding on the reference-ordered products, and its bound."""
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

    first = "layers.0.weight" if variant == "v1" else "density_mlp.density_layers.0.weight"
    prod, mag = product(first, slice(0, PE), ctx.slot("dz_trunk.0")[:, :n])
    assert np.abs(prod).max() > 0
    if variant == "v1":
        got = outs["x"].cpu().double().numpy().T
        err = np.abs(got - prod)
        print(f"\nRECORD {mode} v1 n {n}: d_x_enc worst |err| / bound {float((err / (256 * U24 * mag + 1e-300)).max()):.3f}")
        assert (err <= 256 * U24 * mag).all()
    want, bound = adjoint(prod, mag, pos, 10, 256)
    got = outs["p"].cpu().double().numpy()
    print(f"\nRECORD {mode} {variant} n {n}: d_positions worst |err| / bound {float((np.abs(got - want) / (bound + 1e-300)).max()):.3f}")
    assert (np.abs(got - want) <= bound).all()
    if variant == "v2":
        prod, mag = product("color_mlp.color_layers.0.weight", slice(256, 256 + DE), ctx.slot("dz_c0")[:, :n])
        want, bound = adjoint(prod, mag, dirs, 4, 128)
        got = outs["d"].cpu().double().numpy()
        print(f"\nRECORD {mode} v2 n {n}: d_directions worst |err| / bound {float((np.abs(got - want) / (bound + 1e-300)).max()):.3f}")
        assert np.abs(want).max() > 0 and (np.abs(got - want) <= bound).all()


@pytest.mark.parametrize("mode,cos_min", [("bf16", 0.97), ("f16", 0.995)])
@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_16_bit_input_gradient_end_to_end(N, variant, mode, cos_min):
    """d_positions / d_directions of the 16-bit modes against the fp32-mode result of the same inputs: the project's bars for 16-bit
    gradients (cosine > 0.97 bf16, > 0.995 f16)."""
    n, depth = 3000, 8
    pos, dirs, g_rgb, g_den = inputs(n)
    m32, p = make(N, variant, "f32", scene="fog", n_layers=depth)
    keep = keep_mask(p, variant, pos, dirs)
    g_rgb, g_den = g_rgb * keep, g_den * keep
    _, ref, _ = surface_grads(N, m32, variant, pos, dirs, g_rgb, g_den)
    m16, _ = make(N, variant, mode, scene="fog", n_layers=depth)
    _, got, _ = surface_grads(N, m16, variant, pos, dirs, g_rgb, g_den)
    for name in ("positions",) + (("directions",) if variant == "v2" else ()):
        c = cosine(got[name], ref[name])
        print(f"\nRECORD {mode} {variant} n {n} depth {depth}: cosine(d_{name}, fp32 mode) {c:.5f}")
        assert c > cos_min, (name, c)


@pytest.mark.parametrize("variant,mode", [("v1", "bf16"), ("v2", "bf16"), ("v2", "f32")])
def test_bit_properties(N, L, variant, mode):
    """Two runs give the same bits; a sample's gradient does not depend on the batch around it (the first 3000 rows of an n = 40000
    run, the 8-wave chain geometry in the 16-bit modes, equal an n = 3000 run); rows >= n of a NaN-filled output stay NaN."""
    model, p = make(N, variant, mode, scene="solid", n_layers=3)
    pos, dirs, g_rgb, g_den = inputs(40000)
    want = ("x", "p") if variant == "v1" else ("p", "d")
    rc, big, _, _ = raw_run(N, L, model, variant, pos, dirs, g_rgb, g_den, want)
    assert rc == 0
    k = 3000
    args = (pos[:k], dirs[:k], g_rgb[:k], g_den[:k])
    rc, a, _, _ = raw_run(N, L, model, variant, *args, want, pad=37)
    rc2, b, _, _ = raw_run(N, L, model, variant, *args, want, pad=37)
    assert rc == 0 and rc2 == 0
    for name in want:
        assert torch.isfinite(a[name][:k]).all() and a[name][:k].abs().max() > 0, name
        assert torch.equal(a[name][:k], b[name][:k]), name
        assert torch.equal(a[name][:k], big[name][:k]), name
        assert torch.isnan(a[name][k:]).all(), name
    # one output at a time gives the same bits as all of them together
    for name in want:
        rc, one, _, _ = raw_run(N, L, model, variant, *args, (name,))
        assert rc == 0 and torch.equal(one[name], a[name][:k]), name


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_switch_changes_neither_outputs_nor_parameter_gradients(N, variant):
    n = 1000
    pos, dirs, g_rgb, g_den = inputs(n)
    res = []
    for switch in (False, True):
        model, _ = make(N, variant, "bf16", scene="solid", n_layers=3, input_grad=switch)
        model.zero_grad(set_to_none=True)
        if variant == "v1":
            x = N.PositionalEncoding(10)(pos.cuda())
            out = (model(x.requires_grad_(True)) if switch else model(x),)
            (out[0] * torch.cat([g_rgb, g_den], -1).cuda()).sum().backward()
        else:
            pc, dc = pos.cuda(), dirs.cuda()
            out = model(pc.requires_grad_(True), dc.requires_grad_(True)) if switch else model(pc, dc)
            ((out[0] * g_rgb.cuda()).sum() + (out[1] * g_den.cuda()).sum()).backward()
        res.append(([o.detach().clone() for o in out], {k: q.grad.detach().clone() for k, q in model.named_parameters()}))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert res[0][1].keys() == res[1][1].keys()
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


def test_frozen_parameters_still_give_input_gradients_and_keep_no_grad(N):
    model, p = make(N, "v2", "f32", scene="solid", n_layers=3)
    for q in model.parameters():
        q.requires_grad_(False)
    pos, dirs, g_rgb, g_den = inputs(129)
    keep = keep_mask(p, "v2", pos, dirs)
    _, got, grads = surface_grads(N, model, "v2", pos, dirs, g_rgb * keep, g_den * keep)
    want, _ = oracle_grads(p, "v2", pos, dirs, g_rgb * keep, g_den * keep)
    assert not grads and all(q.grad is None for q in model.parameters())
    assert rel_to_max(got["positions"], want["positions"]) <= 2e-4


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_density_normals(N, variant):
    """(density, -grad sigma / |grad sigma|) against autograd through the oracle: the directions agree (a unit vector within 2e-4 of
    the bar of the gradient itself, relative to 1) on samples off the ReLU thresholds, and no parameter receives a gradient."""
    model, p = make(N, variant, "f32", scene="solid", n_layers=3)
    pos, dirs, _, _ = inputs(257)
    den, nrm = N.density_normals(model, pos.cuda())
    assert all(q.grad is None for q in model.parameters())
    po = pos.clone().requires_grad_(True)
    if variant == "v1":
        sig = O.mlp_v1(p, O.positional_encoding(po, 10))[:, 3:4]
    else:
        sig = O.mlp_v2(p, po, torch.zeros_like(pos))[1]
    (g,) = torch.autograd.grad(sig.sum(), po)
    keep = keep_mask(p, variant, pos, torch.zeros_like(pos))[:, 0] & (g.norm(dim=-1) > 1e-3 * g.norm(dim=-1).max())
    assert keep.float().mean() > 0.5
    want = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-30)
    assert rel_to_max(den, sig) < 1e-4
    assert float((nrm.cpu()[keep] - want[keep]).abs().max()) < 1e-3
    assert float((nrm.cpu().norm(dim=-1)[keep] - 1).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------
# compositor geometry
# ---------------------------------------------------------------------------------------------
def composite_case(R, S, seed=61):
    sig = (0.05 + 3.0 * u01(seed, R, S, 1)) * torch.where(u01(seed + 1, R, S, 1) < 0.25, -1.0, 1.0)      # |sigma| >= 0.05: none on the ReLU
    rgb = u01(seed + 2, R, S, 3)
    z = 2.0 + 4.0 * (torch.arange(S).float()[None, :] + 0.9 * u01(seed + 3, R, S)) / S               # ascending, jittered, in [2,6]
    d = (u01(seed + 4, R, 3) - 0.5) * 2.0 + torch.tensor([0.0, 0.0, -1.5])
    g = dict(rgb=u01(seed + 5, R, 3) - 0.4, depth=u01(seed + 6, R) - 0.3, w=u01(seed + 7, R, S) - 0.45)
    return torch.cat([rgb, sig], -1).contiguous(), z.contiguous(), d.contiguous(), g


def composite_loss(out, g, dev=None):
    mv = (lambda t: t.to(dev)) if dev else (lambda t: t)
    return (out[0] * mv(g["rgb"])).sum() + (out[1] * mv(g["depth"])).sum() + (out[2] * mv(g["w"])).sum()


@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("R,S", [(5, 2), (37, 16), (9, 65), (7, 130), (3, 200)])
def test_composite_geometry_matches_autograd(N, R, S, white):
    """d_z and d_rays_d against autograd through O.volume_render, all three upstream gradients non-zero: 1e-4 of the largest
    element, the bar of test_composite_backward_matches_autograd (the reference's own fp32-vs-float64 difference on these inputs is
    <= 8.4e-7 of the maximum).  Finite everywhere, the 1e10 last interval included; d_rgb / d_sigma are nrf_composite_backward's bits."""
    from nerf_few_shot_limitations_amd import training as TR
    rs, z, d, g = composite_case(R, S)
    a = rs.cuda().requires_grad_(True)
    zc, dc = z.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    composite_loss(TR.composite(a, zc, dc, white, geom_grad=True), g, "cuda").backward()
    b = rs.cuda().requires_grad_(True)
    composite_loss(TR.composite(b, z.cuda(), d.cuda(), white), g, "cuda").backward()
    assert torch.equal(a.grad, b.grad)
    ro, zo, do = rs.clone().requires_grad_(True), z.clone().requires_grad_(True), d.clone().requires_grad_(True)
    composite_loss(O.volume_render(ro[..., :3], ro[..., 3:4], zo, do, white), g).backward()
    assert torch.isfinite(zc.grad).all() and torch.isfinite(dc.grad).all()
    rz, rd = rel_to_max(zc.grad, zo.grad), rel_to_max(dc.grad, do.grad)
    print(f"\nRECORD composite geometry R {R} S {S} white {white}: d_z {rz:.3e} d_rays_d {rd:.3e}")
    assert zo.grad.abs().max() > 0 and do.grad.abs().max() > 0
    assert rz <= 1e-4 and rd <= 1e-4


def test_composite_geometry_single_sample_is_finite(N):
    from nerf_few_shot_limitations_amd import training as TR
    rs, z, d, g = composite_case(6, 1)
    zc, dc = z.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    composite_loss(TR.composite(rs.cuda().requires_grad_(True), zc, dc, False, geom_grad=True), g, "cuda").backward()
    assert torch.isfinite(zc.grad).all() and torch.isfinite(dc.grad).all()


# ---------------------------------------------------------------------------------------------
# nrf_ray_grad
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 65, 130])
@pytest.mark.parametrize("R", [1, 37])
def test_ray_grad_matches_its_definition(N, L, R, S):
    """Against the float64 sums of the definition, |err| <= S * 2^-24 * sum |terms| per output; two runs are bit-equal."""
    dp, dd = u01(71, R * S, 3) - 0.5, u01(72, R * S, 3) - 0.5
    z, d = 2 + 4 * u01(73, R, S), u01(74, R, 3) - 0.5
    dz_in, dd_in = u01(75, R, S) - 0.5, u01(76, R, 3) - 0.5
    lib = L.lib()

    def run():
        t = [x.cuda().contiguous() for x in (dp, dd, z, d, dz_in, dd_in)]
        o = [torch.full((R, 3), float("nan"), device="cuda"), torch.full((R, 3), float("nan"), device="cuda"), torch.full((R, S), float("nan"), device="cuda")]
        L.check(lib.nrf_ray_grad(*[L.ptr(x) for x in t], R, S, *[L.ptr(x) for x in o], L.stream_ptr()))
        torch.cuda.synchronize()
        return [x.cpu() for x in o]
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    P, Dd, Z, D = dp.double().reshape(R, S, 3), dd.double().reshape(R, S, 3), z.double(), d.double()
    want_o, mag_o = P.sum(1), P.abs().sum(1)
    want_d = (Z[..., None] * P + Dd).sum(1) + dd_in.double()
    mag_d = ((Z[..., None] * P).abs() + Dd.abs()).sum(1) + dd_in.double().abs()
    want_z = (D[:, None, :] * P).sum(-1) + dz_in.double()
    mag_z = (D[:, None, :] * P).abs().sum(-1) + dz_in.double().abs()
    for got, want, mag in ((a[0], want_o, mag_o), (a[1], want_d, mag_d), (a[2], want_z, mag_z)):
        assert ((got.double() - want).abs() <= S * U24 * mag + 1e-300).all()


# ---------------------------------------------------------------------------------------------
# the Python routes
# ---------------------------------------------------------------------------------------------
def ray_case(R, seed=81):
    o = torch.tensor([0.1, -0.2, 4.0]) + 0.2 * (u01(seed, R, 3) - 0.5)
    d = torch.tensor([0.0, 0.0, -1.0]) + 0.5 * (u01(seed + 1, R, 3) - 0.5)
    return o.contiguous(), d.contiguous(), u01(seed + 2, R, 3) - 0.4, u01(seed + 3, R) - 0.3


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_routes_agree_and_match_autograd(N, variant):
    """Route A: render_rays on an input_grad module with rays that require grad.  Route B: the same loss through the public pieces
    sample_points_along_rays(ray_grad=True) -> NeRFMLP.forward -> composite(geom_grad=True).  The ray gradients are bit-equal; and
    (fp32 mode, R = 37, S = 16, 'fog') within 2e-4 of the largest element of autograd through the oracle over rays none of whose
    samples is masked, at least 40 % of the rays."""
    from nerf_few_shot_limitations_amd import training as TR
    R, S, near, far = 37, 16, 2.0, 6.0
    model, p = make(N, variant, "f32", scene="fog", n_layers=3)
    o, d, g_rgb, g_depth = ray_case(R)

    def loss(rgb, depth, dev=None):
        return (rgb * (g_rgb.to(dev) if dev else g_rgb)).sum() + (depth * (g_depth.to(dev) if dev else g_depth)).sum()
    oa, da = o.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    out = N.render_rays(model, oa, da, near, far, S, perturb=False)
    loss(out["rgb"], out["depth"], "cuda").backward()
    pa = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
    ob, db = o.cuda().requires_grad_(True), d.cuda().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    pts, z, dirs = N.sample_points_along_rays(ob, db, near, far, S, perturb=False, ray_grad=True, return_dirs=True)
    if variant == "v1":
        o4 = model(N.PositionalEncoding(10)(pts.detach().reshape(-1, 3)), points=pts.reshape(-1, 3))
    else:
        rgb, den = model(pts.reshape(-1, 3), dirs.reshape(-1, 3))
        o4 = torch.cat([rgb, den], -1)
    rgb_b, depth_b, _ = TR.composite(o4.reshape(R, S, 4), z, db, False, geom_grad=True)
    assert torch.equal(rgb_b, out["rgb"]) and torch.equal(depth_b, out["depth"])
    loss(rgb_b, depth_b, "cuda").backward()
    assert torch.equal(oa.grad, ob.grad) and torch.equal(da.grad, db.grad)
    for k, q in model.named_parameters():
        assert torch.equal(q.grad, pa[k]), k
    # the oracle, piece by piece under autograd (O.render_rays itself runs under no_grad)
    oo, do = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    po, zo = O.sample_points_along_rays(oo, do, near, far, S, None)
    pf, df = po.reshape(-1, 3), do[:, None, :].expand(R, S, 3).reshape(-1, 3)
    if variant == "v1":
        x = O.positional_encoding(pf, 10)
        o4o = O.mlp_v1(p, x)
        margin = O.relu_margin(p, "v1", x.detach())
    else:
        rgbo, deno = O.mlp_v2(p, pf, df)
        o4o = torch.cat([rgbo, deno], -1)
        margin = O.relu_margin(p, "v2", pf.detach(), df.detach())
    c, dep, _ = O.volume_render(o4o[:, :3].reshape(R, S, 3), o4o[:, 3:4].reshape(R, S, 1), zo, do, False)
    clean = (margin.reshape(R, S) > MARGIN).all(-1)
    assert clean.float().mean() >= 0.4, float(clean.float().mean())
    # rays are independent: mask the upstream gradient of the others on both sides by comparing clean rays only
    loss(c, dep).backward()
    ro, rd = rel_to_max(oa.grad.cpu()[clean], oo.grad[clean]), rel_to_max(da.grad.cpu()[clean], do.grad[clean])
    print(f"\nRECORD routes {variant}: clean rays {int(clean.sum())}/{R}, d_rays_o {ro:.3e} d_rays_d {rd:.3e}")
    assert ro <= 2e-4 and rd <= 2e-4


def test_render_rays_gives_depth_gradients_for_explicit_depths(N):
    """z_in that requires grad receives dL/d z (the compositor's term + d . d_p), against autograd through the oracle."""
    R, S = 9, 16
    model, p = make(N, "v2", "f32", scene="fog", n_layers=2)
    o, d, g_rgb, g_depth = ray_case(R)
    z = (2.0 + 4.0 * (torch.arange(S).float()[None, :] + 0.9 * u01(91, R, S)) / S).contiguous()
    zc = z.cuda().requires_grad_(True)
    out = N.render_rays(model, o.cuda(), d.cuda(), 2.0, 6.0, S, perturb=False, z_in=zc)
    ((out["rgb"] * g_rgb.cuda()).sum() + (out["depth"] * g_depth.cuda()).sum()).backward()
    zo = z.clone().requires_grad_(True)
    pf = (o[:, None, :] + d[:, None, :] * zo[:, :, None]).reshape(-1, 3)
    df = d[:, None, :].expand(R, S, 3).reshape(-1, 3)
    rgbo, deno = O.mlp_v2(p, pf, df)
    c, dep, _ = O.volume_render(rgbo.reshape(R, S, 3), deno.reshape(R, S, 1), zo, d, False)
    ((c * g_rgb).sum() + (dep * g_depth).sum()).backward()
    clean = (O.relu_margin(p, "v2", pf.detach(), df) .reshape(R, S) > MARGIN).all(-1)
    assert clean.any()
    assert rel_to_max(zc.grad.cpu()[clean], zo.grad[clean]) <= 2e-4


@pytest.mark.parametrize("H,W", [(12, 16), (1, 1)])
def test_get_rays_pose_gradient(N, H, W):
    """The rays are get_rays' bits; d_c2w against autograd through O.get_rays to 1e-5 of the largest element."""
    focal = 20.0
    c2w = torch.from_numpy(O.LEGO_LIKE_C2W.copy())
    o0, d0 = N.get_rays(H, W, focal, c2w.cuda())
    pc = c2w.cuda().requires_grad_(True)
    o1, d1 = N.get_rays(H, W, focal, pc, pose_grad=True)
    assert torch.equal(o0, o1) and torch.equal(d0, d1)
    go, gd = u01(95, H, W, 3) - 0.5, u01(96, H, W, 3) - 0.5
    ((o1 * go.cuda()).sum() + (d1 * gd.cuda()).sum()).backward()
    po = c2w.clone().requires_grad_(True)
    oo, do = O.get_rays(H, W, focal, po)
    ((oo * go).sum() + (do * gd).sum()).backward()
    assert rel_to_max(pc.grad, po.grad) <= 1e-5
    with pytest.raises(NotImplementedError):
        N.sample_points_along_rays(o1.reshape(-1, 3), d1.reshape(-1, 3), 2.0, 6.0, 4, perturb=False)      # rays with a grad_fn, no switch


def pose_matrix(base, xi):
    """base pose moved by xi[:3] and rotated by the axis-angle xi[3:] (the matrix exponential of its cross-product matrix)."""
    z = torch.zeros((), dtype=xi.dtype, device=xi.device)
    K = torch.stack([torch.stack([z, -xi[5], xi[4]]), torch.stack([xi[5], z, -xi[3]]), torch.stack([-xi[4], xi[3], z])])
    top = torch.cat([torch.linalg.matrix_exp(K) @ base[:3, :3], (base[:3, 3] + xi[:3])[:, None]], 1)
    return torch.cat([top, base[3:4]], 0)


def test_pose_recovery(N):
    """The pieces compose: a frozen V2 'smooth' field (3 density layers, f32 mode), 16x16 rays x 32 un-jittered samples, near 2, far 6;
    target = the render at O.LEGO_LIKE_C2W; start = that pose moved by (0.05, -0.03, 0.04) and rotated by the axis-angle (0.01, -0.015,
    0.012); six pose parameters under Adam(lr=2e-3), 200 steps.  The same loop through the oracle on the CPU takes the translation
    error from 7.07e-2 to 8.1e-6 and the loss from 4.7e-4 to 1.9e-12; required here: translation error <= 7e-3 (a tenth of the
    start) and the loss at least 100x down."""
    H = W = 16
    focal = O.focal_for(W)
    model, _ = make(N, "v2", "f32", scene="smooth", n_layers=3)
    for q in model.parameters():
        q.requires_grad_(False)
    base = torch.from_numpy(O.LEGO_LIKE_C2W.copy()).cuda()

    def render(c2w, grad):
        o, d = N.get_rays(H, W, focal, c2w, pose_grad=grad)
        return N.render_rays(model, o.reshape(-1, 3), d.reshape(-1, 3), 2.0, 6.0, 32, perturb=False)["rgb"]
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
    print(f"\nRECORD pose recovery: loss {first:.3e} -> {last:.3e}, translation error 7.07e-2 -> {t_err:.3e}")
    assert t_err <= 7e-3 and last * 100 <= first


# ---------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------
def test_without_the_switch_every_input_is_refused_as_before(N):
    from nerf_few_shot_limitations_amd import training as TR
    pos, dirs, _, _ = inputs(8)
    v1, _ = make(N, "v1", "f32", n_layers=2, input_grad=False)
    v2, _ = make(N, "v2", "f32", n_layers=2, input_grad=False)
    x = N.PositionalEncoding(10)(pos.cuda())
    with pytest.raises(NotImplementedError):
        v1(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        v1(x, points=pos.cuda().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        v2(pos.cuda().requires_grad_(True), dirs.cuda())
    with pytest.raises(NotImplementedError):
        v2(pos.cuda(), dirs.cuda().requires_grad_(True))
    o, d, _, _ = ray_case(4)
    for model in (v1, v2):
        with pytest.raises(NotImplementedError):
            TR.render_rays_train(model, o.cuda().requires_grad_(True), d.cuda(), 2.0, 6.0, 4, perturb=False)
        with pytest.raises(NotImplementedError):
            TR.render_rays_train(model, o.cuda(), d.cuda().requires_grad_(True), 2.0, 6.0, 4, perturb=False)
    with pytest.raises(NotImplementedError):
        N.sample_points_along_rays(o.cuda().requires_grad_(True), d.cuda(), 2.0, 6.0, 4, perturb=False)
    with pytest.raises(ValueError, match="projection and the bilinear fetch"):
        N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64, input_grad=True)
    with pytest.raises(ValueError):
        N.density_normals(v2, pos.cuda())


def test_c_abi_refusals(N, L):
    """Every NRF_EINVAL case of nrf_mlp_backward_inputs, each before any launch; n == 0 succeeds and launches nothing."""
    from nerf_few_shot_limitations_amd import training as TR
    lib = L.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    pos, dirs, g_rgb, g_den = inputs(33)
    for variant in ("v1", "v2"):
        model, _ = make(N, variant, "bf16", n_layers=2)
        rc, outs, buf, _ = raw_run(N, L, model, variant, pos, dirs, g_rgb, g_den, want=("p",))
        assert rc == 0
        h, mode = TR._train_handle(model, dev)
        n, nb, cb = 33, buf.numel(), C.c_void_p(buf.data_ptr())
        pc, dc = pos.cuda().contiguous(), dirs.cuda().contiguous()
        ox, op, od = (torch.full((n, w), float("nan"), device=dev) for w in (PE, 3, 3))
        call = lambda *a: lib.nrf_mlp_backward_inputs(h, mode, *a, L.stream_ptr())
        assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), None, None, None) == -1 and b"no output" in lib.nrf_last_error()
        assert call(n, cb, nb, None, L.ptr(dc), None, L.ptr(op), None) == -1 and b"positions" in lib.nrf_last_error()
        assert call(n, cb, nb - 1, L.ptr(pc), L.ptr(dc), None, L.ptr(op), None) == -1 and b"context" in lib.nrf_last_error()
        assert call(n, None, nb, L.ptr(pc), L.ptr(dc), None, L.ptr(op), None) == -1
        assert call(-1, cb, nb, L.ptr(pc), L.ptr(dc), None, L.ptr(op), None) == -1
        assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), None, C.c_void_p(op.data_ptr() + 2), None) == -1 and b"aligned" in lib.nrf_last_error()
        assert lib.nrf_mlp_backward_inputs(h, 3, n, cb, nb, L.ptr(pc), L.ptr(dc), None, L.ptr(op), None, L.stream_ptr()) == -1
        if variant == "v1":
            assert call(n, cb, nb, L.ptr(pc), None, None, None, L.ptr(od)) == -1 and b"direction" in lib.nrf_last_error()
        else:
            assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), L.ptr(ox), None, None) == -1 and b"V1" in lib.nrf_last_error()
            assert call(n, cb, nb, L.ptr(pc), None, None, None, L.ptr(od)) == -1 and b"directions" in lib.nrf_last_error()
        assert call(0, None, 0, None, None, None, None, None) == 0
        # stale backward weights: the parameters moved and only the forward side of another mode was re-packed
        with torch.no_grad():
            model.flat_params().flat.mul_(1.0)
        L.check(lib.nrf_model_update_device(h, L.ptr(model.flat_params().flat), 1 << L.MMA_MODES["f32"], L.stream_ptr()))
        assert call(n, cb, nb, L.ptr(pc), L.ptr(dc), None, L.ptr(op), None) == -1 and b"older than the parameters" in lib.nrf_last_error()
        torch.cuda.synchronize()
        assert torch.isnan(op).all() and torch.isnan(ox).all() and torch.isnan(od).all()      # nothing was launched
    v3 = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=64, mma_mode="bf16").cuda().train()
    h3, mode3 = TR._train_handle(v3, dev)
    nb3 = lib.nrf_train_context_bytes(h3, mode3, 33)
    buf3 = torch.zeros(nb3, dtype=torch.uint8, device=dev)
    op = torch.full((33, 3), float("nan"), device=dev)
    assert lib.nrf_mlp_backward_inputs(h3, mode3, 33, C.c_void_p(buf3.data_ptr()), nb3, L.ptr(pos.cuda().contiguous()), L.ptr(dirs.cuda().contiguous()),
                                       None, L.ptr(op), None, L.stream_ptr()) == -1
    assert b"projection" in lib.nrf_last_error()
