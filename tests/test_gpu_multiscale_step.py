"""The multiscale trainer's optimisation step on the fused path (src/training/train_multiscale.py:207-211,249-266): density noise
in front of the compositor's ReLU, nerf_mlp.NeRFLoss (rgb + depth + weights regulariser), clip_grad_norm_, AdamW --
nrf_composite_loss_backward, nrf_grad_sqnorm_partials, nrf_adamw_step_loss, and FusedStep / training.Adam / train_cli on top of them.

Tolerances (the project's existing bars, none fitted to this code):
  (i)   gradients within 2e-4 of each tensor's max, losses within 2e-4 relative (the train_grads.npz tests);
        compositor backward within 1e-4 of autograd (test_composite_backward_matches_autograd);
  (ii)  parameters within 1e-6 absolute of torch's optimiser over 5 steps (test_adam_kernel_matches_torch).  For the sampled
        parameters after three whole steps through the network: the plain fp32 autograd replay through the oracle is bit-identical
        to the capture on the build machine (spread 0.0, no bar), so tests/golden/make_golden_multiscale.py measures the spread of
        that replay under one fp32 rounding of the initial parameters (+-2^-24 relative, 6 trials) and stores it in the fixture
        (`cpu_spread`): 6.8e-5 for the parameters (Adam's sign-like first updates turn a gradient that is rounding noise around 0
        into +-lr per step), 7e-7 / 3e-6 / 1.4e-5 relative for the losses / regulariser / norm.  The sampled parameters get 4x that
        spread (the GPU adds one more summation order): 2.7e-4;
  (iii) norm within 1e-5 relative of the float64 value: for non-negative terms a summation whose longest serial chain is L adds
        under a tree of depth d errs by at most (L + d) 2^-24; L <= 128 and d <= 20 gives 8.8e-6.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_training import _CFG, _write_scene, composite_case, make_model, make_v2, make_v3, rel_to_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def normals(seed, n):
    u1 = 1.0 - O.uniform01(seed, n).astype(np.float64)
    u2 = O.uniform01(seed + 1, n).astype(np.float64)
    return torch.from_numpy((np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).astype(np.float32))


def run_loss_backward(L, rgb, sig, z, d, tgt, white=False, w=(1.0, 0.0, 0.0), tdepth=None, noise_std=0.0, noise=None, seed=0, zero_n=0,
                      with_losses=True):
    """nrf_composite_loss_backward on (R,S,3) / (R,S,1) tensors [+ the loss side job of nrf_adamw_step_loss on a dummy parameter
    vector] -> dict of device tensors."""
    lib, st = L.lib(), L.stream_ptr()
    R, S = z.shape
    c, s_ = rgb.contiguous().cuda(), sig.reshape(R, S).contiguous().cuda()
    zc, dc, tc = z.contiguous().cuda(), d.contiguous().cuda(), tgt.contiguous().cuda()
    td = None if tdepth is None else tdepth.contiguous().cuda()
    nz = None if noise is None else noise.reshape(R, S).contiguous().cuda()
    out = dict(pred=torch.empty(R, 3, device="cuda"), d_rgb=torch.full((R, S, 3), 7.0, device="cuda"), d_sigma=torch.full((R, S), 7.0, device="cuda"),
               terms=torch.empty(3, R, device="cuda"), zero=torch.ones(max(zero_n, 1), device="cuda"))
    lo = L.loss_opts(w[0], w[2], w[1], L.ptr(td), noise_std, L.ptr(nz), seed)
    L.check(lib.nrf_composite_loss_backward(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, int(white), L.ptr(tc), C.byref(lo), L.ptr(out["pred"]),
                                            L.ptr(out["d_rgb"]), 3, L.ptr(out["d_sigma"]), 1, L.ptr(out["terms"]), L.ptr(out["zero"]) if zero_n else None,
                                            zero_n, st))
    if with_losses:
        p, g, m, v = (torch.zeros(4, device="cuda") for _ in range(4))
        out["losses"] = torch.empty(4, device="cuda")
        L.check(lib.nrf_adamw_step_loss(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0.0, None, None, L.ptr(out["terms"]),
                                        R, S, w[0], w[1] if tdepth is not None else 0.0, w[2], L.ptr(out["losses"]), st))
    torch.cuda.synchronize()
    return out


def autograd_loss(rgb, sig, z, d, tgt, white, w, tdepth, noise_std, noise):
    """The reference's VolumeRenderer (train mode) + nerf_mlp.NeRFLoss, written out: autograd through oracle.volume_render."""
    r1, s1 = rgb.clone().requires_grad_(True), sig.clone().requires_grad_(True)
    dens = s1 if noise is None else s1 + noise.reshape(sig.shape) * noise_std
    o_rgb, o_dep, o_w = O.volume_render(r1, dens, z, d, white_bkgd=white)
    l_rgb = torch.nn.functional.mse_loss(o_rgb, tgt)
    l_dep = torch.nn.functional.l1_loss(o_dep, tdepth) if tdepth is not None else torch.zeros(())
    l_reg = torch.mean(o_w ** 2)
    total = w[0] * l_rgb + w[1] * l_dep + w[2] * l_reg
    total.backward()
    return dict(pred=o_rgb.detach(), losses=torch.stack([total, l_rgb, l_dep, l_reg]).detach(), d_rgb=r1.grad, d_sigma=s1.grad[..., 0])


def check_against(got, ref, grad_bar):
    assert (got["pred"].cpu() - ref["pred"]).abs().max() < 1e-5
    gl, rl = got["losses"].cpu().double(), ref["losses"].double()
    print("losses", gl.tolist(), rl.tolist())
    assert torch.all((gl - rl).abs() <= 2e-4 * rl.abs() + 1e-12), (gl, rl)
    e_rgb = rel_to_max(got["d_rgb"], ref["d_rgb"])
    # d sigma spans many orders of magnitude (dist = 1e10 on the last sample): relative to each ray's largest entry
    ds, es = got["d_sigma"].cpu(), ref["d_sigma"]
    scale = es.abs().amax(dim=1, keepdim=True).clamp_min(1e-20)
    e_sig = float(((ds - es).abs() / scale).max())
    print("d_rgb err / max", e_rgb, "d_sigma err / ray max", e_sig)
    assert e_rgb < grad_bar and e_sig < grad_bar


# ---------------------------------------------------------------------------------------------
# compositor + loss + backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64])
def test_composite_loss_backward_matches_reference_fixture(N, golden, S):
    """The reference's VolumeRenderer (train(), noise_std 0.5) + NeRFLoss with a depth target; opaque samples and sigma <= 0."""
    from nerf_few_shot_limitations_amd import _lib as L
    g = golden("multiscale_step")
    k = f"c{S}_"
    t = lambda name: torch.from_numpy(g[k + name])
    w = tuple(float(x) for x in g[k + "weights"])
    got = run_loss_backward(L, t("rgb"), t("density"), t("z"), t("rays_d"), t("target"), False, w, t("target_depth"), float(g[k + "noise_std"]), t("noise"))
    ref = dict(pred=t("pred"), losses=t("losses"), d_rgb=t("d_rgb"), d_sigma=t("d_density"))
    check_against(got, ref, 2e-4)                                      # bar (i)
    # sigma_eff <= 0 passes no gradient, exactly
    eff = t("density")[..., 0] + t("noise") * float(g[k + "noise_std"])
    assert (eff <= 0).any() and torch.all(got["d_sigma"].cpu()[eff <= 0] == 0)


@pytest.mark.parametrize("terms", ["rgb", "reg", "depth", "all"])
@pytest.mark.parametrize("S,opaque,white", [(32, False, False), (64, True, False), (100, True, True), (200, False, True)])
def test_composite_loss_backward_matches_autograd(N, S, opaque, white, terms):
    from nerf_few_shot_limitations_amd import _lib as L
    R = 257
    rgb, sig, z, d = composite_case(R, S, 41, opaque)
    tgt = torch.from_numpy(O.uniform01(54, R * 3).reshape(R, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(55, R) * 4 + 2).float() if terms in ("depth", "all") else None
    noise = normals(56, R * S).reshape(R, S, 1)
    w = {"rgb": (1.0, 0.0, 0.0), "reg": (0.0, 0.0, 0.5), "depth": (0.0, 0.3, 0.0), "all": (0.7, 0.3, 0.5)}[terms]
    std = 0.4
    ref = autograd_loss(rgb, sig, z, d, tgt, white, w, tdepth, std, noise)
    got = run_loss_backward(L, rgb, sig, z, d, tgt, white, w, tdepth, std, noise)
    check_against(got, ref, 1e-4)
    eff = sig[..., 0] + noise[..., 0] * std
    assert (eff <= 0).any() and torch.all(got["d_sigma"].cpu()[eff <= 0] == 0)
    assert ((sig[..., 0] <= 0) & (eff > 0)).any()          # network density clamped, noise positive: contributes to the render


@pytest.mark.parametrize("S,opaque,white", [(32, False, False), (64, True, False), (100, True, True), (200, False, True)])
def test_all_options_off_is_the_mse_kernel_bit_for_bit(N, S, opaque, white):
    from nerf_few_shot_limitations_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    R = 300
    rgb, sig, z, d = composite_case(R, S, 61, opaque)
    tgt = torch.from_numpy(O.uniform01(62, R * 3).reshape(R, 3)).float()
    new = run_loss_backward(L, rgb, sig, z, d, tgt, white, (0.7, 0.0, 0.0), zero_n=1000, with_losses=False)
    c, s_ = rgb.contiguous().cuda(), sig.reshape(R, S).contiguous().cuda()
    pred, d_rgb, d_sig, rl = torch.empty(R, 3, device="cuda"), torch.empty(R, S, 3, device="cuda"), torch.empty(R, S, device="cuda"), torch.empty(R, device="cuda")
    zc, dc, tc = z.cuda(), d.cuda(), tgt.cuda()                 # kept alive until the launch has run
    L.check(lib.nrf_composite_mse_backward(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, int(white), L.ptr(tc), 0.7, L.ptr(pred),
                                           L.ptr(d_rgb), 3, L.ptr(d_sig), 1, L.ptr(rl), None, 0, st))
    torch.cuda.synchronize()
    assert torch.equal(new["pred"], pred) and torch.equal(new["d_rgb"], d_rgb) and torch.equal(new["d_sigma"], d_sig)
    assert torch.equal(new["terms"][0], rl)
    assert torch.all(new["zero"] == 0)                      # the side job cleared the buffer
    assert torch.all(new["terms"][2] == 0)                  # no depth target: no depth term


# ---------------------------------------------------------------------------------------------
# in-kernel noise
# ---------------------------------------------------------------------------------------------
def _noisy(L, R, S, seed, zero_n=0, lo=0, hi=None):
    hi = R if hi is None else hi
    rgb, sig, z, d = composite_case(R, S, 71, False)
    tgt = torch.from_numpy(O.uniform01(72, R * 3).reshape(R, 3)).float()
    return run_loss_backward(L, rgb[lo:hi], sig[lo:hi], z[lo:hi], d[lo:hi], tgt[lo:hi], False, (1.0, 0.0, 0.1), None, 0.5, None, seed, zero_n, with_losses=False)


def test_in_kernel_noise_is_reproducible_and_grid_independent(N):
    from nerf_few_shot_limitations_amd import _lib as L
    R, S = 512, 100
    a, b = _noisy(L, R, S, 1234), _noisy(L, R, S, 1234)
    for k in ("pred", "d_rgb", "d_sigma", "terms"):
        assert torch.equal(a[k], b[k]), k
    # a far larger grid (sized by the buffer to clear: 16384 workgroups instead of 128): the same rays get the same draws
    c = _noisy(L, R, S, 1234, zero_n=1 << 24)
    for k in ("pred", "d_rgb", "d_sigma", "terms"):
        assert torch.equal(a[k], c[k]), k
    # the draw is keyed by the ray's index in the call: the first rays of a shorter call see the same noise (their loss
    # gradients scale with 1 / R, so compare the render)
    e = _noisy(L, R, S, 1234, hi=128)
    assert torch.equal(a["pred"][:128], e["pred"])
    f = _noisy(L, R, S, 1235)
    assert not torch.equal(a["pred"], f["pred"]) and not torch.equal(a["d_sigma"], f["d_sigma"])
    noiseless = run_loss_backward(L, *composite_case(R, S, 71, False), torch.from_numpy(O.uniform01(72, R * 3).reshape(R, 3)).float(), False, (1.0, 0.0, 0.1),
                                  with_losses=False)
    assert not torch.equal(a["pred"], noiseless["pred"])


def test_in_kernel_noise_moments(N):
    """2^20 draws observed through the render: sigma = 6 everywhere, noise_std = 1, sample spacing 0.01 and |d| = 1, so that
    alpha_i = 1 - exp(-(6 + n_i) 0.01) stays near 0.06 (|n| <= 5.77 keeps 6 + n positive: the ReLU never acts) and
    d_rgb[i] = w_i g_rgb with g_rgb = 2 (pred - target) / (3 R) known from the outputs.  Dividing out the transmittance front to
    back in float64 gives alpha_i, hence n_i, to ~1e-5.  S = 65: the last sample (dist 1e10) is not observed, 64 per ray are."""
    from nerf_few_shot_limitations_amd import _lib as L
    R, S, dz, s0 = 16384, 65, 0.01, 6.0
    n_draws = R * (S - 1)
    assert n_draws == 1 << 20
    rgb = torch.ones(R, S, 3)
    sig = torch.full((R, S, 1), s0)
    z = (2.0 + dz * torch.arange(S, dtype=torch.float64)).float()[None, :].expand(R, S).contiguous()
    d = torch.zeros(R, 3); d[:, 2] = 1.0
    tgt = torch.full((R, 3), 5.0)
    out = run_loss_backward(L, rgb, sig, z, d, tgt, False, (1.0, 0.0, 0.0), None, 1.0, None, 2024, with_losses=False)
    pred = out["pred"].cpu().numpy()
    g = (np.float32(2.0) * np.float32(1.0) / (np.float32(3.0) * np.float32(R))) * (pred[:, 0] - np.float32(5.0))       # the kernel's fp32 arithmetic
    w = out["d_rgb"].cpu().numpy()[:, :, 0].astype(np.float64) / g.astype(np.float64)[:, None]
    dist = np.diff(z.numpy().astype(np.float32), axis=1).astype(np.float64)                      # fp32 differences, as the kernel forms them
    T = np.ones(R)
    n = np.empty((R, S - 1))
    for i in range(S - 1):
        alpha = w[:, i] / T
        n[:, i] = -np.log1p(-alpha) / dist[:, i] - s0
        T = T * (1.0 - alpha + 1e-10)
    n = n.reshape(-1)
    assert np.isfinite(n).all()
    mean, var = n.mean(), n.var()
    skew = ((n - mean) ** 3).mean() / var ** 1.5
    print("moments over", n.size, "draws: mean", mean, "var", var, "skew", skew, "min", n.min(), "max", n.max())
    assert abs(mean) < 5 / np.sqrt(n_draws) and abs(var - 1) < 5 * np.sqrt(2 / n_draws) and abs(skew) < 5 * np.sqrt(6 / n_draws)
    # neighbouring samples and neighbouring rays are uncorrelated (same 5 sigma bar: a correlation of N pairs has sd 1 / sqrt(N))
    m = n.reshape(R, S - 1)
    assert abs(np.mean(m[:, 1:] * m[:, :-1])) < 5 / np.sqrt(m[:, 1:].size) and abs(np.mean(m[1:] * m[:-1])) < 5 / np.sqrt(m[1:].size)


# ---------------------------------------------------------------------------------------------
# gradient norm, clipped update
# ---------------------------------------------------------------------------------------------
def _norm_of(L, g):
    lib, st = L.lib(), L.stream_ptr()
    n = g.numel()
    ws = torch.empty(lib.nrf_grad_sqnorm_workspace_bytes(n) // 4, device="cuda")
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    norm = torch.full((), -1.0, device="cuda")
    L.check(lib.nrf_grad_sqnorm_partials(L.ptr(g), n, L.ptr(ws), ws.numel() * 4, st))
    L.check(lib.nrf_adamw_step_loss(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 1.0, L.ptr(ws), L.ptr(norm), None, 0, 1,
                                    0.0, 0.0, 0.0, None, st))
    torch.cuda.synchronize()
    return norm.item(), p, m


def _param_counts(N):
    from nerf_few_shot_limitations_amd import _lib as L
    out = []
    for mk, kw in ((make_model, {}), (make_v3, dict(dino_dim=128))):
        model, _ = mk(N, "f32", **kw)
        out.append(int(model.flat_params().ensure().numel()))
        assert out[-1] == L.lib().nrf_param_count(model.handle(torch.device("cuda", 0), "f32"))
    return out


def test_grad_norm_matches_float64_and_is_reproducible(N):
    from nerf_few_shot_limitations_amd import _lib as L
    for n in [1, 255, 100003] + _param_counts(N):
        for k, mag in enumerate((1e-6, 1e-3, 1.0, 1e3)):
            g = (torch.from_numpy(O.uniform01(81 + k, n) - 0.5).float() * mag).cuda()
            want = float(torch.linalg.vector_norm(g.double()))
            a, _, _ = _norm_of(L, g)
            b, _, _ = _norm_of(L, g)
            print("n", n, "magnitude", mag, "norm", a, "float64", want, "rel", abs(a - want) / want)
            assert abs(a - want) <= 1e-5 * want                        # bar (iii)
            assert a == b
        # magnitudes spanning 1e-6 .. 1e3 inside one vector
        g = (torch.from_numpy(O.uniform01(91, n) - 0.5).float() * torch.from_numpy(10.0 ** (O.uniform01(92, n) * 9 - 6)).float()).cuda()
        want = float(torch.linalg.vector_norm(g.double()))
        a, _, _ = _norm_of(L, g)
        assert abs(a - want) <= 1e-5 * want and a == _norm_of(L, g)[0]
    norm, p, m = _norm_of(L, torch.zeros(100003, device="cuda"))
    assert norm == 0.0 and torch.isfinite(p).all() and torch.all(p == 0) and torch.all(m == 0)      # coefficient 1, no NaN


@pytest.mark.parametrize("decoupled", [True, False])
def test_clipped_update_matches_torch(N, decoupled):
    """clip_grad_norm_ (CPU) + torch.optim.AdamW / Adam against nrf_grad_sqnorm_partials + nrf_adamw_step_loss, 5 steps whose
    gradient norms lie on both sides of max_norm (magnitudes 1e-2 .. 1e2 times a vector of norm ~91)."""
    from nerf_few_shot_limitations_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    n, max_norm = 100003, 1.0
    p0 = torch.from_numpy(O.uniform01(71, n) - 0.5).float()
    ref = torch.nn.Parameter(p0.clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref], lr=5e-4, weight_decay=1e-2 if decoupled else 1e-6)
    p = p0.clone().cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws = torch.empty(lib.nrf_grad_sqnorm_workspace_bytes(n) // 4, device="cuda")
    norm = torch.empty((), device="cuda")
    clipped = []
    for step in range(1, 6):
        g = torch.from_numpy(O.uniform01(72 + step, n) - 0.5).float() * (10.0 ** (step - 5))       # norms 0.009 .. 91
        ref.grad = g.clone()
        want = float(torch.nn.utils.clip_grad_norm_([ref], max_norm))
        clipped.append(want > max_norm)
        opt.step()
        gd = g.cuda()
        L.check(lib.nrf_grad_sqnorm_partials(L.ptr(gd), n, L.ptr(ws), ws.numel() * 4, st))
        L.check(lib.nrf_adamw_step_loss(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, 5e-4, 0.9, 0.999, 1e-8, 1e-2 if decoupled else 1e-6, step, int(decoupled),
                                        max_norm, L.ptr(ws), L.ptr(norm), None, 0, 1, 0.0, 0.0, 0.0, None, st))
        assert abs(norm.item() - want) <= 1e-5 * want
    assert any(clipped) and not all(clipped)
    err = (p.cpu() - ref.detach()).abs().max().item()
    print("decoupled", decoupled, "clipped", clipped, "max |p - torch|", err)
    assert err < 1e-6                                                  # bar (ii)


def test_new_entry_points_refuse_bad_arguments_on_the_gpu(N):
    from nerf_few_shot_limitations_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    g = torch.ones(5000, device="cuda")
    ws = torch.empty(8, device="cuda")
    assert lib.nrf_grad_sqnorm_workspace_bytes(5000) == 20
    assert lib.nrf_grad_sqnorm_partials(L.ptr(g), 5000, L.ptr(ws), 16, st) == -1 and b"smaller" in lib.nrf_last_error()
    assert lib.nrf_grad_sqnorm_partials(L.ptr(g), 5000, None, 20, st) == -1
    assert lib.nrf_grad_sqnorm_partials(L.ptr(g), 5000, L.ptr(ws), 32, st) == 0
    torch.cuda.synchronize()
    assert abs(float(ws[:5].sum()) - 5000.0) < 1e-2


# ---------------------------------------------------------------------------------------------
# FusedStep
# ---------------------------------------------------------------------------------------------
# the recipe's own values (experiments/multiscale.yaml: loss.reg_weight, loss.depth_weight, rendering.noise_std, optimizer.weight_decay;
# train_multiscale.py:259-264: max_norm 1.0, AdamW) with a depth target on top, so that every option is on; the learning rate is
# test_fused_step_equals_autograd_route's.  The terms' own arithmetic is held to tighter bars at the kernel level above.
OPTS = dict(reg_weight=1e-4, depth_weight=0.1, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True)
WD = 1e-6


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v1", "bf16"), ("v2", "f32"), ("v2", "bf16"), ("v3", "f32"), ("v3", "bf16"),
                                      ("v3w", "f32"), ("v3w", "bf16")])
def test_fused_step_with_all_options_equals_autograd_route(N, net, mode):
    """The inputs and tolerances of test_fused_step_equals_autograd_route; the autograd route is the drop-in modules, the loss
    written out here, torch.nn.utils.clip_grad_norm_ and torch.optim.AdamW; the noise is a tensor on both sides."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    R, S, steps = 160, 32, 4
    z = torch.sort(torch.from_numpy(O.uniform01(101, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values.cuda()
    rd = torch.from_numpy(O.uniform01(102, R * 3).reshape(R, 3) - 0.5).float().cuda()
    tgt = torch.from_numpy(O.uniform01(103, R * 3).reshape(R, 3)).float().cuda()
    pos = torch.from_numpy(O.uniform01(104, R * S * 3).reshape(R * S, 3) * 4 - 2).float()
    tdepth = torch.from_numpy(O.uniform01(106, R) * 4 + 2).float().cuda()
    noise = normals(107, R * S).reshape(R, S).cuda()
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    dd = None
    if net == "v1":
        a, _ = make_model(N, mode, scene="solid")
        b, _ = make_model(N, mode, scene="solid")
        pts = O.positional_encoding(pos, 10).cuda()
    elif net == "v2":
        a, _ = make_v2(N, mode, scene="solid")
        b, _ = make_v2(N, mode, scene="solid")
        pts = pos.cuda()
    else:
        dd = 128 if net == "v3w" else 64
        seed = 4 if net == "v3w" else 2
        a, _ = make_v3(N, mode, scene="solid", dino_dim=dd, seed=seed)
        b, _ = make_v3(N, mode, scene="solid", dino_dim=dd, seed=seed)
        pts = pos.cuda()
    dino = torch.from_numpy(O.uniform01(105, R * S * dd).reshape(R * S, dd) * 2 - 1).float().cuda() if dd else None
    a.flat_params().ensure()
    params = list(a.parameters())
    opt = torch.optim.AdamW(params, lr=5e-4, weight_decay=WD)
    vr = N.VolumeRenderer()
    ref_losses, ref_norms = [], []
    for _ in range(steps):
        opt.zero_grad()
        if net == "v1":
            o4 = a(pts).view(R, S, 4)
            c, sg = o4[..., :3], o4[..., 3:4]
        else:
            c, sg = a(pts, dirs, dino)
            c, sg = c.view(R, S, 3), sg.view(R, S, 1)
        pred, depth, w = vr(c, sg + noise.view(R, S, 1) * OPTS["noise_std"], z, rd)
        loss = (torch.nn.functional.mse_loss(pred, tgt) + OPTS["depth_weight"] * torch.nn.functional.l1_loss(depth, tdepth)
                + OPTS["reg_weight"] * torch.mean(w ** 2))
        loss.backward()
        ref_norms.append(float(torch.nn.utils.clip_grad_norm_(params, OPTS["max_grad_norm"])))
        opt.step()
        ref_losses.append(loss.item())
    step = FusedStep(b, lr=5e-4, weight_decay=WD, **OPTS)
    got, norms = [], []
    for _ in range(steps):
        got.append(step(pts, z, rd, tgt, dirs=dirs if net != "v1" else None, dino=dino, target_depth=tdepth, noise=noise).item())
        norms.append(step.last_grad_norm.item())
        ll = step.last_losses
        assert abs(ll["total"].item() - (ll["rgb"].item() + OPTS["depth_weight"] * ll["depth"].item() + OPTS["reg_weight"] * ll["reg"].item())) < 1e-6
    print(net, mode, "losses", ref_losses, got, "norms", ref_norms, norms)
    tol = 1e-5 if mode == "f32" else 2e-3
    assert np.allclose(ref_losses, got, rtol=tol, atol=1e-7), (ref_losses, got)
    # the norm: both routes start from the same parameters, so step 1 compares two gradients of one function -- bar (i)'s 2e-4 (f32)
    # resp. the 16-bit loss tolerance; later steps' norms amplify rounding far more than the losses do (printed above; the norm
    # kernel itself is held to 1e-5 of float64 in test_grad_norm_matches_float64_and_is_reproducible)
    assert abs(norms[0] - ref_norms[0]) <= max(2e-4, tol) * ref_norms[0], (ref_norms, norms)
    assert max(ref_norms) > OPTS["max_grad_norm"]          # the clipping acts


def test_fused_step_plain_arguments_take_the_old_path(N):
    """A FusedStep built with the arguments it always had returns the bits of the three-call tail it always ran."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import FusedStep
    R, S = 160, 32
    z = torch.sort(torch.from_numpy(O.uniform01(101, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values.cuda()
    rd = torch.from_numpy(O.uniform01(102, R * 3).reshape(R, 3) - 0.5).float().cuda()
    tgt = torch.from_numpy(O.uniform01(103, R * 3).reshape(R, 3)).float().cuda()
    pts = O.positional_encoding(torch.from_numpy(O.uniform01(104, R * S * 3).reshape(R * S, 3) * 4 - 2).float(), 10).cuda()
    a, _ = make_model(N, "f32", scene="solid")
    b, _ = make_model(N, "f32", scene="solid")
    plain = FusedStep(a, lr=5e-4, weight_decay=1e-6)
    la = [plain(pts, z, rd, tgt).item() for _ in range(2)]
    assert plain.last_grad_norm is None and set(plain.last_losses) == {"total"}
    # the general kernels with every option neutral (Adam's coupled decay, a clip threshold no gradient reaches): same losses
    wide = FusedStep(b, lr=5e-4, weight_decay=1e-6, max_grad_norm=1e30)
    lb = [wide(pts, z, rd, tgt).item() for _ in range(2)]
    assert np.allclose(la, lb, rtol=1e-6)
    assert wide.last_grad_norm.item() > 0 and set(wide.last_losses) == {"total", "rgb", "depth", "reg"}


def _indices(numel, k=64):
    return np.arange(numel) if numel <= k else (np.arange(k) * numel) // k


def test_fused_step_matches_reference_fixture(N, golden):
    """Three steps of the reference's multiscale trainer on one batch (tests/golden/make_golden_multiscale.py): steps 1 and 2 clip
    (pre-clip norms 1.74 and 1.05), step 3 passes through (0.98).  Losses and norms to bar (i), the sampled parameters to bar (ii)."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    g = golden("multiscale_step")
    assert list(g["step_clips"]) == [True, True, False]
    noise_std, rgb_w, depth_w, reg_w, max_norm, lr, wd = (float(x) for x in g["hyper"])
    model, p0 = make_v3(N, "f32", scene="solid", dino_dim=128, seed=int(g["weight_seed"]))
    R, S = g["z"].shape
    cu = lambda k: torch.from_numpy(g[k]).cuda()
    rd = cu("rays_d")
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    dino = torch.from_numpy(g["dino_q"].astype(np.float32) / 128.0).cuda()
    step = FusedStep(model, lr=lr, weight_decay=wd, rgb_weight=rgb_w, reg_weight=reg_w, depth_weight=depth_w, noise_std=noise_std,
                     max_grad_norm=max_norm, decoupled_weight_decay=True)
    for i in range(3):
        total = step(cu("pos"), cu("z"), rd, cu("target"), dirs=dirs, dino=dino, noise=cu("noise")).item()
        ll = {k: v.item() for k, v in step.last_losses.items()}
        norm = step.last_grad_norm.item()
        want = g["step_losses"][i]
        print("step", i + 1, "losses", total, ll, "reference", want.tolist(), "norm", norm, "reference", float(g["step_norms"][i]))
        assert abs(total - want[0]) <= 2e-4 * want[0] and abs(ll["rgb"] - want[1]) <= 2e-4 * want[1] and abs(ll["reg"] - want[2]) <= 2e-4 * want[2]
        assert ll["depth"] == 0.0                                      # the reference's targets carry no depth
        assert abs(norm - float(g["step_norms"][i])) <= 2e-4 * float(g["step_norms"][i])
        assert (norm > max_norm) == bool(g["step_clips"][i])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    errs, moved = [], []
    for k in p0:
        v = sd[k].reshape(-1)
        ref = g["param_" + k]
        errs.append(np.abs(v.numpy()[_indices(v.numel())] - ref))
        moved.append(np.abs(p0[k].reshape(-1).numpy()[_indices(v.numel())] - ref))
        assert abs(float(v.norm()) - float(g["pnorm_" + k])) <= 1e-5 * float(g["pnorm_" + k]) + 1e-6, k
    errs, moved = np.concatenate(errs), np.concatenate(moved)
    bound = 4 * float(g["cpu_spread"][4])
    print("sampled parameters:", errs.size, "max |err|", errs.max(), "bound", bound, "largest move", moved.max())
    assert moved.max() > bound                                         # the parameters moved by more than the bar
    assert errs.max() <= bound                                         # bar (ii), see the module docstring


# ---------------------------------------------------------------------------------------------
# data parallel, train_cli
# ---------------------------------------------------------------------------------------------
def test_data_parallel_with_clipping_equals_one_rank_on_the_whole_batch(N, tmp_path):
    """Two ranks (gloo, sharing the test GPU) on halves of a batch, gradients averaged, the norm taken behind the all-reduce: the
    parameters after 3 steps equal one process on the whole batch, within what Adam's sign-like first steps allow
    (test_data_parallel_two_ranks_equal_one_rank_on_the_whole_batch's bounds)."""
    import importlib.util, socket, subprocess, sys
    from nerf_few_shot_limitations_amd.training import FusedStep
    steps = 3
    out = str(tmp_path / "dp_multiscale.npy")
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = s_.getsockname()[1]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    worker_path = os.path.join(root, "tests", "dp_multiscale_worker.py")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           worker_path, out, str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    got_norms = np.load(out + ".norms.npy")
    spec = importlib.util.spec_from_file_location("dp_multiscale_worker", worker_path)
    worker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(worker)
    x, z, rd, tgt, noise = worker.batch()
    model, _ = make_model(N, "f32", scene="solid")
    step = FusedStep(model, lr=1e-2, **worker.OPTS)
    norms = []
    for _ in range(steps):
        step(x.reshape(-1, 63).cuda(), z.cuda(), rd.cuda(), tgt.cuda(), noise=noise.cuda())
        norms.append(step.last_grad_norm.item())
    ref = model.flat_params().flat.detach().cpu().numpy()
    print("norms", norms, got_norms.tolist(), "max |dp - single|", np.abs(got - ref).max(), "share > 1e-4", np.mean(np.abs(got - ref) > 1e-4))
    assert max(norms) > worker.OPTS["max_grad_norm"]                   # clipping is on and acts
    assert np.allclose(norms, got_norms, rtol=1e-3)
    assert np.abs(got - ref).max() < 2.5 * 1e-2 * steps
    assert np.mean(np.abs(got - ref) > 1e-4) < 0.02


def test_train_cli_multiscale_recipe(N, tmp_path):
    import json
    from nerf_few_shot_limitations_amd import evaluate_cli, train_cli
    root = str(tmp_path / "scene")
    _write_scene(root)
    cfg = tmp_path / "cfg.yaml"
    text = _CFG.format(dino="false", pf=10).replace("reg_weight: 0.0", "reg_weight: 0.0001").replace("white_bkgd: false", "white_bkgd: false, noise_std: 0.1")
    text = text.replace("val_freq: 2, save_freq: 3", "val_freq: 2, save_freq: 2")
    cfg.write_text(text)
    p = dict(O.make_weights("v2", 1, "fog"))
    p["pos_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 9, 10)
    p["dir_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 3, 4)
    torch.save({"epoch": 0, "nerf_model_state_dict": p}, str(tmp_path / "init.pth"))
    common = ["--config", str(cfg), "--data", root, "--mode", "f32", "--epochs", "2", "--checkpoint", str(tmp_path / "init.pth")]
    out = str(tmp_path / "ms")
    log = train_cli.main(common + ["--out", out, "--recipe", "multiscale"])
    print("multiscale recipe log", log)
    assert [r["epoch"] for r in log] == [1, 2]
    assert all(np.isfinite(r["loss"]) for r in log) and log[1]["loss"] < log[0]["loss"]
    ck = torch.load(os.path.join(out, "epoch_2.pth"), map_location="cpu", weights_only=True)
    assert "nerf_model_state_dict" in ck and "nerf_state_dict" in ck
    assert all(torch.equal(ck["nerf_state_dict"][k], ck["nerf_model_state_dict"][k]) for k in ck["nerf_state_dict"])
    m = evaluate_cli.main(["--config", str(cfg), "--data", root, "--checkpoint", os.path.join(out, "epoch_2.pth"), "--mode", "f32"])
    assert m["views"] == 2 and np.isfinite(m["psnr"])
    only_new = {k: v for k, v in ck.items() if k != "nerf_model_state_dict"}          # a checkpoint as train_multiscale.py writes it
    torch.save(only_new, str(tmp_path / "only_new.pth"))
    m2 = evaluate_cli.main(["--config", str(cfg), "--data", root, "--checkpoint", str(tmp_path / "only_new.pth"), "--mode", "f32"])
    assert m2["psnr"] == m["psnr"]
    # the default recipe is `train`, bit for bit
    a = train_cli.main(common + ["--out", str(tmp_path / "a")])
    b = train_cli.main(common + ["--out", str(tmp_path / "b"), "--recipe", "train"])
    assert [r["loss"] for r in a] == [r["loss"] for r in b]
    assert [r["loss"] for r in a] != [r["loss"] for r in log]
    ca = torch.load(os.path.join(str(tmp_path / "a"), "epoch_2.pth"), map_location="cpu", weights_only=True)
    assert "nerf_state_dict" not in ca
