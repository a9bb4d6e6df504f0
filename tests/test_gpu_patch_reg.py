"""The patch-based depth-smoothness term (RegNeRF) of the fused training step on the GPU (nerfhip.h:
nrf_composite_patch_loss_backward, nrf_patch_terms_finish; FusedStep(depth_smooth_weight=, patch_size=), n_patches=;
ray_sampler.patch_rays).

The oracle is float64 autograd through oracle.nerf_oracle.volume_render plus the definitions of the terms (tests/test_ray_reg_host.py,
tests/test_patch_reg_host.py).  The supervised rows and the seven loss values meet tests/test_gpu_multiscale_step.py's check_against.
The patch rows of d_sigma are held to the float64 backward of sum_r gd_r depth_r + the target-free terms, with gd_r the float64
stencil on the depths the kernel reported: the cancellation inside gd is conditioning, not a kernel error, and the stencil's own
rounding has its bound from tests/test_patch_reg_host.py.

    |d_sigma_i - ref_i| <= 1e-4 max_i |ref| + delta_p |d depth_r / d sigma_i|

on every entry whose float64 reference is an fp32 normal number; where it is not (at S = 2 with an opaque first sample some rays'
entries are 1e-39 ... 5e-48, and no fp32 array holds them) the kernel must have written 0 or a denormal.

With patches (n_patches > 0) the kernel runs the compositor bodies with composite_core.hpp's FINE: the transmittance factor formed
from e = exp(-relu(sigma) dist) itself and a true exclusive suffix sum.  Without it -- measured on an MI355X -- six cases missed
their bars: at (S = 2, opaque, terms off) the supervised rows by 0.9 - 3.0 of the ray's maximum (`inclusive - own` loses the second
sample's w v of 1e-11 against the own 1e-1, and the divisor is 1e-10), at (P = 16, S = 16, opaque) the patch rows by 61.9 and 1.37
times their allowance (alpha = 1 - e rounded to fp32 costs every transmittance behind e = 1e-5 a relative 6e-3).  With it the largest
share of the allowance is 0.49 (P = 16, S = 2, terms off).  With n_patches = 0 the bodies are the parent's, for the parent's bits
(test 3)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_multiscale_step import check_against, normals
from tests.test_gpu_ray_reg import KAPPA, Recorder, compacted, models, ray_scene, record, run_reg
from tests.test_patch_reg_host import _train_poses, smooth_of, stencil_bound, stencil_gd
from tests.test_ray_reg_host import case, distortion

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS, NP = 5, 3                     # supervised rays and patches of the raw-entry cases
LAM = 0.9                         # depth_smooth_weight there
ALL = dict(w=(0.7, 0.3, 0.5), std=0.4, dw=0.6, ow=0.8, k=5, white=True)
OFF = dict(w=(1.0, 0.0, 0.0), std=0.0, dw=0.0, ow=0.0, k=0, white=False)


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def L(N):
    from nerf_few_shot_limitations_amd import _lib as L
    return L


def run_patch(L, rgb, sig, z, d, tgt, P, n_p, lam=LAM, white=False, w=(1.0, 0.0, 0.0), tdepth=None, noise_std=0.0, noise=None, reg=None, slot=None,
              zero_n=0, with_losses=True):
    """nrf_composite_patch_loss_backward [+ nrf_patch_terms_finish] -> dict of device tensors.  Dense: rgb (R,S,3), sig (R,S[,1]); with
    `slot` (R,S): rgb (M,3), sig (M) compacted rows.  tgt (R_s,3), tdepth (R_s)."""
    lib, st = L.lib(), L.stream_ptr()
    R, S = z.shape
    c, s_ = rgb.reshape(-1, 3).contiguous().cuda(), sig.reshape(-1).contiguous().cuda()
    rows = c.shape[0]
    zc, dc, tc = z.contiguous().cuda(), d.contiguous().cuda(), tgt.contiguous().cuda()
    td = None if tdepth is None else tdepth.contiguous().cuda()
    nz = None if noise is None else noise.reshape(R, S).contiguous().cuda()
    sl = None if slot is None else slot.reshape(R, S).to(torch.int32).contiguous().cuda()
    out = dict(pred=torch.empty(R, 3, device="cuda"), d_rgb=torch.full((rows, 3), 7.0, device="cuda"), d_sigma=torch.full((rows,), 7.0, device="cuda"),
               terms=torch.full((5, R), float("nan"), device="cuda"), zero=torch.ones(max(zero_n, 1), device="cuda"),
               patch_terms=torch.full((max(n_p, 1),), float("nan"), device="cuda"), patch_depth=torch.full((max(n_p, 1) * P * P,), float("nan"), device="cuda"))
    lo = L.loss_opts(w[0], w[2], w[1], L.ptr(td), noise_std, L.ptr(nz), 0)
    reg = reg if reg is not None else L.ray_reg()
    patch = L.patch_reg(lam, P, n_p)
    L.check(lib.nrf_composite_patch_loss_backward(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, int(white), L.ptr(tc), C.byref(lo), C.byref(reg),
                                                  None if sl is None else sl.data_ptr(), L.ptr(out["pred"]), L.ptr(out["d_rgb"]), 3, L.ptr(out["d_sigma"]), 1,
                                                  L.ptr(out["terms"]), L.ptr(out["zero"]) if zero_n else None, zero_n, st, C.byref(patch),
                                                  L.ptr(out["patch_terms"]), L.ptr(out["patch_depth"])))
    if with_losses:
        out["losses"] = torch.full((7,), float("nan"), device="cuda")
        L.check(lib.nrf_patch_terms_finish(L.ptr(out["terms"]), R, S, C.byref(lo), C.byref(reg), C.byref(patch), L.ptr(out["patch_terms"]),
                                           L.ptr(out["losses"]), st))
    torch.cuda.synchronize()
    out["patch_terms"], out["patch_depth"] = out["patch_terms"][:n_p], out["patch_depth"][: n_p * P * P].reshape(n_p, P, P)
    if slot is None:
        out["d_rgb"], out["d_sigma"] = out["d_rgb"].reshape(R, S, 3), out["d_sigma"].reshape(R, S)
    return out


def target_free(o_w, dens, z64, w, dw, ow, k):
    """reg_weight mean w^2 + dist_weight mean D + occ_weight mean O over all rays, and the three unweighted values."""
    f = torch.float64
    S = z64.shape[1]
    l_reg = torch.mean(o_w ** 2)
    l_dist = distortion(o_w, z64, KAPPA).mean() if dw > 0 else torch.zeros((), dtype=f)
    l_occ = torch.relu(dens[:, : min(k, S), 0]).mean(dim=1).mean() if ow > 0 else torch.zeros((), dtype=f)
    return w[2] * l_reg + dw * l_dist + ow * l_occ, l_reg, l_dist, l_occ


def oracle(rgb, sig, z, d, tgt, P, n_p, lam, white, w, tdepth, noise_std, noise, dw, ow, k, reported_depth):
    """float64 autograd of the total loss of the batch layout; and, for the patch rows, of sum_r gd_r depth_r + the target-free terms
    with gd_r the float64 stencil on the depths the kernel reported, with d depth_r / d sigma_i beside it."""
    f = torch.float64
    R, S = z.shape
    Rs = R - n_p * P * P
    z64, d64 = z.to(f), d.to(f)

    def render():
        r1, s1 = rgb.to(f).requires_grad_(True), sig.to(f).reshape(R, S, 1).requires_grad_(True)
        dens = s1 if noise is None else s1 + noise.to(f).reshape(s1.shape) * noise_std
        return (r1, s1, dens) + tuple(O.volume_render(r1, dens, z64, d64, white_bkgd=white))

    r1, s1, dens, o_rgb, o_dep, o_w = render()
    l_rgb = torch.nn.functional.mse_loss(o_rgb[:Rs], tgt.to(f))
    l_dep = torch.nn.functional.l1_loss(o_dep[:Rs], tdepth.to(f)) if tdepth is not None else torch.zeros((), dtype=f)
    free, l_reg, l_dist, l_occ = target_free(o_w, dens, z64, w, dw, ow, k)
    l_smooth = smooth_of(o_dep[Rs:].reshape(n_p, P, P))
    total = w[0] * l_rgb + w[1] * l_dep + free + lam * l_smooth
    total.backward()
    ref = dict(pred=o_rgb.detach().float(), depth=o_dep.detach(), d_rgb=r1.grad, d_sigma=s1.grad[..., 0],
               losses=torch.stack([total, l_rgb, l_dep, l_reg, l_dist, l_occ, l_smooth]).detach())
    # the patch rows
    gd = stencil_gd(reported_depth.double(), lam)[0].reshape(-1)
    r1, s1, dens, o_rgb, o_dep, o_w = render()
    free = target_free(o_w, dens, z64, w, dw, ow, k)[0]
    ref["patch_d_sigma"] = torch.autograd.grad((gd * o_dep[Rs:]).sum() + free, s1, retain_graph=True)[0][Rs:, :, 0]
    ref["d_depth"] = torch.autograd.grad(o_dep[Rs:].sum(), s1)[0][Rs:, :, 0]
    return ref


def check_patch_case(got, ref, sig, noise, std, P, n_p, lam, S, label):
    """The checks (a) - (f) of one case; returns the largest share of the patch rows' allowance."""
    R = sig.shape[0]
    Rs = R - n_p * P * P
    # (a) the reported depths
    dep, ref_dep = got["patch_depth"].cpu().double().reshape(-1), ref["depth"][Rs:]
    assert torch.all((dep - ref_dep).abs() <= 1e-5 * ref_dep.abs().clamp_min(1.0)), (dep - ref_dep).abs().max()
    # (b) all seven loss values, (c) the supervised rows
    sup = dict(pred=got["pred"][:Rs], losses=got["losses"], d_rgb=got["d_rgb"][:Rs], d_sigma=got["d_sigma"][:Rs])
    check_against(sup, dict(pred=ref["pred"][:Rs], losses=ref["losses"], d_rgb=ref["d_rgb"][:Rs], d_sigma=ref["d_sigma"][:Rs]), 1e-4)
    assert (got["pred"][Rs:].cpu() - ref["pred"][Rs:]).abs().max() < 1e-5
    # (d) the patch rows of d_sigma
    ds, want = got["d_sigma"][Rs:].cpu().double(), ref["patch_d_sigma"]
    delta = stencil_bound(got["patch_depth"].cpu(), lam).repeat_interleave(P * P)[:, None]
    allow = 1e-4 * want.abs().amax(dim=1, keepdim=True) + delta * ref["d_depth"].abs()
    err = (ds - want).abs()
    # d_sigma is an fp32 array.  Exactly the entries whose float64 reference is no fp32 normal number (behind a first sample with
    # 40 dist > 87 they go down to 5e-48 at S = 2; the exact zeros of (f) are among them) are taken out of the relative bar: there
    # the kernel must have written 0 or a denormal
    tiny = want.abs() < 2.0 ** -126
    assert torch.all(ds[tiny].abs() < 2.0 ** -126)
    err = torch.where(tiny, torch.zeros_like(err), err)
    assert torch.any(ds != 0), "no patch ray has a gradient"
    share = float((err / allow.clamp_min(1e-300))[err > 0].max()) if torch.any(err > 0) else 0.0
    print(f"{label}: patch rows of d_sigma reach {share:.3g} of their allowance")
    assert torch.all(err <= allow), share
    # (e) no colour gradient on a patch row: w * 0
    assert torch.all(got["d_rgb"][Rs:] == 0)
    # (f) a density the ReLU rejects passes nothing, on every row
    eff = sig.reshape(R, S) + (noise.reshape(R, S) * std if noise is not None else 0.0)
    assert (eff <= 0).any() and torch.all(got["d_sigma"].cpu()[eff <= 0] == 0)
    # rows 0 and 2 of a patch ray are 0; DS_p is the definition on the reported depths
    assert torch.all(got["terms"][0, Rs:] == 0) and torch.all(got["terms"][2, Rs:] == 0)
    ds_ref = stencil_gd(got["patch_depth"].cpu().double(), lam)[1]
    assert torch.all((got["patch_terms"].cpu().double() - ds_ref).abs() <= 1e-5 * ds_ref + 1e-12)
    return share


def inputs(P, S, n_p, opaque, seed, terms, n_sup=RS):
    R = n_sup + n_p * P * P
    rgb, sig, z, d = case(R, S, seed, opaque, equal=S > 2)        # (at S = 2 the equal pair would leave no patch ray a gradient)
    tgt = torch.from_numpy(O.uniform01(seed + 10, n_sup * 3).reshape(n_sup, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(seed + 11, n_sup) * 4 + 2).float() if terms is ALL else None
    noise = normals(seed + 12, R * S).reshape(R, S, 1) if terms is ALL else None
    return rgb, sig, z, d, tgt, tdepth, noise


# ---------------------------------------------------------------------------------------------
# 1. the raw entry against float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["off", "all"])
@pytest.mark.parametrize("opaque", [False, True])
@pytest.mark.parametrize("S", [2, 16, 65, 130])
@pytest.mark.parametrize("P", [2, 3, 8, 16])
def test_entry_matches_float64(L, P, S, opaque, terms):
    t = ALL if terms == "all" else OFF
    rgb, sig, z, d, tgt, tdepth, noise = inputs(P, S, NP, opaque, 500 + 7 * S + P, t)
    reg = L.ray_reg(t["dw"], KAPPA if t["dw"] > 0 else 0.0, t["ow"], t["k"])
    got = run_patch(L, rgb, sig, z, d, tgt, P, NP, LAM, t["white"], t["w"], tdepth, t["std"], noise, reg)
    ref = oracle(rgb, sig, z, d, tgt, P, NP, LAM, t["white"], t["w"], tdepth, t["std"], noise, t["dw"], t["ow"], t["k"], got["patch_depth"].cpu())
    check_patch_case(got, ref, sig, noise, t["std"], P, NP, LAM, S, f"P={P} S={S} opaque={opaque} terms={terms}")
    assert got["losses"][6].item() > 0


# ---------------------------------------------------------------------------------------------
# 2. constant patches
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S", [(2, 16), (3, 65), (8, 130), (16, 16)])
def test_constant_patches_have_no_term_and_no_gradient(L, P, S):
    rgb, sig, z, d, tgt, _, _ = inputs(P, S, NP, True, 600 + P, OFF)
    for p in range(NP):             # the rays of a patch are copies of one ray
        sl = slice(RS + p * P * P, RS + (p + 1) * P * P)
        rgb[sl], sig[sl], z[sl], d[sl] = rgb[sl][:1].clone(), sig[sl][:1].clone(), z[sl][:1].clone(), d[sl][:1].clone()
    got = run_patch(L, rgb, sig, z, d, tgt, P, NP, LAM)
    assert torch.all(got["patch_terms"] == 0) and got["losses"][6].item() == 0
    assert torch.all(got["d_sigma"][RS:] == 0) and torch.all(got["d_rgb"][RS:] == 0)
    assert torch.any(got["d_sigma"][:RS] != 0) and torch.all(got["patch_depth"] > 0)


# ---------------------------------------------------------------------------------------------
# 3. n_patches = 0: the parent's bits
# ---------------------------------------------------------------------------------------------
def skip_map_with_a_patch_ray(R, S, seed, n_sup):
    """(R,S) bool, True = evaluated: about 40 % of the samples skipped, ray 1 whole, the front of ray 2, and one patch ray whole."""
    keep = torch.from_numpy(O.uniform01(seed, R * S).reshape(R, S)) >= 0.4
    keep[1] = False
    keep[2, : min(3, S - 1)] = False
    keep[n_sup + 2] = False
    return keep


@pytest.mark.parametrize("R,S,opaque,white", [(37, 16, False, False), (9, 65, True, True), (7, 130, True, False)])
def test_no_patches_are_the_parents_bits(L, R, S, opaque, white):
    rgb, sig, z, d = case(R, S, 61, opaque)
    tgt = torch.from_numpy(O.uniform01(62, R * 3).reshape(R, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(63, R) * 4 + 2).float()
    noise = normals(64, R * S).reshape(R, S, 1)
    w, std = (0.7, 0.3, 0.5), 0.4
    reg = L.ray_reg(0.6, KAPPA, 0.8, 5)
    keys = ("pred", "d_rgb", "d_sigma", "terms", "zero")
    old = run_reg(L, rgb, sig, z, d, tgt, white, w, tdepth, std, noise, reg, zero_n=1000)
    new = run_patch(L, rgb, sig, z, d, tgt, 8, 0, LAM, white, w, tdepth, std, noise, reg, zero_n=1000)
    for key in keys:
        assert torch.equal(new[key], old[key]), key
    assert torch.all(new["zero"] == 0) and new["losses"][6].item() == 0
    # the seven values are the parent's six (formed by another kernel: the bar of check_against, not bits)
    assert torch.allclose(new["losses"][:6].cpu(), old["losses"].cpu(), rtol=2e-4, atol=1e-12)
    keep = skip_map_with_a_patch_ray(R, S, 65, 3)
    rc, sc, slot = compacted(rgb, sig, keep)
    old = run_reg(L, rc, sc, z, d, tgt, white, w, tdepth, std, noise, reg, slot=slot, zero_n=1000)
    new = run_patch(L, rc, sc, z, d, tgt, 8, 0, LAM, white, w, tdepth, std, noise, reg, slot=slot, zero_n=1000)
    for key in keys:
        assert torch.equal(new[key], old[key]), key


# ---------------------------------------------------------------------------------------------
# 4. indexed against dense, and two runs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S", [(2, 16), (3, 65), (8, 130), (16, 16)])
def test_indexed_entry_is_the_dense_entry_on_masked_rows_and_runs_repeat(L, P, S):
    t = ALL
    rgb, sig, z, d, tgt, tdepth, noise = inputs(P, S, NP, True, 700 + P, t)
    R = RS + NP * P * P
    keep = skip_map_with_a_patch_ray(R, S, 85, RS)
    rc, sc, slot = compacted(rgb, sig, keep)
    reg = L.ray_reg(t["dw"], KAPPA, t["ow"], t["k"])
    args = (P, NP, LAM, True, t["w"], tdepth, t["std"], noise, reg)
    idx = run_patch(L, rc, sc, z, d, tgt, *args, slot=slot)
    rgb_m = torch.where(keep[..., None], rgb, torch.zeros_like(rgb))
    sig_m = torch.where(keep[..., None], sig, torch.full_like(sig, float("-inf")))
    dense = run_patch(L, rgb_m, sig_m, z, d, tgt, *args)
    for key in ("pred", "terms", "losses", "patch_terms", "patch_depth"):
        assert torch.equal(idx[key], dense[key]) and torch.isfinite(idx[key]).all(), key
    flat = keep.reshape(-1).cuda()
    assert torch.equal(idx["d_rgb"], dense["d_rgb"].reshape(-1, 3)[flat]) and torch.equal(idx["d_sigma"], dense["d_sigma"].reshape(-1)[flat])
    assert torch.all(dense["d_sigma"].reshape(-1)[~flat] == 0)
    assert idx["patch_depth"].reshape(-1)[2].item() == 0 and torch.any(idx["d_sigma"] != 0)        # the patch ray that keeps no sample
    for again, first in ((run_patch(L, rc, sc, z, d, tgt, *args, slot=slot), idx), (run_patch(L, rgb_m, sig_m, z, d, tgt, *args), dense)):
        for key in ("pred", "d_rgb", "d_sigma", "terms", "losses", "patch_terms", "patch_depth"):
            assert torch.equal(again[key], first[key]), key


# ---------------------------------------------------------------------------------------------
# 5. more patches than the grid holds workgroups
# ---------------------------------------------------------------------------------------------
def test_more_patches_than_the_grid_cap(L):
    """cap + 1 patches of 2 x 2 rays at S = 2, with the other terms on (test 1's "all" set).  With them off a patch ray's one nonzero
    entry of d_sigma is gd (z_0 - z_1) T_0 dist e: fp32 forms gd z_0 and gd z_1 apart, and among 65 540 rays with random depth pairs
    some hundred lie within 1e-3 of each other, where that difference alone exceeds 1e-4 of the entry -- the ray's only one, so its
    own scale.  That is the conditioning of the inputs at this count, not the grid-stride walk this test is about."""
    src = open(os.path.join(ROOT, "nerf_few_shot_limitations_amd", "csrc", "patch_reg.hip")).read()
    body = src[src.index("int launch_composite_patch_loss_backward("):src.index("int launch_patch_terms_finish(")]
    caps = re.findall(r"grid_for\(work, kBlock, (\d+)\)", body)
    assert caps == ["16384"], caps
    assert "pt.n_patches * kBlock" in body                        # a workgroup per patch until the cap
    cap, P, S = int(caps[0]), 2, 2
    n_p = cap + 1
    t = ALL
    rgb, sig, z, d, tgt, tdepth, noise = inputs(P, S, n_p, False, 800, t)
    reg = L.ray_reg(t["dw"], KAPPA, t["ow"], t["k"])
    got = run_patch(L, rgb, sig, z, d, tgt, P, n_p, LAM, t["white"], t["w"], tdepth, t["std"], noise, reg)
    ref = oracle(rgb, sig, z, d, tgt, P, n_p, LAM, t["white"], t["w"], tdepth, t["std"], noise, t["dw"], t["ow"], t["k"], got["patch_depth"].cpu())
    check_patch_case(got, ref, sig, noise, t["std"], P, n_p, LAM, S, f"{n_p} patches")
    assert torch.any(got["d_sigma"][-P * P:] != 0) and got["patch_terms"][-1].item() > 0 and torch.any(got["terms"][1, -P * P:] > 0)


# ---------------------------------------------------------------------------------------------
# 6. FusedStep
# ---------------------------------------------------------------------------------------------
NEAR, FAR = 2.0, 6.0
PS, NPS = 4, 3                    # patch size and patches of the step tests
STEP = dict(reg_weight=1e-3, dist_weight=0.05, depth_smooth_weight=0.5)


def step_scene(R_s, S):
    """R_s supervised rays and NPS patches of PS x PS rays from sampled poses; depths in [near, far]."""
    from nerf_few_shot_limitations_amd.ray_sampler import patch_rays, sample_patch_poses
    from tests.test_gpu_train_rays import ray_batch, u01
    o, d = ray_batch(R_s, seed=290)
    poses = sample_patch_poses(_train_poses(), NPS, generator=torch.Generator().manual_seed(4))
    o_p, d_p = patch_rays(40, 40, 30.0, poses.cuda(), PS, generator=torch.Generator().manual_seed(5), stride=3)
    R = R_s + NPS * PS * PS
    z = torch.sort(u01(291, R, S) * (FAR - NEAR) + NEAR, dim=-1).values.cuda()
    return dict(o=torch.cat([o, o_p]).contiguous(), d=torch.cat([d, d_p]).contiguous(), tgt=u01(292, R_s, 3).cuda(), z=z, R=R)


def torch_loss(pred, depth, w, z, tgt, R_s):
    smooth = smooth_of(depth[R_s:].reshape(NPS, PS, PS))
    dist = distortion(w, z, 1.0 / (FAR - NEAR)).mean()
    return (torch.nn.functional.mse_loss(pred[:R_s], tgt) + STEP["reg_weight"] * torch.mean(w ** 2) + STEP["dist_weight"] * dist
            + STEP["depth_smooth_weight"] * smooth), smooth


def compare(mode, ref, got):
    """The tolerances of tests/test_gpu_ray_reg.py's compare: the losses, and the unweighted new term."""
    (ref_losses, ref_parts), (losses, parts) = ref, got
    print(mode, "losses", ref_losses, losses, "smooth", ref_parts, parts)
    tol = 1e-5 if mode == "f32" else 2e-3
    assert np.allclose(ref_losses, losses, rtol=tol, atol=1e-7), (ref_losses, losses)
    assert np.allclose(np.asarray(ref_parts), np.asarray(parts), rtol=max(2e-4, tol), atol=1e-7), (ref_parts, parts)
    assert min(ref_parts) > 0


def fused_loop(step, steps, call):
    losses, parts = [], []
    for _ in range(steps):
        losses.append(call().item())
        ll = step.last_losses
        assert list(ll) == ["total", "rgb", "depth", "reg", "dist", "occ", "smooth"]
        parts.append(ll["smooth"].item())
        want = ll["rgb"].item() + STEP["reg_weight"] * ll["reg"].item() + STEP["dist_weight"] * ll["dist"].item() + STEP["depth_smooth_weight"] * parts[-1]
        assert abs(ll["total"].item() - want) < 1e-6 and ll["total"].item() == losses[-1]
        assert step.last_patch_depth.shape == (NPS, PS, PS)
    return losses, parts


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v1", "bf16"), ("v2", "f32"), ("v2", "bf16")])
def test_fused_step_called_with_patches_equals_autograd_route(N, net, mode):
    from nerf_few_shot_limitations_amd.training import Adam, FusedStep
    R_s, S, steps = 40, 16, 3
    sc = step_scene(R_s, S)
    R, z, rd = sc["R"], sc["z"], sc["d"]
    pos = (sc["o"][:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    pts = N.PositionalEncoding(10)(pos) if net == "v1" else pos
    a, b = models(N, net, mode)
    opt, vr = Adam(a, lr=5e-4), N.VolumeRenderer()
    ref = ([], [])
    for _ in range(steps):
        opt.zero_grad()
        if net == "v1":
            o4 = a(pts).view(R, S, 4)
            c, sg = o4[..., :3], o4[..., 3:4]
        else:
            c, sg = a(pts, dirs, None)
            c, sg = c.view(R, S, 3), sg.view(R, S, 1)
        pred, depth, w = vr(c, sg, z, rd)
        loss, smooth = torch_loss(pred, depth, w, z, sc["tgt"], R_s)
        loss.backward()
        opt.step()
        ref[0].append(loss.item()); ref[1].append(smooth.item())
    step = FusedStep(b, lr=5e-4, dist_span=FAR - NEAR, patch_size=PS, **STEP)
    got = fused_loop(step, steps, lambda: step(pts, z, rd, sc["tgt"], dirs=dirs if net != "v1" else None, n_patches=NPS))
    compare(mode, ref, got)
    with pytest.raises(ValueError):
        step(pts, z, rd, sc["tgt"], dirs=dirs if net != "v1" else None, n_patches=NPS + 3)
    with pytest.raises(ValueError):
        FusedStep(b, lr=5e-4)(pts, z, rd, sc["tgt"], dirs=dirs if net != "v1" else None, n_patches=NPS)


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v2", "f32"), ("v2", "bf16")])
def test_step_rays_with_patches_with_and_without_a_grid(N, net, mode):
    """step_rays with patches (a) against render_rays_train -> the loss in torch -> backward -> training.Adam; (b) its first
    last_patch_depth against the depths of a plain render of the patch rays on the same z; (c) under an all-ones grid, both
    grid_inputs: the dense step's bits -- all but V1 on "staged", whose compacted points are encoded by nrf_encode, not by the ray
    route's in-kernel encoder, and which is held to (a)'s tolerances."""
    from nerf_few_shot_limitations_amd.training import Adam, FusedStep, render_rays_train
    from tests.test_gpu_train_occupancy import grid_of
    R_s, S, steps = 40, 16, 3
    sc = step_scene(R_s, S)
    a, _ = models(N, net, mode)
    opt = Adam(a, lr=5e-4)
    ref, first_depth = ([], []), None
    for _ in range(steps):
        opt.zero_grad()
        with torch.enable_grad():
            out = render_rays_train(a, sc["o"], sc["d"], NEAR, FAR, S, perturb=False, z_in=sc["z"])
            loss, smooth = torch_loss(out["rgb"], out["depth"], out["weights"], sc["z"], sc["tgt"], R_s)
        if first_depth is None:
            first_depth = out["depth"][R_s:].detach().reshape(NPS, PS, PS).clone()
        loss.backward()
        opt.step()
        ref[0].append(loss.item()); ref[1].append(smooth.item())

    def fused(**more):
        _, b = models(N, net, mode)
        step = FusedStep(b, lr=5e-4, patch_size=PS, **STEP)               # dist_span=None: far - near
        depths = []

        def call():
            loss = step.step_rays(sc["o"], sc["d"], sc["tgt"], NEAR, FAR, S, perturb=False, z_in=sc["z"], n_patches=NPS, **more)
            depths.append(step.last_patch_depth.clone())
            return loss
        return fused_loop(step, steps, call), depths, b

    plain, depths, b = fused()
    compare(mode, ref, plain)
    assert torch.all((depths[0] - first_depth).abs() <= 1e-5 * first_depth.abs().clamp_min(1.0)) and torch.any(first_depth > 0)
    ones = grid_of("ones", box=(-12.0, 12.0))
    for route in ("staged", "rays"):
        got, dep, g = fused(occupancy=ones, grid_inputs=route)
        if net == "v2" or route == "rays":          # (V1 "staged" encodes the compacted points in nrf_encode: another kernel, other bits)
            assert got == plain, route
            assert all(torch.equal(x, y) for x, y in zip(dep, depths)), route
            assert torch.equal(g.flat_params().flat, b.flat_params().flat), route
        else:
            compare(mode, ref, got)


@pytest.mark.parametrize("route", ["call", "rays", "grid-staged", "grid-rays"])
def test_a_patch_step_launches_what_a_regularised_step_launches(N, route, monkeypatch):
    from nerf_few_shot_limitations_amd.training import FusedStep
    from tests.test_gpu_train_occupancy import grid_of
    from tests.test_gpu_training import make_v2
    R_s, S = 8, 5
    sc = step_scene(R_s, S)
    R = sc["R"]
    grid = grid_of("random", outside=1, seed=195, box=(-6.0, 6.0))
    tgt_all = torch.cat([sc["tgt"], sc["tgt"][:1].expand(R - R_s, 3)]).contiguous()

    def names(n_patches, **kw):
        model = make_v2(N, "bf16", scene="solid", n_layers=2)[0]
        step = FusedStep(model, lr=1e-3, reg_weight=1e-4, dist_span=FAR - NEAR, **kw)
        tgt = sc["tgt"] if n_patches else tgt_all
        pk = dict(n_patches=n_patches) if n_patches else {}
        if route == "call":
            pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3)
            dirs = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
            return record(lambda: step(pts, sc["z"], sc["d"], tgt, dirs=dirs, **pk), monkeypatch)
        more = {} if route == "rays" else dict(occupancy=grid, grid_inputs=route.split("-")[1])
        return record(lambda: step.step_rays(sc["o"], sc["d"], tgt, NEAR, FAR, S, perturb=True, seed=3, **pk, **more), monkeypatch)

    base = names(0, dist_weight=1e-2)
    got = names(NPS, dist_weight=1e-2, depth_smooth_weight=0.5, patch_size=PS)
    assert base.count("nrf_composite_reg_loss_backward") == 1 and base.count("nrf_ray_terms_finish") == 1
    swap = {"nrf_composite_reg_loss_backward": "nrf_composite_patch_loss_backward", "nrf_ray_terms_finish": "nrf_patch_terms_finish"}
    print(route, got)
    assert got == [swap.get(n, n) for n in base] and len(got) == len(base)
    # with the weight 0 nothing changes, launch for launch
    assert names(0, dist_weight=1e-2, depth_smooth_weight=0.0, patch_size=PS) == base


# ---------------------------------------------------------------------------------------------
# 7. patch_rays against get_rays
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,P,stride", [(20, 30, 8, 1), (33, 17, 4, 3), (16, 16, 16, 1)])
def test_patch_rays_are_get_rays_gathered_at_patch_pixels(N, H, W, P, stride):
    from nerf_few_shot_limitations_amd.ray_sampler import get_rays, patch_pixels, patch_rays, sample_patch_poses
    n, focal = 4, 27.5
    poses = sample_patch_poses(_train_poses(), n, generator=torch.Generator().manual_seed(21))
    o, d = patch_rays(H, W, focal, poses.cuda(), P, generator=torch.Generator().manual_seed(22), stride=stride)
    ids = patch_pixels(H, W, P, n, generator=torch.Generator().manual_seed(22), stride=stride).reshape(n, P * P).cuda()
    assert o.is_cuda and o.shape == d.shape == (n * P * P, 3)
    for p in range(n):
        ro, rd = get_rays(H, W, focal, poses[p])
        sl = slice(p * P * P, (p + 1) * P * P)
        assert (o[sl] - ro.reshape(-1, 3)[ids[p]]).abs().max() <= 1e-6 and (d[sl] - rd.reshape(-1, 3)[ids[p]]).abs().max() <= 1e-6


# ---------------------------------------------------------------------------------------------
# 8. the trainer's staged route with patches
# ---------------------------------------------------------------------------------------------
def test_train_epoch_feeds_patches_behind_every_batch(N, tmp_path):
    """train_cli.train_epoch(patches=) on three views of the generated scene: every batch is one step with n_patches; the draws
    repeat from the generator's seed; the combinations it cannot serve are refused."""
    import importlib.util
    from nerf_few_shot_limitations_amd import train_cli
    from nerf_few_shot_limitations_amd.training import FusedStep
    from tests.test_gpu_training import make_v2
    spec = importlib.util.spec_from_file_location("synthetic_scene", os.path.join(ROOT, "tools", "synthetic_scene.py"))
    scene_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scene_mod)
    scene = str(tmp_path / "scene")
    scene_mod.write_scene(scene, size=32, n_train=3, n_test=1)
    images, poses, (H, W, focal) = N.load_blender_data(scene, "train", img_size=32)
    images = [im.permute(1, 2, 0).float().cuda() for im in images]
    poses = [p.float() for p in poses]
    cfg = dict(training=dict(batch_size=256, progressive_schedule=dict(epochs_0_50=[16, 16, 8], epochs_50_100=[32, 32, 8], epochs_100_plus=[32, 32, 8])))

    class Counting(FusedStep):
        def __call__(self, *a, **k):
            self.seen.append((int(a[1].shape[0]), k.get("n_patches", 0)))          # (rays of the batch, its patches)
            return super().__call__(*a, **k)

    def run(seed, **kw):
        step = Counting(make_v2(N, "bf16", scene="solid", n_layers=2)[0], lr=5e-4, depth_smooth_weight=0.5, patch_size=4)
        step.seen = []
        gen = torch.Generator(device="cuda").manual_seed(0)
        patches = dict(n=3, stride=2, generator=torch.Generator().manual_seed(seed))
        loss, samples = train_cli.train_epoch(step, cfg, 0, images, poses, H, W, focal, 2.0, 6.0, gen, max_batches=3, patches=patches, **kw)
        return loss, samples, step.seen, step

    loss, samples, calls, step = run(1)
    # epoch 0: 16 x 16 rays per view in one batch, 8 samples; behind them 3 patches of 4 x 4 rays
    assert calls == [(256 + 48, 3)] * 3 and samples == 3 * (256 + 48) * 8 and np.isfinite(loss) and step.opt.step_count == 3
    ll = step.last_losses
    assert list(ll) == ["total", "rgb", "depth", "reg", "dist", "occ", "smooth"] and all(np.isfinite(v.item()) for v in ll.values())
    assert step.last_patch_depth.shape == (3, 4, 4)
    again = run(1)
    assert again[0] == loss and torch.equal(again[3].last_patch_depth, step.last_patch_depth)
    assert run(2)[0] != loss                                    # other poses and windows
    for kw in (dict(fused_inputs=True), dict(n_importance=4), dict(draws=object())):
        with pytest.raises(ValueError, match="patches"):
            run(1, **kw)
