"""InfoNeRF's ray-entropy and patch-KL terms of the fused training step on the GPU (nerfhip.h: nrf_composite_info_loss_backward,
nrf_info_terms_finish; FusedStep(ent_weight=, ent_threshold=, kl_weight=)).

The oracle is float64 autograd of the definitions in tests/test_info_reg_host.py, on the CPU.  A run with every other weight 0
leaves the two terms alone in d_sigma; there each entry is held to

    |err_j| <= 1e-4 max_ray |ref| + c 2^-23 ln(1/eps) scale dist_j e_j / (A + eps)

with c the kernel's own count of fp32 roundings (tests/test_info_reg_host.py: allowance, where the count is written out).  A run
with every other term on holds the supervised rows and the loss values to tests/test_gpu_multiscale_step.py's check_against.

The values m_r H_r, K_p and the two loss values are held to 2e-4 relative plus what fp32 cannot resolve: where a ray's distribution
is one p = 1 (S = 2, or one positive sample) its entropy is ln(1 + 1e-10) -- p + eps rounds to 1 -- so each logarithm carries an
absolute 2^-22."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_multiscale_step import check_against, normals
from tests.test_gpu_patch_reg import ALL, LAM, NP, RS, inputs, run_patch, skip_map_with_a_patch_ray, smooth_of, step_scene, target_free, NPS, PS
from tests.test_gpu_ray_reg import KAPPA, OPTS, WD, compacted, compare, models, record
from tests.test_info_reg_host import check_terms_alone, closed_form, distribution, info_loss, middle_threshold
from tests.test_ray_reg_host import case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EW, KW = 0.7, 1.3                 # ent_weight and kl_weight of the raw-entry cases
LOG_FLOOR = 2.0 ** -22            # what one fp32 logarithm next to 1 cannot resolve (module docstring)
NONE = dict(w=(0.0, 0.0, 0.0), std=0.0, dw=0.0, ow=0.0, k=0, white=False)          # every other weight 0, rgb_weight included


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


def run_info(L, rgb, sig, z, d, tgt, P, n_p, info, lam=0.0, white=False, w=(1.0, 0.0, 0.0), tdepth=None, noise_std=0.0, noise=None, reg=None, slot=None,
             zero_n=0, with_losses=True, expect=0):
    """nrf_composite_info_loss_backward [+ nrf_info_terms_finish] -> dict of device tensors, as tests/test_gpu_patch_reg.py's run_patch;
    info = (ent_weight, ent_threshold, kl_weight).  expect: the return code the launch entry must give (the finish is skipped on a
    refusal)."""
    lib, st = L.lib(), L.stream_ptr()
    R, S = z.shape
    c, s_ = rgb.reshape(-1, 3).contiguous().cuda(), sig.reshape(-1).contiguous().cuda()
    rows = c.shape[0]
    zc, dc, tc = z.contiguous().cuda(), d.contiguous().cuda(), tgt.contiguous().cuda()
    td = None if tdepth is None else tdepth.contiguous().cuda()
    nz = None if noise is None else noise.reshape(R, S).contiguous().cuda()
    sl = None if slot is None else slot.reshape(R, S).to(torch.int32).contiguous().cuda()
    nan = float("nan")
    out = dict(pred=torch.full((R, 3), nan, device="cuda"), d_rgb=torch.full((rows, 3), nan, device="cuda"), d_sigma=torch.full((rows,), nan, device="cuda"),
               terms=torch.full((5, R), nan, device="cuda"), zero=torch.ones(max(zero_n, 1), device="cuda"),
               patch_terms=torch.full((max(n_p, 1),), nan, device="cuda"), patch_depth=torch.full((max(n_p, 1) * P * P,), nan, device="cuda"),
               info_terms=torch.full((R,), nan, device="cuda"), patch_kl=torch.full((max(n_p, 1),), nan, device="cuda"))
    lo = L.loss_opts(w[0], w[2], w[1], L.ptr(td), noise_std, L.ptr(nz), 0)
    reg = reg if reg is not None else L.ray_reg()
    patch, inf = L.patch_reg(lam, P, n_p), L.info_reg(*info)
    code = lib.nrf_composite_info_loss_backward(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, int(white), L.ptr(tc), C.byref(lo), C.byref(reg),
                                                None if sl is None else sl.data_ptr(), L.ptr(out["pred"]), L.ptr(out["d_rgb"]), 3, L.ptr(out["d_sigma"]), 1,
                                                L.ptr(out["terms"]), L.ptr(out["zero"]) if zero_n else None, zero_n, st, C.byref(patch),
                                                L.ptr(out["patch_terms"]), L.ptr(out["patch_depth"]), C.byref(inf), L.ptr(out["info_terms"]),
                                                L.ptr(out["patch_kl"]))
    assert code == expect, (code, L.lib().nrf_last_error())
    if with_losses and code == 0:
        out["losses"] = torch.full((9,), nan, device="cuda")
        L.check(lib.nrf_info_terms_finish(L.ptr(out["terms"]), R, S, C.byref(lo), C.byref(reg), C.byref(patch), L.ptr(out["patch_terms"]), C.byref(inf),
                                          L.ptr(out["info_terms"]), L.ptr(out["patch_kl"]), L.ptr(out["losses"]), st))
    torch.cuda.synchronize()
    if code != 0:
        return out
    out["patch_terms"], out["patch_kl"] = out["patch_terms"][:n_p], out["patch_kl"][:n_p]
    out["patch_depth"] = out["patch_depth"][: n_p * P * P].reshape(n_p, P, P)
    if slot is None:
        out["d_rgb"], out["d_sigma"] = out["d_rgb"].reshape(R, S, 3), out["d_sigma"].reshape(R, S)
    return out


def oracle_all(rgb, sig, z, d, tgt, P, n_p, lam, t, tdepth, noise, tau, ew=EW, kw=KW):
    """float64 autograd of the total loss of the batch layout with every term on; the nine loss values, m H and K_p."""
    f = torch.float64
    R, S = z.shape
    Rs = R - n_p * P * P
    z64, d64 = z.to(f), d.to(f)
    r1, s1 = rgb.to(f).requires_grad_(True), sig.to(f).reshape(R, S, 1).requires_grad_(True)
    dens = s1 if noise is None else s1 + noise.to(f).reshape(s1.shape) * t["std"]
    o_rgb, o_dep, o_w = O.volume_render(r1, dens, z64, d64, white_bkgd=t["white"])
    w = t["w"]
    l_rgb = torch.nn.functional.mse_loss(o_rgb[:Rs], tgt.to(f))
    l_dep = torch.nn.functional.l1_loss(o_dep[:Rs], tdepth.to(f)) if tdepth is not None else torch.zeros((), dtype=f)
    free, l_reg, l_dist, l_occ = target_free(o_w, dens, z64, w, t["dw"], t["ow"], t["k"])
    l_smooth = smooth_of(o_dep[Rs:].reshape(n_p, P, P))
    l_info, l_ent, l_kl, mH, K, _ = info_loss(dens[..., 0], z64, d64, tau, P, n_p, ew, kw)
    total = w[0] * l_rgb + w[1] * l_dep + free + lam * l_smooth + l_info
    total.backward()
    return dict(pred=o_rgb.detach().float(), d_rgb=r1.grad, d_sigma=s1.grad[..., 0], mH=mH.detach(), K=K.detach(),
                losses=torch.stack([total, l_rgb, l_dep, l_reg, l_dist, l_occ, l_smooth, l_ent, l_kl]).detach())


def check_values(got, mH, K, l_ent, l_kl, P, label):
    """m_r H_r, K_p and the two loss values: 2e-4 relative plus the logarithms' floor (module docstring)."""
    it, pk = got["info_terms"].cpu().double(), got["patch_kl"].cpu().double()
    e1, e2 = (it - mH).abs(), (pk - K).abs()
    anchors = 2 * (P - 1) ** 2
    print(f"{label}: info_terms err {float(e1.max()):.3g} (largest {float(mH.abs().max()):.3g}); patch_kl err {float(e2.max()) if len(e2) else 0:.3g} "
          f"(largest {float(K.abs().max()) if len(K) else 0:.3g})")
    assert torch.all(e1 <= 2e-4 * mH.abs() + LOG_FLOOR) and torch.all(e2 <= 2e-4 * K.abs() + anchors * LOG_FLOOR)
    assert torch.all(it[mH == 0] == 0), "a masked ray's entropy is exactly 0"
    le, lk = got["losses"][7].item(), got["losses"][8].item()
    assert abs(le - float(l_ent)) <= 2e-4 * abs(float(l_ent)) + LOG_FLOOR and abs(lk - float(l_kl)) <= 2e-4 * abs(float(l_kl)) + 2 * LOG_FLOOR


# ---------------------------------------------------------------------------------------------
# 1. the raw entry against float64
# ---------------------------------------------------------------------------------------------
SHAPES = [(P, S) for P in (2, 3, 8) for S in (2, 3, 16, 65, 66, 130)] + [(16, 48)]          # (16, 48): P^2 S at the LDS cap


@pytest.mark.parametrize("opaque", [False, True])
@pytest.mark.parametrize("P,S", SHAPES)
def test_entry_matches_float64(L, P, S, opaque):
    R = RS + NP * P * P
    seed = 900 + 7 * S + P
    rgb, sig, z, d = case(R, S, seed, opaque, equal=S > 3)
    tgt = torch.from_numpy(O.uniform01(seed + 10, RS * 3).reshape(RS, 3)).float()
    label = f"P={P} S={S} opaque={opaque}"
    # (a) the terms alone: every other weight 0, so d_sigma holds the two terms and nothing else
    dens = sig[..., 0]
    tau = middle_threshold(distribution(dens.double(), z.double(), d.double())[1])
    got = run_info(L, rgb, sig, z, d, tgt, P, NP, (EW, tau, KW), w=NONE["w"])
    ref, mH, K, A = closed_form(dens, z, d, tau, P, NP, EW, KW)
    s64 = dens.double().requires_grad_(True)
    total, l_ent, l_kl, mH_a, K_a, _ = info_loss(s64, z.double(), d.double(), tau, P, NP, EW, KW)
    total.backward()
    # the closed form is the autograd of the definitions (at S = 2 both are the eps terms' cancellation noise: held absolutely)
    assert torch.all((ref - s64.grad).abs() <= 1e-9 * s64.grad.abs().amax(dim=1, keepdim=True).clamp_min(1e-5))
    ds = got["d_sigma"].cpu()
    assert torch.isfinite(ds).all() and torch.all(got["d_rgb"] == 0), "nothing reaches rgb"
    share = check_terms_alone(ds, dens, z, d, tau, P, NP, EW, KW, ref, label + " terms alone")
    masked = A <= tau
    assert masked.any() and (~masked).any() and (S == 2 or torch.any(ds != 0))
    check_values(got, mH_a.detach(), K_a.detach(), l_ent.detach(), l_kl.detach(), P, label + " terms alone")
    assert abs(got["losses"][0].item() - (EW * got["losses"][7].item() + KW * got["losses"][8].item())) < 1e-5          # the total is the two terms'
    # (b) all on: the supervised rows and the loss values through check_against
    t = ALL
    tdepth = torch.from_numpy(O.uniform01(seed + 11, RS) * 4 + 2).float()
    noise = normals(seed + 12, R * S).reshape(R, S, 1)
    dens_n = (sig.double() + noise.double() * t["std"])[..., 0]
    tau_n = middle_threshold(distribution(dens_n, z.double(), d.double())[1])
    reg = L.ray_reg(t["dw"], KAPPA, t["ow"], t["k"])
    got = run_info(L, rgb, sig, z, d, tgt, P, NP, (EW, tau_n, KW), LAM, t["white"], t["w"], tdepth, t["std"], noise, reg)
    ref_all = oracle_all(rgb, sig, z, d, tgt, P, NP, LAM, t, tdepth, noise, tau_n)
    sup = dict(pred=got["pred"][:RS], losses=got["losses"][:7], d_rgb=got["d_rgb"][:RS], d_sigma=got["d_sigma"][:RS])
    check_against(sup, dict(pred=ref_all["pred"][:RS], losses=ref_all["losses"][:7], d_rgb=ref_all["d_rgb"][:RS], d_sigma=ref_all["d_sigma"][:RS]), 1e-4)
    check_values(got, ref_all["mH"], ref_all["K"], ref_all["losses"][7], ref_all["losses"][8], P, label + " all on")
    assert torch.isfinite(got["d_sigma"]).all() and torch.all(got["d_rgb"][RS:] == 0)
    assert share <= 1.0


# ---------------------------------------------------------------------------------------------
# 2. both weights 0: the parent's bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_p", [0, 3])
@pytest.mark.parametrize("S,opaque,white", [(16, False, False), (65, True, True), (130, True, False)])
def test_weights_off_are_the_parents_bits(L, n_p, S, opaque, white):
    P = 3
    R = RS + 3 * P * P                                        # the same rays with and without patches behind them
    n_sup = R - n_p * P * P
    rgb, sig, z, d = case(R, S, 61, opaque)
    tgt = torch.from_numpy(O.uniform01(62, n_sup * 3).reshape(n_sup, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(63, n_sup) * 4 + 2).float()
    noise = normals(64, R * S).reshape(R, S, 1)
    w, std = (0.7, 0.3, 0.5), 0.4
    reg = L.ray_reg(0.6, KAPPA, 0.8, 5)
    keys = ("pred", "d_rgb", "d_sigma", "terms", "zero", "patch_terms", "patch_depth")
    keep = skip_map_with_a_patch_ray(R, S, 65, RS)
    rc, sc, slot = compacted(rgb, sig, keep)
    for args, kw in (((rgb, sig), {}), ((rc, sc), dict(slot=slot))):
        old = run_patch(L, *args, z, d, tgt, P, n_p, LAM, white, w, tdepth, std, noise, reg, zero_n=1000, **kw)
        new = run_info(L, *args, z, d, tgt, P, n_p, (0.0, 0.01, 0.0), LAM, white, w, tdepth, std, noise, reg, zero_n=1000, **kw)
        for key in keys:
            assert torch.equal(new[key], old[key]), key
        assert torch.all(new["zero"] == 0) and torch.all(new["info_terms"] == 0) and torch.all(new["patch_kl"] == 0)
        assert torch.allclose(new["losses"][:7], old["losses"], rtol=2e-4, atol=1e-12)          # (formed by another kernel: check_against's bar)
        assert new["losses"][7].item() == 0 and new["losses"][8].item() == 0


# ---------------------------------------------------------------------------------------------
# 3. indexed against dense, and two runs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S", [(2, 16), (3, 65), (8, 130), (16, 48)])
def test_indexed_entry_is_the_dense_entry_on_masked_rows_and_runs_repeat(L, P, S):
    t = ALL
    rgb, sig, z, d, tgt, tdepth, noise = inputs(P, S, NP, True, 700 + P, t)
    R = RS + NP * P * P
    keep = skip_map_with_a_patch_ray(R, S, 85, RS)
    rc, sc, slot = compacted(rgb, sig, keep)
    reg = L.ray_reg(t["dw"], KAPPA, t["ow"], t["k"])
    sig_m = torch.where(keep[..., None], sig, torch.full_like(sig, float("-inf")))
    tau = 0.05                      # (bits against bits: no oracle here whose mask a rounding could flip)
    args = (P, NP, (EW, tau, KW), LAM, True, t["w"], tdepth, t["std"], noise, reg)
    idx = run_info(L, rc, sc, z, d, tgt, *args, slot=slot)
    rgb_m = torch.where(keep[..., None], rgb, torch.zeros_like(rgb))
    dense = run_info(L, rgb_m, sig_m, z, d, tgt, *args)
    for key in ("pred", "terms", "losses", "patch_terms", "patch_depth", "info_terms", "patch_kl"):
        assert torch.equal(idx[key], dense[key]) and torch.isfinite(idx[key]).all(), key
    flat = keep.reshape(-1).cuda()
    assert torch.equal(idx["d_rgb"], dense["d_rgb"].reshape(-1, 3)[flat]) and torch.equal(idx["d_sigma"], dense["d_sigma"].reshape(-1)[flat])
    assert torch.all(dense["d_sigma"].reshape(-1)[~flat] == 0)
    assert idx["info_terms"][RS + 2].item() == 0 and idx["info_terms"].abs().max().item() > 0 and idx["patch_kl"].abs().max().item() > 0
    # and the terms act: the same run without them differs
    plain = run_patch(L, rc, sc, z, d, tgt, P, NP, LAM, True, t["w"], tdepth, t["std"], noise, reg, slot=slot)
    assert not torch.equal(plain["d_sigma"], idx["d_sigma"]) and torch.equal(plain["pred"], idx["pred"])
    for again, first in ((run_info(L, rc, sc, z, d, tgt, *args, slot=slot), idx), (run_info(L, rgb_m, sig_m, z, d, tgt, *args), dense)):
        for key in ("pred", "d_rgb", "d_sigma", "terms", "losses", "patch_terms", "patch_depth", "info_terms", "patch_kl"):
            assert torch.equal(again[key], first[key]), key


# ---------------------------------------------------------------------------------------------
# 4. degenerate rays
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,S", [(2, 16), (3, 66), (8, 130)])
def test_constant_patches_have_no_kl(L, P, S):
    """The rays of a patch are copies of one ray: every KL compares a distribution with itself.  K_p = 0 up to rounding, and what
    the KL term leaves in d_sigma (the eps terms of p / (p + eps)) is nothing beside the entropy's gradient on the same rays."""
    rgb, sig, z, d, tgt, _, _ = inputs(P, S, NP, False, 600 + P, NONE)
    for p in range(NP):
        sl = slice(RS + p * P * P, RS + (p + 1) * P * P)
        rgb[sl], sig[sl], z[sl], d[sl] = rgb[sl][:1].clone(), sig[sl][:1].clone(), z[sl][:1].clone(), d[sl][:1].clone()
    dens = sig[..., 0]
    kl = run_info(L, rgb, sig, z, d, tgt, P, NP, (0.0, 0.0, KW), w=NONE["w"])
    ent = run_info(L, rgb, sig, z, d, tgt, P, NP, (KW, 0.0, 0.0), w=NONE["w"])
    assert torch.all(kl["patch_kl"].abs() <= 2 * (P - 1) ** 2 * LOG_FLOOR) and abs(kl["losses"][8].item()) <= 2 * LOG_FLOOR
    assert torch.all(kl["info_terms"] == 0) and torch.all(kl["d_sigma"][:RS] == 0), "the KL term touches no supervised ray"
    g_kl, g_ent = kl["d_sigma"][RS:].abs().max().item(), ent["d_sigma"][RS:].abs().max().item()
    print(f"P={P} S={S}: largest |d_sigma| of the KL term {g_kl:.3g}, of the entropy at the same weight {g_ent:.3g}")
    assert g_ent > 0 and g_kl <= 1e-3 * g_ent
    ref = closed_form(dens, z, d, 0.0, P, NP, 0.0, KW)[0]
    check_terms_alone(kl["d_sigma"].cpu(), dens, z, d, 0.0, P, NP, 0.0, KW, ref, f"constant patches P={P} S={S}")


@pytest.mark.parametrize("S", [2, 16, 66, 130])
def test_a_ray_with_one_positive_sample_has_no_entropy(L, S):
    P = 2
    rgb, sig, z, d, tgt, _, _ = inputs(P, S, NP, False, 650 + S, NONE)
    sig[:] = -sig.abs() - 0.1
    hot = torch.arange(sig.shape[0]) % (S - 1)                # one positive density per ray, among the S - 1 that take part
    sig[torch.arange(sig.shape[0]), hot, 0] = 1.5
    got = run_info(L, rgb, sig, z, d, tgt, P, NP, (EW, 0.0, 0.0), w=NONE["w"])
    assert torch.all(got["info_terms"].abs() <= LOG_FLOOR) and abs(got["losses"][7].item()) <= LOG_FLOOR
    dens = sig[..., 0]
    ref = closed_form(dens, z, d, 0.0, P, NP, EW, 0.0)[0]
    check_terms_alone(got["d_sigma"].cpu(), dens, z, d, 0.0, P, NP, EW, 0.0, ref, f"one positive sample S={S}")


# ---------------------------------------------------------------------------------------------
# 5. the refusal past the LDS cap, with a GPU present
# ---------------------------------------------------------------------------------------------
def test_one_past_the_lds_cap_is_refused_and_nothing_is_written(L):
    P, S = 16, 49
    assert P * P * (S - 1) == L.INFO_KL_MAX_LDS_FLOATS
    rgb, sig, z, d, tgt, _, _ = inputs(P, S, 1, False, 660, NONE)
    got = run_info(L, rgb, sig, z, d, tgt, P, 1, (EW, 0.01, KW), zero_n=64, expect=-1)
    assert b"NRF_INFO_KL_MAX_LDS_FLOATS" in L.lib().nrf_last_error()
    for key in ("pred", "d_rgb", "d_sigma", "terms", "patch_terms", "patch_depth", "info_terms", "patch_kl"):
        assert torch.isnan(got[key]).all(), key
    assert torch.all(got["zero"] == 1)
    # the entropy alone has no cap
    ok = run_info(L, rgb, sig, z, d, tgt, P, 1, (EW, 0.01, 0.0))
    assert torch.isfinite(ok["d_sigma"]).all() and ok["losses"][7].item() > 0 and ok["losses"][8].item() == 0


# ---------------------------------------------------------------------------------------------
# 6. FusedStep
# ---------------------------------------------------------------------------------------------
NEAR, FAR = 2.0, 6.0
INFO = dict(ent_weight=0.05, ent_threshold=0.05, kl_weight=0.02)


def info_in_torch(dens, z, rd, n_patches=NPS):
    """(L_ent, L_kl) of the autograd route's densities (R,S,1), by the definitions."""
    _, l_ent, l_kl, _, _, _ = info_loss(dens[..., 0], z, rd, INFO["ent_threshold"], PS, n_patches, INFO["ent_weight"], INFO["kl_weight"])
    return l_ent, l_kl


def autograd_steps(N, a, net, steps, pts, dirs, z, rd, tgt, tdepth, noise, R_s):
    """tests/test_gpu_ray_reg.py's reference loop on the batch layout (rgb and depth terms over the R_s supervised rays) with the
    two terms written in torch."""
    R, S = z.shape
    a.flat_params().ensure()
    params = list(a.parameters())
    opt = torch.optim.AdamW(params, lr=5e-4, weight_decay=WD)
    vr = N.VolumeRenderer()
    losses, norms, parts = [], [], []
    for _ in range(steps):
        opt.zero_grad()
        if net == "v1":
            o4 = a(pts).view(R, S, 4)
            c, sg = o4[..., :3], o4[..., 3:4]
        else:
            c, sg = a(pts, dirs, None)
            c, sg = c.view(R, S, 3), sg.view(R, S, 1)
        dens = sg + noise.view(R, S, 1) * OPTS["noise_std"]
        pred, depth, w = vr(c, dens, z, rd)
        l_ent, l_kl = info_in_torch(dens, z, rd)
        loss = (torch.nn.functional.mse_loss(pred[:R_s], tgt) + OPTS["depth_weight"] * torch.nn.functional.l1_loss(depth[:R_s], tdepth)
                + OPTS["reg_weight"] * torch.mean(w ** 2) + INFO["ent_weight"] * l_ent + INFO["kl_weight"] * l_kl)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, OPTS["max_grad_norm"])))
        opt.step()
        losses.append(loss.item())
        parts.append((l_ent.item(), l_kl.item()))
    return losses, norms, parts


def fused_loop(step, steps, call):
    losses, norms, parts = [], [], []
    for _ in range(steps):
        losses.append(call().item())
        norms.append(step.last_grad_norm.item())
        ll = step.last_losses
        assert list(ll) == ["total", "rgb", "depth", "reg", "dist", "occ", "smooth", "entropy", "kl"]
        parts.append((ll["entropy"].item(), ll["kl"].item()))
        want = (ll["rgb"].item() + OPTS["depth_weight"] * ll["depth"].item() + OPTS["reg_weight"] * ll["reg"].item()
                + INFO["ent_weight"] * parts[-1][0] + INFO["kl_weight"] * parts[-1][1])
        assert abs(ll["total"].item() - want) < 1e-6 and ll["total"].item() == losses[-1]
        assert ll["dist"].item() == 0 and ll["occ"].item() == 0          # ('smooth' is reported unweighted, whatever its weight)
    return losses, norms, parts


def scene(R_s, S):
    sc = step_scene(R_s, S)
    R = sc["R"]
    from tests.test_gpu_train_rays import u01
    sc.update(tdepth=(u01(293, R_s) * 4 + 2).cuda(), noise=normals(294, R * S).reshape(R, S).cuda())
    return sc


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v1", "bf16"), ("v2", "f32"), ("v2", "bf16")])
def test_fused_step_with_the_terms_equals_autograd_route(N, net, mode):
    from nerf_few_shot_limitations_amd.training import FusedStep
    R_s, S, steps = 40, 16, 3
    sc = scene(R_s, S)
    R, z, rd = sc["R"], sc["z"], sc["d"]
    pos = (sc["o"][:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    pts = N.PositionalEncoding(10)(pos) if net == "v1" else pos
    a, b = models(N, net, mode)
    ref = autograd_steps(N, a, net, steps, pts, dirs, z, rd, sc["tgt"], sc["tdepth"], sc["noise"], R_s)
    step = FusedStep(b, lr=5e-4, weight_decay=WD, patch_size=PS, **OPTS, **INFO)
    got = fused_loop(step, steps, lambda: step(pts, z, rd, sc["tgt"], dirs=dirs if net != "v1" else None, target_depth=sc["tdepth"], noise=sc["noise"],
                                               n_patches=NPS))
    compare(net, mode, ref, got)
    assert min(p[0] for p in ref[2]) > 0 and min(p[1] for p in ref[2]) > 0
    with pytest.raises(ValueError, match="kl_weight"):
        step(pts, z, rd, torch.cat([sc["tgt"], sc["tgt"][:1].expand(R - R_s, 3)]), dirs=dirs if net != "v1" else None)      # the KL term without patches
    with pytest.raises(ValueError):
        FusedStep(b, lr=5e-4)(pts, z, rd, sc["tgt"], dirs=dirs if net != "v1" else None, n_patches=NPS)


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v2", "f32"), ("v2", "bf16")])
def test_step_rays_with_the_terms_with_and_without_a_grid(N, net, mode):
    """step_rays with both terms (a) against the autograd route on the step's own depths; (b) under an all-ones grid, both
    grid_inputs: the dense step's bits (V1 on "staged" encodes the compacted points in another kernel: held to (a)'s tolerances)."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    from tests.test_gpu_train_occupancy import grid_of
    R_s, S, steps = 40, 16, 3
    sc = scene(R_s, S)
    R, z, rd = sc["R"], sc["z"], sc["d"]
    pos = (sc["o"][:, None, :] + rd[:, None, :] * z[:, :, None]).reshape(-1, 3)
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    a, _ = models(N, net, mode)
    pts = N.PositionalEncoding(10)(pos) if net == "v1" else pos
    ref = autograd_steps(N, a, net, steps, pts, dirs, z, rd, sc["tgt"], sc["tdepth"], sc["noise"], R_s)

    def fused(**more):
        _, b = models(N, net, mode)
        step = FusedStep(b, lr=5e-4, weight_decay=WD, patch_size=PS, **OPTS, **INFO)
        out = fused_loop(step, steps, lambda: step.step_rays(sc["o"], rd, sc["tgt"], NEAR, FAR, S, perturb=False, z_in=z, target_depth=sc["tdepth"],
                                                             noise=sc["noise"], n_patches=NPS, **more))
        return out, b

    plain, b = fused()
    compare(net, mode, ref, plain)
    ones = grid_of("ones", box=(-12.0, 12.0))
    for route in ("staged", "rays"):
        got, g = fused(occupancy=ones, grid_inputs=route)
        if net == "v2" or route == "rays":
            assert got == plain, route
            assert torch.equal(g.flat_params().flat, b.flat_params().flat), route
        else:
            compare(net, mode, ref, got)


def test_step_view_with_the_entropy_equals_step_rays_on_the_views_rays(N):
    from tests.test_gpu_train_rays import _step_pair, u01
    sa, sb = _step_pair(N, "bf16", lr=5e-4, ent_weight=0.05, ent_threshold=0.05, reg_weight=1e-4)
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
        assert list(sb.last_losses) == ["total", "rgb", "depth", "reg", "dist", "occ", "smooth", "entropy", "kl"]
        assert sb.last_losses["entropy"].item() > 0 and sb.last_losses["kl"].item() == 0
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)


@pytest.mark.parametrize("route", ["call", "rays", "grid-staged", "grid-rays"])
def test_a_step_with_the_terms_launches_what_a_patch_step_launches(N, route, monkeypatch):
    from nerf_few_shot_limitations_amd.training import FusedStep
    from tests.test_gpu_train_occupancy import grid_of
    from tests.test_gpu_training import make_v2
    R_s, S = 8, 5
    sc = step_scene(R_s, S)
    R = sc["R"]
    grid = grid_of("random", outside=1, seed=195, box=(-6.0, 6.0))

    def names(**kw):
        model = make_v2(N, "bf16", scene="solid", n_layers=2)[0]
        step = FusedStep(model, lr=1e-3, reg_weight=1e-4, dist_span=FAR - NEAR, patch_size=PS, **kw)
        if route == "call":
            pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3)
            dirs = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
            return record(lambda: step(pts, sc["z"], sc["d"], sc["tgt"], dirs=dirs, n_patches=NPS), monkeypatch)
        more = {} if route == "rays" else dict(occupancy=grid, grid_inputs=route.split("-")[1])
        return record(lambda: step.step_rays(sc["o"], sc["d"], sc["tgt"], NEAR, FAR, S, perturb=True, seed=3, n_patches=NPS, **more), monkeypatch)

    base = names(depth_smooth_weight=0.5)
    assert base.count("nrf_composite_patch_loss_backward") == 1 and base.count("nrf_patch_terms_finish") == 1
    swap = {"nrf_composite_patch_loss_backward": "nrf_composite_info_loss_backward", "nrf_patch_terms_finish": "nrf_info_terms_finish"}
    for kw in (dict(depth_smooth_weight=0.5, ent_weight=0.05), dict(depth_smooth_weight=0.5, kl_weight=0.02), dict(ent_weight=0.05, kl_weight=0.02)):
        got = names(**kw)
        print(route, kw, got)
        assert got == [swap.get(n, n) for n in base] and len(got) == len(base)
    # with both weights 0 the sequence is today's
    assert names(depth_smooth_weight=0.5, ent_weight=0.0, kl_weight=0.0) == base


# ---------------------------------------------------------------------------------------------
# 7. more supervised groups and more patches than the grid holds workgroups
# ---------------------------------------------------------------------------------------------
def test_past_one_grid_trip(L):
    """cap * 4 + 1 supervised rays (one more than the grid's workgroups take in one trip of four waves) and cap + 1 patches of 2 x 2
    rays at S = 4, both terms on and alone: every ray of the second trip is held to the float64 oracle like the first."""
    src = open(os.path.join(ROOT, "nerf_few_shot_limitations_amd", "csrc", "info_reg.hip")).read()
    body = src[src.index("int launch_composite_info_loss_backward("):src.index("int launch_info_terms_finish(")]
    caps = re.findall(r"grid_for\(work, kBlock, (\d+)\)", body)
    assert caps == ["16384"], caps
    assert "n_sup * 64" in body and "pt.n_patches * kBlock" in body and "kWaves = kBlock / 64" in src and "kBlock = 256" in src
    cap, P, S = int(caps[0]), 2, 4
    n_sup, n_p = 4 * cap + 1, cap + 1
    R = n_sup + n_p * P * P
    rgb, sig, z, d = case(R, S, 800, False, equal=True)
    tgt = torch.zeros(n_sup, 3)
    dens = sig[..., 0]
    tau = middle_threshold(distribution(dens.double(), z.double(), d.double())[1])
    got = run_info(L, rgb, sig, z, d, tgt, P, n_p, (EW, tau, KW), w=NONE["w"])
    ref, mH, K, A = closed_form(dens, z, d, tau, P, n_p, EW, KW)
    total, l_ent, l_kl, _, _, _ = info_loss(dens.double(), z.double(), d.double(), tau, P, n_p, EW, KW)
    ds = got["d_sigma"].cpu()
    share = check_terms_alone(ds, dens, z, d, tau, P, n_p, EW, KW, ref, f"{n_sup} rays + {n_p} patches")
    check_values(got, mH, K, l_ent, l_kl, P, "past one grid trip")
    assert share <= 1.0 and torch.all(got["d_rgb"] == 0)
    # (the outputs were NaN before the launch: a ray or a patch that no workgroup walked would still hold one)
    assert torch.isfinite(ds).all() and torch.isfinite(got["info_terms"]).all() and torch.isfinite(got["patch_kl"]).all()
    assert torch.any(ds[n_sup - 1024:n_sup] != 0) and torch.any(ds[-1024:] != 0)
