"""The few-shot ray regularisers of the fused training step, without a GPU: the O(S) scan form of the distortion term's dL/dw
replayed in fp32 (the kernel's walk: 64-sample segments, prefix carries left by pass 1, suffix carries of pass 2) against float64
autograd of the O(S^2) definition; the exported entries, their refusals, FusedStep's keywords, the hierarchical and train_cli
refusals, and the new unit's resource census (tests/golden/kernel_resources_ray_reg.json)."""
import argparse
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 2), (37, 16), (9, 65), (7, 130), (3, 200), (4, 1100)]


def case(R, S, seed, opaque=True, equal=True):
    """composite_case's inputs (tests/test_gpu_training.py): a third of the densities <= 0, an opaque sample mid-ray -- and two
    equal depths in every ray."""
    rgb = torch.from_numpy(O.uniform01(seed, R * S * 3).reshape(R, S, 3)).float()
    sig = torch.from_numpy(O.uniform01(seed + 1, R * S).reshape(R, S, 1) * 3 - 1).float()
    if opaque:
        sig[:, S // 3] = 40.0
    z = torch.sort(torch.from_numpy(O.uniform01(seed + 2, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values
    if equal and S > 1:
        z[:, S // 2] = z[:, S // 2 - 1]
    d = torch.from_numpy(O.uniform01(seed + 3, R * 3).reshape(R, 3) - 0.5).float()
    return rgb, sig, z, d


def midpoints(z, kappa):
    """m_i, delta_i of the issue's definitions, in z's dtype."""
    m = torch.cat([kappa * (z[:, :-1] + z[:, 1:]) * 0.5, kappa * z[:, -1:]], dim=1)
    delta = torch.cat([kappa * (z[:, 1:] - z[:, :-1]), torch.zeros_like(z[:, -1:])], dim=1)
    return m, delta


def distortion(w, z, kappa):
    """D_r by the O(S^2) definition."""
    m, delta = midpoints(z, kappa)
    return (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum(dim=(1, 2)) + (w * w * delta).sum(dim=1) / 3.0


def scan_dw(w, z, kappa):
    """dD/dw_i = 2 t_i + (2/3) w_i delta_i in fp32 as the kernel walks it: exclusive prefix sums A, B of w, w m (carries entering every
    64-sample segment, then a scan inside it), exclusive suffix sums C, Dm (segments back to front), t = (m A - B) + (Dm - m C)."""
    f = torch.float32
    w, z = w.to(f), z.to(f)
    k = torch.tensor(kappa, dtype=f)
    m = torch.cat([k * ((z[:, :-1] + z[:, 1:]) * 0.5), k * z[:, -1:]], dim=1)
    delta = torch.cat([k * (z[:, 1:] - z[:, :-1]), torch.zeros_like(z[:, -1:])], dim=1)
    R, S = w.shape
    wm = w * m
    n_seg = (S + 63) // 64
    A, B, Cs, Ds = (torch.zeros_like(w) for _ in range(4))
    pa = torch.zeros(R, dtype=f); pb = torch.zeros(R, dtype=f)
    for s in range(n_seg):
        sl = slice(64 * s, min(64 * s + 64, S))
        ia, ib = torch.cumsum(w[:, sl], 1), torch.cumsum(wm[:, sl], 1)
        A[:, sl] = pa[:, None] + torch.cat([torch.zeros(R, 1, dtype=f), ia[:, :-1]], 1)
        B[:, sl] = pb[:, None] + torch.cat([torch.zeros(R, 1, dtype=f), ib[:, :-1]], 1)
        pa, pb = pa + w[:, sl].sum(1), pb + wm[:, sl].sum(1)
    sc = torch.zeros(R, dtype=f); sd = torch.zeros(R, dtype=f)
    for s in reversed(range(n_seg)):
        sl = slice(64 * s, min(64 * s + 64, S))
        rc, rd = torch.flip(torch.cumsum(torch.flip(w[:, sl], [1]), 1), [1]), torch.flip(torch.cumsum(torch.flip(wm[:, sl], [1]), 1), [1])
        Cs[:, sl] = sc[:, None] + torch.cat([rc[:, 1:], torch.zeros(R, 1, dtype=f)], 1)
        Ds[:, sl] = sd[:, None] + torch.cat([rd[:, 1:], torch.zeros(R, 1, dtype=f)], 1)
        sc, sd = sc + rc[:, 0], sd + rd[:, 0]
    t = (m * A - B) + (Ds - m * Cs)
    assert t.dtype == f
    return 2.0 * t + (2.0 / 3.0) * w * delta, (w * t).sum(1) + (w * w * delta).sum(1) / 3.0


@pytest.mark.parametrize("R,S", SHAPES)
def test_scan_form_matches_float64_autograd_of_the_definition(R, S):
    rgb, sig, z, d = case(R, S, 300 + S, equal=S > 2)           # (at S = 2 the equal pair would be the whole ray: D = 0)
    kappa = 0.25
    # float64: the weights of the oracle's compositor, dD/dw and dD/dsigma by autograd of the O(S^2) definition
    s64 = sig.double().requires_grad_(True)
    _, _, w64 = O.volume_render(rgb.double(), s64, z.double(), d.double(), white_bkgd=False)
    w_leaf = w64.detach().clone().requires_grad_(True)
    D64 = distortion(w_leaf, z.double(), kappa)
    D64.sum().backward()
    distortion(w64, z.double(), kappa).sum().backward()
    # the scan form in fp32 on the fp32 rounding of those weights
    got, D32 = scan_dw(w64.detach().float(), z, kappa)
    ref = w_leaf.grad
    err = float(((got.double() - ref).abs() / ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)).max())
    err_D = float(((D32.double() - D64.detach()).abs() / D64.detach().abs().clamp_min(1e-30)).max())
    # fp32 torch on the definition, through the fp32 compositor, on d_sigma
    s32 = sig.clone().requires_grad_(True)
    _, _, w32 = O.volume_render(rgb, s32, z, d, white_bkgd=False)
    distortion(w32, z, kappa).sum().backward()
    ds64 = s64.grad[..., 0]
    err_s = float(((s32.grad[..., 0].double() - ds64).abs() / ds64.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)).max())
    print(f"(R,S)=({R},{S}) scan dL/dw err / ray max {err:.3g}   D rel err {err_D:.3g}   fp32 definition d_sigma err / ray max {err_s:.3g}")
    assert err < 1e-5
    assert err_D < 1e-5


def test_one_sample_has_no_distortion():
    w = torch.tensor([[0.7], [0.0]])
    z = torch.tensor([[3.0], [2.5]])
    g, D = scan_dw(w, z, 0.25)
    assert torch.all(D == 0) and torch.all(g == 0) and torch.all(distortion(w, z, 0.25) == 0)


# ---------------------------------------------------------------------------------------------
# the library's entries and their refusals
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib as L
    L.lib()
    return L


ENTRIES = ("nrf_composite_reg_loss_backward", "nrf_ray_terms_finish")
EINVAL = -1          # NRF_EINVAL


def test_the_library_exports_both_entries(L):
    for name in ENTRIES:
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    for name in ENTRIES + ("nrf_ray_reg",):
        assert name in header
    assert C.sizeof(L.nrf_ray_reg) == 20 and L.ray_reg().struct_bytes == 20
    assert L.lib().nrf_abi_version() == 5 and L.lib().nrf_abi_sizeof(5) == -1          # additive: nrf_abi_sizeof knows nothing of it


def _call(L, reg, S=8, slot=None):
    """nrf_composite_reg_loss_backward on pointers no launch will ever read: every refusal fires before the device is touched."""
    p = 4096
    lo = L.loss_opts()
    return L.lib().nrf_composite_reg_loss_backward(p, 3, p, 1, p, p, 4, S, 0, p, C.byref(lo), C.byref(reg) if reg is not None else None, slot, p, p, 3,
                                                   p, 1, p, None, 0, None)


def _finish(L, reg):
    return L.lib().nrf_ray_terms_finish(4096, 4, C.byref(reg) if reg is not None else None, 4096, 8192, None)


@pytest.mark.parametrize("why,reg_kw,S", [
    ("negative dist_weight", dict(dist_weight=-1.0, dist_inv_span=0.25), 8),
    ("negative occ_weight", dict(occ_weight=-0.5, occ_samples=2), 8),
    ("nan dist_weight", dict(dist_weight=float("nan"), dist_inv_span=0.25), 8),
    ("zero dist_inv_span", dict(dist_weight=1.0, dist_inv_span=0.0), 8),
    ("negative dist_inv_span", dict(dist_weight=1.0, dist_inv_span=-0.25), 8),
    ("infinite dist_inv_span", dict(dist_weight=1.0, dist_inv_span=float("inf")), 8),
    ("nan dist_inv_span", dict(dist_weight=1.0, dist_inv_span=float("nan")), 8),
    ("occ_samples 0", dict(occ_weight=1.0, occ_samples=0), 8),
    ("n_samples > 4096", dict(dist_weight=1.0, dist_inv_span=0.25), 4097),
])
def test_refusals_fire_without_a_gpu(L, why, reg_kw, S):
    reg = L.ray_reg(**reg_kw)
    assert _call(L, reg, S) == EINVAL, why
    assert L.lib().nrf_last_error()
    if S <= 4096:
        assert _finish(L, reg) == EINVAL, why


def test_struct_bytes_null_and_slot_alignment_are_refused(L):
    reg = L.ray_reg(dist_weight=1.0, dist_inv_span=0.25)
    reg.struct_bytes = 16
    assert _call(L, reg) == EINVAL and b"struct_bytes" in L.lib().nrf_last_error()
    assert _finish(L, reg) == EINVAL
    assert _call(L, None) == EINVAL and _finish(L, None) == EINVAL
    assert _call(L, L.ray_reg(occ_weight=1.0, occ_samples=3), slot=4098) == EINVAL and b"aligned" in L.lib().nrf_last_error()
    ok = L.ray_reg()
    assert L.lib().nrf_ray_terms_finish(None, 4, C.byref(ok), 4096, 8192, None) == EINVAL
    assert L.lib().nrf_ray_terms_finish(4096, 0, C.byref(ok), 4096, 8192, None) == EINVAL


# ---------------------------------------------------------------------------------------------
# FusedStep and train_cli
# ---------------------------------------------------------------------------------------------
def _model():
    import nerf_few_shot_limitations_amd as N
    return N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2)


def test_fused_step_takes_the_four_keywords_and_refuses_bad_ones():
    from nerf_few_shot_limitations_amd.training import FusedStep
    p = inspect.signature(FusedStep.__init__).parameters
    assert [p[k].default for k in ("dist_weight", "occ_weight", "occ_samples", "dist_span")] == [0.0, 0.0, 0, None]
    m = _model()
    plain = FusedStep(m)
    assert not plain.ray_reg
    s = FusedStep(m, dist_weight=1e-2, occ_weight=1e-2, occ_samples=4, dist_span=4.0)
    assert s.ray_reg and (s.dist_weight, s.occ_weight, s.occ_samples, s.dist_span) == (1e-2, 1e-2, 4, 4.0)
    for bad in (dict(dist_weight=-1e-3), dict(occ_weight=-1.0, occ_samples=2), dict(occ_weight=1.0), dict(occ_weight=1.0, occ_samples=0),
                dict(occ_samples=-1), dict(dist_weight=1.0, dist_span=0.0), dict(dist_weight=1.0, dist_span=-2.0),
                dict(dist_weight=float("nan")), dict(dist_weight=1.0, dist_span=float("inf"))):
        with pytest.raises(ValueError):
            FusedStep(m, **bad)


def test_calling_with_depths_needs_a_span():
    from nerf_few_shot_limitations_amd.training import FusedStep
    s = FusedStep(_model(), dist_weight=1e-2)
    with pytest.raises(ValueError, match="dist_span"):
        s(torch.zeros(8, 63), torch.zeros(2, 4), torch.zeros(2, 3), torch.zeros(2, 3))


@pytest.mark.parametrize("kw", [dict(dist_weight=1e-2), dict(occ_weight=1e-2, occ_samples=2)])
def test_the_hierarchical_step_refuses_the_terms(kw):
    from nerf_few_shot_limitations_amd.training import FusedStep
    s = FusedStep(_model(), **kw)
    o = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="dist_weight or occ_weight"):
        s.step_rays_hierarchical(o, o, o, 2.0, 6.0, 8, 4)
    with pytest.raises(ValueError, match="dist_weight or occ_weight"):
        s.step_view_hierarchical(None, None, 4, 4, 1.0, None, 2.0, 6.0, 8, 4)


def test_train_cli_flags_and_refusals():
    from nerf_few_shot_limitations_amd import train_cli
    ns = lambda **kw: argparse.Namespace(**{**dict(dist_weight=0.0, occ_weight=0.0, occ_samples=None, n_importance=0), **kw})
    assert train_cli.ray_reg_args_error(ns()) is None
    assert train_cli.ray_reg_args_error(argparse.Namespace()) is None
    assert train_cli.ray_reg_args_error(ns(dist_weight=1e-2, occ_weight=1e-2, occ_samples=4)) is None
    assert "--n-importance" in train_cli.ray_reg_args_error(ns(dist_weight=1e-2, n_importance=8))
    assert "--n-importance" in train_cli.ray_reg_args_error(ns(occ_weight=1e-2, occ_samples=4, n_importance=8))
    assert "--occ-samples" in train_cli.ray_reg_args_error(ns(occ_weight=1e-2))
    assert "--occ-weight" in train_cli.ray_reg_args_error(ns(occ_samples=4))
    assert train_cli.ray_reg_args_error(ns(dist_weight=-1.0)) is not None
    assert train_cli.ray_reg_options(ns(), 2.0, 6.0) == {}
    assert train_cli.ray_reg_options(ns(dist_weight=1e-2), 2.0, 6.0) == dict(dist_weight=1e-2, occ_weight=0.0, occ_samples=0, dist_span=4.0)
    # the command refuses before it reads a config or a data set
    with pytest.raises(SystemExit, match="--n-importance"):
        train_cli.main(["--config", "/nonexistent.yaml", "--data", "/nonexistent", "--n-importance", "8", "--dist-weight", "0.01"])
    doc = " ".join(train_cli.__doc__.split())
    for word in ("--dist-weight W", "--occ-weight W", "--occ-samples K", "mip-NeRF 360", "FreeNeRF", "nrf_ray_reg"):
        assert word in doc, word


# ---------------------------------------------------------------------------------------------
# the new unit's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from nerf_few_shot_limitations_amd import build as B
    sub = os.path.join(B.OBJ, B.RAY_REG_DIR)
    if not os.path.isdir(sub) or not any(f.endswith(".o.remarks") for f in os.listdir(sub)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B


NEW = ("reg_loss_backward_kernel<false>", "reg_loss_backward_kernel<true>", "ray_terms_finish_kernel")


def test_new_kernels_match_their_census_and_spill_nothing(B):
    res = B.kernel_resources(os.path.join(B.OBJ, B.RAY_REG_DIR))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_ray_reg.json")))
    fields = gold["fields"]
    assert set(res) == set(gold["kernels"]) and len(res) == len(NEW), sorted(res)
    for kernel in NEW:
        (name, r), = [(k, v) for k, v in res.items() if "::" + kernel + "(" in k]
        print(kernel, r)
        assert r["tu"] == "ray_reg"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["agprs"] == 0, (name, r)
        assert [r.get(f, 0) for f in fields] == gold["kernels"][name], (name, dict(zip(fields, gold["kernels"][name])), r)


def test_the_unit_stays_out_of_the_main_census_and_the_pinned_tables(B):
    main = B.kernel_resources()
    assert not any(k.startswith("ray_reg:") or "reg_loss_backward_kernel" in k or "ray_terms_finish_kernel" in k for k in main)
    assert not any(src == "ray_reg.hip" for src, *_ in B.SOURCES) and not any(src == "ray_reg.hip" for src, *_ in B.SUBDIR_SOURCES)
    assert [(src, name, sub) for src, name, _, sub in B.RAY_REG_SOURCES] == [("ray_reg.hip", "ray_reg", B.RAY_REG_DIR)]
