"""InfoNeRF's ray-entropy and patch-KL terms of the fused training step, without a GPU: the closed-form gradients of nerfhip.h
(nrf_info_reg) in float64 against float64 autograd of the definitions; their fp32 replay in the kernel's order against the bar the
GPU test holds the kernel to -- and the `1 - e` form of a_i missing it; the exported entries and their refusals; FusedStep's
keywords; train_cli's flags; the new unit's resource census (tests/golden/kernel_resources_info_reg.json).

The definitions, the closed form, the replay and the bar live here; tests/test_gpu_info_reg.py imports them."""
import argparse
import ctypes as C
import inspect
import json
import math
import os

import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_ray_reg_host import case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-10
LN_INV_EPS = math.log(1.0 / EPS)


# ---------------------------------------------------------------------------------------------
# the definitions (any dtype; autograd flows through them)
# ---------------------------------------------------------------------------------------------
def distribution(dens, z, d):
    """(a, A, p, dist e) of rays with effective densities dens (R,S): over the S - 1 samples with a finite interval."""
    dist = (z[:, 1:] - z[:, :-1]) * d.norm(dim=1, keepdim=True)
    x = torch.relu(dens[:, :-1]) * dist
    a = -torch.expm1(-x)
    A = a.sum(dim=1)
    return a, A, a / (A[:, None] + EPS), dist * torch.exp(-x)


def info_terms(dens, z, d, tau, P, n_p):
    """(m_r H_r (R), K_p (n_p), A (R)) by the definitions; the masks are constants."""
    R, S = dens.shape
    a, A, p, _ = distribution(dens, z, d)
    m = (A.detach() > tau).to(dens.dtype)
    lp = torch.log(p + EPS)
    H = -(p * lp).sum(dim=1)
    Rs = R - n_p * P * P
    pp, ll, mm = p[Rs:].reshape(n_p, P, P, S - 1), lp[Rs:].reshape(n_p, P, P, S - 1), m[Rs:].reshape(n_p, P, P)
    an_p, an_l, an_m = pp[:, :-1, :-1], ll[:, :-1, :-1], mm[:, :-1, :-1]
    kr = an_m * mm[:, :-1, 1:] * (an_p * (an_l - ll[:, :-1, 1:])).sum(dim=-1)
    kd = an_m * mm[:, 1:, :-1] * (an_p * (an_l - ll[:, 1:, :-1])).sum(dim=-1)
    return m * H, (kr + kd).sum(dim=(1, 2)), A


def info_loss(dens, z, d, tau, P, n_p, ent_weight, kl_weight):
    """(ent_weight L_ent + kl_weight L_kl, L_ent, L_kl, m H, K_p, A): the divisors are R and N_p (P-1)^2."""
    mH, K, A = info_terms(dens, z, d, tau, P, n_p)
    l_ent = mH.sum() / dens.shape[0]
    l_kl = K.sum() / (n_p * (P - 1) ** 2) if n_p > 0 else torch.zeros((), dtype=dens.dtype)
    return ent_weight * l_ent + kl_weight * l_kl, l_ent, l_kl, mH, K, A


def middle_threshold(A):
    """tau halfway between the two middle values of the sorted A's: about half the rays are masked.  The gap around tau must exceed
    1e-3 tau, so that no fp32 sum can put a ray on the other side; where the middle pair is closer (behind an opaque first sample
    at S = 2 most A's are 1 to nine digits) the nearest pair to the middle that is apart is taken."""
    s = torch.sort(A.double()).values
    mid = (len(s) - 1) // 2
    for k in sorted(range(len(s) - 1), key=lambda i: (abs(i - mid), i)):
        tau = float(0.5 * (s[k] + s[k + 1]))
        if float(s[k + 1] - s[k]) > 1e-3 * tau:
            return tau
    raise AssertionError("a condition on the inputs: some gap between the sorted A's must exceed 1e-3 tau")


# ---------------------------------------------------------------------------------------------
# the closed form, in the kernel's order: float64 it is the gradient, float32 it is the kernel's replay
# ---------------------------------------------------------------------------------------------
def seg_sum(v):
    """Sum over the last axis as the kernel adds it: 64-sample segments, front to back."""
    out = torch.zeros(v.shape[:-1], dtype=v.dtype)
    for s0 in range(0, v.shape[-1], 64):
        out = out + v[..., s0:s0 + 64].sum(dim=-1)
    return out


def closed_form(dens, z, d, tau, P, n_p, ent_weight, kl_weight, dtype=torch.float64, form="expm1"):
    """dL/dsigma (R,S) of ent_weight L_ent + kl_weight L_kl by nerfhip.h's closed form, every operation in `dtype`; form = "1-e":
    a_i = 1 - exp(-x_i) as the compositor forms alpha.  Also returns (m H, K_p, A)."""
    dens, z, d = dens.to(dtype), z.to(dtype), d.to(dtype)
    R, S = dens.shape
    eps = torch.tensor(EPS, dtype=dtype)
    dist = (z[:, 1:] - z[:, :-1]) * d.norm(dim=1, keepdim=True)
    nx = -torch.relu(dens[:, :-1]) * dist
    e = torch.exp(nx)
    a = -torch.expm1(nx) if form == "expm1" else 1.0 - e
    A = seg_sum(a)
    Ae = (A + eps)[:, None]
    m = A > tau
    p = a / Ae
    pe = p + eps
    lp, rp = torch.log(pe), p / pe
    es = torch.tensor(ent_weight, dtype=dtype) / torch.tensor(float(R), dtype=dtype)
    G = torch.where(m[:, None], -(es * (lp + rp)), torch.zeros_like(p))
    K = torch.zeros(n_p, dtype=dtype)
    if n_p > 0 and kl_weight > 0:
        ks = torch.tensor(kl_weight, dtype=dtype) / (torch.tensor(float(n_p), dtype=dtype) * torch.tensor(float((P - 1) ** 2), dtype=dtype))
        Rs = R - n_p * P * P
        shape = (n_p, P, P, S - 1)
        pp, ll, rr, ee, mm = p[Rs:].reshape(shape), lp[Rs:].reshape(shape), rp[Rs:].reshape(shape), pe[Rs:].reshape(shape), m[Rs:].reshape(n_p, P, P)
        Gp = G[Rs:].reshape(shape).clone()
        Kp = torch.zeros(n_p, P, P, dtype=dtype)
        # in the kernel's order of a ray's roles: first argument against the right, then the lower neighbour; second argument of the
        # left, then of the upper anchor
        for (ai, aj), (ni, nj) in (((slice(0, -1), slice(0, -1)), (slice(0, -1), slice(1, None))), ((slice(0, -1), slice(0, -1)), (slice(1, None), slice(0, -1)))):
            on = (mm[:, ai, aj] & mm[:, ni, nj])[..., None]
            dl = ll[:, ai, aj] - ll[:, ni, nj]
            Gp[:, ai, aj] = Gp[:, ai, aj] + torch.where(on, ks * (dl + rr[:, ai, aj]), torch.zeros_like(dl))
            Kp[:, ai, aj] = Kp[:, ai, aj] + seg_sum(torch.where(on, pp[:, ai, aj] * dl, torch.zeros_like(dl)))
        for (ai, aj), (ni, nj) in (((slice(0, -1), slice(0, -1)), (slice(0, -1), slice(1, None))), ((slice(0, -1), slice(0, -1)), (slice(1, None), slice(0, -1)))):
            on = (mm[:, ai, aj] & mm[:, ni, nj])[..., None]
            Gp[:, ni, nj] = Gp[:, ni, nj] - torch.where(on, ks * (pp[:, ai, aj] / ee[:, ni, nj]), torch.zeros_like(pp[:, ai, aj]))
        G = torch.cat([G[:Rs], Gp.reshape(n_p * P * P, S - 1)])
        K = Kp.sum(dim=(1, 2))
    M = seg_sum(p * G)[:, None]
    da = (G - M) / Ae
    ds = torch.where(dens[:, :-1] > 0, (dist * e) * da, torch.zeros_like(da))
    mH = torch.where(m, -seg_sum(p * lp), torch.zeros_like(A)) if ent_weight > 0 else torch.zeros_like(A)
    return torch.cat([ds, torch.zeros(R, 1, dtype=dtype)], dim=1), mH, K, A


def roles(A, tau, P, n_p, ent_weight, kl_weight):
    """Per ray: (the entropy role, the KL roles as the first argument, as the second) that are on, as float64 counts."""
    R = A.shape[0]
    m = A.double() > tau
    first, second = torch.zeros(R, dtype=torch.float64), torch.zeros(R, dtype=torch.float64)
    if n_p > 0 and kl_weight > 0:
        Rs = R - n_p * P * P
        mm = m[Rs:].reshape(n_p, P, P)
        f, s = torch.zeros(n_p, P, P, dtype=torch.float64), torch.zeros(n_p, P, P, dtype=torch.float64)
        right, down = (mm[:, :-1, :-1] & mm[:, :-1, 1:]).double(), (mm[:, :-1, :-1] & mm[:, 1:, :-1]).double()
        f[:, :-1, :-1] += right + down
        s[:, :-1, 1:] += right
        s[:, 1:, :-1] += down
        first[Rs:], second[Rs:] = f.reshape(-1), s.reshape(-1)
    return (m & (ent_weight > 0)).double(), first, second


def allowance(dens, z, d, tau, P, n_p, ent_weight, kl_weight, ref):
    """The bar on the two terms' d_sigma, per entry (R,S):

        |err_j| <= 1e-4 max_ray |ref| + c 2^-23 ln(1/eps) scale dist_j e_j / (A + eps)

    scale: the sum over the ray's roles that are on of the role's weight / divisor (ent_weight / R; kl_weight / (N_p (P-1)^2) per KL
    role); c: the fp32 roundings of the kernel's own expression fl(fl(dist e) fl(fl(G_j - M) / fl(A + eps))) added into d_sigma,
    counted one by one, each moving the result by at most one unit 2^-23 ln(1/eps) scale dist e / (A + eps) since |G|, |M| <=
    (ln(1/eps) + 1) scale:
      dist: z_{i+1} - z_i, |d| *            2      x = relu(sigma) dist                 1      a = -expm1(-x)                  1
      A: a wave tree of 64                  6      A + eps                              1      p = a / (A + eps)               1
      p + eps, log, p / (p + eps)           3      lp + rp, ent_scale *                 2      p G                             1
      M: a wave tree of 64                  6      G - M, / (A + eps)                   2      exp(-x), dist e, (dist e) *     3
      the addition into d_sigma             1                                                                      together   30
      every segment behind the first: one addition more in A and in M                                                          2
      a KL role as the first argument: q = a' / (A' + eps), + eps, log, lp - lq, + rp, kl_scale *, G +                        7
      a KL role as the second argument: p' = a' / (A' + eps), / (p + eps), kl_scale *, G -                                     4
    """
    S = dens.shape[1]
    _, A, _, de = distribution(dens.double(), z.double(), d.double())
    ent, first, second = roles(A, tau, P, n_p, ent_weight, kl_weight)
    es = ent_weight / dens.shape[0]
    ks = kl_weight / (n_p * (P - 1) ** 2) if n_p > 0 else 0.0
    scale = es * ent + ks * (first + second)
    c = 30.0 + 2.0 * ((max(S - 1, 1) + 63) // 64 - 1) + 7.0 * first + 4.0 * second
    unit = 2.0 ** -23 * LN_INV_EPS * (c * scale / (A + EPS))[:, None] * de
    unit = torch.cat([unit, torch.zeros(dens.shape[0], 1, dtype=torch.float64)], dim=1)
    return 1e-4 * ref.abs().amax(dim=1, keepdim=True) + unit, unit


def check_terms_alone(got_ds, dens, z, d, tau, P, n_p, ent_weight, kl_weight, ref, label):
    """The bar above on a d_sigma (R,S) that holds the two terms alone; the exact zeros.  Prints the largest error against a ray's
    largest entry and against the bar's rounding part (the c term) alone; returns the largest share of the whole allowance reached."""
    allow, unit = allowance(dens, z, d, tau, P, n_p, ent_weight, kl_weight, ref)
    err = (got_ds.double() - ref).abs()
    of_unit = float((err / unit.clamp_min(1e-300))[unit > 0].max()) if torch.any(unit > 0) else 0.0
    worst = float((err / ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)).max())
    share = float((err / allow.clamp_min(1e-300))[err > 0].max()) if torch.any(err > 0) else 0.0
    print(f"{label}: err / ray max {worst:.3g}; largest err / (c 2^-23 ln(1/eps) scale dist e / (A + eps)) {of_unit:.3g}; "
          f"largest share of the allowance {share:.3g}")
    assert torch.all(err <= allow), (label, worst, share)
    A = distribution(dens.double(), z.double(), d.double())[1]
    ent, first, second = roles(A, tau, P, n_p, ent_weight, kl_weight)
    none = (ent + first + second) == 0
    assert torch.all(got_ds[none] == 0), "a ray with no role that is on receives exactly nothing"
    assert torch.all(got_ds[dens <= 0] == 0) and torch.all(got_ds[:, -1] == 0)
    return share


def patch_case(P, S, n_p, n_sup, seed, opaque=True):
    R = n_sup + n_p * P * P
    return case(R, S, seed, opaque, equal=S > 3)


# ---------------------------------------------------------------------------------------------
# 1. the closed form against autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ent_weight,kl_weight", [(0.7, 0.0), (0.0, 1.3), (0.7, 1.3)])
@pytest.mark.parametrize("P,S", [(2, 1), (2, 2), (3, 3), (3, 16), (2, 66), (4, 130)])
def test_closed_form_is_float64_autograd_of_the_definitions(P, S, ent_weight, kl_weight):
    n_p, n_sup = 3, 5
    _, sig, z, d = patch_case(P, S, n_p, n_sup, 40 + S + P)
    sig = sig[..., 0]
    sig[1] = -sig[1].abs() - 0.1                              # a ray whose densities are all <= 0: A = 0, masked at any tau
    s64 = sig.double().requires_grad_(True)
    A = distribution(s64.detach(), z.double(), d.double())[1]
    tau = middle_threshold(A) if S > 1 else 0.0
    total, l_ent, l_kl, mH, K, _ = info_loss(s64, z.double(), d.double(), tau, P, n_p, ent_weight, kl_weight)
    if S > 1:
        total.backward()
        ref = s64.grad
    else:
        ref = torch.zeros_like(s64)                           # S - 1 = 0: no sample takes part
    got, mH_c, K_c, A_c = closed_form(sig, z, d, tau, P, n_p, ent_weight, kl_weight)
    # (at S = 2 a ray has one p = 1: its gradient is the eps terms' 1e-17, the float64 cancellation noise of O(1) terms: held absolutely)
    scale = ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-9)
    assert float(((got - ref).abs() / scale).max()) < 1e-10
    assert torch.all(got[1] == 0) and torch.all(got[sig <= 0] == 0) and torch.all(got[:, -1] == 0)
    masked = A <= tau
    assert torch.all(got[masked] == 0) and (S == 1 or (masked.any() and (~masked).any()))
    if ent_weight > 0:
        assert torch.allclose(mH_c, mH.detach(), rtol=1e-12, atol=1e-15)
    if kl_weight > 0:
        assert torch.allclose(K_c, K.detach(), rtol=1e-10, atol=1e-14)
    if S > 3:
        assert ref.abs().max() > 0 and (kl_weight == 0 or K.detach().abs().max() > 0)


def test_both_arguments_of_a_kl_take_gradient_and_the_mask_takes_none():
    P, S, n_p = 2, 8, 1
    _, sig, z, d = patch_case(P, S, n_p, 1, 77, opaque=False)
    s64 = sig[..., 0].double().requires_grad_(True)
    info_loss(s64, z.double(), d.double(), 0.0, P, n_p, 0.0, 1.0)[0].backward()
    g = s64.grad
    # ray 1 + 0 is the anchor (first argument), 1 + 1 and 1 + 2 its neighbours (second argument), 1 + 3 has no role; ray 0 is supervised
    assert g[1].abs().max() > 0 and g[2].abs().max() > 0 and g[3].abs().max() > 0 and torch.all(g[4] == 0) and torch.all(g[0] == 0)
    got = closed_form(sig[..., 0], z, d, 0.0, P, n_p, 0.0, 1.0)[0]
    assert torch.allclose(got, g, rtol=1e-9, atol=1e-15)
    # a threshold between the A's changes which terms count, not their values: no gradient flows through m
    A = distribution(s64.detach(), z.double(), d.double())[1]
    tau = float(0.5 * (A[1:].min() + A[1:].max()))
    s2 = sig[..., 0].double().requires_grad_(True)
    info_loss(s2, z.double(), d.double(), tau, P, n_p, 1.0, 1.0)[0].backward()
    assert torch.allclose(closed_form(sig[..., 0], z, d, tau, P, n_p, 1.0, 1.0)[0], s2.grad, rtol=1e-9, atol=1e-15)


# ---------------------------------------------------------------------------------------------
# 2. the fp32 replay holds the GPU bar; the compositor's 1 - e does not
# ---------------------------------------------------------------------------------------------
def replay_errors(R, S, seed, form, ent_weight=0.7, kl_weight=1.3, P=2):
    """The closed form in fp32, in the kernel's order, and its float64 twin on R rays: 2 (P = 2) or R mod P^2 supervised ones, then
    patches."""
    n_p = (R - 2) // (P * P)
    _, sig, z, d = case(R, S, seed, True, equal=S > 3)
    sig = sig[..., 0]
    A = distribution(sig.double(), z.double(), d.double())[1]
    tau = middle_threshold(A)
    ref = closed_form(sig, z, d, tau, P, n_p, ent_weight, kl_weight)[0]
    got = closed_form(sig, z, d, tau, P, n_p, ent_weight, kl_weight, dtype=torch.float32, form=form)[0]
    assert got.dtype == torch.float32
    return got, sig, z, d, tau, P, n_p, ent_weight, kl_weight, ref


@pytest.mark.parametrize("R,S", [(38, 16), (14, 3), (22, 65), (14, 66), (10, 130), (6, 200)])
def test_fp32_replay_in_the_kernels_order_holds_the_gpu_bar(R, S):
    got, *rest = replay_errors(R, S, 300 + S, "expm1")
    share = check_terms_alone(got, *rest, f"replay (R,S)=({R},{S})")
    assert share <= 1.0


def test_one_minus_e_misses_the_bar():
    """Why a_i is formed with expm1: next to e = 1 the compositor's alpha = 1 - e keeps three digits of a_i, and the KL's gradient
    into its second argument divides by p_i.  On case(38, 16, 334) with 3 x 3 patches the `1 - e` form is off by 4.0e-3 of a ray's
    largest entry (KL alone); the expm1 form by 3e-7."""
    for ew, kw in ((0.0, 1.3), (0.7, 1.3)):
        got, sig, z, d, tau, P, n_p, ew, kw, ref = replay_errors(38, 16, 334, "1-e", ew, kw, P=3)
        allow, _ = allowance(sig, z, d, tau, P, n_p, ew, kw, ref)
        err = (got.double() - ref).abs()
        worst = float((err / ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)).max())
        good = replay_errors(38, 16, 334, "expm1", ew, kw, P=3)[0]
        worst_good = float(((good.double() - ref).abs() / ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-300)).max())
        print(f"weights ({ew}, {kw}): 1 - e form err / ray max {worst:.3g}; expm1 form {worst_good:.3g}")
        assert torch.any(err > allow) and worst > 1e-3
        assert worst_good < 1e-5 and torch.all((good.double() - ref).abs() <= allow)


# ---------------------------------------------------------------------------------------------
# 3. the library's entries and their refusals
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib as L
    L.lib()
    return L


ENTRIES = ("nrf_composite_info_loss_backward", "nrf_info_terms_finish")
EINVAL = -1          # NRF_EINVAL


def test_the_library_exports_both_entries_and_the_abi_stays_5(L):
    for name in ENTRIES:
        assert name in L.SIGNATURES and hasattr(L.lib(), name)
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    for name in ENTRIES + ("nrf_info_reg", "ent_weight", "ent_threshold", "kl_weight", "NRF_INFO_KL_MAX_LDS_FLOATS 12288"):
        assert name in header
    assert [f for f, _ in L.nrf_info_reg._fields_] == ["struct_bytes", "ent_weight", "ent_threshold", "kl_weight"]
    assert C.sizeof(L.nrf_info_reg) == 16 and L.info_reg().struct_bytes == 16 and L.INFO_KL_MAX_LDS_FLOATS == 12288
    assert abs(L.info_reg().ent_threshold - 0.01) < 1e-9 and L.info_reg().ent_weight == 0 and L.info_reg().kl_weight == 0
    assert L.lib().nrf_abi_version() == 5


def _call(L, info, patch="ok", S=8, n_rays=40, reg="ok", lo="ok", slot=None, patch_terms=4096, info_terms=4096, patch_kl=4096):
    """nrf_composite_info_loss_backward on pointers no launch will ever read: every refusal fires before the device is touched."""
    p = 4096
    lo = L.loss_opts() if lo == "ok" else lo
    reg = L.ray_reg() if reg == "ok" else reg
    patch = L.patch_reg(0.1, 2, 1) if patch == "ok" else patch
    return L.lib().nrf_composite_info_loss_backward(p, 3, p, 1, p, p, n_rays, S, 0, p, C.byref(lo) if lo is not None else None,
                                                    C.byref(reg) if reg is not None else None, slot, p, p, 3, p, 1, p, None, 0, None,
                                                    C.byref(patch) if patch is not None else None, patch_terms, None,
                                                    C.byref(info) if info is not None else None, info_terms, patch_kl)


def _finish(L, info, patch="ok", S=8, n_rays=40, reg="ok", lo="ok", info_terms=4096, patch_kl=4096, out=8192):
    lo = L.loss_opts() if lo == "ok" else lo
    reg = L.ray_reg() if reg == "ok" else reg
    patch = L.patch_reg(0.1, 2, 1) if patch == "ok" else patch
    return L.lib().nrf_info_terms_finish(4096, n_rays, S, C.byref(lo) if lo is not None else None, C.byref(reg) if reg is not None else None,
                                         C.byref(patch) if patch is not None else None, 4096, C.byref(info) if info is not None else None,
                                         info_terms, patch_kl, out, None)


@pytest.mark.parametrize("why,kw", [
    ("negative ent_weight", dict(ent_weight=-0.1)), ("nan ent_weight", dict(ent_weight=float("nan"))),
    ("infinite ent_weight", dict(ent_weight=float("inf"))), ("negative threshold", dict(ent_weight=0.1, ent_threshold=-1e-3)),
    ("nan threshold", dict(ent_weight=0.1, ent_threshold=float("nan"))), ("infinite threshold", dict(ent_threshold=float("inf"))),
    ("negative kl_weight", dict(kl_weight=-0.1)), ("nan kl_weight", dict(kl_weight=float("nan"))), ("infinite kl_weight", dict(kl_weight=float("inf"))),
])
def test_bad_weights_are_refused_without_a_gpu(L, why, kw):
    info = L.info_reg(**kw)
    assert _call(L, info) == EINVAL, why
    assert L.lib().nrf_last_error()
    assert _finish(L, info) == EINVAL, why


def test_struct_bytes_null_the_kl_terms_needs_and_the_parents_refusals(L):
    ok = L.info_reg(0.1, 0.01, 0.2)
    bad = L.info_reg(0.1, 0.01, 0.2)
    bad.struct_bytes = 12
    assert _call(L, bad) == EINVAL and b"struct_bytes" in L.lib().nrf_last_error()
    assert _finish(L, bad) == EINVAL and b"struct_bytes" in L.lib().nrf_last_error()
    assert _call(L, None) == EINVAL and _finish(L, None) == EINVAL
    # kl_weight > 0 with no patch to act on; entropy alone needs none
    none = L.patch_reg(0.0, 2, 0)
    assert _call(L, ok, patch=none) == EINVAL and b"n_patches" in L.lib().nrf_last_error()
    assert _finish(L, ok, patch=none) == EINVAL
    # kl_weight > 0 beyond the LDS cap: P^2 S <= 12288 is admitted, one more sample is not; entropy alone has no cap
    for P, S in ((16, 48), (8, 192), (2, 3072)):
        big = L.patch_reg(0.0, P, 1)
        assert P * P * S == L.INFO_KL_MAX_LDS_FLOATS
        assert _call(L, ok, patch=big, S=S + 1, n_rays=400) == EINVAL and b"NRF_INFO_KL_MAX_LDS_FLOATS" in L.lib().nrf_last_error()
        assert _finish(L, ok, patch=big, S=S + 1, n_rays=400) == EINVAL
    # NULL outputs where a term is on
    assert _call(L, ok, info_terms=None) == EINVAL and b"info_terms" in L.lib().nrf_last_error()
    assert _call(L, ok, patch_kl=None) == EINVAL and b"patch_kl" in L.lib().nrf_last_error()
    assert _finish(L, ok, info_terms=None) == EINVAL and _finish(L, ok, patch_kl=None) == EINVAL and _finish(L, ok, out=None) == EINVAL
    # everything the patch entry refuses
    assert _call(L, ok, patch=None) == EINVAL and _finish(L, ok, patch=None) == EINVAL
    assert _call(L, ok, patch=L.patch_reg(0.1, 1, 1)) == EINVAL and _call(L, ok, patch=L.patch_reg(0.1, 17, 1), n_rays=4000) == EINVAL
    assert _call(L, ok, patch=L.patch_reg(-0.1, 2, 1)) == EINVAL and _call(L, ok, patch=L.patch_reg(0.1, 2, -1)) == EINVAL
    assert _call(L, ok, patch=L.patch_reg(0.1, 2, 10)) == EINVAL and _finish(L, ok, patch=L.patch_reg(0.1, 2, 10)) == EINVAL
    assert _call(L, ok, patch_terms=None) == EINVAL
    assert _call(L, ok, S=0) == EINVAL and _call(L, ok, S=4097) == EINVAL and _call(L, ok, n_rays=0) == EINVAL
    assert _call(L, ok, reg=None) == EINVAL and _finish(L, ok, reg=None) == EINVAL
    assert _call(L, ok, reg=L.ray_reg(dist_weight=1.0, dist_inv_span=0.0)) == EINVAL
    assert _call(L, ok, reg=L.ray_reg(occ_weight=1.0, occ_samples=0)) == EINVAL
    assert _call(L, ok, lo=None) == EINVAL and _finish(L, ok, lo=None) == EINVAL
    assert _call(L, ok, lo=L.loss_opts(rgb_weight=-1.0)) == EINVAL and _finish(L, ok, lo=L.loss_opts(rgb_weight=-1.0)) == EINVAL
    assert _call(L, ok, slot=4098) == EINVAL and b"aligned" in L.lib().nrf_last_error()


# ---------------------------------------------------------------------------------------------
# 4. FusedStep and train_cli
# ---------------------------------------------------------------------------------------------
def _model():
    import nerf_few_shot_limitations_amd as N
    return N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2)


def test_fused_step_takes_the_keywords_and_refuses_bad_ones():
    from nerf_few_shot_limitations_amd.training import FusedStep
    p = inspect.signature(FusedStep.__init__).parameters
    assert [p[k].default for k in ("ent_weight", "ent_threshold", "kl_weight")] == [0.0, 0.01, 0.0]
    m = _model()
    plain = FusedStep(m)
    assert not plain.info_reg and not plain.patch_reg and not plain.ray_reg
    s = FusedStep(m, ent_weight=1e-3)
    assert s.info_reg and not s.patch_reg and (s.ent_weight, s.ent_threshold, s.kl_weight) == (1e-3, 0.01, 0.0)
    k = FusedStep(m, kl_weight=1e-5, ent_threshold=0.05, patch_size=4)
    assert k.info_reg and not k.patch_reg and (k.kl_weight, k.ent_threshold, k.patch_size) == (1e-5, 0.05, 4)
    for bad in (dict(ent_weight=-1e-3), dict(ent_weight=float("nan")), dict(ent_weight=float("inf")), dict(kl_weight=-1.0),
                dict(kl_weight=float("nan")), dict(kl_weight=float("inf")), dict(ent_threshold=-0.1), dict(ent_threshold=float("nan"))):
        with pytest.raises(ValueError):
            FusedStep(m, **bad)


def test_patch_counts_with_the_terms_are_checked_on_the_host():
    from nerf_few_shot_limitations_amd.training import FusedStep
    plain, ent, kl = FusedStep(_model()), FusedStep(_model(), ent_weight=0.1, patch_size=2), FusedStep(_model(), kl_weight=0.1, patch_size=2)
    with pytest.raises(ValueError):
        plain._patch_check(40, 1)                              # still refused when all three weights are 0
    assert ent._patch_check(40, 0) == 40 and ent._patch_check(40, 9) == 4 and kl._patch_check(40, 9) == 4
    with pytest.raises(ValueError, match="kl_weight"):
        kl._patch_check(40, 0)                                 # the KL term has no patch to act on
    for bad in (-1, 10, 11):
        with pytest.raises(ValueError):
            ent._patch_check(40, bad)


def test_the_hierarchical_steps_refuse_both_weights_and_step_view_the_kl():
    from nerf_few_shot_limitations_amd.training import FusedStep
    o = torch.zeros(4, 3)
    for kw in (dict(ent_weight=0.1), dict(kl_weight=0.1)):
        s = FusedStep(_model(), **kw)
        with pytest.raises(ValueError, match="ent_weight or kl_weight"):
            s.step_rays_hierarchical(o, o, o, 2.0, 6.0, 8, 4)
        with pytest.raises(ValueError, match="ent_weight or kl_weight"):
            s.step_view_hierarchical(None, None, 4, 4, 1.0, None, 2.0, 6.0, 8, 4)
    with pytest.raises(ValueError, match="kl_weight"):
        FusedStep(_model(), kl_weight=0.1).step_view(None, None, 4, 4, 1.0, None, 2.0, 6.0, 8)
    with pytest.raises(ValueError, match="pixels"):              # ent_weight alone passes that refusal and meets the next one
        FusedStep(_model(), ent_weight=0.1).step_view(None, None, 4, 4, 1.0, None, 2.0, 6.0, 8)


def test_train_cli_flags_and_refusals():
    from nerf_few_shot_limitations_amd import train_cli
    ns = lambda **kw: argparse.Namespace(**{**dict(entropy_weight=0.0, entropy_threshold=None, entropy_unseen=False, kl_weight=0.0, depth_smooth_weight=0.0,
                                                   patch_size=8, patches_per_step=16, patch_stride=1, n_importance=0, fused_inputs=False, occupancy_res=0,
                                                   occupancy_per_view=False, train_extractor=False), **kw})
    err, opts, draws = train_cli.info_reg_args_error, train_cli.info_reg_options, train_cli.draws_patches
    assert err(ns()) is None and err(argparse.Namespace()) is None and opts(ns()) == {} and not draws(ns())
    # the entropy flag: --dist-weight's refusals, and it goes with the routes --dist-weight goes with
    assert err(ns(entropy_weight=0.1)) is None and err(ns(entropy_weight=0.1, fused_inputs=True)) is None
    assert err(ns(entropy_weight=0.1, occupancy_res=64)) is None and err(ns(entropy_weight=0.1, train_extractor=True)) is None
    assert "--n-importance" in err(ns(entropy_weight=0.1, n_importance=8))
    assert err(ns(entropy_weight=-1.0)) is not None and err(ns(entropy_weight=float("nan"))) is not None and err(ns(kl_weight=-1.0)) is not None
    assert "--entropy-threshold" in err(ns(entropy_weight=0.1, entropy_threshold=-0.5)) and "--entropy-threshold" in err(ns(entropy_threshold=0.1))
    assert "--entropy-weight" in err(ns(entropy_unseen=True))
    assert opts(ns(entropy_weight=0.1)) == dict(ent_weight=0.1, ent_threshold=0.01, kl_weight=0.0) and not draws(ns(entropy_weight=0.1))
    assert opts(ns(entropy_weight=0.1, entropy_threshold=0.05, entropy_unseen=True, patch_size=4)) == dict(ent_weight=0.1, ent_threshold=0.05, kl_weight=0.0, patch_size=4)
    assert draws(ns(entropy_weight=0.1, entropy_unseen=True)) and draws(ns(kl_weight=0.1)) and draws(ns(depth_smooth_weight=0.1))
    # the KL flag and --entropy-unseen draw patches: --depth-smooth-weight's refusals
    for on in (dict(kl_weight=0.1), dict(entropy_weight=0.1, entropy_unseen=True)):
        assert err(ns(**on)) is None and err(ns(**on, patch_size=4, patches_per_step=3, patch_stride=2)) is None
        assert "--n-importance" in err(ns(**on, n_importance=8))
        assert "--fused-inputs" in err(ns(**on, fused_inputs=True))
        assert "--occupancy" in err(ns(**on, occupancy_res=64)) and "--occupancy" in err(ns(**on, occupancy_warmup=4))
        assert "--occupancy" in err(ns(**on, occupancy_per_view=True))
        assert "--train-extractor" in err(ns(**on, train_extractor=True))
        assert "--patch-size" in err(ns(**on, patch_size=1)) and "--patch-size" in err(ns(**on, patch_size=17))
        assert "--patches-per-step" in err(ns(**on, patches_per_step=0)) and "--patch-stride" in err(ns(**on, patch_stride=0))
    assert opts(ns(kl_weight=0.2, patch_size=4)) == dict(ent_weight=0.0, ent_threshold=0.01, kl_weight=0.2, patch_size=4)
    # with --depth-smooth-weight the patch size is handed over once
    both = ns(kl_weight=0.2, depth_smooth_weight=0.1, patch_size=4)
    assert "patch_size" not in opts(both) and train_cli.patch_reg_options(both)["patch_size"] == 4
    # the command refuses before it reads a config or a data set
    for flag, more in (("--n-importance", ["--entropy-weight", "0.1", "--n-importance", "8"]), ("--n-importance", ["--kl-weight", "0.1", "--n-importance", "8"]),
                       ("--fused-inputs", ["--kl-weight", "0.1", "--fused-inputs"]), ("--occupancy", ["--kl-weight", "0.1", "--occupancy-res", "64"]),
                       ("--train-extractor", ["--kl-weight", "0.1", "--train-extractor"]),
                       ("--fused-inputs", ["--entropy-weight", "0.1", "--entropy-unseen", "--fused-inputs"]),
                       ("--entropy-weight", ["--entropy-unseen"])):
        with pytest.raises(SystemExit, match=flag):
            train_cli.main(["--config", "/nonexistent.yaml", "--data", "/nonexistent", *more])
    doc = " ".join(train_cli.__doc__.split())
    for word in ("--entropy-weight W", "--entropy-threshold T", "--entropy-unseen", "--kl-weight W", "InfoNeRF", "nrf_info_reg"):
        assert word in doc, word


# ---------------------------------------------------------------------------------------------
# 5. the new unit's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from nerf_few_shot_limitations_amd import build as B
    sub = os.path.join(B.OBJ, B.INFO_REG_DIR)
    if not os.path.isdir(sub) or not any(f.endswith(".o.remarks") for f in os.listdir(sub)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B


NEW = ("info_loss_backward_kernel<false, false>", "info_loss_backward_kernel<false, true>", "info_loss_backward_kernel<true, false>",
       "info_loss_backward_kernel<true, true>", "info_terms_finish_kernel")


def test_new_kernels_match_their_census_and_spill_nothing(B):
    res = B.kernel_resources(os.path.join(B.OBJ, B.INFO_REG_DIR))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_info_reg.json")))
    fields = gold["fields"]
    assert set(res) == set(gold["kernels"]) and len(res) == len(NEW), sorted(res)
    for kernel in NEW:
        (name, r), = [(k, v) for k, v in res.items() if "::" + kernel + "(" in k]
        print(kernel, r)
        assert r["tu"] == "info_reg"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["agprs"] == 0, (name, r)
        assert [r.get(f, 0) for f in fields] == gold["kernels"][name], (name, dict(zip(fields, gold["kernels"][name])), r)


def test_the_unit_stays_out_of_the_main_census_and_the_pinned_tables(B):
    main = B.kernel_resources()
    assert not any(k.startswith("info_reg:") or "info_loss_backward_kernel" in k or "info_terms_finish_kernel" in k for k in main)
    for table in (B.SOURCES, B.SUBDIR_SOURCES, B.RAY_REG_SOURCES, B.FREQ_MASK_SOURCES, B.PATCH_REG_SOURCES):
        assert not any(src == "info_reg.hip" for src, *_ in table)
    assert [(src, name, sub) for src, name, _, sub in B.INFO_REG_SOURCES] == [("info_reg.hip", "info_reg", B.INFO_REG_DIR)]
    for other in (B.RAY_REG_DIR, B.PATCH_REG_DIR):
        assert not any("info_" in k for k in B.kernel_resources(os.path.join(B.OBJ, other)))
