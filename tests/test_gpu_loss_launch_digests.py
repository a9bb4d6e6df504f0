"""The three regularised loss launches and their finish launches, held bit for bit to a record of their outputs (nerfhip.h:
nrf_composite_reg_loss_backward + nrf_ray_terms_finish, nrf_composite_patch_loss_backward + nrf_patch_terms_finish,
nrf_composite_info_loss_backward + nrf_info_terms_finish).

tests/golden/loss_launch_digests.json holds the SHA-256 of every output buffer of every case below, taken on an MI355X before the
batch walk, the finish body and the host derivations of these launches were each written once (csrc/loss_walk.hpp).  The launches
use no atomics and fix every order of summation, so the same inputs give the same bytes: a digest that moves is a change of the
arithmetic.  `python -m tests.test_gpu_loss_launch_digests` prints the JSON of the library it runs on.

Every regulariser weight is on, with a depth target and density noise from the in-kernel counter RNG (a fixed rng_seed).  The
inputs are drawn on the CPU from a seeded torch.Generator -- uniform draws in float64 and exact arithmetic on them only, so that
they do not depend on how a CPU vectorises a transcendental -- and copied over.  The shapes are the smallest at which each part of
the walk can still go wrong: S = 2 (one sample with a finite interval), 16 (one segment), 65 (two segments, the second ragged), 130
(three); P = 2 (P^2 = the waves of a workgroup), 3 (ragged over them), 16 (the whole depth array); 37 supervised rays (the last
group holds one); with and without patches (the two instantiations of the compositor bodies); dense and compacted rows; both
backgrounds; the KL term wherever its rows fit in LDS (at P = 16: S = 48), the info entry also with both of its weights 0 and with
the entropy alone."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_launch_digests.json")
N_SUP = 37
ZERO_N = 1000
RNG_SEED = 0x5EED1234ABCD
W = dict(rgb=0.7, depth=0.3, reg=0.5, std=0.4, dist=0.6, kappa=0.25, occ=0.8, occ_k=5, smooth=0.9, ent=0.7, tau=0.01, kl=1.3)


def _case(entry, S, P=3, n_p=0, idx=False, white=0, ent=True, kl=None):
    kl = (entry == "info" and n_p > 0) if kl is None else kl
    return dict(entry=entry, S=S, P=P, n_p=n_p, idx=idx, white=white, ent=ent, kl=kl)


CASES = [
    _case("reg", 2), _case("reg", 16, idx=True, white=1), _case("reg", 65, white=1), _case("reg", 130, idx=True),
    _case("patch", 2, 2, 3), _case("patch", 16, 3, 3, idx=True, white=1), _case("patch", 65, 3, 0, white=1), _case("patch", 65, 3, 0, idx=True),
    _case("patch", 130, 2, 3, idx=True), _case("patch", 130, 3, 3, white=1), _case("patch", 16, 16, 3),
    _case("info", 2, 2, 3), _case("info", 16, 3, 3, idx=True, white=1), _case("info", 65, 3, 3, white=1), _case("info", 65, 2, 3, idx=True),
    _case("info", 130, 2, 3, idx=True), _case("info", 130, 3, 3), _case("info", 48, 16, 3, white=1), _case("info", 48, 16, 3, idx=True),
    _case("info", 65, 3, 0, idx=True), _case("info", 16, 3, 0, white=1),                                   # no patches: the entropy on every ray
    _case("info", 65, 3, 3, ent=False, kl=False), _case("info", 130, 3, 3, idx=True, white=1, kl=False),   # both weights 0; the entropy alone
]


def case_id(c):
    """The entry and the parameters that mean something to it: the reg entry has no patches, only the info entry the two flags."""
    patch = "" if c["entry"] == "reg" else f"-P{c['P']}-np{c['n_p']}"
    info = f"-ent{int(c['ent'])}-kl{int(c['kl'])}" if c["entry"] == "info" else ""
    return f"{c['entry']}-S{c['S']}{patch}-{'idx' if c['idx'] else 'dense'}-white{c['white']}{info}"


def inputs(c, number):
    """The case's inputs on the CPU: uniform float64 draws of one seeded generator, exact arithmetic, rounded to fp32 once."""
    g = torch.Generator().manual_seed(20240 + number)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    S, PP = c["S"], c["P"] * c["P"]
    R = N_SUP + c["n_p"] * PP
    rgb = u(R, S, 3)
    sig = u(R, S) * 8.0 - 2.0                                # a quarter of the samples fail the ReLU
    sig[::5] -= 100.0                                        # every fifth ray is empty: under the entropy threshold
    sig[1::7] += 30.0                                        # some are opaque
    z = 2.0 + 4.0 * (torch.cumsum(u(R, S) + 0.05, dim=1) / (S * 1.05))
    d = u(R, 3) * 2.0 - 1.0 + 0.25
    tgt, tdepth = u(N_SUP, 3), u(N_SUP) * 4.0 + 2.0
    keep = u(R, S) > 1.0 / 3.0
    keep[3] = False                                          # a ray with every sample skipped
    keep[-1, : S // 2] = False
    f = lambda t: t.float().contiguous()
    return R, f(rgb), f(sig), f(z), f(d), f(tgt), f(tdepth), keep


def run(L, c, number):
    """The case's launch and its finish -> {buffer name: tensor on the CPU}"""
    lib, st = L.lib(), L.stream_ptr()
    R, rgb, sig, z, d, tgt, tdepth, keep = inputs(c, number)
    S, P, n_p = c["S"], c["P"], c["n_p"]
    rows_rgb, rows_sig, sl = rgb.reshape(-1, 3), sig.reshape(-1), None
    if c["idx"]:
        flat = keep.reshape(-1)
        slot = torch.full((flat.numel(),), -1, dtype=torch.int32)
        slot[flat] = torch.arange(int(flat.sum()), dtype=torch.int32)
        rows_rgb, rows_sig, sl = rows_rgb[flat].contiguous(), rows_sig[flat].contiguous(), slot.cuda()
    dev = [t.cuda() for t in (rows_rgb, rows_sig, z, d, tgt, tdepth)]
    c_rgb, c_sig, c_z, c_d, c_tgt, c_td = dev
    rows = c_rgb.shape[0]
    fill = lambda *shape: torch.full(shape, 7.0, device="cuda")
    out = dict(pred=fill(R, 3), d_rgb=fill(rows, 3), d_sigma=fill(rows), ray_terms=fill(5, R), zero=fill(ZERO_N))
    lo = L.loss_opts(W["rgb"], W["reg"], W["depth"], L.ptr(c_td), W["std"], None, RNG_SEED)
    reg = L.ray_reg(W["dist"], W["kappa"], W["occ"], W["occ_k"])
    head = (L.ptr(c_rgb), 3, L.ptr(c_sig), 1, L.ptr(c_z), L.ptr(c_d), R, S, c["white"], L.ptr(c_tgt), C.byref(lo), C.byref(reg),
            None if sl is None else sl.data_ptr(), L.ptr(out["pred"]), L.ptr(out["d_rgb"]), 3, L.ptr(out["d_sigma"]), 1, L.ptr(out["ray_terms"]),
            L.ptr(out["zero"]), ZERO_N, st)
    if c["entry"] == "reg":
        assert R == N_SUP
        L.check(lib.nrf_composite_reg_loss_backward(*head))
        p, g, m, v = (torch.zeros(4, device="cuda") for _ in range(4))
        l4 = fill(4)
        out["losses"] = fill(6)
        L.check(lib.nrf_adamw_step_loss(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0.0, None, None,
                                        L.ptr(out["ray_terms"]), R, S, W["rgb"], W["depth"], W["reg"], L.ptr(l4), st))
        L.check(lib.nrf_ray_terms_finish(L.ptr(out["ray_terms"]), R, C.byref(reg), L.ptr(l4), L.ptr(out["losses"]), st))
    else:
        patch = L.patch_reg(W["smooth"], P, n_p)
        out["patch_terms"], out["patch_depth"] = fill(max(n_p, 1)), fill(max(n_p, 1) * P * P)
        tail = (C.byref(patch), L.ptr(out["patch_terms"]), L.ptr(out["patch_depth"]))
        if c["entry"] == "patch":
            L.check(lib.nrf_composite_patch_loss_backward(*head, *tail))
            out["losses"] = fill(7)
            L.check(lib.nrf_patch_terms_finish(L.ptr(out["ray_terms"]), R, S, C.byref(lo), C.byref(reg), C.byref(patch), L.ptr(out["patch_terms"]),
                                               L.ptr(out["losses"]), st))
        else:
            info = L.info_reg(W["ent"] if c["ent"] else 0.0, W["tau"], W["kl"] if c["kl"] else 0.0)
            out["info_terms"], out["patch_kl"] = fill(R), fill(max(n_p, 1))
            L.check(lib.nrf_composite_info_loss_backward(*head, *tail, C.byref(info), L.ptr(out["info_terms"]), L.ptr(out["patch_kl"])))
            out["losses"] = fill(9)
            L.check(lib.nrf_info_terms_finish(L.ptr(out["ray_terms"]), R, S, C.byref(lo), C.byref(reg), C.byref(patch), L.ptr(out["patch_terms"]),
                                              C.byref(info), L.ptr(out["info_terms"]), L.ptr(out["patch_kl"]), L.ptr(out["losses"]), st))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def digests(out):
    return {k: hashlib.sha256(v.contiguous().numpy().tobytes()).hexdigest() for k, v in out.items()}


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib as L
    L.lib()
    return L


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_cover_the_walk():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for entry in ("patch", "info"):
        cs = [c for c in CASES if c["entry"] == entry]
        assert {c["S"] for c in cs} >= {2, 65, 130} and {c["P"] for c in cs} == {2, 3, 16}
        assert {(c["n_p"] > 0, c["idx"]) for c in cs} == {(a, b) for a in (False, True) for b in (False, True)}       # the four instantiations
    assert {c["S"] for c in CASES if c["entry"] == "reg"} == {2, 16, 65, 130}
    for c in CASES:
        assert not c["kl"] or (c["n_p"] > 0 and c["P"] ** 2 * c["S"] <= 12288)
        assert c["entry"] != "info" or c["n_p"] == 0 or c["kl"] or c in CASES[-2:], "the KL term is on wherever its rows fit"


@pytest.mark.parametrize("number", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_outputs_are_the_recorded_bits(L, golden, number):
    c = CASES[number]
    assert case_id(c) in golden, "every case has a record"
    want = golden[case_id(c)]
    out = run(L, c, number)
    assert torch.all(out["zero"] == 0) and all(torch.isfinite(v).all() for v in out.values())
    got = digests(out)
    keys = {"pred", "d_rgb", "d_sigma", "ray_terms", "zero", "losses"}
    keys |= set() if c["entry"] == "reg" else {"patch_terms", "patch_depth"}
    keys |= {"info_terms", "patch_kl"} if c["entry"] == "info" else set()
    assert set(got) == keys and set(want) == keys
    moved = sorted(k for k in keys if got[k] != want[k])
    assert not moved, f"{case_id(c)}: {moved} differ from the record"


if __name__ == "__main__":
    from nerf_few_shot_limitations_amd import _lib

    _lib.lib()
    print(json.dumps({case_id(c): digests(run(_lib, c, i)) for i, c in enumerate(CASES)}, indent=1, sort_keys=True))
