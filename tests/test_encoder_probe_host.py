"""CPU tests of the encoder probe (tests/encoder_probe.py; its GPU half is tests/test_gpu_encoder_probe.py): the fp32 model of
encode3's reductions keeps what nets.hpp claims, the input set contains what it promises, every planted fault is reported at its
feature and at no unrelated one, and the selector networks are exact wires in the oracle.

RECORD (the model, fp32 numpy with nets.hpp's constants; a record, not a bound):
  path 2 (polynomial), worst |a - e| on the 1531 probe points: 1.83e-07 at L = 10 and at L = 12 (sin, f = 6), 0.915 of the
  documented 2e-7; on 200 001 points of |x| <= 8 at every f <= 13: 1.82e-07 (f = 12), 1.80e-07 at f = 13.  The claim of nets.hpp and
  DESIGN.md ("<= 2e-7 (1.9e-7)") stands for the model.
  path 1 (turns + float64 sine), rounded to the operand type, worst |a - q(e)| / bound of the encoder-stage rule: f16 0.985, bf16 0.842.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import encoder_probe as E


@pytest.fixture(scope="module")
def pts():
    return E.probe_points()


def claim_only(e):
    return np.full_like(e, E.CLAIM)


def path1(points, L, mode, **fault):
    return O.quantize(torch.from_numpy(E.encode_model(points, L, 1, **fault)).float(), mode).double().numpy()


def test_probe_points_are_fixed_and_ragged(pts):
    assert pts.shape == (E.N_POINTS, 3) and pts.dtype == np.float32
    assert E.N_POINTS % 32 and E.N_POINTS % 64
    assert np.array_equal(pts.view(np.uint32), E.probe_points().view(np.uint32))
    assert float(np.abs(pts).max()) == 8.0
    d = E.probe_dirs()
    assert d.shape == pts.shape and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.array_equal(d[:6], np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32))


def test_probe_points_contain_what_they_promise(pts):
    x64 = pts.astype(np.float64)
    ulp = np.spacing(np.abs(pts)).astype(np.float64)
    for c in range(3):
        col = pts[:, c]
        for v in (0.0, 2.0 ** -130, 1e-3, 8.0):
            assert (col == np.float32(v)).any() and (col == np.float32(-v)).any(), (c, v)
        assert (np.signbit(col) & (col == 0)).any(), "-0"
    seams = np.zeros(pts.shape, bool)
    for f in range(12):
        step = np.pi / 2 ** f
        far = np.abs(x64) > 2.0 ** -20                  # not the trivial zero at the origin
        sin0 = (np.abs(x64 - np.rint(x64 / step) * step) <= 4 * ulp) & far
        cos0 = (np.abs(x64 - (np.floor(x64 / step) + 0.5) * step) <= 4 * ulp) & far
        assert sin0.sum(0).min() >= 6 and cos0.sum(0).min() >= 6, (f, sin0.sum(0), cos0.sum(0))      # 2 k x 3 neighbours per component
        assert (sin0 & (np.abs(x64) > 4)).any() and (cos0 & (np.abs(x64) > 4)).any(), f
        turns = x64 * 2 ** f / (2 * np.pi)
        whole = (np.abs(x64 - np.rint(turns) * 2 * np.pi / 2 ** f) <= 4 * ulp) & (np.abs(x64) > 1)
        assert whole.sum(0).min() >= 2, (f, whole.sum(0))        # a whole turn count away from the origin: path 1's fract seam
        seams |= np.abs(turns - np.floor(turns) - 0.5) < 2.0 ** -20
    assert seams.sum(0).min() >= 20, seams.sum(0)       # 4 seams x 5 neighbours per component (and the odd zeros of sin)
    assert (np.abs(pts) > 4).any(1).sum() >= 400
    hi = pts * E.INV2PI_HI
    for j in range(-6, 1):                              # both sides of hi = 2^j
        near = np.abs(np.abs(hi.astype(np.float64)) - 2.0 ** j) < 2.0 ** (j - 20)
        assert (near & (np.abs(hi) >= 2.0 ** j)).sum(0).min() >= 1 and (near & (np.abs(hi) < 2.0 ** j)).sum(0).min() >= 1, j


@pytest.mark.parametrize("L", [10, 12])
def test_model_of_path_2_keeps_the_documented_claim(pts, L):
    findings = E.compare(E.encode_model(pts, L, 2), pts, L, claim_only)
    print("\n" + E.record(f"model path 2 L {L} (bound = the claim, 2e-7)", findings))
    assert len(findings) == E.n_features(L) and not E.failed(findings), E.failed(findings)


def test_model_of_path_2_keeps_the_claim_up_to_2_to_the_14():
    x = np.linspace(-8, 8, 200001).astype(np.float32)
    sweep = np.stack([x, x[::-1].copy(), np.roll(x, 777)], 1)
    findings = E.compare(E.encode_model(sweep, 14, 2), sweep, 14, claim_only)
    top = [f for f in findings if f.feature[1] == 13]
    print("\n" + E.record("model path 2, 200001 points of |x| <= 8, every f <= 13", findings))
    print(E.record("model path 2, the same at f = 13", top))
    assert not E.failed(findings), E.failed(findings)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_model_of_path_1_keeps_the_encoder_stage_rule(pts, mode):
    for L in (10, 12):
        findings = E.compare(path1(pts, L, mode), pts, L, lambda e: E.bound(e, mode, "v2"), lambda e: E.target(e, mode))
        print("\n" + E.record(f"model path 1 {mode} L {L}", findings))
        assert not E.failed(findings), E.failed(findings)


def flagged(pts, trig, fault, fault_f=None):
    """Features that `compare` reports for a fault planted in the model: path 2 under the claim, path 1 under f16's rule."""
    if trig == 2:
        f = E.compare(E.encode_model(pts, 12, 2, fault, fault_f), pts, 12, claim_only)
    else:
        f = E.compare(path1(pts, 12, "f16", fault=fault, fault_f=fault_f), pts, 12, lambda e: E.bound(e, "f16", "v2"),
                      lambda e: E.target(e, "f16"))
    return {x.feature for x in E.failed(f)}


def band(f, kinds=("sin", "cos"), comps=(0, 1, 2)):
    return {(k, f, c) for k in kinds for c in comps}


@pytest.mark.parametrize("trig", [1, 2])
@pytest.mark.parametrize("fault", ["no_inv2pi_lo", "no_lo"])
def test_a_dropped_low_part_is_reported_at_the_top_bands(pts, trig, fault):
    """The phase error is (the dropped part of the turn count) 2^f: at most 8 kInv2PiLo 2^f 2 pi rad for kInv2PiLo, and for the whole
    low part that plus the rounding of hi, 2^-24 x 1.28 turns.  No band where that stays below the smallest bound may be reported."""
    got = flagged(pts, trig, fault)
    assert band(11) <= got and band(10) <= got, sorted(got)
    dropped = 8 * float(E.INV2PI_LO) + (2.0 ** -24 * 1.28 if fault == "no_lo" else 0.0)
    floor = E.CLAIM if trig == 2 else 2.0 ** -10 * 2.0 ** -4
    for kind, f, _ in got:
        assert kind != "raw" and 2 * np.pi * dropped * 2 ** f > 0.5 * floor, (kind, f)      # 0.5: the fault adds to the path's own error


def test_truncation_in_place_of_rint_is_reported(pts):
    got = flagged(pts, 2, "trunc")
    assert not any(k == "raw" for k, _, _ in got)
    assert all(band(f, ("cos",)) <= got for f in range(12)), sorted(got)          # a turn count in (1/2, 1) leaves the fold's range


@pytest.mark.parametrize("trig", [1, 2])
@pytest.mark.parametrize("fault,where", [("wrong_quarter", band(7)), ("swap_yz", band(7, comps=(1, 2))), ("freq_off_by_one", band(7)),
                                         ("wrong_quarter", band(0)), ("swap_yz", band(11, comps=(1, 2))), ("freq_off_by_one", band(11))])
def test_a_fault_in_one_band_is_reported_there_and_nowhere_else(pts, trig, fault, where):
    f = next(iter(where))[1]
    assert flagged(pts, trig, fault, f) == where


def test_the_unfaulted_model_reports_nothing(pts):
    assert flagged(pts, 1, None) == set() and flagged(pts, 2, None) == set()


def test_compare_leaves_no_element_out(pts):
    m = E.encode_model(pts, 10, 2)
    for i, j in ((0, 0), (E.N_POINTS - 1, E.n_features(10) - 1), (777, 31)):
        bad = m.copy()
        bad[i, j] += 1e-3
        f = E.failed(E.compare(bad, pts, 10, claim_only))
        assert [(x.feature, x.index) for x in f] == [(E.feature_name(j), i)]
    bad = m.copy()
    bad[5, 5] = np.nan
    assert [x.index for x in E.failed(E.compare(bad, pts, 10, claim_only))] == [5]
    with pytest.raises(AssertionError):
        E.compare(m[:-1], pts, 10, claim_only)


# ---------------------------------------------------------------------------------------------
# the selector networks are exact wires in the oracle (float64 weights on the float64 encoding)
# ---------------------------------------------------------------------------------------------
def to64(p):
    return {k: v.double() for k, v in p.items()}


def test_v2_selector_is_an_exact_wire(pts):
    p = to64(E.v2_selector())
    pe = O.positional_encoding64(torch.from_numpy(pts), 10)
    for k in range(E.n_features(10)):
        d = []
        for sign in (1.0, -1.0):
            p["density_mlp.density_head.weight"] = E.density_row(k, sign).double()
            d.append(O.density_mlp(p, "density_mlp.", pe)[0][:, 0])
        assert torch.equal(d[0] - d[1], pe[:, k]) and bool(((d[0] == 0) | (d[1] == 0)).all()), k


def test_v3_selector_is_an_exact_wire_and_its_gate_is_one_half(pts):
    p = to64(E.v3_selector())
    pe = O.positional_encoding64(torch.from_numpy(pts), 12)
    dino = torch.from_numpy(O.uniform01(9, E.N_POINTS * 64).reshape(-1, 64)).double() * 2 - 1
    x = torch.cat([pe, dino], -1)
    h = torch.relu(O._lin(p, "dino_fusion.fusion.2", torch.relu(O._lin(p, "dino_fusion.fusion.0", x))))
    w = torch.softmax(O._lin(p, "dino_fusion.attention.2", torch.relu(O._lin(p, "dino_fusion.attention.0", h))), -1)
    assert bool((w == 0.5).all())
    fused = O.dino_fusion(p, "dino_fusion.", pe, dino)
    for k in range(E.n_features(12)):
        d = []
        for sign in (1.0, -1.0):
            p["density_mlp.density_head.weight"] = E.density_row(k, sign).double()
            d.append(O.density_mlp(p, "density_mlp.", fused)[0][:, 0])
        assert torch.equal(d[0] - d[1], pe[:, k]), k


def test_direction_selector_is_an_exact_wire():
    p = to64(E.v2_selector())
    de = O.positional_encoding64(torch.from_numpy(E.probe_dirs()), 4)
    assert float(de.abs().max()) <= 1.0                                            # the sigmoid's slope bound holds on |e| <= 1
    feat = torch.zeros(E.N_POINTS, 256, dtype=torch.float64)
    for t in range(E.n_features(4) // 3):
        p["color_mlp.color_layers.4.weight"] = E.colour_rows(t).double()
        rgb = O.color_mlp(p, "color_mlp.", feat, de)
        assert float((rgb - torch.sigmoid(de[:, 3 * t: 3 * t + 3])).abs().max()) <= 2.0 ** -52, t      # the logits are equal; torch's vector and scalar sigmoid differ in the last bit
        assert np.abs(E.logit64(rgb.numpy()) - de[:, 3 * t: 3 * t + 3].numpy()).max() < 1e-14


def test_v1_selector_is_an_exact_wire(pts):
    p = to64(E.v1_selector())
    pe = O.positional_encoding64(torch.from_numpy(pts), 10)
    for t in range(E.n_features(10) // 3):
        p["rgb_out.weight"] = E.v1_rgb_rows(t).double()
        out = O.mlp_v1(p, pe)
        e = pe[:, 3 * t: 3 * t + 3] / (E.RAW_GAIN if t == 0 else 1.0)
        assert bool((out[:, 3] == 1.0).all())
        assert float((out[:, :3] - torch.sigmoid(e)).abs().max()) <= 2.0 ** -52, t
        assert np.abs(E.logit64(out[:, :3].numpy()) - e.numpy()).max() < 1e-14
        assert float(e.abs().max()) <= 1.0
