"""Host-side checks of occupancy grids pruned by rendered weights (no GPU): the two marking entry points against their ctypes
declarations, their refusals before any launch, the grid algebra on CPU tensors, evaluate_cli's pruning flags, and the build's
resource figures of the marker kernels.

The refusals need neither a model nor a device: fake pointers and a NULL stream, as in tests/test_occupancy_host.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"nrf_occupancy_mark_rays": 14, "nrf_occupancy_mark_camera": 17}


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def test_header_ctypes_and_library_agree_on_the_entry_points(L):
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = L.lib()
    for name, n_args in ENTRIES.items():
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]) == n_args, name
        assert "uint32_t* hit_bits" in decl and "uint32_t* seen_bits" in decl and "float weight_threshold" in decl and "float seen_eps" in decl
        assert hasattr(lib, name)
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(5) == -1
    # the rule is documented next to the two existing builders
    doc = header[header.index("nrf_occupancy_dilate("):header.index("nrf_occupancy_mark_camera(")]
    for word in ("weight_threshold", "seen_eps", "floor", "NaN", "ORs into"):
        assert word in doc, word


def test_refusals_before_any_launch(L):
    lib = L.lib()
    i3, f3 = C.c_int32 * 3, C.c_float * 3
    c2w = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4)
    good = dict(o=0x1000, d=0x2000, n=8, S=16, z=0x3000, w=0x4000, res=(64, 48, 512), lo=(-1.0, -2.0, -3.0), scale=(8.0, 4.0, 2.0), tau=0.0,
                eps=0.01, hit=0x5000, seen=0x6000)

    def calls(**kw):
        a = {**good, **kw}
        box = (i3(*a["res"]), f3(*a["lo"]), f3(*a["scale"]))
        yield lib.nrf_occupancy_mark_rays(a["o"], a["d"], a["n"], a["S"], a["z"], a["w"], *box, a["tau"], a["eps"], a["hit"], a["seen"], None)
        if "o" in kw or "d" in kw:                                            # the camera entry has no ray pointers
            return
        yield lib.nrf_occupancy_mark_camera(1 << 16, 1 << 16, 100.0, c2w, 0, a["n"], a["S"], a["z"], a["w"], *box, a["tau"], a["eps"], a["hit"],
                                            a["seen"], None)

    def refused(word, **kw):
        n = 0
        for rc in calls(**kw):
            assert rc == -1, (word, kw, rc)                                    # NRF_EINVAL
            assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())
            n += 1
        assert n >= 1

    refused("null ray", o=None)
    refused("null ray", d=None)
    refused("z_vals or weights", z=None)
    refused("z_vals or weights", w=None)
    refused("both NULL", hit=None, seen=None)
    refused("4-byte aligned", hit=0x5002)
    refused("4-byte aligned", seen=0x6001)
    refused("4-byte aligned", hit=None, seen=0x6002)
    for res in ((0, 32, 32), (64, 513, 32), (64, 32, 0), (544, 32, 32)):
        refused("res must be in 1..512", res=res)
    refused("multiple of 32", res=(48, 32, 32))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused("scale", scale=(8.0, bad, 2.0))
    for bad in (float("inf"), float("nan")):
        refused("lo must be finite", lo=(0.0, 0.0, bad))
    refused("n_samples", S=0)
    refused("n_samples", S=-3)
    refused("2^31", n=1 << 31)
    for bad in (-1e-3, float("inf"), float("nan")):
        refused("weight_threshold", tau=bad)
    for bad in (-1e-3, 1.0, 2.0, float("nan")):
        refused("seen_eps", eps=bad)
    # the camera entry's own arguments
    box = (i3(*good["res"]), f3(*good["lo"]), f3(*good["scale"]))
    assert lib.nrf_occupancy_mark_camera(0, 8, 100.0, c2w, 0, 8, 16, 0x3000, 0x4000, *box, 0.0, 0.01, 0x5000, 0x6000, None) == -1
    assert b"camera" in lib.nrf_last_error()
    assert lib.nrf_occupancy_mark_camera(4, 4, 100.0, c2w, 3, 17, 16, 0x3000, 0x4000, *box, 0.0, 0.01, 0x5000, 0x6000, None) == -1
    assert b"ray range" in lib.nrf_last_error()
    # nothing to mark: NRF_OK without a launch, with either output alone too
    assert list(calls(n=0)) == [0, 0]
    assert list(calls(n=0, hit=None)) == [0, 0]
    assert list(calls(n=0, seen=None, eps=0.0, tau=0.5)) == [0, 0]


def test_grid_algebra_on_cpu_tensors():
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid as G
    rng = np.random.default_rng(5)
    lo, hi = (-1.0, -2.0, -3.0), (1.0, 2.0, 3.5)
    ma, mb = (torch.from_numpy(rng.random((3, 5, 64)) < p) for p in (0.4, 0.6))
    ma[1, 2, 31] = True                                                      # the sign bit of a word, in one operand only
    mb[1, 2, 31] = False
    a, b = G.from_mask(ma, lo, hi), G.from_mask(mb, lo, hi)
    for got, want in ((a & b, ma & mb), (a | b, ma | mb), (~a, ~ma), (~(a | b) | a, ~(ma | mb) | ma), (a & ~a, torch.zeros_like(ma))):
        assert isinstance(got, G) and got.bits.dtype == torch.int32 and got.bits.device.type == "cpu"
        assert (got.res, got.lo, got.hi, got.outside) == (a.res, a.lo, a.hi, a.outside)
        assert torch.equal(got.to_mask(), want)
        assert torch.equal(got.bits, G.from_mask(want, lo, hi).bits)
    assert torch.equal(a.to_mask(), ma) and torch.equal(b.to_mask(), mb)      # the operands are left alone
    for other in (G.from_mask(mb[:, :4], lo, hi),                             # res
                  G.from_mask(mb, lo, (1.0, 2.0, 3.0)),                       # box
                  G.from_mask(mb, (-1.5, -2.0, -3.0), hi),
                  G.from_mask(mb, lo, hi, outside=1)):                        # outside
        with pytest.raises(ValueError, match="same res"):
            a & other
        with pytest.raises(ValueError, match="same res"):
            a | other
    with pytest.raises(TypeError):
        a & mb


def test_evaluate_cli_carries_the_pruning_flags():
    from nerf_few_shot_limitations_amd import evaluate_cli
    base = ["--config", os.path.join(ROOT, "no_such_config.yaml"), "--data", "y"]
    flags = ["--occupancy-prune-views", "3", "--occupancy-weight-threshold", "1e-3", "--occupancy-seen-eps", "0.02", "--occupancy-unseen", "drop"]
    # parses: with the flags the command gets as far as reading the (missing) config
    with pytest.raises((FileNotFoundError, OSError)):
        evaluate_cli.main([*base, "--occupancy-res", "64", *flags])
    with pytest.raises((FileNotFoundError, OSError)):
        evaluate_cli.main([*base, "--occupancy-res", "64", "--occupancy-prune-views", "2"])
    # each of them needs --occupancy-res
    for k in range(0, len(flags), 2):
        with pytest.raises(SystemExit) as e:
            evaluate_cli.main([*base, *flags[k:k + 2]])
        assert "--occupancy-res" in str(e.value)
    with pytest.raises(SystemExit):
        evaluate_cli.main([*base, "--occupancy-res", "64", "--occupancy-unseen", "maybe"])
    with pytest.raises(SystemExit):
        evaluate_cli.main([*base, "--occupancy-res", "64", "--occupancy-prune-views", "-1"])
    # the three settings do nothing without --occupancy-prune-views: refused, not ignored
    for k in range(2, len(flags), 2):
        with pytest.raises(SystemExit) as e:
            evaluate_cli.main([*base, "--occupancy-res", "64", *flags[k:k + 2]])
        assert "--occupancy-prune-views" in str(e.value)
    # out-of-range values are refused with the arguments, before the config is read
    for flag, bad in (("--occupancy-weight-threshold", "-1e-3"), ("--occupancy-weight-threshold", "nan"), ("--occupancy-weight-threshold", "inf"),
                      ("--occupancy-seen-eps", "1.0"), ("--occupancy-seen-eps", "-0.1"), ("--occupancy-seen-eps", "nan")):
        with pytest.raises(SystemExit) as e:
            evaluate_cli.main([*base, "--occupancy-res", "64", "--occupancy-prune-views", "2", f"{flag}={bad}"])
        assert flag in str(e.value)


def test_marker_kernels_use_no_scratch_and_spill_nothing():
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    marks = {n: r for n, r in B.kernel_resources().items() if "occupancy_mark_kernel" in n}
    assert len(marks) == 2, sorted(marks)                                      # explicit rays, camera rays
    for name, r in marks.items():
        print(name, r)
        assert r["tu"] == "staged_kernels"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
