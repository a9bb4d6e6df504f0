"""Host-side checks of empty-space skipping (no GPU): the C ABI struct and entry points against their ctypes declarations, the
refusals that answer before any launch, the bit layout of OccupancyGrid.from_mask on CPU tensors, evaluate_cli's flags, and the
build's resource figures of the skipping ray-queue kernels next to their plain siblings.

The refusals need no model: the grid and the ray count are looked at first (tests/test_train_rays_host.py does the same for the
ray-input training forward)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nrf_render_rays_occ", "nrf_render_camera_occ", "nrf_render_cameras_tiles_occ")


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def test_header_and_ctypes_agree_on_the_struct_and_the_entry_points(L):
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    lib = L.lib()
    body = re.search(r"typedef struct nrf_occupancy \{(.*?)\} nrf_occupancy;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.match(r".*?(\w+)(\[\d+\])?$", d.strip(), re.S).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f for f, _ in L.nrf_occupancy._fields_]
    assert fields == ["struct_bytes", "outside", "bits", "res", "lo", "scale", "stats"]
    T = L.nrf_occupancy
    assert C.sizeof(T) == 64 and T.bits.offset == 8 and T.res.offset == 16 and T.lo.offset == 28 and T.scale.offset == 40 and T.stats.offset == 56
    assert L.occupancy().struct_bytes == 64
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(3) == C.sizeof(L.nrf_render_opts) and lib.nrf_abi_sizeof(5) == -1
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        plain = re.search(r"\b" + name[:-4] + r"\s*\((.*?)\);", code, re.S).group(1)
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert "const nrf_occupancy* occ" in decl
        assert len(decl.split(",")) == len(plain.split(",")) + 1 == len(L.SIGNATURES[name][1])
        assert hasattr(lib, name)
    for name, n_args in (("nrf_occupancy_pack", 6), ("nrf_occupancy_dilate", 4)):
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]) == n_args and hasattr(lib, name)


def _opts(L, **kw):
    o = L.nrf_render_opts()
    o.near, o.far, o.n_samples, o.mma_mode = 2.0, 6.0, 16, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_refusals_before_any_launch(L):
    lib = L.lib()
    good = dict(bits=0x1000, res=(64, 48, 512), lo=(-1.0, -2.0, -3.0), scale=(8.0, 4.0, 2.0))
    c2w = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4)

    def calls(occ, n_rays=8):
        """The three entry points on a frame of n_rays rays, model == NULL."""
        ref = None if occ is None else C.byref(occ)
        o = _opts(L)
        yield lib.nrf_render_rays_occ(None, 0x2000, 0x3000, n_rays, C.byref(o), ref, 0x4000, 0x5000, None, None, None)
        yield lib.nrf_render_camera_occ(None, 1 << 16, 1 << 16, 100.0, c2w, 0, n_rays, C.byref(o), ref, 0x4000, 0x5000, None, None, None)
        yield lib.nrf_render_cameras_tiles_occ(None, 1 << 16, 1 << 16, 100.0, C.cast(c2w, C.c_void_p), 1, n_rays, 0, 1, 1, C.byref(o), ref,
                                               0x4000, 0x5000, None, None, None)

    def refused(word, occ, **kw):
        for rc in calls(occ, **kw):
            assert rc == -1, (word, rc)                                            # NRF_EINVAL
            assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())

    refused("occ is NULL", None)
    short = L.occupancy(**good)
    short.struct_bytes = 56
    refused("struct_bytes", short)
    refused("outside", L.occupancy(**good, outside=2))
    refused("outside", L.occupancy(**good, outside=-1))
    refused("bits", L.occupancy(**{**good, "bits": None}))
    refused("bits", L.occupancy(**{**good, "bits": 0x1002}))
    for res in ((0, 32, 32), (64, 513, 32), (64, 32, 0), (544, 32, 32)):
        refused("res must be in 1..512", L.occupancy(**{**good, "res": res}))
    refused("multiple of 32", L.occupancy(**{**good, "res": (48, 32, 32)}))
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused("scale", L.occupancy(**{**good, "scale": (8.0, bad, 2.0)}))
    for bad in (float("inf"), float("nan")):
        refused("lo must be finite", L.occupancy(**{**good, "lo": (0.0, 0.0, bad)}))
    refused("2^31", L.occupancy(**good), n_rays=1 << 31)
    # everything the grid and the ray count decide is in order: the next thing looked at is the model
    refused("model is NULL", L.occupancy(**good))
    refused("model is NULL", L.occupancy(**good, outside=1, stats=0x6000), n_rays=(1 << 31) - 1)
    # the two builders
    assert lib.nrf_occupancy_pack(0x1000, 48, 1, 0.0, 0x2000, None) == -1 and b"multiple of 32" in lib.nrf_last_error()
    assert lib.nrf_occupancy_pack(0x1000, 64, 0, 0.0, 0x2000, None) == -1
    assert lib.nrf_occupancy_pack(None, 64, 1, 0.0, 0x2000, None) == -1 and b"null" in lib.nrf_last_error()
    assert lib.nrf_occupancy_pack(None, 0, 1, 0.0, None, None) == 0
    res = (C.c_int32 * 3)(48, 8, 8)
    assert lib.nrf_occupancy_dilate(0x1000, res, 0x2000, None) == -1 and b"multiple of 32" in lib.nrf_last_error()
    res = (C.c_int32 * 3)(64, 8, 8)
    assert lib.nrf_occupancy_dilate(0x1000, res, 0x1000, None) == -1
    assert lib.nrf_occupancy_dilate(None, res, 0x1000, None) == -1


def test_from_mask_bit_layout_on_cpu_tensors():
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    rz, ry, rx = 3, 5, 64
    rng = np.random.default_rng(3)
    mask = rng.random((rz, ry, rx)) < 0.4
    mask[1, 2, 31] = True                                                   # the sign bit of a word
    mask[2, 4, 63] = True
    g = OccupancyGrid.from_mask(torch.from_numpy(mask), (-1.0, -2.0, -3.0), (1.0, 2.0, 3.0))
    assert g.res == (rx, ry, rz) and g.bits.dtype == torch.int32 and g.bits.numel() == rz * ry * rx // 32
    words = g.bits.numpy().view(np.uint32)
    for iz, iy, ix in ((0, 0, 0), (1, 2, 31), (2, 4, 63), (2, 0, 33), (1, 4, 5)):
        index = (iz * ry + iy) * rx + ix
        assert bool((words[index >> 5] >> np.uint32(index & 31)) & 1) == bool(mask[iz, iy, ix]), (iz, iy, ix)
    assert torch.equal(g.to_mask(), torch.from_numpy(mask))
    assert torch.equal(OccupancyGrid.from_mask(g.to_mask(), g.lo, g.hi).bits, g.bits)
    assert abs(g.occupied_fraction - mask.mean()) < 1e-6
    assert g.scale == (32.0, 1.25, 0.5)                                     # res / (hi - lo) in float32
    with pytest.raises(ValueError):
        OccupancyGrid.from_mask(torch.zeros((4, 4, 48), dtype=torch.bool), -1.0, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_mask(torch.zeros((4, 4, 32), dtype=torch.bool), 1.0, 1.0)
    with pytest.raises(ValueError):
        OccupancyGrid.from_mask(torch.zeros((4, 4, 32), dtype=torch.bool), -1.0, 1.0, outside=2)
    # the points a build probes: deterministic, sample 0 the cell centre, the rest inside the cell
    p = OccupancyGrid.cell_points((32, 4, 2), -1.0, 1.0, 32, 64, 3, seed=5)
    assert p.shape == (64, 3, 3) and torch.equal(p, OccupancyGrid.cell_points((32, 4, 2), -1.0, 1.0, 32, 64, 3, seed=5))
    assert not torch.equal(p[:, 1:], OccupancyGrid.cell_points((32, 4, 2), -1.0, 1.0, 32, 64, 3, seed=6)[:, 1:])
    size = torch.tensor([2 / 32, 2 / 4, 2 / 2])
    cell = torch.arange(32, 96)
    lo = -1.0 + torch.stack([cell % 32, (cell // 32) % 4, cell // 128], -1).float() * size
    assert torch.allclose(p[:, 0], lo + 0.5 * size)
    assert bool(((p >= lo[:, None] - 1e-6) & (p <= lo[:, None] + size + 1e-6)).all())


def test_evaluate_cli_carries_the_flags():
    from nerf_few_shot_limitations_amd import evaluate_cli
    flags = ["--occupancy-res", "64", "--occupancy-threshold", "0.5", "--occupancy-samples", "2", "--occupancy-dilate", "0",
             "--occupancy-box", "-1.5", "1.5"]
    # parses: with the flags the command gets as far as reading the (missing) config, without them too
    for extra in ([], flags):
        with pytest.raises((FileNotFoundError, OSError)):
            evaluate_cli.main(["--config", os.path.join(ROOT, "no_such_config.yaml"), "--data", "y", *extra])
    with pytest.raises(SystemExit):
        evaluate_cli.main(["--config", "x", "--data", "y", "--occupancy-res", "many"])
    with pytest.raises(SystemExit):
        evaluate_cli.main(["--config", "x", "--data", "y", "--occupancy-box", "1.0"])


# ---------------------------------------------------------------------------------------------
# the build's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res():
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B.kernel_resources()


def _queue_kernels(res, kernel):
    """{(family arguments, mode): figures} of the instantiations of `kernel`, e.g. ('NetV3<12, 4>', 'ModeF16')."""
    out = {}
    for name, r in res.items():
        m = re.search(r"nrf::" + kernel + r"<nrf::(NetV\d)<nrf::(Mode\w+), \d+, ([^>]*)>,", name)
        if m:
            out[(f"{m.group(1)}<{m.group(3)}>", m.group(2))] = r
    return out


def test_a_skipping_kernel_is_built_for_every_family_and_mode(res):
    occ, plain = _queue_kernels(res, "render_queue_occ_kernel"), _queue_kernels(res, "render_queue_kernel")
    assert set(occ) == set(plain) and len(occ) == 16, sorted(occ)
    assert {f for f, _ in occ} == {"NetV1<10>", "NetV2<10>", "NetV3<12, 2>", "NetV3<12, 4>"}
    assert {m for _, m in occ} == {"ModeBF16", "ModeF16", "ModeF32", "ModeF16X3"}
    for key, r in occ.items():
        assert r["tu"].startswith("fused_occ_"), (key, r["tu"])              # translation units of their own
        assert plain[key]["tu"].startswith("fused_v"), (key, plain[key]["tu"])


def test_v1_and_v2_skipping_kernels_spill_no_more_than_their_plain_siblings(res):
    occ, plain = _queue_kernels(res, "render_queue_occ_kernel"), _queue_kernels(res, "render_queue_kernel")
    for key in sorted(occ):
        o, p = occ[key], plain[key]
        print(key, "occ", o["vgpr_spill"], o["scratch"], o["sgpr_spill"], "plain", p["vgpr_spill"], p["scratch"], p["sgpr_spill"])
        if key[0].startswith("NetV3"):
            continue                                                         # reported in DESIGN.md section 7 next to its sibling
        assert o["vgpr_spill"] <= p["vgpr_spill"] and o["scratch"] <= p["scratch"], (key, o, p)
