"""Build-time checks of the tail mode (include/nerfhip.h: nrf_tail; fused_impl.hpp: render_march): the two kernels of a tail
render are held to the standards tests/test_kernel_resources.py sets for the renderers they are cut from, and the library
exports the new entry points."""
import ctypes
import os
import re

import pytest

from nerf_few_shot_limitations_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def res():
    if not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)) if os.path.isdir(B.OBJ) else True:
        pytest.skip("no object directory (the library was built elsewhere: the GPU box receives the .so only)")
    return B.kernel_resources()


def pick(res, *needles):
    return {k: v for k, v in res.items() if all(n in k for n in needles)}


def test_tail_kernels_spill_nothing(res):
    """The split-f16 last-sample kernels: V1 / V2 no spilled register and at most the 36-byte reservation of private segment (the
    standard of test_split_mode_kernels_spill_nothing); V3 no worse than the split-mode render_kernel of the same feature width,
    read from the same build."""
    ks = pick(res, "fused_tail", "nrf::render_tail_kernel<", "ModeF16X3")
    assert len(ks) == 4, sorted(ks)                              # V1, V2, V3 (64-d), V3 (128-d)
    for name, r in ks.items():
        if "NetV3" in name:
            width = re.search(r"NetV3<nrf::ModeF16X3, 1, 12, (\d)>", name).group(1)
            (ref,) = pick(res, "nrf::render_kernel<", f"NetV3<nrf::ModeF16X3, 1, 12, {width}>").values()
            assert r["vgpr_spill"] <= ref["vgpr_spill"] and r["scratch"] <= ref["scratch"], (name, r, ref)
        else:
            assert r["vgpr_spill"] == 0 and r["scratch"] <= 36, (name, r)
        assert r["occupancy"] == 1, (name, r)


@pytest.mark.parametrize("mode", ["ModeBF16", "ModeF16,"])
def test_prefix_kernels_meet_the_16bit_renderers_limits(res, mode):
    """render_hold_kernel is render_kernel minus the last sample and the image epilogue: the limits of
    test_16bit_fused_kernels_use_no_scratch_and_park_operands_in_agprs for render_kernel hold for it unchanged."""
    ks = pick(res, "fused_", "nrf::render_hold_kernel<", f"<nrf::{mode}")
    assert len(ks) == 4, sorted(ks)
    for name, r in ks.items():
        if "NetV3" in name:
            if "ModeBF16" in name:
                lim = (60, 256) if ", 12, 4>," in name else (12, 52)
            else:
                lim = (5, 56)
            assert r["vgpr_spill"] <= lim[0] and r["scratch"] <= lim[1], (name, r)
        else:
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["agprs"] > 0 and r["occupancy"] == 1, (name, r)


def test_plain_renderers_keep_their_names_and_the_tail_kernels_their_modes(res):
    """The plain renderers keep their names: the tail mode's kernels are separate entry points around the shared march, the prefix
    built for the 16-bit modes only and the last-sample kernel for split-f16 only."""
    for fam in ("NetV1", "NetV2", "NetV3"):
        for mode in ("ModeBF16", "ModeF16,", "ModeF16X3", "ModeF32"):
            assert pick(res, "nrf::render_kernel<", f"{fam}<nrf::{mode}"), (fam, mode)
    assert not pick(res, "render_tail_kernel<", "ModeF32") and not pick(res, "render_hold_kernel<", "ModeF16X3")


def test_library_exports_the_tail_entry_points():
    from nerf_few_shot_limitations_amd import _lib as L
    lib = L.lib()
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    for name in ("nrf_render_tail_bytes", "nrf_render_rays_tail", "nrf_render_camera_tail", "nrf_render_cameras_tiles_tail"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.nrf_abi_version() == 5                            # additive: no existing struct or signature changed
    assert lib.nrf_abi_sizeof(4) == ctypes.sizeof(L.nrf_tail) == 24
    assert lib.nrf_abi_sizeof(5) == -1
    # 24 bytes of carried compositor state per ray, rounded up to the 16-byte alignment the workspace must have
    for n, want in ((0, 0), (1, 32), (2, 48), (10000, 240000), (10001, 240032)):
        assert lib.nrf_render_tail_bytes(n) == want, n
    assert lib.nrf_render_tail_bytes(-1) == -1 and b"n_rays" in lib.nrf_last_error()


def test_tail_mode_names_are_checked_before_any_gpu_work():
    from nerf_few_shot_limitations_amd import _lib as L
    assert L.tail_arg(None, "f16", 10, "cuda:0") == (None, None)
    with pytest.raises(ValueError):
        L.tail_arg("f32", "f16", 10, "cuda:0")
    for base in ("f32", "f16x3"):
        with pytest.raises(ValueError):
            L.tail_arg("f16x3", base, 10, "cuda:0")
