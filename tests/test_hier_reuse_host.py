"""Host-side checks of the hierarchical render that evaluates only the new samples in its fine pass (no GPU needed):
the emitting kernels' register allocation, the merge rule against the oracle's sorted union, the workspace formula, and what
the new C entry points refuse from their arguments alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from nerf_few_shot_limitations_amd import _lib as L
from nerf_few_shot_limitations_amd import build as B
from oracle import nerf_oracle as O


@pytest.fixture(scope="module")
def res():
    if not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)) if os.path.isdir(B.OBJ) else True:
        pytest.skip("no object directory (the library was built elsewhere: the GPU box receives the .so only)")
    # one object directory holds every kernel (the census of tests/golden/kernel_resources.json covers all of them by name); the tests
    # below pick the feature's kernels and their plain siblings out of it by kernel and unit name
    everything = B.kernel_resources()
    return {"plain": everything, "hier": everything}


def template_args(name):
    return re.search(r"render(?:_emit)?_kernel<(.*)>\(", name).group(1)


def test_emitting_kernels_meet_the_register_bar(res):
    """Every (family, mode) has a render_emit_kernel beside its render_kernel.  V1 / V2 in the 16-bit modes: no spilled register, no
    scratch, one wave per SIMD, operand images in AGPRs; V3 (either feature width): no more spills / scratch than the plain sibling."""
    emit = {template_args(k): v for k, v in res["hier"].items() if "nrf::render_emit_kernel<" in k and k.startswith("fused_emit_")}
    plain = {template_args(k): v for k, v in res["plain"].items() if "nrf::render_kernel<" in k and k.startswith("fused_v")}
    assert len(plain) == 16 and set(emit) == set(plain)          # V1, V2, V3 (64-d), V3 (128-d) x four modes
    for args, r in emit.items():
        sib = plain[args]
        assert r["tu"].replace("fused_emit_", "fused_") == sib["tu"], args          # built in the same half as its sibling
        if "NetV3" in args:
            assert r["vgpr_spill"] <= sib["vgpr_spill"] and r["scratch"] <= sib["scratch"], (args, r, sib)
        elif "ModeBF16" in args or "ModeF16," in args:
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (args, r)
        if "ModeBF16" in args or "ModeF16," in args:
            assert r["agprs"] > 0 and r["occupancy"] == 1, (args, r)
        assert r["occupancy"] == sib["occupancy"] and r["lds"] == sib["lds"], (args, r, sib)


def test_staged_kernels_of_the_route_spill_nothing(res):
    for kernel, n in (("composite_merge_kernel<", 2), ("sample_pdf_sorted_kernel(", 1)):
        ks = {k: v for k, v in res["hier"].items() if "::" + kernel in k}
        assert len(ks) == n, (kernel, sorted(ks))
        for name, r in ks.items():
            assert r["tu"] == "hier_kernels" and r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["agprs"] == 0, (name, r)


def merge_two_pointer(zc, zn):
    """The merge rule of the compositor: the coarse sample is taken while z_coarse <= z_new."""
    i = j = 0
    out, from_coarse = [], []
    while i < len(zc) or j < len(zn):
        coarse = j >= len(zn) or (i < len(zc) and zc[i] <= zn[j])
        out.append(zc[i] if coarse else zn[j])
        from_coarse.append(coarse)
        i, j = (i + 1, j) if coarse else (i, j + 1)
    return np.asarray(out, np.float32), from_coarse


def test_two_pointer_merge_reproduces_the_sorted_union():
    R, S, Ni = 64, 12, 9
    z = O.z_steps(2.0, 6.0, S).expand(R, S).contiguous()
    w = torch.from_numpy(O.uniform01(5, R * S).reshape(R, S)).float() ** 4
    w[torch.arange(R), torch.arange(R) % S] += 1.0
    w = w / w.sum(-1, keepdim=True)
    u = torch.from_numpy(O.uniform01(6, R * Ni).reshape(R, Ni)).float()
    u = (u * 4).floor() / 4                                      # repeated values inside every row
    u[:, 0], u[:, -1] = 0.0, 1.0                                 # both ends: a new sample on the first and on the last coarse depth
    smp, union = O.sample_pdf(z, w, Ni, u=u)
    assert bool((smp[:, 0] == z[:, 0]).all()) and bool((smp[:, -1] == z[:, -1]).any())
    assert any(len(np.unique(r)) < Ni for r in smp.numpy())      # equal new samples
    for r in range(R):
        zn = np.sort(smp[r].numpy(), kind="stable")
        merged, from_coarse = merge_two_pointer(z[r].numpy(), zn)
        assert np.array_equal(merged, union[r].numpy()), r
        assert from_coarse[0]                                    # the coarse depth goes in front of an equal new sample ...
        if smp[r, -1] == z[r, -1]:
            assert not from_coarse[-1] and from_coarse[-2]       # ... so an equal new one is the ray's last (1e10) sample


def test_workspace_formula():
    lib = L.lib()
    for n, S, Ni in ((1, 128, 64), (1 << 15, 128, 64), (333, 2, 1), (7, 70, 0)):
        assert lib.nrf_hier_workspace_bytes(n, S, Ni) == n * (S * (4 + 4 + 16) + Ni * (4 + 16)), (n, S, Ni)
    assert lib.nrf_hier_workspace_bytes(1, 128, 64) == 4352
    assert lib.nrf_hier_workspace_bytes(-1, 128, 64) == -1 and lib.nrf_hier_workspace_bytes(1, 0, 64) == -1


def test_new_entries_check_their_arguments_before_any_launch():
    lib = L.lib()
    assert lib.nrf_abi_version() == 5                            # additive: no existing struct or signature changed
    a16 = 1 << 20                                                # (never dereferenced: every call below is refused or empty)
    f = lambda *a: lib.nrf_composite_merge(*a)
    assert f(a16, a16, None, None, a16, 0, 12, 0, 1, 0, 0, a16, a16, None, None, None) == 0          # no rays: nothing to do
    assert f(a16, a16, None, None, a16, 4, 12, 5, 1, 0, 0, a16, a16, None, None, None) == -1         # Ni > 0 without the new rows
    assert f(a16, a16 + 4, None, None, a16, 4, 12, 0, 1, 0, 0, a16, a16, None, None, None) == -1     # misaligned rows
    assert b"16-byte" in lib.nrf_last_error()
    assert f(a16, a16, None, None, a16, 4, 0, 0, 1, 0, 0, a16, a16, None, None, None) == -1          # no coarse samples
    assert f(a16, a16, None, None, a16, 4, 12, 0, 9, 0, 0, a16, a16, None, None, None) == -1         # unknown mode
    assert f(a16, a16, None, None, None, 4, 12, 0, 1, 0, 0, a16, a16, None, None, None) == -1        # no directions
    c2w = (C.c_float * 12)(*([0.0] * 12))
    cam = lambda *a: lib.nrf_composite_merge_camera(*a)
    assert cam(a16, a16, None, None, 4, 4, 1.0, c2w, 0, 17, 12, 0, 1, 0, 0, a16, a16, None, None, None) == -1      # range outside the image
    assert cam(a16, a16, None, None, 4, 4, 1.0, c2w, 3, 3, 12, 0, 1, 0, 0, a16, a16, None, None, None) == 0        # empty range
    assert lib.nrf_sample_pdf_sorted(a16, a16, 4, 12, 5, None, 0, None, None, None, None) == -1                     # no output asked for
    assert lib.nrf_sample_pdf_sorted(a16, a16, 0, 12, 5, None, 0, None, a16, None, None) == 0
    # the emitting renders look at the model first, like their plain siblings
    assert lib.nrf_render_rays_emit(None, a16, a16, 4, None, a16, a16, None, None, a16, 0, None) == -1
