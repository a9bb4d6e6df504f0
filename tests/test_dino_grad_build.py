"""Build-time check of the DINO feature-gradient kernels: dino_grad_kernel needs 2 * DT accumulator tiles and two operand tiles
in flight -- far under the register file -- and the fetch adjoint is a plain slab kernel, so none of them may spill or use
scratch; and the chain kernel they sit behind keeps the register figures it has without them."""
import os

import pytest

from nerf_few_shot_limitations_amd import build as B


@pytest.fixture(scope="module")
def res():
    if not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)) if os.path.isdir(B.OBJ) else True:
        pytest.skip("no object directory (the library was built elsewhere: the GPU box receives the .so only)")
    return B.kernel_resources()


def pick(res, *needles):
    return {k: v for k, v in res.items() if all(n in k for n in needles)}


def test_dino_grad_kernels_spill_nothing(res):
    ks = pick(res, "train_dino_grad", "dino_grad_kernel<")
    assert len(ks) == 6, sorted(ks)                              # bf16, f16, f32 x DT 2, 4
    for mode in ("ModeBF16", "ModeF16,", "ModeF32"):
        for dt in (2, 4):
            assert pick(ks, f"{mode}", f" {dt}>"), (mode, dt)
    for name, r in ks.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_fetch_backward_kernels_spill_nothing(res):
    for kernel in ("project_fetch_backward_kernel(", "fetch_backward_reduce_kernel("):
        ks = pick(res, "staged_kernels", kernel)
        assert len(ks) == 1, (kernel, sorted(ks))
        for name, r in ks.items():                               # (the taps are wave-uniform: they live in scalar registers)
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)


def test_the_feature_gradient_is_a_translation_unit_of_its_own(res):
    """train_backward_v3_kernel is untouched: the new kernel lives in its own object, the chain kernels in theirs."""
    assert not pick(res, "train_v3:", "dino_grad_kernel") and pick(res, "train_v3:", "train_backward_v3_kernel<")
