"""GPU tests of the 16-bit V2 and V3 training chains, stage by stage (nrf_mlp_forward_train, nrf_mlp_backward,
nrf_mlp_backward_dino through the C ABI): what tests/test_gpu_training.py:test_saved_tensors_stage_consistent_16bit is to V1.

End to end, two correct 16-bit implementations differ by half the whole mode error (one flipped last bit cascades through the
layers), so the end-to-end bars cannot tell a rounding from a truncation.  Here every saved tensor of a forward_train / backward
pair -- every slot of csrc/train_slots.hpp's SlotsV2 / SlotsV3, every ReLU bit plane, the V3 gate -- is decoded
(tests/train_ctx.py) and held to the oracle's rounding model (oracle.train_stages, float64 accumulation) applied to the GPU's
OWN saved inputs of that stage.  The bounds come from the number formats and from V1's test, not from these kernels; they are
stated in tests/train_ctx.py and asserted there by compare_stages / failed:

  network stages      ulp |e| + 1e-6 max|e| (ulp = 2^-10 f16, 2^-7 bf16), at most 4 + n // 2000 elements outside, at most 10 % of
                      the non-zero elements different at all (tests/test_train_stage_model.py: the reference alone, fp32
                      against float64 accumulation, keeps half of both caps, and truncation, swapped K rows, a dropped
                      encoder column, an exchanged gate and a missing bias are each reported at their stage)
  encoder stages      ulp max(|e|, 2^-4) against the float64 encoding, no element outside; padding rows exactly zero
  gate                1e-6 (f16) / 2e-3 (bf16, __expf) against the float64 softmax of the saved attention.0; |w0 + w1 - 1| <= 1e-6
  d_gate              ulp |e| + 32 KT0 2^-24 (|w0 dw0| + |w1 dw1|)
  every dZ            exactly zero for padded samples, head gradients exactly zero past their rows
  parameter gradients every weight and bias of the family (density_head and attention.2 included) within 1e-4 of its tensor's
                      largest value of the products and sums of the saved tensors (fp32 accumulation on both sides: V1's figure)
  d_dino              W0d^T d1 + w1 W0d^T d2 from the saved dZ(fusion.0) slots, the saved gate and the rounded weight columns: 1e-4
  rgb, density        from the last saved stages: 2e-3 (V1's bound for the sigmoid heads), 1e-4 of the largest density

Cases: bf16 and f16; V2, V3 at dino_dim 64 and 128; depth 8 and 2 (the slot numbers depend on it); n = 300 (4-wave geometry)
and 33000 (8-wave geometry).  Weights are 'solid' sets whose density ReLU is open for 20 .. 80 % of the samples.

Record (a record, not a bound).  Every case prints a RECORD line under -s: the largest |a - e| / bound inside any stage, the
most elements of one stage outside its bound (cap 4 at n = 300, 20 at n = 33000), the largest share of differing elements.
    MI355X: NOT RECORDED YET -- this file has not run on the GPU at the time of writing.
    CPU, the reference alone (fp32 against float64 accumulation, tests/test_train_stage_model.py), n = 33000, depth 8:
        bf16  V2 / V3: at most 1 outlier in a stage (a ReLU plane), differing share 1e-4, gate 3e-5 of its bound, d_gate 0.46
        f16   V2 / V3: at most 1 outlier in a stage (a ReLU plane), differing share 1.3e-3, gate 0.11 of its bound, d_gate 0.93

forward_train against the inference forward: bit-equal for V2 and V3 in f32, bf16 and f16 (a column's arithmetic
does not depend on the geometry) -- asserted below.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import train_ctx as T
from tests.test_training_host import train_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


def make_model(N, variant, dino_dim, depth, mode, p):
    m = N.NeRFMLP(pos_freq=12 if variant == "v3" else 10, dir_freq=4, hidden_dim=256, num_density_layers=depth, use_dino=variant == "v3",
                  dino_dim=dino_dim, mma_mode=mode)
    m.load_state_dict(p, strict=False)
    return m.cuda().train()


def run_raw(model, x, want_dino_grad):
    """One forward_train / backward (/ backward_dino) through the C ABI: rgb, density, {name: gradient}, context, d_dino."""
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    h, mode = _train_handle(model, dev)
    n = x["pos"].shape[0]
    d = {k: (v.cuda().contiguous() if v is not None else None) for k, v in x.items()}
    rgb, den = torch.empty((n, 3), device=dev), torch.empty((n, 1), device=dev)
    nbytes = L.lib().nrf_train_context_bytes(h, mode, n)
    assert nbytes > 0
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    ctx = C.c_void_p(buf.data_ptr())
    L.check(L.lib().nrf_mlp_forward_train(h, mode, L.ptr(d["pos"]), L.ptr(d["dirs"]), L.ptr(d["dino"]), n, L.ptr(rgb), L.ptr(den), ctx, nbytes, L.stream_ptr()))
    fp = model.flat_params()
    grad = torch.zeros(fp.flat.numel(), device=dev)
    L.check(L.lib().nrf_mlp_backward(h, mode, L.ptr(rgb), L.ptr(den), L.ptr(d["g_rgb"]), L.ptr(d["g_den"]), n, ctx, nbytes, L.ptr(grad), L.stream_ptr()))
    d_dino = None
    if want_dino_grad:
        d_dino = torch.empty((n, model.dino_dim), device=dev)
        L.check(L.lib().nrf_mlp_backward_dino(h, mode, n, ctx, nbytes, L.ptr(d_dino), L.stream_ptr()))
    torch.cuda.synchronize()
    names = [f"{nm}.{part}" for nm, _, _ in O.layer_shapes("v3" if model.dino_dim else "v2", n_layers=model.n_layers, dino_dim=model.dino_dim)
             for part in ("weight", "bias")]
    views = fp.views(grad)
    assert len(views) == len(names)
    return rgb.cpu(), den.cpu(), {k: v.cpu() for k, v in zip(names, views)}, buf, (d_dino.cpu() if d_dino is not None else None)


def rel_to_max(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("n", [300, 33000])
@pytest.mark.parametrize("depth", [8, 2])
@pytest.mark.parametrize("variant,dino_dim", T.FAMILIES)
@pytest.mark.parametrize("mode", ["bf16", "f16"])
def test_every_stage_against_the_rounding_model(N, mode, variant, dino_dim, depth, n):
    from nerf_few_shot_limitations_amd import _lib as L
    p, x = T.stage_case(variant, dino_dim, depth, n)
    assert 0.2 < T.density_open_share(p, variant, x) < 0.8
    model = make_model(N, variant, dino_dim, depth, mode, p)
    rgb, den, grads, buf, d_dino = run_raw(model, x, variant == "v3")
    ctx = T.SavedContext(train_plan(L, variant, p, depth, dino_dim, with_planes=True), variant, depth, mode, n, buf)
    got, zeros = T.saved_stages(ctx, variant, depth, dino_dim)
    del buf, ctx
    got["rgb"], got["density"] = rgb, den
    exp, exp_grads = T.model_on(p, variant, x, mode, given=got)
    findings = T.compare_stages(got, exp, variant, depth, mode, n)
    inside = [f for f in findings if f.outliers <= f.allowed]
    print(f"\nRECORD {mode} {variant} dino {dino_dim} depth {depth} n {n}: largest |a-e|/bound inside a stage "
          f"{max((f.worst for f in inside if f.outliers == 0), default=0.0):.3f}; most outliers "
          f"{max(findings, key=lambda f: f.outliers).outliers} ({max(findings, key=lambda f: f.outliers).stage}); "
          f"largest differing share {max(f.differ for f in findings):.4f} ({max(findings, key=lambda f: f.differ).stage})")
    for f in findings:
        if f.stage.startswith(("gate", "d_gate")):
            print("      ", f)
    assert not T.failed(findings), T.failed(findings)
    for what, z in zeros:
        assert z.size == 0 or np.abs(z).max() == 0.0, what
    # the outputs, from the last saved stages
    assert (rgb - exp["rgb"]).abs().max() < 2e-3, float((rgb - exp["rgb"]).abs().max())
    assert rel_to_max(den, exp["density"]) < 1e-4
    assert (den > 0).float().mean() > 0.1 and (den == 0).float().mean() > 0.1          # both branches of the density ReLU
    # every parameter gradient, from the products and sums of the saved tensors
    assert set(grads) == set(p) == set(exp_grads)
    worst = max(grads, key=lambda k: rel_to_max(grads[k], exp_grads[k]))
    print(f"       worst parameter gradient: {worst} {rel_to_max(grads[worst], exp_grads[worst]):.2e}")
    for name in grads:
        assert rel_to_max(grads[name], exp_grads[name]) < 1e-4, (name, rel_to_max(grads[name], exp_grads[name]))
    if variant == "v3":
        e = O.dino_grad_from_stages(p, got, mode, acc=torch.float64)
        print(f"       d_dino: {rel_to_max(d_dino, e):.2e}")
        assert rel_to_max(d_dino, e) < 1e-4


@pytest.mark.parametrize("variant,dino_dim", T.FAMILIES)
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
def test_forward_train_equals_inference_forward(N, mode, variant, dino_dim):
    """Same chain, same arithmetic: the saving forward must reproduce nrf_mlp_forward bit for bit (as V1's does), whatever the
    geometry either kernel runs."""
    p, x = T.stage_case(variant, dino_dim, 8, 1000)
    model = make_model(N, variant, dino_dim, 8, mode, p)
    rgb, den, _, _, _ = run_raw(model, x, False)
    with torch.no_grad():
        r2, d2 = model.eval()(x["pos"].cuda(), x["dirs"].cuda(), x["dino"].cuda() if x["dino"] is not None else None)
    assert torch.equal(rgb, r2.cpu()) and torch.equal(den, d2.cpu())
