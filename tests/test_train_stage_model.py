"""CPU tests of the oracle's rounding model of the V2 / V3 training chains (oracle.train_stages) and of the stage comparer the GPU
stage tests are built on (tests/train_ctx.py):

  * with mode='f32' the model is mlp_v2 / mlp_v3 and autograd through them, at the bounds of the fp32 GPU tests;
  * the reference alone keeps the comparer's caps: on the committed cases of tests/test_gpu_train_stages.py, the model
    accumulated in fp32 against the model accumulated in float64, on the same stage inputs, stays at or below HALF of the outlier
    cap and of the differing-share cap in every stage (so a correct kernel has the other half for itself);
  * the comparer bites: five deliberately wrong variants of the model are each reported at the stage where the fault was put in,
    and nowhere else.
"""
import pytest
import torch

from oracle import nerf_oracle as O
from tests import train_ctx as T

MARGIN = 2e-5          # as tests/test_gpu_training.py: samples whose ReLU masks are decided by summation order carry no gradient


def rel_to_max(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("variant,dino_dim,depth", [("v2", 0, 8), ("v2", 0, 2), ("v3", 64, 8), ("v3", 128, 8), ("v3", 64, 2)])
def test_f32_mode_is_the_oracle_and_its_autograd(variant, dino_dim, depth):
    p, x = T.stage_case(variant, dino_dim, depth, 700)
    keep = (O.relu_margin(p, variant, x["pos"], x["dirs"], x["dino"]) > MARGIN)[:, None]
    assert keep.float().mean() > 0.85
    g_rgb, g_den = x["g_rgb"] * keep, x["g_den"] * keep
    pp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    o_rgb, o_den = O.mlp_v3(pp, x["pos"], x["dirs"], x["dino"]) if variant == "v3" else O.mlp_v2(pp, x["pos"], x["dirs"])
    ((o_rgb * g_rgb).sum() + (o_den * g_den).sum()).backward()
    pe = O.positional_encoding(x["pos"], 12 if variant == "v3" else 10)
    st, grads = O.train_stages(p, variant, pe, O.positional_encoding(x["dirs"], 4), g_rgb, g_den, dino=x["dino"], mode="f32")
    assert (st["rgb"] - o_rgb.detach()).abs().max() < 1e-4 and rel_to_max(st["density"], o_den) < 1e-4
    assert set(grads) == set(p)
    for name, g in grads.items():
        assert rel_to_max(g, pp[name].grad) < 2e-4, (name, rel_to_max(g, pp[name].grad))
    fwd, bwd = O.train_stage_names(variant, depth)
    assert set(fwd + bwd) <= set(st) and len(fwd + bwd) == T.slot_numbers(variant, depth)[2] + (variant == "v3")     # every slot, and the gate


def test_f32_mode_dino_gradient_is_autograd():
    p, x = T.stage_case("v3", 64, 2, 500)
    keep = (O.relu_margin(p, "v3", x["pos"], x["dirs"], x["dino"]) > MARGIN)[:, None]
    g_rgb, g_den = x["g_rgb"] * keep, x["g_den"] * keep
    dino = x["dino"].clone().requires_grad_(True)
    o_rgb, o_den = O.mlp_v3(p, x["pos"], x["dirs"], dino)
    ((o_rgb * g_rgb).sum() + (o_den * g_den).sum()).backward()
    st, _ = O.train_stages(p, "v3", O.positional_encoding(x["pos"], 12), O.positional_encoding(x["dirs"], 4), g_rgb, g_den, dino=x["dino"], mode="f32")
    assert rel_to_max(O.dino_grad_from_stages(p, st, "f32"), dino.grad) < 2e-4


CASES = [(v, dd, depth, n) for (v, dd) in T.FAMILIES for depth in (8, 2) for n in (300, 33000)]


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("variant,dino_dim,depth,n", CASES)
def test_the_reference_alone_keeps_half_of_the_caps(variant, dino_dim, depth, n, mode):
    """The outlier cap 4 + n // 2000 and the differing-share cap are conditions on the comparison, not on the kernel alone: two
    correct implementations that differ in the accumulation (fp32 against float64) must stay well inside them."""
    p, x = T.stage_case(variant, dino_dim, depth, n)
    assert 0.2 < T.density_open_share(p, variant, x) < 0.8
    chain, _ = T.model_on(p, variant, x, mode)                                  # float64 accumulation: the reference and the stage inputs
    got, _ = T.model_on(p, variant, x, mode, acc=torch.float32, given=chain)
    for f in T.compare_stages(got, chain, variant, depth, mode, n):
        assert f.outliers <= f.allowed // 2 and f.differ <= T.DIFFER_SHARE / 2, f


# ---------------------------------------------------------------------------------------------
# deliberately wrong models
# ---------------------------------------------------------------------------------------------
truncate, fault = T.truncate, T.fault          # the planted-fault helpers, shared with tests/test_render_link_host.py


def swap_k(w):
    w = w.clone()
    w[:, [5, 77]] = w[:, [77, 5]]
    return w


def drop_last(e):
    e = e.clone()
    e[:, -1] = 0
    return e


FAULTS = {
    "truncation": lambda mode: (fault("round", "trunk.1", lambda t: truncate(t, mode)), "trunk.1"),
    "swapped-K-rows": lambda mode: (fault("weight", "density_mlp.density_layers.2", swap_k), "trunk.1"),
    "dropped-dir-column": lambda mode: (fault("encoding", "dir", drop_last), "colour.in"),
    "exchanged-gate": lambda mode: (fault("gate", 1, lambda w: w.flip(-1)), "input.1"),
    "missing-bias": lambda mode: (fault("bias", "color_mlp.color_layers.0", torch.zeros_like), "colour.c0"),
}


@pytest.mark.parametrize("mode", ["bf16", "f16"])
@pytest.mark.parametrize("which,variant,dino_dim", [(w, v, dd) for w in sorted(FAULTS) for v, dd in (("v2", 0), ("v3", 64))
                                                     if (w, v) != ("exchanged-gate", "v2")])        # V2 has no gate
def test_the_comparer_reports_a_fault_at_its_stage(which, variant, dino_dim, mode):
    n, depth = 300, 8
    tap, stage = FAULTS[which](mode)
    p, x = T.stage_case(variant, dino_dim, depth, n)
    wrong, _ = T.model_on(p, variant, x, mode, tap=tap)                         # the faulty implementation's own chain
    exp, _ = T.model_on(p, variant, x, mode, given=wrong)                       # the model on ITS stage inputs
    bad = T.failed(T.compare_stages(wrong, exp, variant, depth, mode, n))
    assert bad and {f.stage.replace("mask.", "").split("[")[0] for f in bad} == {stage}, bad
    right, _ = T.model_on(p, variant, x, mode)
    assert not T.failed(T.compare_stages(right, T.model_on(p, variant, x, mode, given=right)[0], variant, depth, mode, n))


# ---------------------------------------------------------------------------------------------
# the decoder, against the lane maps of tests/mfma_emulator.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("variant,depth", [("v1", 8), ("v2", 2), ("v3", 2), ("v3", 8)])
def test_saved_context_decoder_inverts_the_store_layout(variant, depth, mode):
    """A context written the way train_core.hpp stores it -- a tile as the lanes hold it, 16 B per lane and vector, the ReLU bits
    of tile m in half m & 1 of dword m >> 1, the gate pairs behind the planes -- from known matrices, by way of the emulator's
    independent register image: SavedContext must return the matrices, for every slot, plane and the gate."""
    import numpy as np
    from nerf_few_shot_limitations_amd import _lib as L
    from tests import mfma_emulator as E
    from tests.test_training_host import train_plan
    L.lib()
    n = 300                                                      # two 256-sample groups: 16 sample tiles
    p = O.make_weights(variant, 1, "fog", n_layers=depth)
    plan = train_plan(L, variant, p, depth, with_planes=True)
    slot_tiles, n_planes = plan[1], plan[3]
    T32 = 16
    rng = np.random.default_rng(7)
    mats = [E.quantize(rng.standard_normal((32 * kt, 32 * T32)).astype(np.float32), mode) for kt in slot_tiles]
    parts = []
    for m in mats:
        kt = m.shape[0] // 32
        for st in range(T32):
            regs = E.tiles_from_matrix(m[:, 32 * st:32 * st + 32])               # (kt, 64 lanes, 16 registers)
            for t in range(kt):
                if mode == "f32":
                    parts.append(regs[t].reshape(64, 4, 4).transpose(1, 0, 2).astype(np.float32).tobytes())
                else:
                    v = regs[t].reshape(64, 2, 8).transpose(1, 0, 2)
                    u = (np.ascontiguousarray(v).view(np.uint32) >> 16).astype(np.uint16) if mode == "bf16" else v.astype(np.float16)
                    parts.append(np.ascontiguousarray(u).tobytes())
    names, planes, count, _ = T.slot_numbers(variant, depth)
    assert sorted(names.values()) == list(range(count)) and sorted(planes.values()) == list(range(n_planes))
    by_plane = {v: k for k, v in planes.items()}
    bits = {}
    for pl in range(n_planes):
        kt = slot_tiles[names[by_plane[pl]]]
        b = rng.random((32 * kt, 32 * T32)) < 0.5
        bits[by_plane[pl]] = b
        for st in range(T32):
            regs = E.tiles_from_matrix(b[:, 32 * st:32 * st + 32].astype(np.float32)).astype(np.uint32)      # (kt, 64, 16)
            w = np.zeros((64, 4), np.uint32)
            for m in range(kt):
                for r in range(16):
                    w[:, m >> 1] |= regs[m, :, r] << (16 * (m & 1) + 15 - r)
            parts.append(w.tobytes())
    gate = rng.random((32 * T32, 2)).astype(np.float32)
    parts.append(gate.tobytes())
    ctx = T.SavedContext(plan, variant, depth, mode, n, np.frombuffer(b"".join(parts), np.uint8))
    for name, slot in names.items():
        assert np.array_equal(ctx.slot(name), mats[slot]), name
    for name in planes:
        assert np.array_equal(ctx.plane(name), bits[name]), name
    assert np.array_equal(ctx.gate(), gate)


@pytest.mark.parametrize("variant,dino_dim", T.FAMILIES)
def test_saved_stages_restores_the_reference_feature_order(variant, dino_dim):
    """saved_stages on slots laid out the way the kernels lay them out (encoder tiles in feature_map.hpp's order, by way of
    test_training_host.kernel_order_rows; head gradients in rows 0..; padded samples behind n) gives the model's stages back."""
    import numpy as np
    from tests.test_training_host import kernel_order_rows
    n, depth, pad = 40, 2, 64
    p, x = T.stage_case(variant, dino_dim, depth, n)
    chain, _ = T.model_on(p, variant, x, "f16")
    pe_l = 12 if variant == "v3" else 10
    n_pe = O.encoded_dim(pe_l)

    def rows(name):
        a = chain[name].numpy()
        if name == "input":
            m = kernel_order_rows(a, pe_l)
        elif name.startswith("input."):
            m = np.concatenate([kernel_order_rows(a[:, :n_pe], pe_l), a[:, n_pe:].T], 0)
        elif name == "colour.in":
            m = np.concatenate([a[:, :256].T, kernel_order_rows(a[:, 256:], 4)], 0)
        else:
            m = np.zeros(((a.shape[1] + 31) // 32 * 32, n), np.float32)
            m[:a.shape[1]] = a.T
        return np.concatenate([m, np.zeros((m.shape[0], pad - n), np.float32)], 1)

    class Ctx:
        planes = T.slot_numbers(variant, depth)[1]
        slot = staticmethod(rows)
        plane = staticmethod(lambda name: np.concatenate([chain["mask." + name].numpy().T, np.zeros((chain[name].shape[1], pad - n), bool)], 1))
        gate = staticmethod(lambda: np.concatenate([chain["gate"].float().numpy(), np.zeros((pad - n, 2), np.float32)], 0))
    Ctx.n = n
    got, zeros = T.saved_stages(Ctx, variant, depth, dino_dim)
    fwd, bwd = O.train_stage_names(variant, depth)
    for name in fwd + bwd + ["mask." + k for k in Ctx.planes]:
        assert torch.equal(got[name], chain[name].float() if name == "gate" else chain[name]), name
    assert zeros and all(np.abs(z).max() == 0 for _, z in zeros if z.size)
