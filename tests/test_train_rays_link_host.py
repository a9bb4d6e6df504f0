"""CPU half of tests/test_gpu_train_rays_link.py (no GPU): the two helpers that file rests on (tests/train_ctx.py:
context_differences, x_enc_from_input_slot) and the premise of its sections 2b and 3.

  permutation    kernel_feature_order(10) / (12) hit every reference feature exactly once; x_enc_from_input_slot inverts the
                 packing SavedContext.slot_number decodes, on a context buffer built here on the host with the plan the library
                 reports (nrf_debug_train_plan), in f32, bf16 and f16, and hands back the padding rows
  planted        context_differences reports a flipped element of a trunk slot, a flipped ReLU-plane bit and a changed gate pair
                 at their stage and nowhere else, counts them and names the first (row, sample); a difference in a padded column
                 is not reported; a stage that is not asked for is not looked at
  idempotence    oracle.quantize(q, mode) == q, bit for bit, for EVERY finite f16 / bf16 bit pattern (subnormals and -0
                 included): a staged forward that is handed an already rounded encoding rounds nothing
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import train_ctx as T
from tests.test_training_host import train_plan

MODES = ["f32", "bf16", "f16"]


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


# ---------------------------------------------------------------------------------------------
# the inverse of SavedContext's decoders: matrices -> context bytes
# ---------------------------------------------------------------------------------------------
def _row(r, h):
    return (r & 3) + 8 * (r >> 2) + 4 * h                      # accumulator row map (train_ctx.SavedContext.slot_number)


def write_slot(ctx, slot, M):
    """(32 KT, 32 T) fp32 matrix, values already in the operand type -> the bytes of `slot` (csrc/train_core.hpp layout)."""
    Tn, KT = ctx.tiles32, ctx.slot_tiles[slot]
    m = np.asarray(M, np.float32).reshape(KT, 32, Tn, 32)
    if ctx.mode == "f32":
        v = np.zeros((Tn, KT, 4, 2, 32, 4), np.float32)
    else:
        v = np.zeros((Tn, KT, 2, 2, 32, 8), np.uint16)
    nv, ne = v.shape[2], v.shape[5]
    for vec in range(nv):
        for e in range(ne):
            for h in range(2):
                rows = m[:, _row(ne * vec + e, h)].transpose(1, 0, 2)          # (T, KT, column)
                if ctx.mode == "f32":
                    v[:, :, vec, h, :, e] = rows
                elif ctx.mode == "bf16":
                    v[:, :, vec, h, :, e] = (np.ascontiguousarray(rows).view(np.uint32) >> 16).astype(np.uint16)
                else:
                    v[:, :, vec, h, :, e] = np.ascontiguousarray(rows.astype(np.float16)).view(np.uint16)
    ctx.buf[int(ctx.slot_off[slot]):int(ctx.slot_off[slot + 1])] = v.reshape(-1).view(np.uint8)


def write_plane(ctx, name, B):
    """(32 KT, 32 T) bool -> the bit plane of forward stage `name`."""
    Tn, KT = ctx.tiles32, ctx.slot_tiles[ctx.slots[name]]
    b = np.asarray(B, bool).reshape(KT, 32, Tn, 32)
    w = np.zeros((Tn, 2, 32, 4), np.uint32)
    for m in range(KT):
        for r in range(16):
            for h in range(2):
                w[:, h, :, m >> 1] |= b[m, _row(r, h)].astype(np.uint32) << (16 * (m & 1) + 15 - r)
    off = ctx.plane_off + ctx.planes[name] * Tn * 1024
    ctx.buf[off:off + Tn * 1024] = w.reshape(-1).view(np.uint8)


def write_gate(ctx, G):
    g = np.ascontiguousarray(G, np.float32)
    ctx.buf[ctx.gate_off:ctx.gate_off + g.nbytes] = g.reshape(-1).view(np.uint8)


def operand_values(seed, shape, mode):
    """Values in (-2, 2) that the operand type of `mode` holds exactly."""
    u = torch.from_numpy(O.uniform01(seed, int(np.prod(shape))).reshape(shape) * 4 - 2).float()
    return O.quantize(u, mode).numpy()


def host_context(L, variant, depth, dino_dim, mode, n, seed=1):
    """A context of the library's plan, every slot, plane and the gate filled from the counter hash."""
    kw = dict(dino_dim=dino_dim) if variant == "v3" else {}
    p = O.make_weights(variant, 0, "fog", n_layers=depth, **kw)
    plan = train_plan(L, variant, p, depth, dino_dim or 64, with_planes=True)
    Tn = (n + 255) // 256 * 8
    tb = 4096 if mode == "f32" else 2048
    nbytes = sum(plan[1]) * Tn * tb + plan[3] * Tn * 1024 + (Tn * 32 * 8 if variant == "v3" else 0)
    ctx = T.SavedContext(plan, variant, depth, mode, n, np.zeros(nbytes, np.uint8))
    for s, kt in enumerate(ctx.slot_tiles):
        write_slot(ctx, s, operand_values(seed + s, (32 * kt, 32 * Tn), mode))
    for k, name in enumerate(ctx.planes):
        write_plane(ctx, name, O.uniform01(seed + 100 + k, 32 * ctx.slot_tiles[ctx.slots[name]] * 32 * Tn).reshape(-1, 32 * Tn) < 0.5)
    if variant == "v3":
        write_gate(ctx, O.uniform01(seed + 200, Tn * 32 * 2).reshape(-1, 2))
    return ctx


def twin(ctx, variant, depth):
    return T.SavedContext((None, ctx.slot_tiles, None, len(ctx.planes)), variant, depth, ctx.mode, ctx.n, ctx.buf.copy())


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_freq", [10, 12])
def test_kernel_feature_order_is_a_permutation_with_padding(L_freq):
    order = T.kernel_feature_order(L_freq)
    real = order[order >= 0]
    assert sorted(real.tolist()) == list(range(O.encoded_dim(L_freq)))          # every reference feature exactly once
    assert len(order) == 32 * ((3 * L_freq + 2 + 15) // 16) and int((order < 0).sum()) == len(order) - O.encoded_dim(L_freq)


@pytest.mark.parametrize("mode", MODES)
def test_writers_invert_the_decoders(L, mode):
    """The packers of this file against SavedContext's decoders, over every slot, plane and the gate of a V3 plan."""
    n = 300
    ctx = host_context(L, "v3", 2, 64, mode, n)
    Tn = ctx.tiles32
    for s, kt in enumerate(ctx.slot_tiles):
        assert np.array_equal(ctx.slot_number(s), operand_values(1 + s, (32 * kt, 32 * Tn), mode)), s
    for k, name in enumerate(ctx.planes):
        exp = O.uniform01(101 + k, 32 * ctx.slot_tiles[ctx.slots[name]] * 32 * Tn).reshape(-1, 32 * Tn) < 0.5
        assert np.array_equal(ctx.plane(name), exp), name
    assert np.array_equal(ctx.gate(), O.uniform01(201, Tn * 32 * 2).reshape(-1, 2).astype(np.float32))


@pytest.mark.parametrize("mode", MODES)
def test_x_enc_from_input_slot_inverts_the_packing(L, mode):
    n = 300                                                     # 9 whole sample tiles and 12 columns of a tenth; padded to 512
    ctx = host_context(L, "v1", 8, 0, mode, n)
    Tn = ctx.tiles32
    x = operand_values(77, (n, 63), mode)
    x[0, :4] = [0.0, -0.0, 2.0 ** -20 if mode != "f32" else 2.0 ** -140, -1.0]      # zeros of both signs, an f16 subnormal
    order = T.kernel_feature_order(10)
    M = np.zeros((64, 32 * Tn), np.float32)
    M[order >= 0, :n] = x[:, order[order >= 0]].T
    M[:, n:] = 5.0                                              # padded columns hold whatever the route left there
    write_slot(ctx, ctx.slots["input"], M)
    got, pad = T.x_enc_from_input_slot(ctx)
    assert got.shape == (n, 63) and got.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.uint32), x.view(np.uint32))
    assert pad.shape == (1, n) and np.abs(pad).max() == 0.0
    M[order < 0, 17] = 0.25                                     # a planted non-zero in the padding row reaches the caller
    write_slot(ctx, ctx.slots["input"], M)
    _, pad = T.x_enc_from_input_slot(ctx)
    assert pad[0, 17] == 0.25 and np.count_nonzero(pad) == 1


@pytest.mark.parametrize("mode", MODES)
def test_context_differences_reports_planted_differences_at_their_stage(L, mode):
    variant, depth, dd, n = "v3", 2, 64, 300
    a = host_context(L, variant, depth, dd, mode, n)
    fwd, bwd = T.stage_names(variant, depth)
    every = fwd + bwd
    diff = lambda b, stages=every: T.context_differences(a, b, variant, depth, dd, stages)
    assert diff(twin(a, variant, depth)) == []

    def flipped_slot(name, row, sample, b=None):
        b = b or twin(a, variant, depth)
        M = b.slot(name)
        M[row, sample] = -M[row, sample] if M[row, sample] != 0 else 1.0
        write_slot(b, b.slots[name], M)
        return b

    # one element of a trunk slot: in a whole sample tile, in the ragged last one, in its last real column
    for sample in (5, 290, n - 1):
        assert diff(flipped_slot("trunk.1", 77, sample)) == [T.Difference("trunk.1", 1, (77, sample))]
    # a backward slot, and only where it is asked for
    b = flipped_slot("dz_fusion0.1", 3, 40)
    assert diff(b) == [T.Difference("dz_fusion0.1", 1, (3, 40))]
    assert diff(b, fwd) == [] and diff(b, bwd) == [T.Difference("dz_fusion0.1", 1, (3, 40))]
    # one ReLU-plane bit
    for name, row, sample in (("fusion2.0", 200, 7), ("attention0", 33, 299)):
        b = twin(a, variant, depth)
        B = b.plane(name)
        B[row, sample] = ~B[row, sample]
        write_plane(b, name, B)
        assert diff(b) == [T.Difference("mask." + name, 1, (row, sample))]
    # one gate pair
    b = twin(a, variant, depth)
    G = b.gate().copy()
    G[123] = [0.25, 0.75]
    write_gate(b, G)
    assert diff(b) == [T.Difference("gate", 2, (0, 123))]
    assert diff(b, [s for s in every if s != "gate"]) == []
    # padded columns: every slot, every plane and the gate differ past n, nothing is reported
    b = twin(a, variant, depth)
    for s in range(len(b.slot_tiles)):
        M = b.slot_number(s)
        M[:, n:] = 9.0
        write_slot(b, s, M)
    for name in b.planes:
        B = b.plane(name)
        B[:, n:] = ~B[:, n:]
        write_plane(b, name, B)
    G = b.gate().copy()
    G[n:] = 0.5
    write_gate(b, G)
    assert not np.array_equal(a.buf, b.buf) and diff(b) == []
    # several at once: chain order, counts, the first by sample
    b = flipped_slot("proj", 9, 200)
    b = flipped_slot("proj", 250, 31, b)
    b = flipped_slot("input.0", 0, 0, b)
    assert diff(b) == [T.Difference("input.0", 1, (0, 0)), T.Difference("proj", 2, (250, 31))]


def test_context_differences_names_v1_stages(L):
    a = host_context(L, "v1", 2, 0, "bf16", 70)
    b = twin(a, "v1", 2)
    M = b.slot("dz_head")
    M[2, 69] += 1.0
    write_slot(b, b.slots["dz_head"], M)
    fwd, bwd = T.stage_names("v1", 2)
    assert (fwd, bwd) == (["input", "trunk.0", "trunk.1"], ["dz_head", "dz_trunk.1", "dz_trunk.0"])
    assert T.context_differences(a, b, "v1", 2, 0, fwd) == []
    assert T.context_differences(a, b, "v1", 2, 0, fwd + bwd) == [T.Difference("dz_head", 1, (2, 69))]


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_operand_rounding_is_idempotent_on_every_bit_pattern(mode):
    """The premise of feeding a staged forward the ray route's decoded encoding: rounding a value that is in the operand type
    already changes no bit -- all 2^16 patterns, the finite ones kept (subnormals and both zeros among them)."""
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = u.view(np.float16).astype(np.float32) if mode == "f16" else (u.astype(np.uint32) << 16).view(np.float32)
    v = v[np.isfinite(v)]
    assert len(v) == (65536 - 2 * 1024 if mode == "f16" else 65536 - 2 * 128)
    assert (v == 0).sum() == 2 and np.signbit(v[v == 0]).sum() == 1
    tiny = 2.0 ** -14 if mode == "f16" else 2.0 ** -126
    assert int(((v != 0) & (np.abs(v) < tiny)).sum()) == (2 * 1023 if mode == "f16" else 2 * 127)          # every subnormal
    q = O.quantize(torch.from_numpy(v), mode).numpy()
    assert np.array_equal(q.view(np.uint32), v.view(np.uint32))
