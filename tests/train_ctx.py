"""The saved context of the training path, decoded, and the stage-wise comparer built on it (test infrastructure shared by
tests/test_gpu_training.py, tests/test_gpu_train_stages.py and the CPU tests of the comparer, tests/test_train_stage_model.py);
and the bit-for-bit comparer of TWO contexts (context_differences, x_enc_from_input_slot: tests/test_gpu_train_rays_link.py and
its CPU half, tests/test_train_rays_link_host.py).

Slot sizes, the number of ReLU bit planes and with them the place of the V3 gate pairs come from the plan the library reports
(nrf_debug_train_plan, parsed by tests/test_training_host.py:train_plan); the context is laid out as train_impl.hpp:fill_slots
lays it out: the slots, the bit planes (1 KiB per 32 samples each), then the gate (two fp32 per padded sample).  Which slot
holds what is csrc/train_slots.hpp, restated here by name; the restatement is checked against the plan's counts.

The comparer holds every stage of a forward_train / backward pair to oracle.train_stages applied to the SAME stage inputs
(`given`), so that no flipped last bit or ReLU mask travels from one stage into the next:

  network stage   |a - e| <= ulp |e| + 1e-6 max|e|   ulp = 2^-10 (f16), 2^-7 (bf16): one operand-type ulp, as V1's test;
                  at most 4 + n // 2000 elements outside (mask and rounding flips); ReLU planes: as many mismatches
  encoder stage   |a - e| <= ulp max(|e|, 2^-4)       e = the float64 encoding rounded to the operand type: one flipped last
                  bit where the value is resolved, an absolute floor below; no element outside.  The PE rows of the gated
                  input [pe w0 | dino w1] are held to this bound too (the kernel re-encodes: the encoder's error is absolute,
                  not relative to a value near a zero crossing); its DINO rows are a network stage (exact fp32 inputs)
  gate            |w - softmax64(logits from the saved attention.0)| <= 1e-6 (f16: libm expf) or 2e-3 (bf16: __expf; no error
                  figure for that intrinsic is documented here, so the bound V1's test grants the fast sigmoid is reused),
                  and |w0 + w1 - 1| <= 1e-6
  d_gate          |a - e| <= ulp |e| + 32 KT0 2^-24 (|w0 dw0| + |w1 dw1|): a difference of two fp32 dot products over 32 KT0
                  terms, bounded by the terms before the cancellation

One operand ulp is also what truncation (round toward zero) stays within, element by element.  What gives it away is how MANY
elements differ at all: both sides round the same sum, accumulated in two orders, so they differ only where the two sums
straddle a rounding boundary -- a share of 2 delta / spacing of the non-zero elements, delta the accumulation error.  Its worst
case over a K = 256 layer, delta = K 2^-24 |sum|, against the f16 spacing of at least 2^-11 |sum| is 6 % (bf16: 0.8 %); truncation
changes every element whose dropped bits round up, half of them.  So every rounded stage may differ from the reference in at most
DIFFER_SHARE = 10 % of its non-zero elements (d_gate, whose bound is about cancellation, and the fp32 gate are exempt).
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import nerf_oracle as O

ULP = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10, "f32": 2.0 ** -23}


def kernel_feature_order(L=10):
    """Row of an encoder tile -> index into the reference's 3(2L+1) encoded features (-1 = padding); feature_map.hpp."""
    KT = (3 * L + 2 + 15) // 16
    idx = np.full(32 * KT, -1)
    for u in range(16 * KT):
        for h in range(2):
            t, r = u // 16, u % 16
            k = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h
            if u < 3 * L:
                idx[k] = 3 + 6 * (u // 3) + 3 * h + (u % 3)
            elif u == 3 * L:
                idx[k] = 2 if h else 0
            elif u == 3 * L + 1:
                idx[k] = -1 if h else 1
    return idx


def slot_numbers(variant, n):
    """csrc/train_slots.hpp by name: ({stage: slot}, {forward stage: ReLU bit plane}, slots, planes)."""
    s, pl = {}, {}

    def colour(fwd, bwd, plane):
        s.update({"colour.in": fwd, "colour.c0": fwd + 1, "colour.c2": fwd + 2, "dz_density": bwd, "d_feature": bwd + 1,
                  "dz_c0": bwd + 2, "dz_c2": bwd + 3, "d_logits": bwd + 4})
        pl.update({"colour.c0": plane, "colour.c2": plane + 1})
    if variant == "v1":
        s["input"] = 0
        for j in range(n):
            s[f"trunk.{j}"], s[f"dz_trunk.{j}"], pl[f"trunk.{j}"] = 1 + j, n + 1 + j, j
        s["dz_head"] = 2 * n + 1
        return s, pl, 2 * n + 2, n
    if variant == "v2":
        s["input"] = 0
        for j in range(n):
            s[f"trunk.{j}"], s[f"dz_trunk.{j}"], pl[f"trunk.{j}"] = 1 + j, n + 4 + j, j
        colour(n + 1, 2 * n + 4, n)
        return s, pl, 2 * n + 9, n + 2
    for ps in (0, 1):
        s[f"input.{ps}"], s[f"fusion0.{ps}"], s[f"fusion2.{ps}"] = 4 * ps, 1 + 4 * ps, 2 + 4 * ps
        s[f"dz_fusion0.{ps}"], s[f"dz_fusion2.{ps}"] = 11 + n + 4 * ps, 12 + n + 4 * ps
        pl[f"fusion0.{ps}"], pl[f"fusion2.{ps}"] = 3 * ps, 1 + 3 * ps
    s.update({"attention0": 3, "proj": 7, "dz_attention0": 13 + n, "d_gate": 14 + n, "dz_proj": 17 + n})
    pl["attention0"] = 2
    for j in range(n):
        s[f"trunk.{j}"], s[f"dz_trunk.{j}"], pl[f"trunk.{j}"] = 8 + j, 18 + n + j, 5 + j
    colour(8 + n, 18 + 2 * n, 5 + n)
    return s, pl, 23 + 2 * n, 7 + n


class SavedContext:
    """The context buffer of one forward_train / backward pair.  plan = train_plan(..., with_planes=True)."""

    def __init__(self, plan, variant, n_layers, mode, n, buf):
        _, self.slot_tiles, _, n_planes = plan
        self.slots, self.planes, count, planes = slot_numbers(variant, n_layers)
        assert count == len(self.slot_tiles) and planes == n_planes, "train_slots.hpp and the reported plan disagree"
        self.mode, self.n = mode, n
        self.tiles32 = (n + 255) // 256 * 8
        self.tb = 4096 if mode == "f32" else 2048
        self.buf = buf                        # a device tensor stays where it is: a decoder fetches the bytes of its own slot only
        self.slot_off = np.concatenate([[0], np.cumsum(np.asarray(self.slot_tiles, np.int64) * self.tiles32 * self.tb)])
        self.plane_off = int(self.slot_off[-1])
        self.gate_off = self.plane_off + n_planes * self.tiles32 * 1024

    def bytes(self, start, stop):
        """Bytes start .. stop of the context as a numpy uint8 array on the host."""
        part = self.buf[int(start):int(stop)]
        return part.cpu().numpy() if isinstance(part, torch.Tensor) else part

    def slot_number(self, slot):
        """Saved-tensor slot -> (features, padded samples) fp32 matrix."""
        T, KT = self.tiles32, self.slot_tiles[slot]
        raw = self.bytes(self.slot_off[slot], self.slot_off[slot + 1])
        if self.mode == "f32":
            v = raw.view(np.float32).reshape(T, KT, 4, 2, 32, 4)              # sample tile, tile, vec, lane half, column, e
        else:
            u = raw.view(np.uint16).reshape(T, KT, 2, 2, 32, 8)
            v = (u.astype(np.uint32) << 16).view(np.float32) if self.mode == "bf16" else u.view(np.float16).astype(np.float32)
        nv, ne = v.shape[2], v.shape[5]
        out = np.zeros((KT, 32, T, 32), np.float32)
        for vec in range(nv):
            for e in range(ne):
                r = ne * vec + e
                for h in range(2):
                    out[:, (r & 3) + 8 * (r >> 2) + 4 * h] = v[:, :, vec, h, :, e].transpose(1, 0, 2)      # accumulator row map
        return out.reshape(32 * KT, 32 * T)

    def slot(self, name):
        return self.slot_number(self.slots[name])

    def plane(self, name):
        """ReLU bit plane of a forward stage -> (features, padded samples) bool (train_core.hpp: tile m in half m & 1 of
        dword m >> 1, accumulator register r at bit 15 - r of that half)."""
        T, KT = self.tiles32, self.slot_tiles[self.slots[name]]
        off = self.plane_off + self.planes[name] * T * 1024
        w = self.bytes(off, off + T * 1024).view(np.uint32).reshape(T, 2, 32, 4)                          # sample tile, half, column, dword
        out = np.zeros((KT, 32, T, 32), bool)
        for m in range(KT):
            half = (w[..., m >> 1] >> (16 * (m & 1))) & 0xffff
            for r in range(16):
                for h in range(2):
                    out[m, (r & 3) + 8 * (r >> 2) + 4 * h] = ((half[:, h] >> (15 - r)) & 1).astype(bool)
        return out.reshape(32 * KT, 32 * T)

    def gate(self):
        """(padded samples, 2) fp32: the V3 softmax gate (w0, w1)."""
        return self.bytes(self.gate_off, self.gate_off + self.tiles32 * 32 * 8).view(np.float32).reshape(-1, 2)


def _encoder_rows(rows, L, zeros, what):
    """(32 KT kernel-order rows, samples) -> (samples, 3(2L+1)) reference order; the padding rows go to `zeros`."""
    order = kernel_feature_order(L)
    out = np.zeros((rows.shape[1], 3 * (2 * L + 1)), np.float32)
    out[:, order[order >= 0]] = rows[order >= 0].T
    zeros.append((what + ": padding rows of the encoder tile", rows[order < 0]))
    return out


def saved_stages(ctx, variant, n_layers, dino_dim=0):
    """Every slot, plane and the gate of a decoded context under oracle.train_stages' names, (n, features) torch tensors in the
    reference's feature order; and the list of (what, array) the kernels promise to be exactly zero: padding rows of the
    encoder tiles and of the head gradients, and every gradient of a padded sample."""
    n, st, zeros = ctx.n, {}, []
    fwd, bwd = O.train_stage_names(variant, n_layers)
    pe_l = 12 if variant == "v3" else 10
    for name in fwd + bwd:
        if name == "gate":
            st[name] = torch.from_numpy(ctx.gate()[:n].copy())
            continue
        m = ctx.slot(name)
        if name in bwd:
            zeros.append((name + ": padded samples", m[:, n:]))
        m = m[:, :n]
        if name == "input":
            a = _encoder_rows(m, pe_l, zeros, name)
        elif name.startswith("input."):
            pt = 32 * ((3 * pe_l + 2 + 15) // 16)
            assert m.shape[0] == pt + dino_dim
            a = np.concatenate([_encoder_rows(m[:pt], pe_l, zeros, name), m[pt:].T], 1)
        elif name == "colour.in":
            a = np.concatenate([m[:256].T, _encoder_rows(m[256:], 4, zeros, name)], 1)
        elif name in ("d_logits", "dz_density", "d_gate"):
            k = {"d_logits": 3, "dz_density": 1, "d_gate": 2}[name]
            zeros.append((name + ": rows past the head's outputs", m[k:]))
            a = m[:k].T
        else:
            a = m.T
        st[name] = torch.from_numpy(np.ascontiguousarray(a))
    for name in ctx.planes:
        st["mask." + name] = torch.from_numpy(np.ascontiguousarray(ctx.plane(name)[:, :n].T))
    return st, zeros


def x_enc_from_input_slot(ctx, L=10):
    """V1's `input` slot as the (n, 3(2L+1)) fp32 tensor the staged entry points take (nrf_mlp_forward_train_v1's x_enc), in the
    reference's column order -- the inverse of kernel_feature_order -- and the slot's padding rows over the real samples, which
    the kernels promise to be exactly zero.  The values are in the operand type already, so the staged kernel's own rounding of
    them is the identity (tests/test_train_rays_link_host.py)."""
    zeros = []
    x = _encoder_rows(ctx.slot("input")[:, :ctx.n], L, zeros, "input")
    return torch.from_numpy(x), zeros[0][1]


# ---------------------------------------------------------------------------------------------
# two contexts of the same plan, bit for bit
# ---------------------------------------------------------------------------------------------
Difference = namedtuple("Difference", "stage count first")      # first: (row of the slot / plane in operand order, or gate component; sample)


def stage_names(variant, n_layers):
    """oracle.train_stage_names, and V1's chain under the same naming: (forward stages, backward stages) in chain order."""
    if variant == "v1":
        return (["input"] + [f"trunk.{j}" for j in range(n_layers)],
                ["dz_head"] + [f"dz_trunk.{j}" for j in range(n_layers - 1, -1, -1)])
    return O.train_stage_names(variant, n_layers)


def _equal_below_n(a, b, start, unit, inner, n):
    """Bytes of a region of sample tiles (`unit` bytes per 32 samples from `start`; inside a tile [.., 32 columns, `inner` bytes])
    over the samples < n: the whole tiles are contiguous, the ragged last one is compared column by column."""
    full, rem = divmod(n, 32)
    start = int(start)
    stop = start + full * unit
    if not torch.equal(a[start:stop], b[start:stop]):
        return False
    if rem:
        ra, rb = (t[stop:stop + unit].view(-1, 32, inner)[:, :rem] for t in (a, b))
        return torch.equal(ra, rb)
    return True


def _name_difference(stage, ma, mb, n):
    """Two decoded (rows, padded samples) matrices -> the Difference over the samples < n (None: bit-equal there)."""
    bits = lambda m: np.ascontiguousarray(m[:, :n]).view(np.uint8 if m.dtype == bool else np.uint32)
    d = bits(ma) != bits(mb)
    if not d.any():
        return None
    sample, row = (int(v) for v in np.argwhere(d.T)[0])
    return Difference(stage, int(d.sum()), (row, sample))


def context_differences(ctx_a, ctx_b, variant, n_layers, dino_dim, stages):
    """The stages (of `stages`, names as stage_names gives them) in which two decoded contexts of the same plan, mode and n hold
    different BITS: every named slot, the ReLU plane of every named forward stage ('mask.<stage>') and, under 'gate', the V3
    gate pairs.  One Difference per differing stage, in chain order; [] = the contexts are bit-equal there.

    Only the columns of real samples (< n) are compared.  The padded columns of the last 256-sample group are not owed: a chain
    kernel runs them on a copy of the LAST real sample's inputs (train_impl.hpp: ChainTile::sid), and a forward that derives its
    inputs (RaySample on row sid) rather than reading them is free to fill them otherwise; the backward zeroes them on every
    route (saved_stages' `zeros`).  Inside a real sample's column every byte is compared, the padding rows of an encoder tile
    and of a head gradient included: they are exact zeros on every route.

    The comparison runs on the raw bytes where the buffers live (on the GPU for device tensors): in each slot the sample tiles
    wholly below n are contiguous (fill_slots: [sample tile][tile][tile bytes]); only a slot that differs is decoded, to count
    and name the difference."""
    assert (ctx_a.mode, ctx_a.n, list(ctx_a.slot_tiles), ctx_a.gate_off) == (ctx_b.mode, ctx_b.n, list(ctx_b.slot_tiles), ctx_b.gate_off)
    slots, planes, _, _ = slot_numbers(variant, n_layers)
    assert slots == ctx_a.slots and (variant == "v3") == bool(dino_dim)
    fwd, bwd = stage_names(variant, n_layers)
    unknown = set(stages) - set(fwd) - set(bwd)
    assert not unknown, unknown
    n, T = ctx_a.n, ctx_a.tiles32
    a, b = (torch.from_numpy(c.buf) if isinstance(c.buf, np.ndarray) else c.buf for c in (ctx_a, ctx_b))
    out = []
    for name in fwd + bwd:
        if name not in stages:
            continue
        if name == "gate":
            if not _equal_below_n(a, b, ctx_a.gate_off, 32 * 8, 8, n):
                out.append(_name_difference(name, ctx_a.gate().T, ctx_b.gate().T, n))
            continue
        s = slots[name]
        if not _equal_below_n(a, b, ctx_a.slot_off[s], ctx_a.slot_tiles[s] * ctx_a.tb, 16, n):
            out.append(_name_difference(name, ctx_a.slot_number(s), ctx_b.slot_number(s), n))
        if name in planes and not _equal_below_n(a, b, ctx_a.plane_off + planes[name] * T * 1024, 1024, 16, n):
            out.append(_name_difference("mask." + name, ctx_a.plane(name), ctx_b.plane(name), n))
    assert None not in out, "the bytes differ where the decoded values do not: a decoder of this file is wrong"
    return out


# ---------------------------------------------------------------------------------------------
# the comparer
# ---------------------------------------------------------------------------------------------
Finding =namedtuple("Finding", "stage outliers allowed worst differ")      # worst: the largest |a - e| / bound; differ: share of non-zero elements that differ
DIFFER_SHARE = 0.10


def outlier_cap(n):
    return 4 + n // 2000


def gate_bound(mode):
    return 2e-3 if mode == "bf16" else 1e-6


def compare_stages(got, exp, variant, n_layers, mode, n):
    """got, exp: stage dicts (saved_stages / oracle.train_stages); exp = the model on got's own stage inputs.  One Finding per
    stage (the encoder rows of a concatenated input count as a stage of their own), in chain order."""
    ulp, cap = ULP[mode], outlier_cap(n)
    fwd, bwd = O.train_stage_names(variant, n_layers)
    n_pe = O.encoded_dim(12 if variant == "v3" else 10)
    out = []

    def add(stage, a, e, bound, allowed, rounded=True):
        a, e = a.double(), e.double()
        ratio = (a - e).abs() / bound
        differ = float((a != e).sum()) / max(1, int(((a != 0) | (e != 0)).sum())) if rounded else 0.0
        out.append(Finding(stage, int((ratio > 1).sum()), allowed, float(ratio.max()), differ))

    network = lambda stage, a, e: add(stage, a, e, ulp * e.double().abs() + 1e-6 * e.double().abs().max() + 1e-300, cap)
    encoder = lambda stage, a, e: add(stage, a, e, ulp * e.double().abs().clamp_min(2.0 ** -4), 0)
    for name in fwd + bwd:
        a, e = got[name], exp[name]
        assert a.shape == e.shape, (name, a.shape, e.shape)
        if name in ("input", "input.0"):
            encoder(name, a, e)
        elif name == "input.1":
            encoder(name + "[pe]", a[:, :n_pe], e[:, :n_pe])
            network(name + "[dino]", a[:, n_pe:], e[:, n_pe:])
        elif name == "colour.in":
            network(name + "[feature]", a[:, :256], e[:, :256])
            encoder(name + "[dir]", a[:, 256:], e[:, 256:])
        elif name == "gate":
            add(name, a, e, torch.full_like(e.double(), gate_bound(mode)), 0, rounded=False)
            add(name + "[sum]", a.double().sum(-1), torch.ones(a.shape[0]), torch.full((a.shape[0],), 1e-6).double(), 0, rounded=False)
        elif name == "d_gate":
            kt0 = 3 + (got["input.0"].shape[1] - n_pe) // 32          # 75 PE features in 3 tiles, dino_dim / 32 more
            add(name, a, e, ulp * e.double().abs() + 32 * kt0 * 2.0 ** -24 * exp["d_gate.terms"].double() + 1e-300, cap, rounded=False)
        else:
            network(name, a, e)
        if "mask." + name in got:
            out.append(Finding("mask." + name, int((got["mask." + name] != exp["mask." + name]).sum()), cap, 0.0, 0.0))
    return out


def failed(findings):
    return [f for f in findings if f.outliers > f.allowed or f.differ > DIFFER_SHARE]


# ---------------------------------------------------------------------------------------------
# planted faults: taps for oracle.train_stages (tests/test_train_stage_model.py, tests/test_render_link_host.py)
# ---------------------------------------------------------------------------------------------
def truncate(t, mode):
    """Round toward zero to the operand type (a normal-range value: clear the dropped mantissa bits)."""
    drop = 16 if mode == "bf16" else 13
    return (t.contiguous().view(torch.int32) & ~((1 << drop) - 1)).view(torch.float32)


def fault(kind, name, fn):
    return lambda k, nm, t: fn(t) if (k, nm) == (kind, name) else t


# ---------------------------------------------------------------------------------------------
# the committed cases of the stage tests: weights and inputs, from counter-based hashes (no torch RNG)
# ---------------------------------------------------------------------------------------------
FAMILIES = [("v2", 0), ("v3", 64), ("v3", 128)]                 # (family, dino_dim)
SEEDS = {("v2", 8): 4, ("v2", 2): 5, ("v3", 8): 4, ("v3", 2): 4}      # (family, depth): seeds whose 'solid' density ReLU is open for 55 .. 75 % of the samples


def stage_case(variant, dino_dim, depth, n):
    """Weights ('solid': the density ReLU is open for a fair share of the samples, so both of its branches are exercised) and
    inputs of one case."""
    kw = dict(dino_dim=dino_dim) if variant == "v3" else {}
    p = O.make_weights(variant, SEEDS[(variant, depth)], "solid", n_layers=depth, **kw)
    u = lambda seed, shape: torch.from_numpy(O.uniform01(seed, int(np.prod(shape))).reshape(shape)).float()
    seed = 45
    x = dict(pos=u(seed, (n, 3)) * 4 - 2, dirs=u(seed + 1, (n, 3)) * 2 - 1, g_rgb=u(seed + 2, (n, 3)) - 0.5, g_den=u(seed + 3, (n, 1)) - 0.5,
             dino=u(seed + 9, (n, dino_dim)) * 2 - 1 if variant == "v3" else None)
    return p, x


def density_open_share(p, variant, x):
    with torch.no_grad():
        den = (O.mlp_v3(p, x["pos"], x["dirs"], x["dino"]) if variant == "v3" else O.mlp_v2(p, x["pos"], x["dirs"]))[1]
    return float((den > 0).float().mean())


def model_on(p, variant, x, mode, acc=torch.float64, given=None, tap=None):
    """oracle.train_stages on a case's inputs, the encodings in float64."""
    return O.train_stages(p, variant, O.positional_encoding64(x["pos"], 12 if variant == "v3" else 10), O.positional_encoding64(x["dirs"], 4),
                          x["g_rgb"], x["g_den"], dino=x["dino"], mode=mode, acc=acc, given=given, tap=tap)
