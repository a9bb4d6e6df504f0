"""The feature-by-feature probe of the in-kernel positional encoders (test infrastructure of tests/test_gpu_encoder_probe.py and
of its CPU half, tests/test_encoder_probe_host.py).  No kernels here.

THE PROBE.  encode3 (csrc/nets.hpp) has three implementations, chosen by Mode::TRIG: the hardware sine on split-product turns
(1: bf16, f16), a polynomial on the same reduction (2: f16x3) and ocml sincosf (0: f32).  An encoder fault looks to a trained
network like a slightly different scene, so nothing behind 256-wide layers can localise it.  A SELECTOR network can: weights in
{0, +-1, +-2, 1/2} and zero biases that make the network an exact wire from ONE encoder feature to an output.

  V2 / V3 position features   first Linear: feature k -> unit 2k with +1 (V3: +2), unit 2k+1 with -1 (-2): relu(e), relu(-e).
                              Later layers: the identity.  density_head = [+1 at 2k, -1 at 2k+1]: density = relu(e_k); the
                              sign-flipped row gives relu(-e_k); e_k = d+ - d-, exact because one of the two is 0.  Only the
                              head row changes between forwards.  V3: attention.2 = 0 with bias (0, 0), so the gate is exactly
                              (1/2, 1/2) in every mode (exp(0) = 1), and fusion.0's +-2 undoes encode3's `v * scale` exactly;
                              fusion.0's DINO columns are 0 and the DINO input is random: it must not leak.
  direction features (L = 4)  color_layers.0 takes the +- pair from the direction tile, color_layers.2 is the identity,
                              color_layers.4 row c = h+ - h-: rgb_c = sigmoid(e), three features per forward,
                              e = logit(rgb) in float64.  The same state dict carries the V2 position wire.
  V1 (L = 10)                 reachable only through a one-sample render (render_probe.py's premise): sigma_out = 0 x h + 1, so
                              alpha = 1 exactly and the pixel is sigmoid(e) bit for bit.  The rays are (o, d, z) = (0, p, 1), whose
                              point render_probe.points32 gives as p itself, so the special inputs survive.  The raw x, y, z rows
                              (|e| <= 8, where a sigmoid is flat) travel through weights 1/2, 1/2, 1/2: the pixel is
                              sigmoid(e / 8) and e = 8 logit(rgb); the scaling is exact in every operand type.

THE REFERENCE is oracle.positional_encoding64: float64 sin / cos of the exact product x 2^f of the fp32 input.

THE BOUNDS (U = 2^-24; e the float64 encoding, a the observed value).  None comes from what the kernels give.

  bf16, f16   the wire carries q(e) exactly (weights +-1, +-2, 1/2: powers of two; already-rounded activations; fp32
              accumulation of one non-zero product).  The project's encoder-stage rule (tests/train_ctx.py):
              |a - q(e)| <= ulp max(|q(e)|, 2^-4), ulp = train_ctx.ULP[mode], q = round to the operand type.
  f32         the wire is exact.  4 ulp: 4 x 2^-23 max(|e|, 2^-4) -- OpenCL's full-profile bound for sincos, which ocml is built to
              meet; the floor has the form of the project's own rule.
  f16x3       2e-7 + k 2^-22 |e| + k_abs 2^-25.  2e-7 is the documented claim of nets.hpp.  Every conversion of an fp32 activation
              to a split-f16 operand (mlp_core.hpp: ModeF16X3::to_act) keeps hi + lo with |x - hi - lo| <= 2^-22 |x| (lo = f16(x -
              hi) rounds a value below 2^-11 |x| to 11 bits) plus half the f16 subnormal step, 2^-25, where lo is subnormal.  k is
              the number of such conversions between the encoder and the output; k_abs counts the absolute term in units of e
              (a conversion of e / s weighs s).  The products are exact (weights are powers of two: W_lo = 0).
                V2 position   encoder tile, layer 0, layer 1 -> density_head                          k = 3, k_abs = 3
                V3 position   encoder tile (at half scale: weighs 2), fusion.0, fusion.2, output_proj,
                              trunk 0, trunk 1 -> density_head                                         k = 6, k_abs = 7
                directions    encoder tile, color_layers.0, color_layers.2 -> color_layers.4          k = 3, k_abs = 3
                V1            encoder tile, layers.0, layers.1 -> rgb_out                             k = 3, k_abs = 3
                V1 raw rows   the same at scales 1, 1/2, 1/4                                          k = 3, k_abs = 1 + 2 + 4 = 7
              Where k_abs > k this is LOOSER than the k (2^-22 |e| + 2^-25) one gets by counting every conversion once: by 2^-25 = 3e-8
              for V3 and by 4 x 2^-25 = 1.2e-7 for V1's raw rows.  Counting once would not be a bound: the half step of a conversion
              taken at e / s is 2^-25 in units of e / s, s 2^-25 in units of e.
  through a sigmoid (directions, V1)   the kernel's 1 / (1 + expf(-x)) (device_math.hpp: sigmoid_precise), t = e^-x, s = 1 / (1 + t):
              ocml expf one ulp = 2 U t; the add U (1 + t); the divide U; one rounding of the stored colour U.  Relative to s:
              2 U t / (1 + t) + 3 U = U (2 (1 - s) + 3), so |ds| <= U s (5 - 2 s) <= 2.59 U on |x| <= 1 (s <= 0.7311):
              SIGMOID_ERR = 3 U.  e = logit(s) has slope 1 / (s (1 - s)) <= 5.1 on |e| <= 1 (5.086 at 1), so the bound grows by
              5.1 x 3 U (V1's raw rows: 8 times that, for the factor that undoes the 1/8).
  V1's raw rows   travel as e / 8 (not through the +-1 wire of the other rows: sigmoid(8) = 0.9997 is flat, logit(rgb) could not
              give e back), so in f32 and f16x3 their bound is dominated by 8 x 5.1 x 3 U = 7.3e-6.  That catches an exchanged, scaled or
              missing row, not a last-bit error; the raw rows of V2 / V3, which reach the density without a sigmoid, carry that check.
  bf16 through a sigmoid   sigmoid_fast (v_exp, v_rcp) has no documented error here; the 5e-3 that
              test_mlp_layout_exact_integers grants it is reused: 5.1 x 5e-3.  This case checks the WIRING only (a permuted, swapped
              or missing feature is off by O(1)); f16 runs the same TRIG == 1 code and carries the last-bit check.

THE INPUTS.  probe_points: 1531 points (ragged against 32 and 64), the bulk uniform in [-8, 8]^3, and in each of the three
components every special value: +-0, +-2^-130, +-1e-3, +-8; the fp32 neighbours of k pi / 2^f and (k + 1/2) pi / 2^f for three k
(k = 1, an even k at mid range -- a whole turn count, where path 1's fract wraps -- and one with |x| in (4, 8]) and
every f < 12 (the zeros of sin and cos, where an absolute error is all there is); values whose turn count is within 2 ulp of a
half-integer (the rint / fract seams); values just above and below 2 pi 2^j, where hi 2^f crosses a power of two.
probe_dirs: as many unit vectors, the six axis vectors among them.

THE MODEL.  encode_model replays the reductions of paths 1 and 2 in fp32 numpy with nets.hpp's constants (fma = a float64
product-and-sum rounded once; path 1 ends in float64 sin(2 pi rev) for the hardware sine).  It exists so that the comparer, the
inputs and the planted faults can be tested without a GPU; it is not a second source of bounds.
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import nerf_oracle as O
from tests.train_ctx import ULP

U = 2.0 ** -24
N_POINTS = 1531
MODES = ("f32", "f16x3", "f16", "bf16")
TRIG = {"bf16": 1, "f16": 1, "f16x3": 2, "f32": 0}
CLAIM = 2e-7                                    # nets.hpp: path 2, |x| <= 8, every frequency up to 2^14
SLOPE = 5.1                                     # 1 / (s (1 - s)) on |e| <= 1
SIGMOID_ERR = {"f32": 3 * U, "f16x3": 3 * U, "f16": 3 * U, "bf16": 5e-3}
K_SPLIT = {"v2": (3, 3), "v3": (6, 7), "dir": (3, 3), "v1": (3, 3), "v1raw": (3, 7)}        # (k, k_abs) of the f16x3 bound
RAW_GAIN = 8.0                                  # V1's raw rows travel as e / 8

f32 = np.float32
INV2PI_HI = f32(float.fromhex("0x1.45f306p-3"))
INV2PI_LO = f32(float.fromhex("0x1.b9391p-28"))
TWO_PI_HI = f32(float.fromhex("0x1.921fb6p+2"))
TWO_PI_LO = f32(float.fromhex("-0x1.777a5cp-23"))
POLY = [f32(float.fromhex(c)) for c in ("0x1.419126p+5", "-0x1.328822p+6", "0x1.466ad6p+6", "-0x1.4abbcep+5")]


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _neighbours(x, offsets):
    """fp32 values `offsets` ulps away from fl32(x)."""
    base = np.float32(x)
    out = []
    for o in offsets:
        v = base
        for _ in range(abs(o)):
            v = np.nextafter(v, f32(np.inf) if o > 0 else f32(-np.inf))
        out.append(v)
    return out


def special_values():
    """The 1-D special inputs, fp32 (module docstring: THE INPUTS)."""
    v = [0.0, -0.0, 2.0 ** -130, -2.0 ** -130, 1e-3, -1e-3, 8.0, -8.0]
    for f in range(12):
        sign = -1.0 if f & 1 else 1.0
        k_far = int(7.3 * 2 ** f / np.pi)                       # |x| in (4, 8]
        for k in (1, k_far):
            v += _neighbours(sign * k * np.pi / 2 ** f, (-1, 0, 1))                 # sin(2^f x) = 0
            v += _neighbours(-sign * (k + 0.5) * np.pi / 2 ** f, (-1, 0, 1))        # cos(2^f x) = 0
        k_mid = max(2, 2 * int(2.5 * 2 ** f / (2 * np.pi)))     # an even k at mid range: a whole turn count, path 1's fract seam
        v += _neighbours(-sign * k_mid * np.pi / 2 ** f, (-1, 1))
        v += _neighbours(sign * (k_mid + 0.5) * np.pi / 2 ** f, (-1, 1))
    for f, sign in ((0, 1.0), (5, -1.0), (9, 1.0), (11, -1.0)):                     # turn count m + 1/2: the rint / fract seams
        m = int(6.5 * 2 ** f / (2 * np.pi) - 0.5)                      # |x| <= 6.5
        v += _neighbours(sign * (m + 0.5) * 2 * np.pi / 2 ** f, (-2, -1, 0, 1, 2))
    for j in range(-6, 1):                                                          # hi 2^f crosses a power of two at x = 2 pi 2^j
        v += _neighbours((-1.0 if j & 1 else 1.0) * 2 * np.pi * 2.0 ** j, (-1, 1))
    return np.asarray(v, np.float32)


def probe_points(seed=7):
    """(1531, 3) fp32: every special value in each component (the other two uniform), then the uniform bulk."""
    sp = special_values()
    pts = (O.uniform01(seed, N_POINTS * 3).reshape(N_POINTS, 3) * f32(16.0) - f32(8.0)).astype(np.float32)
    assert 3 * len(sp) < N_POINTS // 2
    for i, x in enumerate(sp):
        for c in range(3):
            pts[3 * i + c, c] = x
    return pts


def probe_dirs(seed=8):
    """(1531, 3) fp32 unit vectors; the first six are the axis vectors and their negatives."""
    d = (O.uniform01(seed, N_POINTS * 3).reshape(N_POINTS, 3) * f32(2.0) - f32(1.0)).astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(np.float32)
    d[:6] = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    return d


# ---------------------------------------------------------------------------------------------
# features, bounds, comparer
# ---------------------------------------------------------------------------------------------
def n_features(L):
    return 3 * (2 * L + 1)


def feature_name(j):
    """Index into the reference's 3(2L+1) features -> ('raw' | 'sin' | 'cos', f (-1 for raw), component)."""
    if j < 3:
        return ("raw", -1, j)
    return ("cos" if (j - 3) % 6 >= 3 else "sin", (j - 3) // 6, (j - 3) % 3)


def feature_index(kind, f, c):
    return c if kind == "raw" else 3 + 6 * f + (3 if kind == "cos" else 0) + c


def target(e, mode):
    """The float64 encoding as the wire carries it: rounded to the operand type in the 16-bit modes."""
    e = np.asarray(e, np.float64)
    if mode in ("f16", "bf16"):
        t = torch.from_numpy(e).float()             # the encoder rounds an fp32 value; |e| <= 8: no double-rounding case matters at 2^-4 ulp
        return O.quantize(t, mode).double().numpy()
    return e


def bound(e, mode, wire, sigmoid=False):
    """(n, F) bound on |a - target(e)| for the selector `wire` ('v2' | 'v3' | 'dir' | 'v1') in `mode` (module docstring)."""
    e = np.abs(np.asarray(e, np.float64))
    if mode in ("f16", "bf16"):
        b = ULP[mode] * np.maximum(e, 2.0 ** -4)
    elif mode == "f32":
        b = 4 * ULP["f32"] * np.maximum(e, 2.0 ** -4)
    else:
        k, k_abs = K_SPLIT[wire]
        b = CLAIM + k * 2.0 ** -22 * e + k_abs * 2.0 ** -25
        if wire == "v1":
            k, k_abs = K_SPLIT["v1raw"]
            b[:, :3] = CLAIM + k * 2.0 ** -22 * e[:, :3] + k_abs * 2.0 ** -25
    if sigmoid:
        b = b + SLOPE * SIGMOID_ERR[mode]
        if wire == "v1":
            b[:, :3] += (RAW_GAIN - 1) * SLOPE * SIGMOID_ERR[mode]
    return b


Finding = namedtuple("Finding", "feature worst point index")        # worst: the largest |a - e| / bound; point: the offending input


def compare(observed, points, L, bound_fn, target_fn=None):
    """observed (n, 3(2L+1)) against the float64 encoding of `points` -> one Finding per feature.  Every point is checked: there is
    no cap and no element is left out (a NaN counts as infinitely far)."""
    e = O.positional_encoding64(torch.from_numpy(np.asarray(points, np.float32)), L).numpy()
    a = np.asarray(observed, np.float64)
    assert a.shape == e.shape == (len(points), n_features(L)), (a.shape, e.shape)
    t = e if target_fn is None else target_fn(e)
    ratio = np.abs(a - t) / bound_fn(t)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    out = []
    for j in range(e.shape[1]):
        i = int(np.argmax(ratio[:, j]))
        out.append(Finding(feature_name(j), float(ratio[i, j]), tuple(float(x) for x in points[i]), i))
    return out


def failed(findings):
    return [f for f in findings if not f.worst <= 1.0]


def worst(findings):
    return max(findings, key=lambda f: f.worst)


def record(what, findings):
    w = worst(findings)
    return f"RECORD {what}: worst |a-e|/bound {w.worst:.3f} at {w.feature[0]} f={w.feature[1]} c={w.feature[2]}, input {w.point}"


# ---------------------------------------------------------------------------------------------
# the fp32 model of encode3's paths 1 and 2
# ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _poly(v):
    """sin_turns_poly."""
    w = v * v
    q = np.full_like(v, POLY[0])
    for c in POLY[1:]:
        q = _fma(q, w, c)
    t = _fma(q, w, TWO_PI_LO)
    return _fma(v, TWO_PI_HI, v * t)


def _sin_or_cos_turns(u, want_cos):
    au = np.abs(u)
    if want_cos:
        return _poly(f32(0.25) - au)
    vs = np.minimum(au, f32(0.5) - au)
    return _poly(np.where(np.signbit(u), -vs, vs))              # the kernel XORs u's sign bit onto vs


def encode_model(points, L, trig, fault=None, fault_f=None):
    """(n, 3) fp32 -> (n, 3(2L+1)) in the reference's feature order: encode3 with Mode::TRIG = `trig` (1 or 2), fp32 operation by
    fp32 operation.  Path 1's hardware sine is float64 sin(2 pi rev).  `fault` plants one of FAULTS (at band `fault_f` where the
    fault has a band)."""
    assert trig in (1, 2) and fault in (None,) + FAULTS
    p = np.asarray(points, np.float32)
    out = np.zeros((len(p), n_features(L)), np.float64)
    out[:, :3] = p
    with np.errstate(under="ignore"):
        hi = p * INV2PI_HI
        lo = _fma(p, INV2PI_HI, -hi) + (f32(0) * p if fault == "no_inv2pi_lo" else p * INV2PI_LO)
        if fault == "no_lo":
            lo = np.zeros_like(hi)
        for f in range(L):
            here = fault_f == f
            scale = f32(2.0 ** (f + 1 if fault == "freq_off_by_one" and here else f))
            for h in (0, 1):
                want_cos = h ^ 1 if fault == "wrong_quarter" and here else h
                a = hi * scale
                if trig == 1:
                    fr = np.minimum(a - np.floor(a), f32(float.fromhex("0x1.fffffep-1")))
                    rev = _fma(lo, scale, fr) + (f32(0.25) if want_cos else f32(0.0))
                    v = np.sin(2.0 * np.pi * rev.astype(np.float64))
                else:
                    g = a - (np.trunc(a) if fault == "trunc" else np.rint(a))
                    v = _sin_or_cos_turns(_fma(lo, scale, g), want_cos).astype(np.float64)
                if fault == "swap_yz" and here:
                    v = v[:, [0, 2, 1]]
                out[:, 3 + 6 * f + 3 * h: 6 + 6 * f + 3 * h] = v
    return out


FAULTS = ("no_inv2pi_lo", "no_lo", "trunc", "wrong_quarter", "swap_yz", "freq_off_by_one")


# ---------------------------------------------------------------------------------------------
# selector networks
# ---------------------------------------------------------------------------------------------
def _zeros(variant, **kw):
    p = {}
    for name, o, i in O.layer_shapes(variant, **kw):
        p[name + ".weight"], p[name + ".bias"] = torch.zeros(o, i), torch.zeros(o)
    return p


def _pairs(w, n, gain=1.0, col0=0):
    """Feature k of columns col0 .. col0 + n -> unit 2k with +gain, unit 2k+1 with -gain."""
    for k in range(n):
        w[2 * k, col0 + k], w[2 * k + 1, col0 + k] = gain, -gain


def pair_row(width, k, sign=1.0, gain=1.0):
    """A head row that reads feature k off its +- pair: sign (h+ - h-)."""
    row = torch.zeros(width)
    row[2 * k], row[2 * k + 1] = sign * gain, -sign * gain
    return row


def v2_selector():
    """V2 (L = 10, trunk depth 2) with the position wire into density_head and the direction wire (L = 4) into color_layers.4;
    both head matrices are zero until a test sets a row (density_row / colour_rows).  f16x3: k = 3 on either wire."""
    p = _zeros("v2", pos_freq=10, n_layers=2)
    _pairs(p["density_mlp.density_layers.0.weight"], n_features(10))
    p["density_mlp.density_layers.2.weight"] = torch.eye(256)
    _pairs(p["color_mlp.color_layers.0.weight"], n_features(4), col0=256)
    p["color_mlp.color_layers.2.weight"][:, :64] = torch.eye(64)
    return p


def v3_selector(dino_dim=64):
    """V3 (L = 12, trunk depth 2): the gate is exactly (1/2, 1/2), fusion.0 selects with +-2.  f16x3: k = 6, k_abs = 7."""
    p = _zeros("v3", pos_freq=12, n_layers=2, dino_dim=dino_dim)
    _pairs(p["dino_fusion.fusion.0.weight"], n_features(12), gain=2.0)
    for name in ("dino_fusion.fusion.2", "dino_fusion.output_proj", "density_mlp.density_layers.0", "density_mlp.density_layers.2"):
        p[name + ".weight"] = torch.eye(256)
    return p


def density_row(k, sign):
    return pair_row(256, k, sign)[None]


def colour_rows(triple):
    """color_layers.4 (3, 64): row c reads direction feature 3 triple + c."""
    return torch.stack([pair_row(64, 3 * triple + c) for c in range(3)])


def v1_selector():
    """V1 (L = 10, two layers): sigma_out = 0 x h + 1; the raw rows travel through weights 1/2 (layers.0, layers.1, rgb_out).
    f16x3: k = 3, k_abs = 3 (raw rows 7)."""
    p = _zeros("v1", pos_freq=10, n_layers=2)
    _pairs(p["layers.0.weight"], n_features(10))
    p["layers.0.weight"][:6] *= 0.5
    p["layers.1.weight"] = torch.eye(256)
    p["layers.1.weight"][:6] *= 0.5
    p["sigma_out.bias"] = torch.ones(1)
    return p


def v1_rgb_rows(triple):
    """rgb_out (3, 256): row c reads position feature 3 triple + c (the raw triple with 1/2)."""
    return torch.stack([pair_row(256, 3 * triple + c, gain=0.5 if triple == 0 else 1.0) for c in range(3)])


def logit64(rgb):
    s = np.asarray(rgb, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(s) - np.log1p(-s)
