"""The per-sample probe of the fused renderers and the arithmetic the render-link tests share (test infrastructure of
tests/test_gpu_render_link.py and of its CPU half, tests/test_render_link_host.py).

THE PROBE.  A render with ONE sample per ray composites that sample with dist = 1e10 |d| (device_math.hpp: Composite, the
reference's tail rule), so its opacity is a step function of the network's density:

    alpha = 1 - expf(-max(sigma, 0) * 1e10 |d|)  ==  1.0 exactly for sigma >= 1e-8,  0.0 exactly for sigma <= 0

(the premise, proved for the tests' range of |d| in test_render_link_host.py).  Without a white background the pixel of an
open sample (w == 1) is 0 + 1 * sigmoid(logit): the network's colour at that point, bit for bit; of a closed one (w == 0)
it is 0 and tells nothing.  `z_in` puts the one sample at any depth, so probe() reads the network out column by column on
the depths of an S-sample render.  Samples that are neither open nor closed (0 < sigma < ~2e-9) are left out; a case may
lose at most LEFT_OUT_CAP of its samples that way and must keep MIN_SHARE of them open and MIN_SHARE closed.

THE BOUNDS of the compositor check (u = 2^-24, the unit roundoff of fp32; every operation of Composite::add_alpha is one
rounded fp32 operation, device_math.hpp):

  rgb, depth   the kernel adds S rounded products w_s c_s front to back: S - 1 rounded additions of partial sums that never
               exceed sum_s w_s |c_s| (1 + S u), and S rounded products.  The worst case of a correct implementation against
               the exact sum of the SAME w_s, c_s is therefore  S u sum_s w_s |c_s|.  With the white background the image is
               fl(rgb + fl(1 - acc)), acc the recursive fp32 sum of the weights: (S - 1) u sum w for acc, u |1 - sum w| for the
               subtraction, u |rgb + 1 - sum w| for the addition.  The tests assert TWICE that worst case (so that the
               reference alone is provably within half of what is asserted), plus S 2^-149 for products that underflow:

                   bound_rgb   = 2 u (S sum w c + white ((S - 1) sum w + |1 - sum w| + |rgb_expected|)) / (1 - (S + 2) u) + S 2^-149
                   bound_depth = 2 u  S sum w z / (1 - (S + 2) u) + S 2^-149

  weights      w_s = alpha_s T_s from the staged forward's density (V2 / V3: bit-equal to what the renderer's network
               computes, which is the other half of the link).  In units of u, absolute:
                 dist = fl(fl(z' - z) |d|): both operations are replayed in fp32; |d| = sqrtf(...) is granted one ulp -> 2 u dist
                 x = fl(-sigma dist): 3 u |x| with the above; through e^x: 3 u |x| e^-|x| <= 3 u / e = 1.11 u
                 e = expf(x) <= 1: one ulp of a value below 1 = u (f32, f16x3, f16: libm expf, 1 ulp in the HIP
                   math API's table).  bf16: __expf(x) = v_exp_f32(fl(x fl(log2 e))): two roundings in the exponent, 2 u |y|,
                   through 2^y: 2 u |x| e^-|x| <= 0.74 u, plus v_exp_f32 itself, '1 ULP accuracy, denormals are flushed' in
                   AMD's GCN3 / Vega / CDNA instruction set guides (V_EXP_F32) = u, and a flushed result, 2^-126
                 alpha = fl(1 - e): u
               so  d_alpha = ALPHA_ERR u  with ALPHA_ERR = 4 (1.11 + 1 + 1, rounded up) and 5 for bf16 (1.11 + 0.74 + 1 + 1).
               The transmittance factor f = fl(fl(1 - alpha) + 1e-10f) adds two roundings of values <= 1: d_f = d_alpha + 2 u;
               T_{s+1} = fl(T_s f_s) with T, f <= 1 + 1e-10: d_T(s) <= s (d_f + u); w = fl(alpha T): d_alpha T + alpha d_T + u w.

                   bound_w(s) = 2 u (ALPHA_ERR + 1 + s (ALPHA_ERR + 3)) (1 + 1e-6)        (again twice the worst case)
"""
import numpy as np
import torch

from oracle import nerf_oracle as O

U = 2.0 ** -24
H, W = 19, 31                   # 589 rays: ragged against 64, 256 and the unit of 4
NEAR, FAR = 2.0, 6.0
S_VALUES = (2, 12, 70)          # 70: more than one 64-sample pass, and a ragged last one
# the even-deal cases: a frame with enough rays for the launcher to take the even deal (ray_deal.hpp: pick_deal) at these S
EVEN_H, EVEN_W = 67, 63
EVEN_CASES = [(70, "jitter"), (48, "z_in")]          # 70: two passes at SPW = 1, the last ragged; 48: inside one 64-sample pass
MODES = ("f32", "f16x3", "f16", "bf16")
LEFT_OUT_CAP = 0.01
MIN_SHARE = 0.10
SIGMA_FLOOR = 1e-8              # at and above: alpha of the one-sample render is exactly 1
ALPHA_ERR = {"f32": 4.0, "f16x3": 4.0, "f16": 4.0, "bf16": 5.0}

# net -> (family, dino_dim, make_weights seed, scene, source view of tests/golden/dino_views.npz ('own': the rendered camera), shift).
# The scene is make_weights' scene with the density head's bias moved by `shift`, so that the density ReLU is open on a fair
# share of THIS frame's samples and closed on another (the oracle's raw densities on the frame, fp32: median -0.107 for V1 'fog'
# seed 0, -8.5 / -8.9 for V3 'solid' seed 2 seen from 'orbit' / the rendered camera, +2.8 for the 128-d seed 3;
# test_render_link_host.py holds every case to MIN_SHARE of each).  V1 keeps 'fog', the scene for which
# test_render_end_to_end_golden_16bit states the 16-bit bounds that the V1 link reuses.
NETS = {
    "v1": ("v1", 0, 0, "fog", None, 0.1),
    "v2": ("v2", 0, 4, "solid", None, 0.0),
    "v3": ("v3", 64, 2, "solid", "orbit", 8.7),
    "v3w": ("v3", 128, 3, "solid", "orbit", -1.5),
    "v3own": ("v3", 64, 2, "solid", "own", 8.7),
}


def T(a):
    return torch.from_numpy(np.asarray(a))


def weights_of(net):
    fam, dd, seed, scene, _, shift = NETS[net]
    p = O.make_weights(fam, seed, scene, **(dict(dino_dim=dd) if dd == 128 else {}))
    head = "sigma_out.bias" if fam == "v1" else "density_mlp.density_head.bias"
    p[head] = p[head] + shift
    return p


def frame_rays():
    """The 19 x 31 frame's rays (589, 3) on the CPU, bit-equal to the library's get_rays."""
    ro, rd = O.get_rays(H, W, O.focal_for(W), T(O.LEGO_LIKE_C2W))
    return ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()


def source_view(g, net):
    """The V3 side channel of a net: another view's map and camera, or the rendered camera itself ('own')."""
    _, dd, _, _, name, _ = NETS[net]
    if name is None:
        return None
    if name == "own":
        return dict(features=T(g[f"map{dd}"]), pose=T(O.LEGO_LIKE_C2W), focal=O.focal_for(W), H=H, W=W)
    return dict(features=T(g[f"map{dd}"]), pose=T(g[f"{name}_pose"]), focal=float(g[f"{name}_focal"]), H=int(g[f"{name}_H"]),
                W=int(g[f"{name}_W"]))


def random_depths(n_rays, S, seed=71):
    """Sorted depths in [NEAR, FAR) from the oracle's counter hash: the explicit z_in of the tests."""
    u = O.uniform01(seed + S, n_rays * S).reshape(n_rays, S)
    return T(np.sort(np.float32(NEAR) + np.float32(FAR - NEAR) * u, axis=1).astype(np.float32))


def points32(ro, rd, z):
    """o + d z with the product rounded before the sum (device_math.hpp: point_on_ray) -> (R, S, 3) fp32, CPU."""
    ro, rd, z = ro.cpu().float(), rd.cpu().float(), z.cpu().float()
    return ro[:, None, :] + rd[:, None, :] * z[..., None]


def oracle_outputs(net, ro, rd, z, g=None):
    """The CPU oracle in fp32 at the samples (R, S): (rgb (R,S,3), raw sigma (R,S) in front of the density ReLU).  V2 / V3 go
    through oracle.train_stages in its fp32 mode (mlp_v2 / mlp_v3 up to summation order), which keeps 'density_raw'."""
    fam = NETS[net][0]
    p = weights_of(net)
    pts = points32(ro, rd, z).reshape(-1, 3)
    dirs = rd[:, None, :].expand(-1, z.shape[1], -1).reshape(-1, 3)
    with torch.no_grad():
        if fam == "v1":
            out = O.mlp_v1(p, O.positional_encoding(pts, 10))
            rgb, sig = out[:, :3], out[:, 3]
        else:
            feats = None
            if fam == "v3":
                src = source_view(g, net)
                xy, _, _ = O.project_points_to_image(pts, src["pose"], src["focal"], src["H"], src["W"])
                feats = O.sample_features_at_points(src["features"], xy)
            st, _ = O.train_stages(p, fam, O.positional_encoding(pts, 12 if fam == "v3" else 10), O.positional_encoding(dirs, 4),
                                   torch.zeros(pts.shape[0], 3), torch.zeros(pts.shape[0], 1), dino=feats, mode="f32")
            rgb, sig = st["rgb"], st["density_raw"][:, 0]
    return rgb.reshape(*z.shape, 3), sig.reshape(z.shape)


# ---------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------
class Probe:
    def __init__(self, colour, w):
        self.colour, self.w = colour, w
        self.open, self.closed = w == 1.0, w == 0.0
        self.left_out = ~(self.open | self.closed)

    def shares(self):
        n = self.w.numel()
        return float(self.open.sum()) / n, float(self.closed.sum()) / n, float(self.left_out.sum()) / n


def probe(N, model, ro, rd, z, **render_kw):
    """Column by column a one-sample render at z[:, s] -> Probe(colour (R,S,3), w (R,S)), CPU tensors.  Asserts that the render
    marched the depths it was given."""
    z = z.to(ro.device).contiguous()
    colour, w = [], []
    for s in range(z.shape[1]):
        zs = z[:, s:s + 1].contiguous()
        out = N.render_rays(model, ro, rd, NEAR, FAR, 1, z_in=zs, white_bkgd=False, return_z=True, **render_kw)
        assert torch.equal(out["z_vals"], zs), f"the one-sample render of column {s} did not march its z_in"
        colour.append(out["rgb"])
        w.append(out["weights"][:, 0])
    return Probe(torch.stack(colour, 1).cpu(), torch.stack(w, 1).cpu())


# ---------------------------------------------------------------------------------------------
# the compositor in fp32 (a replay of device_math.hpp: Composite) and in float64
# ---------------------------------------------------------------------------------------------
def ray_norm32(rd):
    d = rd.cpu().numpy().astype(np.float32)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def dist32(z, norm):
    """(R, S) fp32: fl(fl(z' - z) |d|), the last sample fl(1e10f |d|)."""
    z = z.cpu().numpy().astype(np.float32)
    out = np.empty_like(z)
    out[:, :-1] = (z[:, 1:] - z[:, :-1]) * norm[:, None]
    out[:, -1] = np.float32(1e10) * norm
    return out


def alpha32(sigma, dist):
    with np.errstate(under="ignore", over="ignore"):
        x = (-np.maximum(sigma.astype(np.float32), np.float32(0.0))) * dist.astype(np.float32)
        return (np.float32(1.0) - np.exp(x.astype(np.float32)).astype(np.float32)).astype(np.float32)


def composite32(alpha, colour, z, white):
    """Composite::add_alpha sample by sample, every operation one fp32 operation in the kernel's order ->
    (rgb (R,3), depth (R,), weights (R,S)) fp32."""
    f = np.float32
    alpha, colour, z = alpha.astype(f), colour.astype(f), z.astype(f)
    R, S = alpha.shape
    Tr, acc, depth = np.ones(R, f), np.zeros(R, f), np.zeros(R, f)
    rgb, w_all = np.zeros((R, 3), f), np.zeros((R, S), f)
    with np.errstate(under="ignore"):
        for s in range(S):
            w = alpha[:, s] * Tr
            for k in range(3):
                rgb[:, k] = rgb[:, k] + w * colour[:, s, k]
            depth = depth + w * z[:, s]
            acc = acc + w
            Tr = Tr * ((f(1.0) - alpha[:, s]) + f(1e-10))
            w_all[:, s] = w
    if white:
        rgb = rgb + (f(1.0) - acc)[:, None]
    return rgb, depth, w_all


def weights64(sigma, dist):
    """The weights in float64 from fp32 densities and fp32 dists (the constant is the kernel's 1e-10f)."""
    sigma, dist = np.maximum(np.asarray(sigma, np.float64), 0.0), np.asarray(dist, np.float64)
    alpha = -np.expm1(-sigma * dist)
    f = 1.0 - alpha + np.float64(np.float32(1e-10))
    trans = np.concatenate([np.ones_like(f[:, :1]), np.cumprod(f, 1)[:, :-1]], 1)
    return alpha * trans


def expected_image(w, colour, z, white):
    """rgb (R,3) and depth (R,) in float64 from fp32 weights, colours and depths, and the magnitudes the bounds are built on."""
    w, colour, z = np.asarray(w, np.float64), np.asarray(colour, np.float64), np.asarray(z, np.float64)
    rgb = (w[..., None] * colour).sum(1)
    mag_rgb = (w[..., None] * np.abs(colour)).sum(1)
    acc = w.sum(1)
    if white:
        rgb = rgb + (1.0 - acc)[:, None]
    return rgb, (w * z).sum(1), mag_rgb, (w * np.abs(z)).sum(1), acc


def image_bounds(S, rgb_expected, mag_rgb, mag_depth, acc, white):
    k = 2.0 * U / (1.0 - (S + 2) * U)
    tiny = S * 2.0 ** -149
    b_rgb = S * mag_rgb
    if white:
        b_rgb = b_rgb + ((S - 1) * acc + np.abs(1.0 - acc))[:, None] + np.abs(rgb_expected)
    return k * b_rgb + tiny, k * S * mag_depth + tiny


def weight_bound(S, mode):
    a = ALPHA_ERR[mode]
    s = np.arange(S, dtype=np.float64)
    return 2.0 * U * (a + 1.0 + s * (a + 3.0)) * (1.0 + 1e-6) + 2.0 ** -126
