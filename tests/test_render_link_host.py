"""CPU half of the render link (tests/test_gpu_render_link.py; the shared arithmetic and the derivation of every bound are in
tests/render_probe.py):

  * the probe's premise: in fp32, 1 - expf(-sigma 1e10 |d|) is exactly 1 for every sigma >= 1e-8 and exactly 0 for sigma <= 0,
    over the range of |d| of the tests' rays;
  * the scenes: on the tests' own points -- every S with the ladder, the disparity ladder, the oracle's stratified jitter and the
    explicit depths, the 3-ray call, and every 7th ray of the even-deal frame at its two cases -- the fp32 oracle has no density
    in (0, 1e-8), nothing the probe would have to leave out, and the density ReLU is open on >= 10 % and closed on >= 10 % of
    the samples of every case;
  * the reference alone passes: a float32 replay of Composite::add_alpha (the same operations in the same order) against float64
    stays within HALF of every bound the GPU test asserts, on the tests' S values and on adversarial rows (an opaque wall first,
    all-closed rows, a density just above 0 on the last sample, a transmittance that underflows);
  * the checks bite, on the oracle's rounding model (oracle.train_stages): truncation instead of rounding in one layer changes
    the colour bits of more than 90 % of the samples (bit equality, or any cap on the share of differing samples up to 10 %,
    cannot pass it); two exchanged sample columns break the compositor bound by more than 100 x.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import render_probe as P
from tests.train_ctx import fault, truncate


@pytest.fixture(scope="module")
def g(golden):
    return golden("dino_views")


def uniform(seed, shape):
    return O.uniform01(seed, int(np.prod(shape))).reshape(shape)


def ladder(S, n_rays, lindisp=False):
    return O.z_steps(P.NEAR, P.FAR, S, lindisp)[None].expand(n_rays, -1).contiguous()


# ------------------------------------------------------------------ the premise
def test_one_sample_alpha_is_a_step_function_of_the_density():
    _, rd = P.frame_rays()
    norm = P.ray_norm32(rd)
    norms = np.unique(np.concatenate([norm, np.float32([norm.min(), norm.max(), 1.0, 1.25])]))
    assert norms.min() >= 1.0 and norms.max() <= 1.25                  # a pinhole camera's directions: dz = -1
    sig = np.concatenate([np.float32(P.SIGMA_FLOOR) * np.float32(1.0 + 2.0 ** -23) ** np.arange(4, dtype=np.float32),
                          np.logspace(-8, 30, 2000).astype(np.float32), np.float32([1e-8, 3.4e38, np.inf])])
    sig = sig[sig >= np.float32(P.SIGMA_FLOOR)]
    dist = (np.float32(1e10) * norms)[:, None]
    assert np.all(P.alpha32(sig[None, :], dist) == np.float32(1.0))
    closed = np.float32([0.0, -0.0, -1e-30, -1e-8, -1.0, -3.4e38, -np.inf])
    assert np.all(P.alpha32(closed[None, :], dist) == np.float32(0.0))
    # and the composited pixel of an open sample is the colour itself: 0 + 1 * c, T = 1
    c = uniform(3, (5, 1, 3)).astype(np.float32)
    rgb, _, w = P.composite32(np.ones((5, 1), np.float32), c, np.full((5, 1), 3.0, np.float32), white=False)
    assert np.array_equal(rgb, c[:, 0]) and np.all(w == 1.0)


# ------------------------------------------------------------------ the scenes
def jittered(S, ro, rd, seed):
    """The oracle's stratified jitter (the kernel's own draws come from its counter RNG: same intervals, other uniforms)."""
    t = P.T(uniform(seed, (ro.shape[0], S)).astype(np.float32))
    return O.sample_points_along_rays(ro, rd, P.NEAR, P.FAR, S, t)[1]


def even_deal_rays(stride=7):
    """Every 7th ray of the 67 x 63 frame of the GPU file's even-deal cases (603 rays spread over the whole frame)."""
    ro, rd = O.get_rays(P.EVEN_H, P.EVEN_W, O.focal_for(P.EVEN_W), P.T(O.LEGO_LIKE_C2W))
    return ro.reshape(-1, 3)[::stride].contiguous(), rd.reshape(-1, 3)[::stride].contiguous()


@pytest.mark.parametrize("net", sorted(P.NETS))
def test_scene_is_open_and_closed_and_has_no_density_the_probe_leaves_out(net, g):
    ro, rd = P.frame_rays()
    R = ro.shape[0]
    eo, ed = even_deal_rays()
    cases = [("S2 ladder", ro, rd, ladder(2, R)), ("S12 ladder", ro, rd, ladder(12, R)), ("S70 ladder", ro, rd, ladder(70, R)),
             ("S2 lindisp", ro, rd, ladder(2, R, True)), ("S12 lindisp", ro, rd, ladder(12, R, True)), ("S70 lindisp", ro, rd, ladder(70, R, True)),
             ("S2 jitter", ro, rd, jittered(2, ro, rd, 31)), ("S12 jitter", ro, rd, jittered(12, ro, rd, 32)),
             ("S70 jitter", ro, rd, jittered(70, ro, rd, 33)),
             ("S2 z_in", ro, rd, P.random_depths(R, 2)), ("S12 z_in", ro, rd, P.random_depths(R, 12)), ("S70 z_in", ro, rd, P.random_depths(R, 70)),
             ("3 rays S12", ro[293:296], rd[293:296], P.random_depths(3, 12)),
             ("even deal S70 jitter", eo, ed, jittered(70, eo, ed, 34)), ("even deal S48 z_in", eo, ed, P.random_depths(eo.shape[0], 48))]
    for tag, o, d, z in cases:
        _, sig = P.oracle_outputs(net, o, d, z, g)
        assert int(((sig > 0) & (sig < P.SIGMA_FLOOR)).sum()) == 0, (net, tag)
        if o.shape[0] > 3:
            open_, closed = float((sig > 0).float().mean()), float((sig <= 0).float().mean())
            assert open_ >= P.MIN_SHARE and closed >= P.MIN_SHARE, (net, tag, open_, closed)


# ------------------------------------------------------------------ the reference alone keeps half of the bounds
def adversarial_rows(S):
    """(sigma (n,S), what): an opaque wall first; all closed; a density just above 0 on the last sample (behind open and behind
    closed samples); a transmittance that underflows (alpha ~ 1 - e^-3 .. 1 - e^-60 per step)."""
    rows = []
    wall = uniform(11, (4, S)).astype(np.float32) * 20 - 5
    wall[:, 0] = [1e3, 1e6, 50.0, 3e4]
    rows.append(wall)
    rows.append(-uniform(12, (3, S)).astype(np.float32) * 30)
    rows.append(np.zeros((1, S), np.float32))
    last = uniform(13, (6, S)).astype(np.float32) * 2 - 1
    last[:3] = -np.abs(last[:3])
    last[:, -1] = [1e-8, 1.0000001e-8, 2e-8, 1e-8, 1e-7, 1e-8]
    rows.append(last)
    under = np.tile(np.float32([[50.0], [400.0], [1000.0], [5000.0]]), (1, S))
    rows.append(under)
    return np.concatenate(rows, 0)


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("S", P.S_VALUES)
def test_fp32_replay_of_the_compositor_keeps_half_of_every_bound(S, mode):
    ro, rd = P.frame_rays()
    R = ro.shape[0]
    rows = adversarial_rows(S)
    sigma = np.concatenate([uniform(21 + S, (R, S)).astype(np.float32) * 24 - 12, rows], 0)          # the scenes' range of densities
    n = sigma.shape[0]
    colour = uniform(22 + S, (n, S, 3)).astype(np.float32)
    norm = np.concatenate([P.ray_norm32(rd), np.full(len(rows), 1.05, np.float32)])
    z = np.concatenate([P.random_depths(R, S).numpy(), P.random_depths(len(rows), S, seed=5).numpy()], 0)
    dist = P.dist32(torch.from_numpy(z), norm)
    if S == 70:
        assert (P.composite32(P.alpha32(rows, dist[R:]), colour[R:], z[R:], False)[2][-4:, -1] == 0).all()      # T did underflow
    alpha = P.alpha32(sigma, dist)
    for white in (False, True):
        rgb, depth, w = P.composite32(alpha, colour, z, white)
        e_rgb, e_depth, mag_rgb, mag_depth, acc = P.expected_image(w, colour, z, white)
        b_rgb, b_depth = P.image_bounds(S, e_rgb, mag_rgb, mag_depth, acc, white)
        assert np.all(np.abs(rgb - e_rgb) <= 0.5 * b_rgb), float(np.max(np.abs(rgb - e_rgb) / b_rgb))
        assert np.all(np.abs(depth - e_depth) <= 0.5 * b_depth), float(np.max(np.abs(depth - e_depth) / b_depth))
    assert np.all(np.abs(w - P.weights64(sigma, dist)) <= 0.5 * P.weight_bound(S, mode)[None, :])


# ------------------------------------------------------------------ planted faults on the rounding model
def model_chain(mode, tap=None, n_rays=48, S=12):
    """oracle.train_stages' forward (float64 accumulation) of the V2 scene on n_rays of the frame x S explicit depths."""
    ro, rd = P.frame_rays()
    pick = torch.arange(n_rays) * (ro.shape[0] // n_rays)
    ro, rd = ro[pick], rd[pick]
    z = P.random_depths(n_rays, S)
    pts = P.points32(ro, rd, z).reshape(-1, 3)
    dirs = rd[:, None, :].expand(-1, S, -1).reshape(-1, 3)
    n = pts.shape[0]
    st, _ = O.train_stages(P.weights_of("v2"), "v2", O.positional_encoding64(pts, 10), O.positional_encoding64(dirs, 4), torch.zeros(n, 3),
                           torch.zeros(n, 1), mode=mode, acc=torch.float64, tap=tap)
    return st["rgb"].reshape(n_rays, S, 3).numpy(), st["density_raw"].reshape(n_rays, S).numpy(), z.numpy(), P.ray_norm32(rd)


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_truncation_in_one_layer_changes_nearly_every_colour(mode):
    right, sig, _, _ = model_chain(mode)
    wrong, _, _, _ = model_chain(mode, tap=fault("round", "trunk.1", lambda t: truncate(t, mode)))
    differ = float((right != wrong).any(-1).mean())
    assert differ > 0.9, differ
    assert float((right != wrong).any(-1)[sig > 0].mean()) > 0.9                # on the samples the probe can read, too


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_exchanged_sample_columns_break_the_compositor_bound(mode):
    S = 12
    colour, sig, z, norm = model_chain(mode, S=S)
    alpha = P.alpha32(sig, P.dist32(torch.from_numpy(z), norm))
    swapped = colour.copy()
    swapped[:, [3, 7]] = swapped[:, [7, 3]]                     # the renderer composites column 3 with column 7's colour
    for white in (False, True):
        worst = {}
        for name, c in (("right", colour), ("swapped", swapped)):
            rgb, depth, w = P.composite32(alpha, c, z, white)
            e_rgb, e_depth, mag_rgb, mag_depth, acc = P.expected_image(w, colour, z, white)      # the probe's colours
            b_rgb, _ = P.image_bounds(S, e_rgb, mag_rgb, mag_depth, acc, white)
            worst[name] = float(np.max(np.abs(rgb - e_rgb) / b_rgb))
        assert worst["right"] <= 0.5 and worst["swapped"] > 100, worst
