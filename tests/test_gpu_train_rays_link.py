"""The ray-input training forward (nrf_mlp_forward_train_rays) held to the staged chain bit for bit, slot by slot (run with
-m gpu on an MI355X); and, through its saved encoding, the fused V1 renderers held to the staged V1 forward bit for bit.

tests/test_gpu_train_rays.py holds V2 to torch.equal outputs and gradients; V1 and V3 in the 16-bit modes it holds by cosines
and five losses, bars that cannot tell a rounding from a truncation (tests/test_gpu_train_stages.py).  Here every saved tensor
of the ray route -- every slot of csrc/train_slots.hpp, every ReLU bit plane, the V3 gate -- is compared with the same tensor of
the staged route on a twin model (tests/train_ctx.py: context_differences; raw bytes on the GPU, the columns of real samples
only), after the forward and again after the backward, and so are the outputs, the flat gradient and d_dino.  The staged chain
itself is held stage by stage to the rounding model by test_gpu_train_stages.py and test_saved_tensors_stage_consistent_16bit.

  1. V3   forward_rays(dino = the source view) against nrf_mlp_forward_train(points_out, expanded rays_d_out,
          nrf_project_fetch(points_out)): the in-kernel gather (nets.hpp: dino_taps, DinoRaw, dino_scaled_tiles) against
          staged_kernels.hip: project_fetch_kernel + the staged `v * w1` (train_v3_impl.hpp).  dino_dim 64 / 128; f32, bf16, f16;
          jittered depths; depth 8 at (R, S) = (100, 32) (4 waves), depth 2 at (77, 48), depth 8 at (1031, 32) (n = 32 992: 8 waves,
          ragged against 256; bf16 and f32).  Conditions, asserted on the CPU with the oracle before the run: at least 50 % of the
          samples have a tap on the source map and at least 5 % have none (the source camera stands 1.0 beside the rendered
          one); the density ReLU is open for 20 .. 80 % of the samples ('solid' seeds of train_ctx.SEEDS).
  2. V1   the staged route takes an fp32 encoding, the ray route encodes in the kernel (nets.hpp: encode3), so the two are tied
          in two steps.  (a) the saved `input` slot, decoded to the reference's 63 columns (train_ctx.x_enc_from_input_slot),
          against oracle.positional_encoding64(points_out) under tests/encoder_probe.py's encoder-stage rule
          (bound(t, mode, 'v1') on t = target(e, mode), no sigmoid term), no element outside, padding rows exactly zero.
          (b) nrf_mlp_forward_train_v1 on a twin model with x_enc := that decoded slot -- already in the operand type, so the
          staged kernel's rounding of it is the identity (test_train_rays_link_host.py) -- then nrf_mlp_backward_v1 on both
          contexts: out4, every slot and plane, the flat gradient.  f32, bf16, f16; depth 8 and 2; (100, 32) and (1031, 32);
          explicit depths; pixel mode.  |p| <= 8 (asserted), the range the encoder bounds are documented for; the n = 32 992
          f16 case must hold an f16-subnormal encoder value (asserted from the float64 encoding).
  3. the fused V1 renderers   render_probe.py's one-sample probe of render_kernel<NetV1> on each of its three routes (plain,
          NRF_SPW=3, the ray queue) against nrf_mlp_forward_v1(x_enc := the input slot forward_rays(z_in = the render's depths)
          saved): the colour of EVERY open sample torch.equal to the staged rgb, a sample open exactly where the staged sigma is
          > 0; LEFT_OUT_CAP and MIN_SHARE of render_probe.py as they are.  Modes f32, f16, bf16; the rays and depth kinds of
          test_gpu_render_link.py (S = 2, 12, 70; the 19 x 31 frame and the 3-ray call; ladder, disparity ladder, jitter, explicit
          depths).  f16x3 has no training kernel (it trains in fp32), so there is no saved encoding to read back in that mode: it
          stays on the 1e-4 bound of test_gpu_render_link.py, section b.
  4. sensitivity   the staged twin is fed an input off by ONE operand ulp in ONE element (a feature of a sample of V1's x_enc,
          a channel of a sample of V3's dino): context_differences must then report the first stage with exactly the elements
          that hold that value, and stages behind it.

No exception to the equality is claimed: every case must print "0 differing stages".

RECORD (a record, not a bound).  Every case prints a RECORD line under -s (samples; open share; V3: on-map / off-map share; V1:
f16-subnormal encoder values; differing stages).
  MI355X, gfx950; every case of this file, 45 tests in 8 s, the slowest 1.0 s (the V1 render link at S = 70):
    1. V3, every case: forward 0 differing stages, backward 0 differing stages; rgb, density, flat gradient, d_dino torch.equal.
         depth 8  n 3 200    dino 64: open 0.674   dino 128: open 0.649   on-map 0.677 / off-map 0.323   (f32, bf16, f16)
         depth 2  n 3 696    dino 64: open 0.762   dino 128: open 0.718   on-map 0.666 / off-map 0.334   (f32, bf16, f16)
         depth 8  n 32 992   dino 64: open 0.670   dino 128: open 0.651   on-map 0.684 / off-map 0.316   (f32, bf16)
    2. V1, every case: forward 0 differing stages, backward 0 differing stages; out4 and flat gradient torch.equal.
       sigma > 0 on 0.05 (depth 8) / 0.39 (depth 2) of the samples.  The saved encoding, worst |a - t| / bound and the number of
       float64 encoder values that are f16 subnormals:
         n 3 200 jitter   f32 0.242  bf16 0.901  f16 0.974   7 subnormal      n 32 992 jitter   f32 0.254  bf16 0.921  f16 0.993   51 subnormal
         n 3 200 z_in     f16 0.972   5 subnormal                             n 3 200 pixels    bf16 0.762   2 subnormal
       (0.9 .. 1.0 in the 16-bit modes is one flipped last bit of a value at the bottom of its binade: what the rule grants)
    3. V1 renderers, f32 / f16 / bf16 at S = 2, 12, 70: 14 208 / 85 248 / 497 280 probed samples over the three routes, open
       0.48 .. 0.50, 0 findings: every open colour bit-equal to the staged forward on the saved encoding, no open/closed flip.
    4. sensitivity, stages reported (elements; every one in the perturbed sample's column, no other column touched):
         v3 f32   dino[3446, 5] + 1 ulp: input.0 1, fusion0.0 15, fusion2.0 50, attention0 20, gate 2, input.1 131, fusion0.1 106,
                  fusion2.1 107, proj 239, trunk.0 114, trunk.1 110, colour.in 244, colour.c0 57, colour.c2 31
         v3 bf16  input.0 1, fusion0.0 27, fusion2.0 45, attention0 21, gate 2, input.1 27, fusion0.1 66, fusion2.1 63, proj 159,
                  trunk.0 89, trunk.1 83, mask.trunk.1 1, colour.in 179, colour.c0 41, colour.c2 27
         v3 f16   input.0 1, fusion0.0 30, fusion2.0 26, mask.fusion2.0 1, attention0 8, gate 2, input.1 4, fusion0.1 45,
                  fusion2.1 48, proj 148, trunk.0 76, trunk.1 88, colour.in 174, colour.c0 43, colour.c2 26
         v1 f32   x_enc[2381, 40] + 1 ulp: input 1, trunk.0 24, trunk.1 79       v1 bf16  x_enc[12, 40]: input 1, trunk.0 56,
                  trunk.1 67, mask.trunk.1 1                                     v1 f16   x_enc[61, 40]: input 1, trunk.0 53, trunk.1 49
    tests/test_gpu_train_rays.py, the two promoted assertions, same run: the parameters of the two V3 routes bit-equal after each
    of five steps (bf16, f16; dino_dim 64, 128); the f32 V3 forward bit-equal to the staged fetch + forward.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import encoder_probe as EP
from tests import render_probe as P
from tests import test_gpu_render_link as RL
from tests import train_ctx as T
from tests.test_gpu_train_rays import backward_v2, expand_dirs, forward_rays, ray_batch, u01
from tests.test_gpu_train_stages import make_model as make_v23
from tests.test_gpu_training import make_model as make_v1
from tests.test_training_host import train_plan

pytestmark = pytest.mark.gpu

NEAR, FAR = 2.0, 6.0
V1_NEAR, V1_FAR = 0.5, 5.0                  # with ray_batch's |o| <= 0.35, |d| <= 1.5: |p| <= 7.85
MODES = ["f32", "bf16", "f16"]
SOURCE_SHIFT = 1.0                          # the source camera beside the rendered one: 2/3 of the samples project into its map


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


# ---------------------------------------------------------------------------------------------
# the staged route, split into its calls (the context is compared between them)
# ---------------------------------------------------------------------------------------------
def _staged(model, n, v1):
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.training import _train_handle
    dev = torch.device("cuda", 0)
    h, mode = _train_handle(model, dev)
    nbytes = L.lib().nrf_train_context_bytes(h, mode, n)
    assert nbytes > 0
    return dict(h=h, mode=mode, n=n, nbytes=nbytes, buf=torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                a=torch.empty((n, 4 if v1 else 3), device=dev), b=None if v1 else torch.empty((n, 1), device=dev))


def staged_forward(model, pts, dirs, dino):
    """nrf_mlp_forward_train -> the dict forward_rays returns (a = rgb, b = density, the context)."""
    from nerf_few_shot_limitations_amd import _lib as L
    f = _staged(model, pts.shape[0], False)
    L.check(L.lib().nrf_mlp_forward_train(f["h"], f["mode"], L.ptr(pts), L.ptr(dirs), L.ptr(dino), f["n"], L.ptr(f["a"]), L.ptr(f["b"]),
                                          C.c_void_p(f["buf"].data_ptr()), f["nbytes"], L.stream_ptr()))
    torch.cuda.synchronize()
    return f


def staged_forward_v1(model, x_enc):
    from nerf_few_shot_limitations_amd import _lib as L
    f = _staged(model, x_enc.shape[0], True)
    L.check(L.lib().nrf_mlp_forward_train_v1(f["h"], f["mode"], L.ptr(x_enc), f["n"], L.ptr(f["a"]), C.c_void_p(f["buf"].data_ptr()), f["nbytes"],
                                             L.stream_ptr()))
    torch.cuda.synchronize()
    return f


def backward_v1(model, f, g):
    from nerf_few_shot_limitations_amd import _lib as L
    grad = torch.zeros(model.flat_params().flat.numel(), device="cuda")
    L.check(L.lib().nrf_mlp_backward_v1(f["h"], f["mode"], L.ptr(f["a"]), L.ptr(g), f["n"], C.c_void_p(f["buf"].data_ptr()), f["nbytes"], L.ptr(grad),
                                        L.stream_ptr()))
    torch.cuda.synchronize()
    return grad


def backward_dino(model, f):
    from nerf_few_shot_limitations_amd import _lib as L
    d = torch.empty((f["n"], model.dino_dim), device="cuda")
    L.check(L.lib().nrf_mlp_backward_dino(f["h"], f["mode"], f["n"], C.c_void_p(f["buf"].data_ptr()), f["nbytes"], L.ptr(d), L.stream_ptr()))
    torch.cuda.synchronize()
    return d


def context(variant, p, depth, dino_dim, mode, f):
    from nerf_few_shot_limitations_amd import _lib as L
    return T.SavedContext(train_plan(L, variant, p, depth, dino_dim or 64, with_planes=True), variant, depth, mode, f["n"], f["buf"])


def one_operand_ulp(v, mode):
    """The operand-type neighbour (away from zero) of the rounded value of a 0-d fp32 tensor."""
    q = O.quantize(v.reshape(1).cpu(), mode)
    if mode == "f16":
        return (q.half().view(torch.int16) + 1).view(torch.float16).float()[0]
    return (q.view(torch.int32) + (1 << 16 if mode == "bf16" else 1)).view(torch.float32)[0]


def named(diffs):
    return "0 differing stages" if not diffs else "DIFFERING: " + ", ".join(f"{d.stage} x{d.count} first {d.first}" for d in diffs)


# ---------------------------------------------------------------------------------------------
# 1. V3
# ---------------------------------------------------------------------------------------------
def link_scene(dino_dim, R):
    """test_gpu_train_rays.py's _v3_scene with room for 1031 rays (a 40 x 40 view) and the source camera moved until a fair share
    of the samples has no tap on its map."""
    import nerf_few_shot_limitations_amd as N
    H = W = 40
    focal = O.focal_for(W)
    ro, rd = N.get_rays(H, W, focal, torch.from_numpy(O.LEGO_LIKE_C2W))
    pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(3))[:R].cuda()
    src = O.LEGO_LIKE_C2W.copy()
    src[0, 3] += SOURCE_SHIFT
    cam = dict(features=(u01(120, 1, 9, 9, dino_dim) * 2 - 1).cuda(), pose=torch.from_numpy(src), focal=focal, H=H, W=W)
    return ro.reshape(-1, 3)[pix].contiguous(), rd.reshape(-1, 3)[pix].contiguous(), cam


def on_map_share(cam, pts):
    """Share of the (n,3) CPU points with at least one bilinear tap inside the source map: the oracle's projection and
    sample_features_at_points' tap test."""
    xy, _, _ = O.project_points_to_image(pts, cam["pose"], cam["focal"], cam["H"], cam["W"])
    Hp, Wp = cam["features"].shape[1:3]
    gx, gy = ((xy[:, 0] + 1) * Wp - 1) / 2, ((xy[:, 1] + 1) * Hp - 1) / 2
    x0, y0 = torch.floor(gx), torch.floor(gy)
    hit = torch.zeros(pts.shape[0], dtype=torch.bool)
    for dy in (0, 1):
        for dx in (0, 1):
            hit |= (x0 + dx >= 0) & (x0 + dx <= Wp - 1) & (y0 + dy >= 0) & (y0 + dy <= Hp - 1)
    return float(hit.float().mean())


def v3_conditions(p, cam, pts, dirs):
    """(on-map share, open share) of a case, from the oracle alone, asserted."""
    pts, dirs = pts.cpu(), dirs.cpu()
    on = on_map_share(cam, pts)
    assert on >= 0.5 and 1.0 - on >= 0.05, on
    xy, _, _ = O.project_points_to_image(pts, cam["pose"], cam["focal"], cam["H"], cam["W"])
    with torch.no_grad():
        den = O.mlp_v3(p, pts, dirs, O.sample_features_at_points(cam["features"].cpu(), xy))[1]
    open_ = float((den > 0).float().mean())
    assert 0.2 <= open_ <= 0.8, open_
    return on, open_


V3_SHAPES = [(8, 100, 32), (2, 77, 48), (8, 1031, 32)]              # depth, R, S
V3_CASES = [(mode, dd, depth, R, S) for depth, R, S in V3_SHAPES for dd in (64, 128) for mode in MODES if not (R * S > 30000 and mode == "f16")]


class V3Pair:
    """One case: the ray route on one model, the staged route on its twin, both forwards done."""

    def __init__(self, N, mode, dino_dim, depth, R, S, feats_edit=None):
        from nerf_few_shot_limitations_amd import train_cli
        from nerf_few_shot_limitations_amd.renderer import make_dino
        self.mode, self.dd, self.depth, self.n = mode, dino_dim, depth, R * S
        self.p = O.make_weights("v3", T.SEEDS[("v3", depth)], "solid", n_layers=depth, dino_dim=dino_dim)
        self.rays_model, self.staged_model = (make_v23(N, "v3", dino_dim, depth, mode, self.p) for _ in range(2))
        o, d, cam = link_scene(dino_dim, R)
        seed = 4242 + R
        pts, _ = N.sample_points_along_rays(o, d, NEAR, FAR, S, perturb=True, seed=seed)
        pts = pts.reshape(-1, 3).contiguous()
        self.on, self.open = v3_conditions(self.p, cam, pts, expand_dirs(d, S))
        self.rays = forward_rays(self.rays_model, S, o, d, perturb=True, seed=seed, dino=cam)
        assert self.rays["intact"] and torch.equal(self.rays["pts"], pts) and torch.equal(self.rays["d_out"], d)
        self.feats = train_cli.fetch_features(make_dino(**cam), self.rays["pts"])
        if feats_edit is not None:
            feats_edit(self.feats)
        self.staged = staged_forward(self.staged_model, self.rays["pts"], expand_dirs(self.rays["d_out"], S), self.feats)
        self.fwd, self.bwd = T.stage_names("v3", depth)

    def differences(self, stages):
        a, b = (context("v3", self.p, self.depth, self.dd, self.mode, f) for f in (self.rays, self.staged))
        return T.context_differences(a, b, "v3", self.depth, self.dd, stages)


@pytest.mark.parametrize("mode,dino_dim,depth,R,S", V3_CASES)
def test_v3_ray_route_is_the_staged_route(N, mode, dino_dim, depth, R, S):
    c = V3Pair(N, mode, dino_dim, depth, R, S)
    n = c.n
    fwd = c.differences(c.fwd)
    print(f"\nRECORD v3 {mode} dino {dino_dim} depth {depth} n {n}: open {c.open:.3f}, on-map {c.on:.3f} / off-map {1 - c.on:.3f}; forward: {named(fwd)}")
    assert fwd == [], named(fwd)
    assert torch.equal(c.rays["a"], c.staged["a"]) and torch.equal(c.rays["b"], c.staged["b"])
    den = c.rays["b"]
    assert float((den > 0).float().mean()) > 0.1 and float((den == 0).float().mean()) > 0.1          # both branches ran on the GPU too
    g_rgb, g_den = (u01(71, n, 3) - 0.5).cuda(), (u01(72, n, 1) - 0.5).cuda()
    grad_r, grad_s = backward_v2(c.rays_model, c.rays, g_rgb, g_den), backward_v2(c.staged_model, c.staged, g_rgb, g_den)
    d_r, d_s = backward_dino(c.rays_model, c.rays), backward_dino(c.staged_model, c.staged)
    both = c.differences(c.fwd + c.bwd)
    print(f"RECORD v3 {mode} dino {dino_dim} depth {depth} n {n}: backward: {named(both)}")
    assert both == [], named(both)
    assert torch.equal(grad_r, grad_s) and float(grad_s.abs().max()) > 0
    assert torch.equal(d_r, d_s) and float(d_s.abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# 2. V1
# ---------------------------------------------------------------------------------------------
V1_CASES = [(mode, depth, R, 32, "jitter") for depth in (8, 2) for R in (100, 1031) for mode in MODES] + [("f16", 8, 100, 32, "z_in"),
                                                                                                        ("bf16", 8, 100, 32, "pixels")]


class V1Pair:
    def __init__(self, N, mode, depth, R, S, kind, x_edit=None):
        self.mode, self.depth, self.n = mode, depth, R * S
        self.rays_model, self.p = make_v1(N, mode, scene="solid", n_layers=depth)
        self.staged_model, _ = make_v1(N, mode, scene="solid", n_layers=depth)
        if kind == "pixels":
            H, W = 40, 56
            pix = torch.randint(0, H * W, (R,), generator=torch.Generator().manual_seed(R), dtype=torch.int64).cuda()
            cam = dict(H=H, W=W, focal=O.focal_for(W), pose=torch.from_numpy(O.LEGO_LIKE_C2W))
            self.rays = forward_rays(self.rays_model, S, pixels=pix, cam=cam, perturb=True, seed=7, near=NEAR, far=FAR)
        else:
            o, d = ray_batch(R, seed=140)
            kw = dict(perturb=True, seed=99 + R)
            if kind == "z_in":
                kw = dict(z_in=torch.sort(u01(141, R, S) * (V1_FAR - V1_NEAR) + V1_NEAR, dim=-1).values.cuda())
            self.rays = forward_rays(self.rays_model, S, o, d, near=V1_NEAR, far=V1_FAR, **kw)
        assert self.rays["intact"]
        self.pts = self.rays["pts"].cpu()
        assert float(self.pts.abs().max()) <= 8.0
        self.ctx_rays = context("v1", self.p, depth, 0, mode, self.rays)
        self.x_enc, self.pad = T.x_enc_from_input_slot(self.ctx_rays)
        x = self.x_enc.clone()
        if x_edit is not None:
            x_edit(x)
        self.staged = staged_forward_v1(self.staged_model, x.cuda().contiguous())
        self.fwd, self.bwd = T.stage_names("v1", depth)

    def differences(self, stages):
        return T.context_differences(self.ctx_rays, context("v1", self.p, self.depth, 0, self.mode, self.staged), "v1", self.depth, 0, stages)


@pytest.mark.parametrize("mode,depth,R,S,kind", V1_CASES)
def test_v1_ray_route_is_the_staged_route_on_its_own_encoding(N, mode, depth, R, S, kind):
    c = V1Pair(N, mode, depth, R, S, kind)
    n = c.n
    # a. the saved encoding
    e64 = O.positional_encoding64(c.pts, 10).numpy()
    t = EP.target(e64, mode)
    ratio = np.abs(c.x_enc.double().numpy() - t) / EP.bound(t, mode, "v1")
    subnormal = int(((np.abs(e64) < 2.0 ** -14) & (np.abs(e64) >= 2.0 ** -24)).sum())
    if (mode, n) == ("f16", 32992):
        assert subnormal >= 1
    assert np.abs(c.pad).max() == 0.0
    # b. the chain
    fwd = c.differences(c.fwd)
    sigma = c.rays["a"][:, 3]
    print(f"\nRECORD v1 {mode} depth {depth} n {n} {kind}: open {float((sigma > 0).float().mean()):.3f}; encoder values that are f16 subnormals "
          f"{subnormal}; worst |a-t|/bound of the saved encoding {float(ratio.max()):.3f}; forward: {named(fwd)}")
    assert not (ratio > 1).any() and np.isfinite(ratio).all(), (int((ratio > 1).sum()), float(ratio.max()))
    assert fwd == [], named(fwd)
    assert torch.equal(c.rays["a"], c.staged["a"])
    g = (u01(111, n, 4) - 0.5).cuda()
    grad_r, grad_s = backward_v1(c.rays_model, c.rays, g), backward_v1(c.staged_model, c.staged, g)
    both = c.differences(c.fwd + c.bwd)
    print(f"RECORD v1 {mode} depth {depth} n {n} {kind}: backward: {named(both)}")
    assert both == [], named(both)
    assert torch.equal(grad_r, grad_s) and float(grad_s.abs().max()) > 0


# ---------------------------------------------------------------------------------------------
# 3. the fused V1 renderers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", P.S_VALUES)
@pytest.mark.parametrize("mode", MODES)
def test_v1_renderers_read_the_staged_network(N, mode, S, monkeypatch):
    link = RL.Link(N, None, "v1", mode)                         # V1 has no source view: the golden maps are not touched
    ro, rd = (t.cuda() for t in P.frame_rays())
    n_open = n_all = 0
    for o, d in ((ro, rd), (ro[293:296].contiguous(), rd[293:296].contiguous())):
        R = o.shape[0]
        for tag, kw in (("ladder", {}), ("lindisp", dict(lindisp=True)), ("jitter", RL.JITTER), ("z_in", dict(z_in=P.random_depths(R, S).cuda()))):
            case = RL.Case(link, monkeypatch, o, d, S, tag, kw)
            f = forward_rays(link.model, S, o, d, z_in=case.z.contiguous(), near=P.NEAR, far=P.FAR)
            assert f["intact"] and torch.equal(f["z"], case.z)
            assert torch.equal(f["pts"].cpu(), P.points32(o, d, case.z).reshape(-1, 3)), case.tag
            x_enc, pad = T.x_enc_from_input_slot(context("v1", P.weights_of("v1"), 8, 0, mode, f))
            assert np.abs(pad).max() == 0.0
            with torch.no_grad():                               # nrf_mlp_forward_v1: under grad the module would take the training forward
                out = link.model(x_enc.cuda().contiguous()).cpu()
            assert torch.equal(out, f["a"].cpu()), case.tag     # forward_train_rays is that forward on its own encoding (section 2, again)
            rgb, sig = out[:, :3].reshape(R, S, 3), out[:, 3].reshape(R, S)
            for name, spw, extra in RL.PROBES:
                what = f"{case.tag} probe:{name}"
                pr = case.probe if name == "plain" else case.run_probe(spw, **extra)
                open_, closed, left = pr.shares()
                if left > P.LEFT_OUT_CAP or (R > 3 and min(open_, closed) < P.MIN_SHARE):
                    link.fail(what, f"shares: open {open_:.3f} closed {closed:.3f} left out {left:.4f}")
                same = (pr.colour == rgb).all(-1)
                if not bool(same[pr.open].all()):
                    link.fail(what, f"colour: {int((~same[pr.open]).sum())} of {int(pr.open.sum())} open samples differ bitwise, max "
                                    f"{float((pr.colour.double() - rgb.double()).abs()[pr.open].max()):.3e}")
                flips = (pr.open != (sig > 0)) & ~pr.left_out
                if bool(flips.any()):
                    link.fail(what, f"open != (sigma > 0) on {int(flips.sum())} samples, |sigma| up to {float(sig[flips].abs().max()):.3e}")
                n_open += int(pr.open.sum()); n_all += pr.w.numel()
    torch.cuda.synchronize()
    print(f"\nRECORD v1 render {mode} S={S}: {n_all} probed samples over the three routes, open {n_open / n_all:.3f}; findings: {len(link.fails)}")
    assert not link.fails, f"{len(link.fails)} findings:\n" + "\n".join(link.fails[:20])


# ---------------------------------------------------------------------------------------------
# 4. sensitivity: one operand ulp in one element of the staged twin's input
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_ulp_in_one_dino_channel_is_reported_from_the_first_stage(N, mode):
    where = {}

    def edit(feats):
        s = int(feats[:, 5].abs().argmax())                      # a sample with a tap on the map, the channel's largest value
        feats[s, 5] = one_operand_ulp(feats[s, 5], mode).item()
        where["s"] = s
    c = V3Pair(N, mode, 64, 2, 77, 48, feats_edit=edit)
    diffs = c.differences(c.fwd)
    print(f"\nRECORD sensitivity v3 {mode}: one ulp in dino[{where['s']}, 5]: {named(diffs)}")
    assert diffs and diffs[0].stage == "input.0" and diffs[0].count == 1 and diffs[0].first[1] == where["s"]
    assert all(d.first[1] == where["s"] for d in diffs)          # no other sample is touched
    assert len(diffs) > 1                                        # and the stages behind it see it


@pytest.mark.parametrize("mode", MODES)
def test_one_ulp_in_one_encoder_feature_is_reported_from_the_first_stage(N, mode):
    k, where = 40, {}

    def edit(x):
        where["s"] = int(x[:, k].abs().argmax())
        x[where["s"], k] = one_operand_ulp(x[where["s"], k], mode)
    c = V1Pair(N, mode, 2, 100, 32, "jitter", x_edit=edit)
    s = where["s"]
    diffs = c.differences(c.fwd)
    print(f"\nRECORD sensitivity v1 {mode}: one ulp in x_enc[{s}, {k}]: {named(diffs)}")
    row = int(np.nonzero(T.kernel_feature_order(10) == k)[0][0])
    assert diffs and diffs[0] == T.Difference("input", 1, (row, s))
    assert all(d.first[1] == s for d in diffs) and len(diffs) > 1
