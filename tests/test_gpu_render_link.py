"""The fused renderers tied to the staged forward, sample by sample and bit for bit (run with -m gpu on an MI355X).

forward_train is held stage by stage to the oracle's rounding model (test_gpu_train_stages.py) and forward_kernel is bit-equal to
forward_train (test_forward_train_equals_inference_forward); this file closes the chain at render_kernel / render_queue_kernel,
which run the same Net::eval behind their own point_on_ray, encoder inputs, feature-map gather, column-to-owner exchange and
ray deal.  The tool is the one-sample probe of tests/render_probe.py (its premise, the derivation of every bound used here and
the proof that the reference alone keeps half of them: that file and tests/test_render_link_host.py).

Per net (V1, V2, V3 at dino_dim 64 and 128 conditioned on ANOTHER view, V3 conditioned on the rendered camera in the 16-bit
modes), mode (f32, f16x3, f16, bf16) and S (2, 12, 70), on the 19 x 31 frame and on a 3-ray call, with the plain ladder, the
disparity ladder, the in-kernel jitter and explicit sorted depths:

  a. network link, V2 / V3   the probe's colour of every open sample is torch.equal to the rgb of model.eval()(pts, dirs[, feats])
                             at the staged sampler's points (feats: nrf_project_fetch of the same source view), and a sample is
                             open exactly where that forward's density is > 0 -- for the probe on EACH route a one-sample render
                             can take (PROBES): render_kernel at one sample per column, render_kernel through the SPW = 8
                             column-to-owner exchange (NRF_SPW=3), and render_queue_kernel (ert_eps = 1e-30), whose input
                             lambdas and gather are its own.  No share cap is needed: the build compiles with
                             -ffp-contract=off, so DinoRaw::finish and project_fetch_kernel run the same rounded multiply-adds
                             in the same tap order.  ONE documented exception to "the fetch as it is": f16 at dino_dim 128 holds
                             the gathered channels between NetV3's two fusion passes already rounded to f16 (nets.hpp: DinoHeld,
                             PACKED: round16(round16(e) w1) in the second pass), so in that mode the renderer is by design NOT
                             bit-equal to nrf_mlp_forward on the same fp32 features; the staged forward is handed the fetch
                             rounded to f16 -- which makes its two passes exactly that arithmetic -- and the equality asserted is
                             the same bit equality.
  b. V1                      the staged V1 forward takes an fp32 encoding and the renderer encodes in the kernel: against the
                             staged forward on TORCH's encoding, which is what this file feeds it, bit equality is not owed.
                             A RECORD line per case gives the share of bit-equal open samples and the largest difference;
                             asserted are the existing bounds (1e-4 for f32 / f16x3; 4e-3 / 4e-2 for f16 / bf16, as
                             test_render_end_to_end_golden_16bit states them for this 'fog' scene) on the colours, and
                             open == (sigma > 0) wherever the staged |sigma| is at or above that bound; and the SPW = 8 and
                             queue probes are torch.equal to the plain probe (colours and weights).  The bit-level anchor of
                             the V1 renderers is tests/test_gpu_train_rays_link.py, section 3: the ray-input training forward
                             saves the kernel's own encoding of these very samples, and on THAT encoding the staged forward
                             equals the probe colour for colour, open for open, on each of the three routes in f32, f16 and
                             bf16 (same nets, rays, S and depth kinds as here).  f16x3 has no training kernel, hence no saved
                             encoding: the 1e-4 bound of this section is what holds it.
  c. compositor and plumbing every net: the S-sample render under the launcher's deal, the uniform deal at SPW = 1 and SPW = 8
                             (NRF_SPW, as tests/test_gpu_even_deal.py) and, for the jittered depths, the ray-queue kernel
                             (ert_eps = 1e-30), with and without the white background: z_vals are the staged sampler's bits; rgb
                             and depth equal the float64 sums of the render's OWN weights times the plain probe's colours / its
                             depths within bound_rgb / bound_depth; a closed sample weighs exactly 0; the render_kernel routes
                             are torch.equal to one another; V2 / V3: the weights equal the float64 weights of the staged
                             forward's densities within bound_w (render_probe.py).
  even deal                  589 rays are too few for the launcher to take the even deal (it needs fewer passes than the uniform
                             one), and NRF_SPW pins the uniform deal, so two more cases per net and mode render 67 x 63 rays
                             where the launcher does take it (asserted): S = 70 with jitter and S = 48 with explicit depths,
                             through a and c.  A one-sample render never takes the even deal (it cannot need fewer passes), so
                             the even deal's colours cannot be probed; its S-sample renders are held by c's bound and are
                             torch.equal to the SPW = 1 and SPW = 8 renders of the same rays, whose paths the probes read.

RECORD (MI355X, gfx950; every case of this file, 90 tests in 28 s, the slowest 2.5 s):
  V2, V3 (64), V3 (128), V3 on the rendered camera, all four modes, S = 2 / 12 / 70, every depth kind, both ray sets and both
  even-deal cases: bit-equal to the staged forward on 1.0000 of the open samples (2 248 .. 194 225 per case) for EACH of the three
  probes (plain, SPW = 8, queue); no open/closed flip, no sample left out; the render_kernel routes, the even deal among them,
  bit-equal to one another.  (That the equality notices a rounding, measured once with the plain probe: v3w f16 with the fetch NOT
  rounded to f16 is bit-equal on 0.31 of its open samples, v3 f16 and v3w bf16 WITH it rounded on 0.38 / 0.31.)
  V1 (b), over all cases and probes of a mode (the three probes of a case are bit-equal to one another):
  share of bit-equal open samples / max |colour diff| / largest staged |sigma| of an open/closed flip
    f32    0.0000 .. 0.0005   1.8e-06   none         f16x3  0.0006 .. 0.0035   1.6e-06   none
    f16    0.9738 .. 0.9790   1.6e-03   3.4e-04      bf16   0.9957 .. 0.9969   1.2e-02   2.2e-03
  c, largest |difference| / asserted bound over all nets, modes and routes: rgb 0.47, depth 0.46 (both at S = 2, where the worst
  case of a correct implementation is exactly 0.5), weights 0.11.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import render_probe as P

pytestmark = pytest.mark.gpu

V1_BOUND = {"f32": 1e-4, "f16x3": 1e-4, "f16": 4e-3, "bf16": 4e-2}
COLS = {"f32": 32, "f16x3": 32, "f16": 64, "bf16": 64}            # sample columns of a wave (fused_impl.hpp: dispatch)
CASES = [(net, mode) for net in ("v1", "v2", "v3", "v3w") for mode in P.MODES] + [("v3own", "f16"), ("v3own", "bf16")]
EVEN_H, EVEN_W, EVEN_CASES = P.EVEN_H, P.EVEN_W, P.EVEN_CASES
JITTER = dict(perturb=True, seed=5)


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def g(golden):
    return golden("dino_views")


def make_model(N, net, mode):
    fam, dd = P.NETS[net][:2]
    if fam == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
    else:
        m = N.NeRFMLP(pos_freq=12 if fam == "v3" else 10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=fam == "v3",
                      dino_dim=dd, mma_mode=mode)
    m.load_state_dict(P.weights_of(net), strict=False)
    return m.cuda().eval()


class Link:
    """One net in one mode: the model, its source view, and the findings of a test."""

    def __init__(self, N, g, net, mode):
        self.N, self.net, self.mode, self.fam, self.dd = N, net, mode, P.NETS[net][0], P.NETS[net][1]
        self.model = make_model(N, net, mode)
        self.src = P.source_view(g, net)
        if self.src is not None:
            self.src = dict(self.src, features=self.src["features"].cuda().contiguous())
        self.fails = []
        self.equal_open, self.n_open = {"plain": 0, "spw8": 0, "queue": 0}, {"plain": 0, "spw8": 0, "queue": 0}      # per probe route
        self.max_diff, self.max_sigma_flip = 0.0, 0.0
        self.worst = dict(rgb=0.0, depth=0.0, weights=0.0)          # the largest |difference| / bound of section c

    def render(self, ro, rd, S, **kw):
        if self.src is not None:
            kw["dino"] = self.src
        return self.N.render_rays(self.model, ro, rd, P.NEAR, P.FAR, S, return_z=True, **kw)

    @torch.no_grad()                                  # nrf_mlp_forward: under grad the module would take the training forward
    def forward(self, pts, dirs):
        """The staged forward at (n,3) device points -> (rgb (n,3), sigma (n,): V1 raw, V2 / V3 behind the density ReLU), CPU."""
        if self.fam == "v1":
            out = self.model(O.positional_encoding(pts.cpu(), 10).cuda())
            return out[:, :3].cpu(), out[:, 3].cpu()
        feats = None
        if self.fam == "v3":
            from nerf_few_shot_limitations_amd import _lib as L
            d, keep = self.N.make_dino(**self.src)
            n = pts.shape[0]
            feats = torch.empty((n, self.dd), device="cuda")
            L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(pts), n, L.ptr(feats), None, L.stream_ptr()))
            if self.mode == "f16" and self.dd == 128:
                feats = feats.half().float()              # nets.hpp: DinoHeld<ModeF16, 4> holds the channels rounded to f16
        rgb, den = self.model(pts, dirs, feats)
        return rgb.cpu(), den[:, 0].cpu()

    def fail(self, *what):
        self.fails.append(" ".join(str(w) for w in what))


def deal_is_even(n_rays, n_samples, cols):
    from nerf_few_shot_limitations_amd import _lib as L
    head, n = (C.c_int64 * 4)(), C.c_int64(0)
    cu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    L.check(L.lib().nrf_debug_ray_deal(n_rays, n_samples, cols, cu, head, None, 0, C.byref(n)))
    return bool(head[0])


class Case:
    """One set of device rays with one kind of depths: the S-sample render under the launcher's deal, its depths, the staged
    sampler's points, the plain probe and the staged forward on those points."""

    def __init__(self, link, monkeypatch, ro, rd, S, tag, kw):
        self.link, self.mp, self.ro, self.rd, self.S, self.kw = link, monkeypatch, ro, rd, S, kw
        self.R = ro.shape[0]
        self.tag = f"{link.net} {link.mode} S={S} R={self.R} {tag}"
        monkeypatch.delenv("NRF_SPW", raising=False)
        self.base = link.render(ro, rd, S, **kw)
        self.z = self.base["z_vals"]
        self.pts = self.points()
        dirs = rd[:, None, :].expand(-1, S, -1).reshape(-1, 3).contiguous()
        rgb, sig = link.forward(self.pts.reshape(-1, 3).contiguous(), dirs)
        self.rgb_f, self.sig_f = rgb.reshape(self.R, S, 3), sig.reshape(self.R, S)
        self.probe = self.run_probe(None)

    def points(self):
        """The staged sampler's points; its depths must be the render's (explicit depths: point_on_ray in fp32 on the CPU)."""
        link, kw, z = self.link, self.kw, self.z
        if "z_in" in kw:
            if not torch.equal(z, kw["z_in"]):
                link.fail(self.tag, "z_vals are not the z_in")
            return P.points32(self.ro, self.rd, z).cuda()
        pts, z_staged = link.N.sample_points_along_rays(self.ro, self.rd, P.NEAR, P.FAR, self.S, perturb=kw.get("perturb", False),
                                                        lindisp=kw.get("lindisp", False), seed=kw.get("seed"))
        if not torch.equal(z, z_staged):
            link.fail(self.tag, "z_vals differ from the staged sampler's:", int((z != z_staged).sum()), "of", z.numel())
        if not torch.equal(pts.cpu(), P.points32(self.ro, self.rd, z)):
            link.fail(self.tag, "the staged sampler's points are not point_on_ray(o, d, z)")
        return pts

    def run_probe(self, spw, **extra):
        if spw is None:
            self.mp.delenv("NRF_SPW", raising=False)
        else:
            self.mp.setenv("NRF_SPW", spw)
        if self.link.src is not None:
            extra["dino"] = self.link.src
        pr = P.probe(self.link.N, self.link.model, self.ro, self.rd, self.z, **extra)
        self.mp.delenv("NRF_SPW", raising=False)
        return pr


# the routes a one-sample render can take: render_kernel at one sample per column (what the launcher picks for S = 1), render_kernel
# through the SPW = 8 column-to-owner exchange (NRF_SPW=3: seven of a ray's eight columns idle), render_queue_kernel.  The even deal
# cannot be probed -- with S = 1 it never needs fewer passes than the uniform deal -- so its S-sample renders are held bit for bit
# to the uniform deal's instead (check_routes).
PROBES = [("plain", None, {}), ("spw8", "3", {}), ("queue", None, dict(ert_eps=1e-30))]


def check_network(case, want_shares):
    """a / b of the header, for the probe on each of its routes."""
    link, mode = case.link, case.link.mode
    rgb_f, sig_f, plain = case.rgb_f, case.sig_f, case.probe
    for name, spw, extra in PROBES:
        tag = f"{case.tag} probe:{name}"
        pr = plain if name == "plain" else case.run_probe(spw, **extra)
        open_, closed, left = pr.shares()
        if left > P.LEFT_OUT_CAP or (want_shares and min(open_, closed) < P.MIN_SHARE):
            link.fail(tag, f"shares: open {open_:.3f} closed {closed:.3f} left out {left:.4f}")
        same = (pr.colour == rgb_f).all(-1)
        diff = float((pr.colour.double() - rgb_f.double()).abs()[pr.open].max()) if bool(pr.open.any()) else 0.0
        flips = (pr.open != (sig_f > 0)) & ~pr.left_out
        link.equal_open[name] += int(same[pr.open].sum()); link.n_open[name] += int(pr.open.sum())
        link.max_diff = max(link.max_diff, diff)
        if link.fam == "v1":
            bound = V1_BOUND[mode]
            if diff > bound:
                link.fail(tag, f"colour: max |probe - staged| {diff:.3e} > {bound:g}")
            if bool(flips.any()):
                link.max_sigma_flip = max(link.max_sigma_flip, float(sig_f[flips].abs().max()))
            if bool((flips & (sig_f.abs() >= bound)).any()):
                link.fail(tag, f"open != (sigma > 0) at |sigma| up to {float(sig_f[flips].abs().max()):.3e} >= {bound:g}")
            if not (torch.equal(pr.colour, plain.colour) and torch.equal(pr.w, plain.w)):         # V1's strict tie between the routes
                link.fail(tag, f"differs from the plain probe on {int((pr.colour != plain.colour).any(-1).sum())} samples")
        else:
            if not bool(same[pr.open].all()):
                link.fail(tag, f"colour: {int((~same[pr.open]).sum())} of {int(pr.open.sum())} open samples differ bitwise, max {diff:.3e}")
            if bool(flips.any()):
                link.fail(tag, f"open != (density > 0) on {int(flips.sum())} samples")


def check_routes(case, routes, whites):
    """c of the header: every route's S-sample render against its own weights and the plain probe's colours."""
    link, S, z, pr = case.link, case.S, case.z, case.probe
    norm = P.ray_norm32(case.rd)
    zc, colour = z.cpu().numpy(), pr.colour.numpy()
    whole = ~pr.left_out.any(1).numpy()                      # rays without a left-out sample
    w_staged = P.weights64(case.sig_f.numpy(), P.dist32(z, norm)) if link.fam != "v1" else None
    first = {}
    for route, spw, extra in routes:
        if spw is None:
            case.mp.delenv("NRF_SPW", raising=False)
        else:
            case.mp.setenv("NRF_SPW", spw)
        for white in whites:
            what = f"{case.tag} {route}{' white' if white else ''}"
            out = case.base if (route, white) == ("launcher", False) else link.render(case.ro, case.rd, S, white_bkgd=white, **case.kw, **extra)
            if not torch.equal(out["z_vals"], z):
                link.fail(what, "z_vals differ from the launcher's")
            if route != "queue":                             # the deals and splits of render_kernel are invisible: bit for bit
                ref = first.setdefault(white, out)
                if not all(torch.equal(out[k], ref[k]) for k in ("rgb", "depth", "weights")):
                    link.fail(what, "differs bitwise from the launcher's render")
            w = out["weights"].cpu()
            if bool((w[pr.closed] != 0).any()):
                link.fail(what, f"{int((w[pr.closed] != 0).sum())} closed samples carry weight")
            e_rgb, e_depth, mag_rgb, mag_depth, acc = P.expected_image(w.numpy(), colour, zc, white)
            b_rgb, b_depth = P.image_bounds(S, e_rgb, mag_rgb, mag_depth, acc, white)
            r_rgb = (np.abs(out["rgb"].cpu().numpy().astype(np.float64) - e_rgb) / b_rgb)[whole]
            r_depth = (np.abs(out["depth"].cpu().numpy().astype(np.float64) - e_depth) / b_depth)[whole]
            if r_rgb.size:
                link.worst["rgb"], link.worst["depth"] = max(link.worst["rgb"], float(r_rgb.max())), max(link.worst["depth"], float(r_depth.max()))
                if r_rgb.max() > 1 or r_depth.max() > 1:
                    link.fail(what, f"rgb {r_rgb.max():.3g} x its bound, depth {r_depth.max():.3g} x its bound")
            if w_staged is not None:
                r_w = np.abs(w.numpy().astype(np.float64) - w_staged) / P.weight_bound(S, link.mode)[None, :]
                link.worst["weights"] = max(link.worst["weights"], float(r_w.max()))
                if r_w.max() > 1:
                    link.fail(what, f"weights {r_w.max():.3g} x their bound")
    case.mp.delenv("NRF_SPW", raising=False)


def finish(link, what):
    torch.cuda.synchronize()
    shares = " ".join(f"{k} {link.equal_open[k] / max(1, link.n_open[k]):.4f} of {link.n_open[k]}" for k in link.n_open)
    print(f"RECORD {link.net} {link.mode} {what}: open samples bit-equal to the staged forward, per probe route: {shares}; "
          f"max |colour diff| {link.max_diff:.3e}" + (f", largest staged |sigma| of an open/closed flip {link.max_sigma_flip:.3e}"
                                                      if link.fam == "v1" else "")
          + "; of its bound: " + " ".join(f"{k} {v:.3f}" for k, v in link.worst.items() if k != "weights" or link.fam != "v1"))
    assert not link.fails, f"{len(link.fails)} findings:\n" + "\n".join(link.fails)


UNIFORM = [("launcher", None, {}), ("spw1", "0", {}), ("spw8", "3", {})]
QUEUE = [("queue", None, dict(ert_eps=1e-30))]


@pytest.mark.parametrize("S", P.S_VALUES)
@pytest.mark.parametrize("net,mode", CASES)
def test_render_link(N, g, net, mode, S, monkeypatch):
    link = Link(N, g, net, mode)
    ro, rd = (t.cuda() for t in P.frame_rays())
    for o, d in ((ro, rd), (ro[293:296].contiguous(), rd[293:296].contiguous())):
        R = o.shape[0]
        for tag, kw in (("ladder", {}), ("lindisp", dict(lindisp=True)), ("jitter", JITTER), ("z_in", dict(z_in=P.random_depths(R, S).cuda()))):
            case = Case(link, monkeypatch, o, d, S, tag, kw)
            check_network(case, want_shares=R > 3)
            check_routes(case, UNIFORM + (QUEUE if tag == "jitter" else []), (False, True))
    finish(link, f"S={S}")


@pytest.mark.parametrize("mode", P.MODES)
def test_emitting_render_link_at_dino_dim_128(N, g, mode, monkeypatch):
    """render_emit_kernel of V3 at dino_dim 128 (objects fused_emit_v3w_16 / fused_emit_v3w_32), the one (kind, family) no other GPU
    test launches: tests/test_gpu_hier_reuse.py emits with V1, V2 and V3 at 64.  300 rays (one full 256-column tile and a ragged one)
    at 3 explicit depths (odd, more than one): the render's outputs are the plain render's bits, and the emitted rows are the staged
    forward's outputs sample by sample -- the density in front of the ReLU, and the colour as the compositor reads it out of the row
    (nrf_composite_merge on one sample, where an open sample weighs exactly 1), torch.equal on every open sample; a sample is open
    exactly where the staged density is > 0.  The scene opens and closes a fair share of these samples (asserted)."""
    monkeypatch.delenv("NRF_SPW", raising=False)
    link, R, S = Link(N, g, "v3w", mode), 300, 3
    ro, rd = (t[:R].cuda().contiguous() for t in P.frame_rays())
    z = P.random_depths(R, S).cuda()
    plain = link.render(ro, rd, S, z_in=z)
    emit = N.render_rays_emit(link.model, ro, rd, P.NEAR, P.FAR, S, dino=link.src, z_in=z)
    for k in ("rgb", "depth", "weights", "z_vals"):
        assert torch.equal(emit[k], plain[k]), k
    assert torch.equal(emit["z_vals"], z)
    dirs = rd[:, None, :].expand(-1, S, -1).reshape(-1, 3).contiguous()
    rgb_f, den_f = link.forward(P.points32(ro, rd, z).cuda().reshape(-1, 3).contiguous(), dirs)
    rgb_f, den_f = rgb_f.reshape(R, S, 3), den_f.reshape(R, S)
    raw = emit["raw4"]
    assert torch.equal(torch.relu(raw[..., 3]).cpu(), den_f)
    cols = [N.composite_merge(z[:, s:s + 1].contiguous(), raw[:, s:s + 1].contiguous(), rd, mma_mode=mode) for s in range(S)]
    pr = P.Probe(torch.stack([c["rgb"] for c in cols], 1).cpu(), torch.stack([c["weights"][:, 0] for c in cols], 1).cpu())
    open_, closed, left = pr.shares()
    print(f"RECORD emit v3w {mode}: open {open_:.3f} closed {closed:.3f} left out {left:.4f}")
    assert left <= P.LEFT_OUT_CAP and min(open_, closed) >= P.MIN_SHARE, (open_, closed, left)
    assert torch.equal(pr.colour[pr.open], rgb_f[pr.open])
    assert not bool(((pr.open != (den_f > 0)) & ~pr.left_out).any())


@pytest.mark.parametrize("S,tag", EVEN_CASES)
@pytest.mark.parametrize("net,mode", CASES)
def test_render_link_under_the_even_deal(N, g, net, mode, S, tag, monkeypatch):
    monkeypatch.delenv("NRF_SPW", raising=False)
    assert deal_is_even(EVEN_H * EVEN_W, S, COLS[mode]), "the case was chosen so that the launcher takes the even deal"
    link = Link(N, g, net, mode)
    ro, rd = N.get_rays(EVEN_H, EVEN_W, O.focal_for(EVEN_W), P.T(O.LEGO_LIKE_C2W))
    ro, rd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous()
    kw = JITTER if tag == "jitter" else dict(z_in=P.random_depths(ro.shape[0], S).cuda())
    case = Case(link, monkeypatch, ro, rd, S, "even deal, " + tag, kw)
    check_network(case, want_shares=True)
    check_routes(case, UNIFORM, (False, True))              # the launcher's render (even) first: the uniform deals must equal it
    finish(link, f"even deal S={S} {tag}")
