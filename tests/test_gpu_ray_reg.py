"""The few-shot ray regularisers of the fused training step on the GPU (nerfhip.h: nrf_composite_reg_loss_backward,
nrf_ray_terms_finish; FusedStep(dist_weight=, occ_weight=, occ_samples=, dist_span=)).

The oracle of the two terms is float64 autograd through oracle.nerf_oracle.volume_render plus their definitions written out
below (the reference has no counterpart).  The bars are tests/test_gpu_multiscale_step.py's check_against; what leaves them a
margin is measured without a GPU in tests/test_ray_reg_host.py."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_multiscale_step import check_against, normals, run_loss_backward
from tests.test_gpu_training import make_model, make_v2, make_v3
from tests.test_ray_reg_host import case, distortion

pytestmark = pytest.mark.gpu

SHAPES = [(5, 2), (37, 16), (9, 64), (9, 65), (7, 130), (3, 200)]
KAPPA = 0.25                      # 1 / (far - near) of the depths in [2, 6]


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def L(N):
    from nerf_few_shot_limitations_amd import _lib as L
    return L


def run_reg(L, rgb, sig, z, d, tgt, white=False, w=(1.0, 0.0, 0.0), tdepth=None, noise_std=0.0, noise=None, reg=None, slot=None, with_losses=True,
            zero_n=0):
    """nrf_composite_reg_loss_backward [+ nrf_adamw_step_loss's loss side job on a dummy parameter vector + nrf_ray_terms_finish] ->
    dict of device tensors.  Dense: rgb (R,S,3), sig (R,S[,1]); with `slot` (R,S): rgb (M,3), sig (M) compacted rows."""
    lib, st = L.lib(), L.stream_ptr()
    R, S = z.shape
    c, s_ = rgb.reshape(-1, 3).contiguous().cuda(), sig.reshape(-1).contiguous().cuda()
    rows = c.shape[0]
    zc, dc, tc = z.contiguous().cuda(), d.contiguous().cuda(), tgt.contiguous().cuda()
    td = None if tdepth is None else tdepth.contiguous().cuda()
    nz = None if noise is None else noise.reshape(R, S).contiguous().cuda()
    sl = None if slot is None else slot.reshape(R, S).to(torch.int32).contiguous().cuda()
    out = dict(pred=torch.empty(R, 3, device="cuda"), d_rgb=torch.full((rows, 3), 7.0, device="cuda"), d_sigma=torch.full((rows,), 7.0, device="cuda"),
               terms=torch.full((5, R), float("nan"), device="cuda"), zero=torch.ones(max(zero_n, 1), device="cuda"))
    lo = L.loss_opts(w[0], w[2], w[1], L.ptr(td), noise_std, L.ptr(nz), 0)
    reg = reg if reg is not None else L.ray_reg()
    L.check(lib.nrf_composite_reg_loss_backward(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, int(white), L.ptr(tc), C.byref(lo), C.byref(reg),
                                                None if sl is None else sl.data_ptr(), L.ptr(out["pred"]), L.ptr(out["d_rgb"]), 3, L.ptr(out["d_sigma"]), 1,
                                                L.ptr(out["terms"]), L.ptr(out["zero"]) if zero_n else None, zero_n, st))
    if with_losses:
        p, g, m, v = (torch.zeros(4, device="cuda") for _ in range(4))
        l4 = torch.empty(4, device="cuda")
        out["losses"] = torch.full((6,), float("nan"), device="cuda")
        L.check(lib.nrf_adamw_step_loss(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 0, 0.0, None, None, L.ptr(out["terms"]),
                                        R, S, w[0], w[1] if tdepth is not None else 0.0, w[2], L.ptr(l4), st))
        L.check(lib.nrf_ray_terms_finish(L.ptr(out["terms"]), R, C.byref(reg), L.ptr(l4), L.ptr(out["losses"]), st))
    torch.cuda.synchronize()
    if slot is None:
        out["d_rgb"], out["d_sigma"] = out["d_rgb"].reshape(R, S, 3), out["d_sigma"].reshape(R, S)
    return out


def oracle(rgb, sig, z, d, tgt, white, w, tdepth, noise_std, noise, dist_weight, occ_weight, occ_samples):
    """float64 autograd: the reference's VolumeRenderer (train mode) + nerf_mlp.NeRFLoss as tests/test_gpu_multiscale_step.py writes
    them out, + dist_weight mean D + occ_weight mean O by their definitions.  A term whose weight is 0 reports 0, as the library does."""
    f = torch.float64
    r1, s1 = rgb.to(f).requires_grad_(True), sig.to(f).reshape(*z.shape, 1).requires_grad_(True)
    dens = s1 if noise is None else s1 + noise.to(f).reshape(s1.shape) * noise_std
    o_rgb, o_dep, o_w = O.volume_render(r1, dens, z.to(f), d.to(f), white_bkgd=white)
    l_rgb = torch.nn.functional.mse_loss(o_rgb, tgt.to(f))
    l_dep = torch.nn.functional.l1_loss(o_dep, tdepth.to(f)) if tdepth is not None else torch.zeros((), dtype=f)
    l_reg = torch.mean(o_w ** 2)
    S = z.shape[1]
    l_dist = distortion(o_w, z.to(f), KAPPA).mean() if dist_weight > 0 else torch.zeros((), dtype=f)
    m = min(occ_samples, S)
    l_occ = torch.relu(dens[:, :m, 0]).mean(dim=1).mean() if occ_weight > 0 else torch.zeros((), dtype=f)
    total = w[0] * l_rgb + w[1] * l_dep + w[2] * l_reg + dist_weight * l_dist + occ_weight * l_occ
    total.backward()
    return dict(pred=o_rgb.detach().float(), losses=torch.stack([total, l_rgb, l_dep, l_reg, l_dist, l_occ]).detach(), d_rgb=r1.grad,
                d_sigma=s1.grad[..., 0])


# ---------------------------------------------------------------------------------------------
# 1. the raw entry against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("terms", ["dist", "occ", "all"])
@pytest.mark.parametrize("R,S", SHAPES)
def test_entry_matches_float64_autograd(L, R, S, terms):
    tgt = torch.from_numpy(O.uniform01(54, R * 3).reshape(R, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(55, R) * 4 + 2).float() if terms == "all" else None
    noise = normals(56, R * S).reshape(R, S, 1) if terms == "all" else None
    std = 0.4 if terms == "all" else 0.0
    w = (0.7, 0.3, 0.5) if terms == "all" else (0.0, 0.0, 0.0)
    dw = 0.0 if terms == "occ" else 0.6
    ow = 0.0 if terms == "dist" else 0.8
    for opaque in (False, True):
        rgb, sig, z, d = case(R, S, 41 + S, opaque)
        assert torch.all(z[:, S // 2] == z[:, S // 2 - 1])                   # a pair of equal depths in every ray
        for white in (False, True):
            for k in ((1,) if terms == "dist" else (1, 5, 70, S + 3)):
                reg = L.ray_reg(dw, KAPPA if dw > 0 else 0.0, ow, k if ow > 0 else 0)
                got = run_reg(L, rgb, sig, z, d, tgt, white, w, tdepth, std, noise, reg)
                ref = oracle(rgb, sig, z, d, tgt, white, w, tdepth, std, noise, dw, ow, k)
                print(f"(R,S)=({R},{S}) {terms} opaque={opaque} white={white} occ_samples={k}")
                check_against(got, ref, 1e-4)
                eff = sig[..., 0] + (noise[..., 0] * std if noise is not None else 0.0)
                assert (eff <= 0).any() and torch.all(got["d_sigma"].cpu()[eff <= 0] == 0)      # the occlusion term included
                if terms != "occ":
                    assert got["losses"][4].item() > 0 or S == 2
                if terms != "dist":
                    assert got["losses"][5].item() > 0
                    assert torch.any(got["d_sigma"].cpu()[:, : min(k, S)] != 0)


def test_one_sample_per_ray_is_finite_and_has_no_distortion(L):
    """volume_render returns no weights at S = 1 (the appended 1e10 column comes from an empty slice): no oracle, D = 0 and finiteness."""
    R = 6
    rgb, sig, z, d = case(R, 1, 77, False)
    tgt = torch.from_numpy(O.uniform01(54, R * 3).reshape(R, 3)).float()
    got = run_reg(L, rgb, sig, z, d, tgt, False, (1.0, 0.0, 0.1), reg=L.ray_reg(0.6, KAPPA, 0.8, 3))
    for k in ("pred", "d_rgb", "d_sigma", "terms", "losses"):
        assert torch.isfinite(got[k]).all(), k
    assert torch.all(got["terms"][3] == 0) and got["losses"][4].item() == 0
    assert torch.equal(got["terms"][4].cpu(), torch.relu(sig[:, 0, 0]))


# ---------------------------------------------------------------------------------------------
# 2. options off: the parents' bits
# ---------------------------------------------------------------------------------------------
def skip_map(R, S, seed, k_front):
    """(R,S) bool, True = evaluated: about 40 % of the samples skipped, ray 1 whole, and the first k_front samples of ray 2."""
    keep = torch.from_numpy(O.uniform01(seed, R * S).reshape(R, S)) >= 0.4
    keep[1] = False
    keep[2, :k_front] = False
    keep[2, min(k_front, S - 1):] |= True
    return keep


def compacted(rgb, sig, keep):
    """The evaluated rows in ascending flat order and their slot map (-1 = skipped), as nrf_occupancy_compact_rays leaves them."""
    flat = keep.reshape(-1)
    slot = torch.full((flat.numel(),), -1, dtype=torch.int32)
    slot[flat] = torch.arange(int(flat.sum()), dtype=torch.int32)
    return rgb.reshape(-1, 3)[flat].contiguous(), sig.reshape(-1)[flat].contiguous(), slot.reshape(keep.shape)


@pytest.mark.parametrize("R,S,opaque,white", [(37, 16, False, False), (9, 65, True, True), (7, 130, True, False)])
def test_options_off_are_the_parents_bits(L, R, S, opaque, white):
    lib, st = L.lib(), L.stream_ptr()
    rgb, sig, z, d = case(R, S, 61, opaque)
    tgt = torch.from_numpy(O.uniform01(62, R * 3).reshape(R, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(63, R) * 4 + 2).float()
    noise = normals(64, R * S).reshape(R, S, 1)
    w, std = (0.7, 0.3, 0.5), 0.4
    old = run_loss_backward(L, rgb, sig, z, d, tgt, white, w, tdepth, std, noise, zero_n=1000, with_losses=False)
    new = run_reg(L, rgb, sig, z, d, tgt, white, w, tdepth, std, noise, reg=L.ray_reg(0.0, 0.0, 0.0, 4), zero_n=1000, with_losses=False)
    assert torch.equal(new["pred"], old["pred"]) and torch.equal(new["d_rgb"], old["d_rgb"]) and torch.equal(new["d_sigma"], old["d_sigma"])
    assert torch.equal(new["terms"][:3], old["terms"]) and torch.isfinite(new["terms"][3:]).all()
    assert torch.all(new["zero"] == 0)
    # the indexed parent
    keep = skip_map(R, S, 65, 3)
    rc, sc, slot = compacted(rgb, sig, keep)
    M = rc.shape[0]
    c, s_, zc, dc, tc, td, nz, sl = (t.contiguous().cuda() for t in (rc, sc, z, d, tgt, tdepth, noise.reshape(R, S), slot))
    pred, d_rgb, d_sig, terms = torch.empty(R, 3, device="cuda"), torch.full((M, 3), 7.0, device="cuda"), torch.full((M,), 7.0, device="cuda"), torch.empty(3, R, device="cuda")
    lo = L.loss_opts(w[0], w[2], w[1], L.ptr(td), std, L.ptr(nz), 0)
    L.check(lib.nrf_composite_loss_backward_indexed(L.ptr(c), 3, L.ptr(s_), 1, L.ptr(zc), L.ptr(dc), R, S, int(white), L.ptr(tc), C.byref(lo), sl.data_ptr(),
                                                    L.ptr(pred), L.ptr(d_rgb), 3, L.ptr(d_sig), 1, L.ptr(terms), None, 0, st))
    torch.cuda.synchronize()
    new = run_reg(L, rc, sc, z, d, tgt, white, w, tdepth, std, noise, reg=L.ray_reg(), slot=slot, with_losses=False)
    assert torch.equal(new["pred"], pred) and torch.equal(new["d_rgb"], d_rgb) and torch.equal(new["d_sigma"], d_sig)
    assert torch.equal(new["terms"][:3], terms) and torch.isfinite(new["terms"][3:]).all()


# ---------------------------------------------------------------------------------------------
# 3. indexed against dense, terms on; 4. two runs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S,k", [(37, 16, 5), (9, 65, 5), (7, 130, 70), (3, 200, 203)])
def test_indexed_entry_is_the_dense_entry_on_masked_rows_and_runs_repeat(L, R, S, k):
    rgb, sig, z, d = case(R, S, 81, True)
    tgt = torch.from_numpy(O.uniform01(82, R * 3).reshape(R, 3)).float()
    tdepth = torch.from_numpy(O.uniform01(83, R) * 4 + 2).float()
    noise = normals(84, R * S).reshape(R, S, 1)
    w, std = (0.7, 0.3, 0.5), 0.4
    keep = skip_map(R, S, 85, min(k, S))
    frac = 1.0 - keep.float().mean().item()
    assert 0.3 < frac < 0.6 or R < 5, frac
    rc, sc, slot = compacted(rgb, sig, keep)
    reg = L.ray_reg(0.6, KAPPA, 0.8, k)
    idx = run_reg(L, rc, sc, z, d, tgt, True, w, tdepth, std, noise, reg, slot=slot)
    rgb_m = torch.where(keep[..., None], rgb, torch.zeros_like(rgb))
    sig_m = torch.where(keep[..., None], sig, torch.full_like(sig, float("-inf")))
    dense = run_reg(L, rgb_m, sig_m, z, d, tgt, True, w, tdepth, std, noise, reg)
    assert torch.equal(idx["pred"], dense["pred"]) and torch.equal(idx["terms"], dense["terms"]) and torch.equal(idx["losses"], dense["losses"])
    assert torch.isfinite(idx["terms"]).all() and torch.isfinite(idx["losses"]).all()
    flat = keep.reshape(-1).cuda()
    assert torch.equal(idx["d_rgb"], dense["d_rgb"].reshape(-1, 3)[flat]) and torch.equal(idx["d_sigma"], dense["d_sigma"].reshape(-1)[flat])
    assert torch.all(dense["d_sigma"].reshape(-1)[~flat] == 0)
    assert torch.all(idx["terms"][3:, 1] == 0)                       # the ray that keeps no sample: no weight, no density
    # two runs give the same bits, kernels and losses6
    for again, first in ((run_reg(L, rc, sc, z, d, tgt, True, w, tdepth, std, noise, reg, slot=slot), idx),
                         (run_reg(L, rgb_m, sig_m, z, d, tgt, True, w, tdepth, std, noise, reg), dense)):
        for key in ("pred", "d_rgb", "d_sigma", "terms", "losses"):
            assert torch.equal(again[key], first[key]), key


# ---------------------------------------------------------------------------------------------
# 5. FusedStep against the autograd route
# ---------------------------------------------------------------------------------------------
OPTS = dict(reg_weight=1e-4, depth_weight=0.1, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True)
REG = dict(dist_weight=0.05, occ_weight=0.02, occ_samples=4)
WD = 1e-6
NEAR, FAR = 2.0, 6.0


def torch_terms(w, dens, z, keep=None):
    """mean D and mean O in torch from the autograd route's weights and densities (the definitions above)."""
    dist = distortion(w, z, 1.0 / (FAR - NEAR)).mean()
    occ = torch.relu(dens[:, : REG["occ_samples"], 0]).mean(dim=1).mean()
    return dist, occ


def models(N, net, mode):
    if net == "v1":
        return make_model(N, mode, scene="solid", n_layers=2)[0], make_model(N, mode, scene="solid", n_layers=2)[0]
    if net == "v2":
        return make_v2(N, mode, scene="solid", n_layers=2)[0], make_v2(N, mode, scene="solid", n_layers=2)[0]
    return make_v3(N, mode, scene="solid", n_layers=2)[0], make_v3(N, mode, scene="solid", n_layers=2)[0]


def autograd_steps(N, a, net, steps, pts, dirs, dino, z, rd, tgt, tdepth, noise, keep=None):
    """test_fused_step_with_all_options_equals_autograd_route's reference loop with the two terms added in torch; keep (R,S): the
    samples a grid evaluates -- the others composite as colour 0 and density -inf."""
    R, S = z.shape
    a.flat_params().ensure()
    params = list(a.parameters())
    opt = torch.optim.AdamW(params, lr=5e-4, weight_decay=WD)
    vr = N.VolumeRenderer()
    losses, norms, parts = [], [], []
    for _ in range(steps):
        opt.zero_grad()
        if net == "v1":
            o4 = a(pts).view(R, S, 4)
            c, sg = o4[..., :3], o4[..., 3:4]
        else:
            c, sg = a(pts, dirs, dino)
            c, sg = c.view(R, S, 3), sg.view(R, S, 1)
        dens = sg + noise.view(R, S, 1) * OPTS["noise_std"]
        if keep is not None:
            c = torch.where(keep[..., None], c, torch.zeros_like(c))
            dens = torch.where(keep[..., None], dens, torch.full_like(dens, float("-inf")))
        pred, depth, w = vr(c, dens, z, rd)
        dist, occ = torch_terms(w, dens, z)
        loss = (torch.nn.functional.mse_loss(pred, tgt) + OPTS["depth_weight"] * torch.nn.functional.l1_loss(depth, tdepth)
                + OPTS["reg_weight"] * torch.mean(w ** 2) + REG["dist_weight"] * dist + REG["occ_weight"] * occ)
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, OPTS["max_grad_norm"])))
        opt.step()
        losses.append(loss.item())
        parts.append((dist.item(), occ.item()))
    return losses, norms, parts


def compare(net, mode, ref, got):
    (ref_losses, ref_norms, ref_parts), (losses, norms, parts) = ref, got
    print(net, mode, "losses", ref_losses, losses, "norms", ref_norms, norms, "dist, occ", ref_parts, parts)
    tol = 1e-5 if mode == "f32" else 2e-3
    assert np.allclose(ref_losses, losses, rtol=tol, atol=1e-7), (ref_losses, losses)
    assert np.allclose(np.asarray(ref_parts), np.asarray(parts), rtol=max(2e-4, tol), atol=1e-7), (ref_parts, parts)
    assert abs(norms[0] - ref_norms[0]) <= max(2e-4, tol) * ref_norms[0], (ref_norms, norms)


def fused_loop(step, steps, call):
    losses, norms, parts = [], [], []
    for _ in range(steps):
        losses.append(call().item())
        norms.append(step.last_grad_norm.item())
        ll = step.last_losses
        assert sorted(ll) == ["depth", "dist", "occ", "reg", "rgb", "total"]
        parts.append((ll["dist"].item(), ll["occ"].item()))
        want = (ll["rgb"].item() + OPTS["depth_weight"] * ll["depth"].item() + OPTS["reg_weight"] * ll["reg"].item()
                + REG["dist_weight"] * ll["dist"].item() + REG["occ_weight"] * ll["occ"].item())
        assert abs(ll["total"].item() - want) < 1e-6 and ll["total"].item() == losses[-1]
    return losses, norms, parts


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v1", "bf16"), ("v2", "f32"), ("v2", "bf16"), ("v3", "f32"), ("v3", "bf16")])
def test_fused_step_with_the_terms_equals_autograd_route(N, net, mode):
    from nerf_few_shot_limitations_amd.training import FusedStep
    R, S, steps = 64, 16, 3
    z = torch.sort(torch.from_numpy(O.uniform01(101, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values.cuda()
    rd = torch.from_numpy(O.uniform01(102, R * 3).reshape(R, 3) - 0.5).float().cuda()
    tgt = torch.from_numpy(O.uniform01(103, R * 3).reshape(R, 3)).float().cuda()
    pos = torch.from_numpy(O.uniform01(104, R * S * 3).reshape(R * S, 3) * 4 - 2).float()
    tdepth = torch.from_numpy(O.uniform01(106, R) * 4 + 2).float().cuda()
    noise = normals(107, R * S).reshape(R, S).cuda()
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    a, b = models(N, net, mode)
    pts = O.positional_encoding(pos, 10).cuda() if net == "v1" else pos.cuda()
    dino = torch.from_numpy(O.uniform01(105, R * S * 64).reshape(R * S, 64) * 2 - 1).float().cuda() if net == "v3" else None
    ref = autograd_steps(N, a, net, steps, pts, dirs, dino, z, rd, tgt, tdepth, noise)
    step = FusedStep(b, lr=5e-4, weight_decay=WD, dist_span=FAR - NEAR, **OPTS, **REG)
    got = fused_loop(step, steps, lambda: step(pts, z, rd, tgt, dirs=dirs if net != "v1" else None, dino=dino, target_depth=tdepth, noise=noise))
    compare(net, mode, ref, got)
    assert max(ref[1]) > OPTS["max_grad_norm"]          # the clipping acts
    assert min(p[0] for p in ref[2]) > 0 and min(p[1] for p in ref[2]) > 0


def ray_scene(R, S):
    from tests.test_gpu_train_rays import ray_batch, u01
    o, d = ray_batch(R, seed=190)
    return dict(o=o, d=d, tgt=u01(191, R, 3).cuda(), tdepth=(u01(192, R) * 4 + 2).cuda(), noise=normals(193, R * S).reshape(R, S).cuda(),
                t_rand=u01(194, R, S).cuda())


@pytest.mark.parametrize("net,mode", [("v1", "f32"), ("v2", "f32"), ("v2", "bf16")])
def test_step_rays_with_the_terms_with_and_without_a_grid(N, net, mode):
    """step_rays with the terms on: (a) against the autograd route on the step's own depths; (b) under an all-ones grid, both
    grid_inputs: the bits of (a)'s fused run (V2; V1's staged route encodes the compacted points in another kernel: its own bars);
    (c) under a grid with holes, both grid_inputs, against the autograd route with the skipped samples masked."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    from tests.test_gpu_train_occupancy import grid_of, keep_replay
    R, S, steps = 64, 16, 3
    sc = ray_scene(R, S)
    kw = dict(perturb=True, t_rand=sc["t_rand"], target_depth=sc["tdepth"], noise=sc["noise"])

    def fused(**more):
        _, b = models(N, net, mode)
        step = FusedStep(b, lr=5e-4, weight_decay=WD, **OPTS, **REG)           # dist_span=None: far - near
        out = fused_loop(step, steps, lambda: step.step_rays(sc["o"], sc["d"], sc["tgt"], NEAR, FAR, S, **kw, **more))
        return out, step

    def reference(z, keep=None):
        a, _ = models(N, net, mode)
        pos = (sc["o"][:, None, :] + sc["d"][:, None, :] * z[:, :, None]).reshape(-1, 3)
        dirs = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
        pts = N.PositionalEncoding(10)(pos) if net == "v1" else pos
        return autograd_steps(N, a, net, steps, pts, dirs, None, z, sc["d"], sc["tgt"], sc["tdepth"], sc["noise"], keep)

    plain, step = fused()
    z = step.last_z.clone()
    compare(net, mode, reference(z), plain)
    ones = grid_of("ones", box=(-12.0, 12.0))
    holes = grid_of("random", outside=1, seed=195, box=(-6.0, 6.0))
    keep = torch.from_numpy(keep_replay(holes, sc["o"], sc["d"], z)[0]).cuda()
    assert 0.2 < keep.float().mean().item() < 0.8 and not keep[:, : REG["occ_samples"]].all()
    masked = reference(z, keep)
    for route in ("staged", "rays"):
        got, st = fused(occupancy=ones, grid_inputs=route)
        assert st.last_count == R * S
        if net == "v2":
            assert got == plain, route
        else:
            compare(net, mode, reference(z), got)
        got, st = fused(occupancy=holes, grid_inputs=route)
        assert st.last_count == int(keep.sum())
        compare(net, mode, masked, got)


# ---------------------------------------------------------------------------------------------
# 6. the library calls of a regularised step
# ---------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for the loaded library: forwards everything, keeps the names of the nrf_* calls (tests/test_gpu_train_launch_order.py)."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nrf_"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def record(run, monkeypatch):
    from nerf_few_shot_limitations_amd import _lib
    run()
    torch.cuda.synchronize()
    gc.collect()
    rec = Recorder(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", rec)
        run()
    torch.cuda.synchronize()
    return rec.names


@pytest.mark.parametrize("route", ["call", "rays", "grid-staged", "grid-rays"])
def test_a_regularised_step_is_the_multi_term_step_with_one_launch_more(N, route, monkeypatch):
    from nerf_few_shot_limitations_amd.training import FusedStep
    from tests.test_gpu_train_occupancy import grid_of
    R, S = 8, 5
    multi = dict(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True)
    sc = ray_scene(R, S)
    grid = grid_of("random", outside=1, seed=195, box=(-6.0, 6.0))

    def names(**reg):
        model = make_v2(N, "bf16", scene="solid", n_layers=2)[0]
        step = FusedStep(model, lr=1e-3, **multi, **reg)
        if route == "call":
            z = (NEAR + (FAR - NEAR) * (torch.arange(S) + 0.5) / S).expand(R, S).contiguous().cuda()
            pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * z[:, :, None]).reshape(-1, 3)
            dirs = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
            return record(lambda: step(pts, z, sc["d"], sc["tgt"], dirs=dirs, noise=sc["noise"]), monkeypatch)
        kw = {} if route == "rays" else dict(occupancy=grid, grid_inputs=route.split("-")[1])
        return record(lambda: step.step_rays(sc["o"], sc["d"], sc["tgt"], NEAR, FAR, S, perturb=True, seed=3, noise=sc["noise"], **kw), monkeypatch)

    base = names()
    got = names(dist_weight=1e-2, occ_weight=1e-2, occ_samples=2, dist_span=FAR - NEAR)
    loss = "nrf_composite_loss_backward_indexed" if route.startswith("grid") else "nrf_composite_loss_backward"
    assert base.count(loss) == 1 and base.count("nrf_adamw_step_loss") == 1 and "nrf_ray_terms_finish" not in base
    want = ["nrf_composite_reg_loss_backward" if n == loss else n for n in base]
    at = want.index("nrf_adamw_step_loss")
    want.insert(at + 1, "nrf_ray_terms_finish")
    print(route, got)
    assert got == want
