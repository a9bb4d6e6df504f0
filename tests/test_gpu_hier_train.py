"""The hierarchical training step (include/nerfhip.h: nrf_composite_hier_loss_backward; FusedStep.step_rays_hierarchical /
step_view_hierarchical; train_cli --n-importance) against code the library had before it:

  G1  the entry against nrf_composite_mse_backward / nrf_composite on the coarse rows and on the union gathered by a stable sort on
      the host, bit for bit, on hand-made rows;
  G2  the step's links at step 1: the new depths are sample_pdf_sorted's on the step's own depths and weights, the weights and the
      coarse image are those of render_rays in train() mode;
  G3  the step's gradient against the sum of two plain FusedStep.step_rays steps (the coarse ladder, and the union through z_in);
  G4  it trains, and the pixel-id form equals the ray form on the gathered rays;
  G5  train_cli --n-importance runs, checkpoints and validates through the hierarchical evaluator.

The resampling is re-derived nowhere but in G2: every other test takes `last_z_new` from the step (on the synthetic fields the
smallest pdf step sits on the resampler's `denom < 1e-5` guard, where one ulp of a weight moves a sample by a bin)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_train_rays import NEAR, FAR, _v3_scene, ray_batch, u01
from tests.test_gpu_training import _CFG, _write_scene, cosine, make_model, make_v2, make_v3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


# ---------------------------------------------------------------------------------------------
# G1. the entry against the parent's kernels
# ---------------------------------------------------------------------------------------------
def _rows(buf, n, v1):
    """(rgb (n,3) view, sigma (n) view, the compositor's (ptr, stride, ptr, stride)) of an (n,4) buffer in the layout _heads builds."""
    from nerf_few_shot_limitations_amd.training import _addr, _heads
    a, b, args = _heads(buf, n, v1)
    rgb, sigma = (a[:, :3], a[:, 3]) if v1 else (a, b[:, 0])
    return rgb, sigma, (args[0], args[1], _addr(args[2]), args[3])


def _mse_backward(rgb, sigma, z, d, tgt, white, weight):
    """nrf_composite_mse_backward on contiguous rgb (R,S,3) / sigma (R,S): pred, d_rgb, d_sigma, the rays' squared errors."""
    from nerf_few_shot_limitations_amd import _lib as L
    R, S = z.shape
    rgb, sigma = rgb.contiguous(), sigma.contiguous()
    pred, d_rgb, d_sigma, se = torch.empty((R, 3), device="cuda"), torch.empty_like(rgb), torch.empty_like(sigma), torch.empty((R,), device="cuda")
    L.check(L.lib().nrf_composite_mse_backward(L.ptr(rgb), 3, L.ptr(sigma), 1, L.ptr(z), L.ptr(d), R, S, white, L.ptr(tgt), weight, L.ptr(pred),
                                               L.ptr(d_rgb), 3, L.ptr(d_sigma), 1, L.ptr(se), None, 0, L.stream_ptr()))
    return pred, d_rgb, d_sigma, se


def _weights(rgb, sigma, z, d, white):
    from nerf_few_shot_limitations_amd import _lib as L
    R, S = z.shape
    rgb, sigma = rgb.contiguous(), sigma.contiguous()
    out, w = torch.empty((R, 3), device="cuda"), torch.empty((R, S), device="cuda")
    L.check(L.lib().nrf_composite(L.ptr(rgb), 3, L.ptr(sigma), 1, L.ptr(z), L.ptr(d), R, S, white, L.ptr(out), None, L.ptr(w), L.stream_ptr()))
    return w


@pytest.fixture(scope="module")
def g1_inputs(N):
    """Per (S, Ni): hand-made rows, depths and the yardstick's union, computed once and left unchanged."""
    from nerf_few_shot_limitations_amd.ray_sampler import sample_pdf_sorted
    out = {}
    R = 5                                               # more rays than a workgroup has waves: the ray loops stride
    for S, Ni in ((3, 1), (64, 64), (70, 61)):
        seed = 1000 + S
        rgb_c, rgb_n = u01(seed, R, S, 3).cuda(), u01(seed + 1, R, Ni, 3).cuda()
        sig_c, sig_n = (u01(seed + 2, R, S) * 3 - 0.5).cuda(), (u01(seed + 3, R, Ni) * 3 - 0.5).cuda()       # some densities <= 0
        sig_c[1, S // 2] = 1e6                                   # an opaque coarse sample mid-ray: the 1e-10 divisor
        sig_c[2], sig_n[2] = -sig_c[2].abs(), -sig_n[2].abs()      # a ray whose densities are all <= 0
        z_c = torch.sort(u01(seed + 4, R, S) * 4 + 2, dim=-1).values.cuda().contiguous()
        _, d = ray_batch(R, seed=seed + 5)
        tgt = u01(seed + 8, R, 3).cuda()
        z_n = sample_pdf_sorted(z_c, _weights(rgb_c, sig_c, z_c, d, 0), Ni).clone()      # the shared linspace row: ties with coarse depths
        if Ni >= 3:                                              # ray 0: two equal new depths, and a new depth equal to an interior coarse one
            z_n[0, 1] = z_n[0, 0]
            z_n[0, Ni // 2] = z_c[0, S // 2]
            z_n[0] = torch.sort(z_n[0]).values
        assert bool((z_n[:, 1:] >= z_n[:, :-1]).all())
        ties = int((z_n[:, :, None] == z_c[:, None, :]).any(-1).sum())
        zu, idx = torch.sort(torch.cat([z_c, z_n], 1), dim=1, stable=True)               # a stable sort of the concatenation IS the merge rule
        g_rgb = torch.gather(torch.cat([rgb_c, rgb_n], 1), 1, idx[..., None].expand(-1, -1, 3)).contiguous()
        g_sig = torch.gather(torch.cat([sig_c, sig_n], 1), 1, idx).contiguous()
        out[(S, Ni)] = dict(R=R, rgb_c=rgb_c, rgb_n=rgb_n, sig_c=sig_c, sig_n=sig_n, z_c=z_c, z_n=z_n.contiguous(), d=d, tgt=tgt, zu=zu.contiguous(),
                            idx=idx, g_rgb=g_rgb, g_sig=g_sig, ties=ties)
    torch.cuda.synchronize()
    return out


def _run_entry(c, S, Ni, v1, white, wc, wf, zero=None):
    from nerf_few_shot_limitations_amd import _lib as L
    R, M = c["R"], S + Ni
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    bufs = {k: f(R * n, 4) for k, n in (("c", S), ("n", Ni), ("dc", S), ("dn", Ni))}
    views = {k: _rows(b, b.shape[0], v1) for k, b in bufs.items()}
    for k, rgb, sig in (("c", c["rgb_c"], c["sig_c"]), ("n", c["rgb_n"], c["sig_n"])):
        views[k][0].copy_(rgb.reshape(-1, 3))
        views[k][1].copy_(sig.reshape(-1))
    o = dict(pred_c=f(R, 3), pred_f=f(R, 3), ray_loss=f(R), parts=f(2, R), zu=f(R, M), w=f(R, M))
    ws = torch.empty(L.lib().nrf_hier_train_workspace_bytes(R, S, Ni) // 4 + 16, device="cuda")
    ws[-16:] = -777.25
    (rc, rs_, sc, ss), (rn, _, sn, _), (drc, _, dsc, _), (drn, _, dsn, _) = (views[k][2] for k in ("c", "n", "dc", "dn"))
    a = L.hier_loss(white_bkgd=white, rgb_stride=rs_, sigma_stride=ss, rgb_coarse=rc, sigma_coarse=sc, rgb_new=rn, sigma_new=sn,
                    z_coarse=L.ptr(c["z_c"]), z_new=L.ptr(c["z_n"]), rays_d=L.ptr(c["d"]), target=L.ptr(c["tgt"]), w_coarse=wc, w_fine=wf,
                    d_rgb_coarse=drc, d_sigma_coarse=dsc, d_rgb_new=drn, d_sigma_new=dsn, pred_coarse=L.ptr(o["pred_c"]), pred_fine=L.ptr(o["pred_f"]),
                    ray_loss=L.ptr(o["ray_loss"]), ray_parts=L.ptr(o["parts"]), z_union=L.ptr(o["zu"]), weights_fine=L.ptr(o["w"]),
                    zero_buf=L.ptr(zero), zero_n=0 if zero is None else zero.numel(), workspace=ws.data_ptr(), workspace_bytes=(ws.numel() - 16) * 4)
    L.check(L.lib().nrf_composite_hier_loss_backward(C.byref(a), R, S, Ni, L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((ws[-16:] == -777.25).all()), "the entry wrote behind its workspace"
    o.update(d_rgb_c=views["dc"][0].reshape(R, S, 3).clone(), d_sig_c=views["dc"][1].reshape(R, S).clone(),
             d_rgb_n=views["dn"][0].reshape(R, Ni, 3).clone(), d_sig_n=views["dn"][1].reshape(R, Ni).clone())
    return o


@pytest.mark.parametrize("wc,wf", [(1.0, 1.0), (0.0, 1.0), (0.35, 0.7)])
@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("layout", ["v1", "v2"])
@pytest.mark.parametrize("S,Ni", [(3, 1), (64, 64), (70, 61)])
def test_entry_equals_the_parents_kernels_on_the_gathered_union(N, g1_inputs, S, Ni, layout, white, wc, wf):
    c = g1_inputs[(S, Ni)]
    R = c["R"]
    if Ni >= 3:
        assert c["ties"] >= 1 and bool((c["z_n"][0, 1:] == c["z_n"][0, :-1]).any()), c["ties"]      # the planted ties are there
    # the yardstick: the parent's loss kernel on the coarse rows, and on the rows gathered in the stable-sort order
    pred_c, d_rgb_c, d_sig_c, se_c = _mse_backward(c["rgb_c"], c["sig_c"], c["z_c"], c["d"], c["tgt"], white, wc)
    pred_f, dg_rgb, dg_sig, se_f = _mse_backward(c["g_rgb"], c["g_sig"], c["zu"], c["d"], c["tgt"], white, wf)
    w_f = _weights(c["g_rgb"], c["g_sig"], c["zu"], c["d"], white)
    back_rgb = torch.zeros_like(dg_rgb).scatter_(1, c["idx"][..., None].expand(-1, -1, 3), dg_rgb)       # d rows back to [coarse | new] order
    back_sig = torch.zeros_like(dg_sig).scatter_(1, c["idx"], dg_sig)
    wc32, wf32 = torch.tensor(wc, dtype=torch.float32, device="cuda"), torch.tensor(wf, dtype=torch.float32, device="cuda")
    want = dict(pred_c=pred_c, pred_f=pred_f, parts=torch.stack([se_c, se_f]), ray_loss=wc32 * se_c + wf32 * se_f, zu=c["zu"], w=w_f,
                d_rgb_c=d_rgb_c + back_rgb[:, :S], d_sig_c=d_sig_c + back_sig[:, :S], d_rgb_n=back_rgb[:, S:], d_sig_n=back_sig[:, S:])
    zero = torch.ones(1000, device="cuda")
    got = _run_entry(c, S, Ni, layout == "v1", white, wc, wf, zero)
    for k, v in want.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(got[k], v), (k, float((got[k] - v).abs().max()))
    assert float(zero.abs().max()) == 0.0                # the clearing side job
    assert float(got["d_sig_c"][2].abs().max()) == 0.0 and float(got["d_sig_n"][2].abs().max()) == 0.0     # densities <= 0: masked
    assert float(want["d_rgb_n"].abs().max()) > 0 and float(se_f.min()) > 0
    again = _run_entry(c, S, Ni, layout == "v1", white, wc, wf)
    for k in want:
        assert torch.equal(again[k], got[k]), k          # two runs, the same bits


# ---------------------------------------------------------------------------------------------
# G2 / G3. the step at step 1
# ---------------------------------------------------------------------------------------------
R2, S2, NI2 = 67, 16, 9
NETS = [("v2", "f32"), ("v2", "bf16"), ("v1", "f32"), ("v3", "f32")]


def _make(N, net, mode):
    return {"v1": make_model, "v2": make_v2, "v3": make_v3}[net](N, mode, scene="solid")[0]


def _scene(net):
    if net == "v3":
        o, d, cam = _v3_scene(64, R2, S2)
    else:
        (o, d), cam = ray_batch(R2, seed=300), None
    return o, d, cam, u01(301, R2, 3).cuda(), u01(302, R2, S2).cuda(), u01(303, R2, NI2).cuda()


def _hier(N, net, mode, coarse_weight=1.0, rgb_weight=1.0, **step_kw):
    """One hierarchical step of a fresh model on the fixed scene: (step object, its loss, the scene)."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    o, d, cam, tgt, tr, u = sc = _scene(net)
    step = FusedStep(_make(N, net, mode), lr=5e-4, rgb_weight=rgb_weight, **step_kw)
    loss = step.step_rays_hierarchical(o, d, tgt, NEAR, FAR, S2, NI2, t_rand=tr, u=u, dino=cam, coarse_weight=coarse_weight)
    return step, loss, sc


@pytest.mark.parametrize("net,mode", NETS)
def test_links_of_the_step(N, net, mode):
    from nerf_few_shot_limitations_amd.ray_sampler import sample_pdf_sorted
    o, d, cam, tgt, tr, u = _scene(net)
    ref = None
    if net == "v2":                                      # the ray route's V2 is the staged chain bit for bit: render_rays in train() mode under grad
        ref = N.render_rays(_make(N, net, mode), o, d, NEAR, FAR, S2, perturb=True, t_rand=tr)
        assert ref["rgb"].grad_fn is not None
    step, loss, _ = _hier(N, net, mode)
    assert step.last_z.shape == (R2, S2) and step.last_weights.shape == (R2, S2) and step.last_z_new.shape == (R2, NI2)
    assert step.pred.shape == step.pred_coarse.shape == (R2, 3)
    assert torch.equal(step.last_z_new, sample_pdf_sorted(step.last_z, step.last_weights, NI2, u=u))
    assert bool((step.last_z_new[:, 1:] >= step.last_z_new[:, :-1]).all())
    if ref is not None:
        assert torch.equal(step.last_weights, ref["weights"].detach())
        assert torch.equal(step.pred_coarse, ref["rgb"].detach())
    ls = step.last_losses
    assert set(ls) == {"total", "coarse", "fine"} and torch.equal(ls["total"], loss)
    mse = lambda p: float(((p - tgt) ** 2).mean())
    assert float(ls["coarse"]) == pytest.approx(mse(step.pred_coarse), rel=1e-5) and float(ls["fine"]) == pytest.approx(mse(step.pred), rel=1e-5)
    assert float(loss) == pytest.approx(float(ls["coarse"]) + float(ls["fine"]), rel=1e-5)


def _yardstick(N, net, mode, step, sc, w_coarse, w_fine):
    """(g_ref, loss_ref): two plain steps of the parent on model copies -- the ladder at w_coarse, the union (z_in) at w_fine."""
    from nerf_few_shot_limitations_amd.training import FusedStep
    o, d, cam, tgt, tr, u = sc
    union = torch.sort(torch.cat([step.last_z, step.last_z_new], 1), dim=1, stable=True).values.contiguous()
    g, loss = 0.0, 0.0
    if w_coarse is not None:
        a1 = FusedStep(_make(N, net, mode), lr=5e-4, rgb_weight=w_coarse)
        loss = loss + a1.step_rays(o, d, tgt, NEAR, FAR, S2, t_rand=tr, dino=cam)
        g = g + a1.grad
    a2 = FusedStep(_make(N, net, mode), lr=5e-4, rgb_weight=w_fine)
    loss = loss + a2.step_rays(o, d, tgt, NEAR, FAR, S2 + NI2, perturb=False, z_in=union, dino=cam)
    return g + a2.grad, loss


def _compare(step, loss, g_ref, loss_ref, mode):
    fp = step.model.flat_params()
    got, want = fp.views(step.grad), fp.views(g_ref)
    rel_loss = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
    big = float(g_ref.abs().max())
    worst = max(float((a - b).abs().max()) / big for a, b in zip(got, want))
    cos = min(cosine(a, b) for a, b in zip(got, want) if a.dim() == 2)
    print(f"{mode}: loss {float(loss):.6g} vs {float(loss_ref):.6g} (rel {rel_loss:.2e}); worst gradient error {worst:.2e} of the largest element; "
          f"smallest weight-tensor cosine {cos:.5f}")
    assert big > 0 and np.isfinite(float(loss))
    if mode == "f32":
        assert rel_loss < 1e-5 and worst < 2e-4, (rel_loss, worst)
    else:
        assert rel_loss < 2e-3 and cos >= 0.97, (rel_loss, cos)


@pytest.mark.parametrize("net,mode", NETS)
def test_gradient_equals_two_plain_steps(N, net, mode):
    """f32: loss within 1e-5 relative, every parameter tensor within 2e-4 of the yardstick's largest element -- the project's bounds
    for the same kernels in another summation order (tests/test_gpu_training.py, tests/test_gpu_train_rays.py): the coarse rows go
    through one dZ chain with the summed d rows instead of two.  bf16: loss within 2e-3, every weight tensor's cosine >= 0.97 (the
    16-bit chain rounds the summed d rows once where the yardstick rounds two)."""
    wc = 0.35
    step, loss, sc = _hier(N, net, mode, coarse_weight=wc, rgb_weight=0.7)
    w_coarse = float(np.float32(0.7) * np.float32(wc))
    g_ref, loss_ref = _yardstick(N, net, mode, step, sc, w_coarse, 0.7)
    _compare(step, loss, g_ref, loss_ref, mode)


def test_coarse_weight_zero_is_the_fine_step_alone(N):
    step, loss, sc = _hier(N, "v2", "f32", coarse_weight=0.0)
    g_ref, loss_ref = _yardstick(N, "v2", "f32", step, sc, None, 1.0)
    _compare(step, loss, g_ref, loss_ref, "f32")
    assert float(step.last_losses["coarse"]) > 0          # the coarse image is still rendered and scored, it just carries no weight


def test_clipping_acts_behind_the_gradient(N):
    step, loss, sc = _hier(N, "v2", "f32", max_grad_norm=1.0, decoupled_weight_decay=True, weight_decay=1e-2)
    norm = float(step.grad.norm())
    assert norm > 0 and float(step.last_grad_norm) == pytest.approx(norm, rel=1e-5)
    plain, loss_p, _ = _hier(N, "v2", "f32")
    assert torch.equal(plain.grad, step.grad) and float(loss) == pytest.approx(float(loss_p), rel=1e-6)
    assert set(step.last_losses) == {"total", "coarse", "fine"} and torch.equal(step.last_losses["total"], loss)
    assert not torch.equal(plain.model.flat_params().flat, step.model.flat_params().flat)


# ---------------------------------------------------------------------------------------------
# G4. it trains; pixel ids equal gathered rays
# ---------------------------------------------------------------------------------------------
def test_six_steps_on_a_fixed_batch_reduce_the_loss(N):
    from nerf_few_shot_limitations_amd.training import FusedStep
    R, S, Ni = 160, 16, 16
    o, d = ray_batch(R, seed=400)
    tgt = (0.6 + 0.4 * u01(401, R, 3)).cuda()
    step = FusedStep(make_v2(N, "bf16", scene="solid")[0], lr=5e-4)
    losses = [float(step.step_rays_hierarchical(o, d, tgt, NEAR, FAR, S, Ni, perturb=False)) for _ in range(6)]
    print("hierarchical bf16 losses:", losses)
    assert all(np.isfinite(l) for l in losses) and losses[-1] < losses[0]


def test_step_view_equals_step_rays_on_the_gathered_rays(N):
    from nerf_few_shot_limitations_amd.training import FusedStep
    sa = FusedStep(make_v2(N, "bf16", scene="solid")[0], lr=5e-4)
    sb = FusedStep(make_v2(N, "bf16", scene="solid")[0], lr=5e-4)
    H, W, R, S, Ni = 24, 24, 200, 16, 8
    focal = O.focal_for(W)
    pose = torch.from_numpy(O.LEGO_LIKE_C2W)
    image = u01(90, H, W, 3).cuda()
    ro, rd = N.get_rays(H, W, focal, pose)
    for i in range(3):
        pix = torch.randperm(H * W, generator=torch.Generator().manual_seed(i))[:R].cuda()
        u = u01(500 + i, R, Ni).cuda()
        la = sa.step_rays_hierarchical(ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix], image.reshape(-1, 3)[pix], NEAR, FAR, S, Ni, seed=5 + i, u=u)
        lb = sb.step_view_hierarchical(image, pose, H, W, focal, pix, NEAR, FAR, S, Ni, seed=5 + i, u=u)
        assert torch.equal(la, lb) and torch.equal(sa.last_z, sb.last_z) and torch.equal(sa.last_z_new, sb.last_z_new)
    assert torch.equal(sa.model.flat_params().flat, sb.model.flat_params().flat)
    # a plain step on the same object afterwards takes its own buffers again
    lp = sa.step_rays(ro.reshape(-1, 3)[pix], rd.reshape(-1, 3)[pix], image.reshape(-1, 3)[pix], NEAR, FAR, S + 3, seed=1)
    assert sa.last_z.shape == (R, S + 3) and np.isfinite(float(lp)) and set(sa.last_losses) == {"total"}


# ---------------------------------------------------------------------------------------------
# G5. train_cli
# ---------------------------------------------------------------------------------------------
def test_train_cli_trains_and_validates_hierarchically(N, tmp_path, monkeypatch):
    from nerf_few_shot_limitations_amd import train_cli
    asked, real = [], train_cli.evaluate_views
    monkeypatch.setattr(train_cli, "evaluate_views", lambda *a, **kw: (asked.append(kw.get("N_importance")), real(*a, **kw))[1])
    root = str(tmp_path / "scene")
    _write_scene(root)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino="false", pf=10))
    out = str(tmp_path / "run")
    p = dict(O.make_weights("v2", 1, "fog"))
    p["pos_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 9, 10)
    p["dir_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 3, 4)
    torch.save({"epoch": 0, "nerf_model_state_dict": p}, str(tmp_path / "init.pth"))
    log = train_cli.main(["--config", str(cfg), "--data", root, "--out", out, "--mode", "f32", "--epochs", "2", "--checkpoint", str(tmp_path / "init.pth"),
                          "--n-importance", "8", "--coarse-weight", "0.5", "--max-batches", "2"])
    assert [r["epoch"] for r in log] == [1, 2] and all(np.isfinite(r["loss"]) for r in log)
    assert "psnr" in log[1] and np.isfinite(log[1]["psnr"])                     # val_freq 2: validated through evaluate_views(N_importance=8)
    files = sorted(os.listdir(out))
    assert "best_tiny.pth" in files and "train_log.json" in files and "val_2" in files
    ck = torch.load(os.path.join(out, "best_tiny.pth"), map_location="cpu", weights_only=True)
    moved = max(float((ck["nerf_model_state_dict"][k] - p[k]).abs().max()) for k in p if k.endswith("weight"))
    assert moved > 1e-5
    assert asked == [8]                                  # one validation, through evaluate_views(N_importance=8)
