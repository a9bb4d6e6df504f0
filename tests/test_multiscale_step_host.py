"""Host-side checks of the multiscale trainer's step (no GPU): the new C ABI entry points and their ctypes declarations, the
refusals that answer before any launch, train_cli's recipe mapping, the build's resource figures of the new kernels, and the
committed fixture tests/golden/multiscale_step.npz against a torch-autograd replay through the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nrf_composite_loss_backward", "nrf_grad_sqnorm_workspace_bytes", "nrf_grad_sqnorm_partials", "nrf_adamw_step_loss")


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def test_header_and_ctypes_agree_on_the_new_struct_and_symbols(L):
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    lib = L.lib()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    body = re.search(r"typedef struct nrf_loss_opts \{(.*?)\} nrf_loss_opts;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert fields == [f for f, _ in L.nrf_loss_opts._fields_]
    assert C.sizeof(L.nrf_loss_opts) == 48 and L.nrf_loss_opts.target_depth.offset == 16 and L.nrf_loss_opts.rng_seed.offset == 40
    assert L.loss_opts().struct_bytes == 48
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(5) == -1 and lib.nrf_abi_sizeof(99) == -1
    # argument counts of the declarations
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]), name


def test_norm_workspace_size(L):
    lib = L.lib()
    for n, want in ((1, 4), (1024, 4), (1025, 8), (100003, 4 * 98), (1 << 20, 4096), (1 << 26, 4096)):
        assert lib.nrf_grad_sqnorm_workspace_bytes(n) == want, n
    assert lib.nrf_grad_sqnorm_workspace_bytes(0) == -1 and lib.nrf_last_error()


def test_new_entry_points_refuse_bad_arguments_before_any_launch(L):
    lib = L.lib()
    P = lambda a: C.c_void_p(a)
    ok = dict(rgb=P(0x1000), rs=4, sig=P(0x100C), ss=4, z=P(0x2000), d=P(0x3000), R=8, S=16, white=0, tgt=P(0x4000), pred=None,
              drgb=P(0x5000), drs=4, dsig=P(0x500C), dss=4, rl=P(0x6000), zb=None, zn=0)

    def call(lo, **kw):
        a = dict(ok, **kw)
        return lib.nrf_composite_loss_backward(a["rgb"], a["rs"], a["sig"], a["ss"], a["z"], a["d"], a["R"], a["S"], a["white"], a["tgt"],
                                               None if lo is None else C.byref(lo), a["pred"], a["drgb"], a["drs"], a["dsig"], a["dss"], a["rl"],
                                               a["zb"], a["zn"], None)
    assert call(None) == -1 and b"loss is NULL" in lib.nrf_last_error()
    wrong_size = L.loss_opts()
    wrong_size.struct_bytes = 40
    assert call(wrong_size) == -1 and b"struct_bytes" in lib.nrf_last_error()
    for kw in (dict(rgb_weight=-1.0), dict(reg_weight=-1e-3), dict(depth_weight=-0.5), dict(reg_weight=float("nan"))):
        assert call(L.loss_opts(**kw)) == -1 and b"weights" in lib.nrf_last_error(), kw
    assert call(L.loss_opts(noise_std=-0.1)) == -1 and b"noise_std" in lib.nrf_last_error()
    good = L.loss_opts(reg_weight=1e-4, noise_std=0.1)
    for bad in (dict(R=0), dict(R=-3), dict(S=0), dict(S=5000), dict(rs=2), dict(ss=0), dict(drs=1), dict(dss=0), dict(rgb=None), dict(sig=None),
                dict(z=None), dict(d=None), dict(tgt=None), dict(drgb=None), dict(dsig=None), dict(rl=None), dict(zn=-1), dict(zn=4)):
        assert call(good, **bad) == -1, bad
        assert lib.nrf_last_error()
    # norm partials: NULL / short / misaligned workspace
    assert lib.nrf_grad_sqnorm_partials(P(0x1000), 5000, None, 64, None) == -1 and b"workspace is NULL" in lib.nrf_last_error()
    assert lib.nrf_grad_sqnorm_partials(P(0x1000), 5000, P(0x2000), 16, None) == -1 and b"smaller" in lib.nrf_last_error()
    assert lib.nrf_grad_sqnorm_partials(P(0x1000), 5000, P(0x2002), 64, None) == -1 and b"aligned" in lib.nrf_last_error()
    assert lib.nrf_grad_sqnorm_partials(None, 5000, P(0x2000), 64, None) == -1
    assert lib.nrf_grad_sqnorm_partials(P(0x1000), 0, P(0x2000), 64, None) == -1

    def adamw(**kw):
        g = lambda k, dflt: kw.get(k, dflt)
        return lib.nrf_adamw_step_loss(g("p", P(0x1000)), g("g", P(0x2000)), g("m", P(0x3000)), g("v", P(0x4000)), g("n", 100), 1e-3, g("b1", 0.9), 0.999,
                                       1e-8, 0.0, g("step", 1), 1, g("max_norm", 1.0), g("parts", P(0x7000)), g("norm", None), g("rl", P(0x5000)),
                                       g("R", 8), g("S", 16), g("w", 1.0), 0.0, 0.0, g("loss", P(0x6000)), None)
    for bad in (dict(n=0), dict(step=0), dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(b1=1.0), dict(rl=None), dict(loss=None),
                dict(R=0), dict(S=0), dict(w=-1.0), dict(parts=None), dict(parts=None, max_norm=0.0, norm=P(0x8000)), dict(max_norm=float("nan"))):
        assert adamw(**bad) == -1, bad
        assert lib.nrf_last_error()
    assert adamw(parts=None) == -1 and b"max_norm > 0 needs" in lib.nrf_last_error()


def test_python_surface_checks_its_arguments():
    from nerf_few_shot_limitations_amd import training

    class Stub:
        net = 1
    with pytest.raises(ValueError, match="max_grad_norm"):
        training.Adam(Stub(), max_grad_norm=0.0)
    with pytest.raises(ValueError, match=">= 0"):
        training.FusedStep(Stub(), reg_weight=-1.0)
    s = training.FusedStep(Stub())                                     # today's arguments: nothing extended
    assert not s.opt.extended and s.last_losses is None and s.last_grad_norm is None
    assert training.FusedStep(Stub(), decoupled_weight_decay=True).opt.extended and training.FusedStep(Stub(), max_grad_norm=1.0).opt.extended


def test_train_cli_recipe_maps_the_yaml():
    from nerf_few_shot_limitations_amd import load_config, train_cli
    cfg = load_config(os.path.join(ROOT, "tests", "golden", "experiments", "multiscale.yaml"))
    plain = train_cli.step_options(cfg, "train")
    assert plain == dict(lr=2e-4, weight_decay=1e-6, rgb_weight=1.0)                       # what FusedStep was given before the recipe existed
    ms = train_cli.step_options(cfg, "multiscale")
    assert ms == dict(lr=2e-4, weight_decay=1e-6, rgb_weight=1.0, reg_weight=1e-4, depth_weight=0.1, noise_std=0.1, max_grad_norm=1.0,
                      decoupled_weight_decay=True)
    base = load_config(os.path.join(ROOT, "tests", "golden", "experiments", "baseline.yaml"))
    assert train_cli.step_options(base, "multiscale")["noise_std"] == float(base.get("rendering", {}).get("noise_std", 0.0))
    with pytest.raises(ValueError):
        train_cli.step_options(cfg, "other")
    with pytest.raises(SystemExit):
        train_cli.main(["--config", "x", "--data", "y", "--recipe", "other"])


def test_new_kernels_use_no_scratch():
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    res = B.kernel_resources()
    seen = 0
    for name, r in res.items():
        if any(t in name for t in ("composite_loss_backward_kernel", "adam_kernel", "grad_sqnorm_partials_kernel")):
            seen += 1
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
    assert seen == 5                       # the compositor/loss kernel and the optimiser in both instantiations, the norm partials


# ---------------------------------------------------------------------------------------------
# the committed fixture
# ---------------------------------------------------------------------------------------------
def _indices(numel, k=64):
    return np.arange(numel) if numel <= k else (np.arange(k) * numel) // k


def test_fixture_is_reproduced_by_autograd_through_the_oracle(golden):
    """The three captured steps of the reference's multiscale trainer, replayed with torch autograd through oracle.mlp_v3 /
    oracle.volume_render, the loss written out, clip_grad_norm_ and torch.optim.AdamW.  Bars (i) and (ii) of
    tests/test_gpu_multiscale_step.py (on the build machine the replay was bit-identical to the capture; another CPU's summation
    order is one more rounding, which the stored `cpu_spread` measures)."""
    g = golden("multiscale_step")
    noise_std, rgb_w, depth_w, reg_w, max_norm, lr, wd = (float(x) for x in g["hyper"])
    assert (noise_std, rgb_w, depth_w, reg_w, max_norm, lr, wd) == (0.1, 1.0, 0.1, 1e-4, 1.0, 2e-4, 1e-6)       # multiscale.yaml / train_multiscale.py
    R, S = g["z"].shape
    assert (R, S) == (64, 32)
    norms = g["step_norms"]
    assert list(g["step_clips"]) == [bool(n > max_norm) for n in norms] == [True, True, False]       # both branches are taken
    t = lambda k: torch.from_numpy(g[k])
    p0 = O.make_weights("v3", int(g["weight_seed"]), "solid", dino_dim=128)
    q = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    params = list(q.values())
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd)
    rd, dino = t("rays_d"), torch.from_numpy(g["dino_q"].astype(np.float32) / 128.0)
    dirs = rd[:, None, :].expand(R, S, 3).reshape(-1, 3)
    for i in range(3):
        col, den = O.mlp_v3(q, t("pos"), dirs, dino, 12, 4)
        rgb, depth, w = O.volume_render(col.view(R, S, 3), den.view(R, S, 1) + t("noise").view(R, S, 1) * noise_std, t("z"), rd)
        l_rgb, l_reg = torch.nn.functional.mse_loss(rgb, t("target")), torch.mean(w ** 2)
        total = rgb_w * l_rgb + reg_w * l_reg
        opt.zero_grad()
        total.backward()
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        opt.step()
        want = g["step_losses"][i]
        for got, ref in ((total.item(), want[0]), (l_rgb.item(), want[1]), (l_reg.item(), want[2]), (norm, norms[i])):
            assert abs(got - ref) <= 2e-4 * abs(ref), (i, got, ref)
    errs = []
    for k in p0:
        v = q[k].detach().reshape(-1)
        errs.append(np.abs(v.numpy()[_indices(v.numel())] - g["param_" + k]))
        assert abs(float(v.norm()) - float(g["pnorm_" + k])) <= 1e-5 * float(g["pnorm_" + k]) + 1e-6, k
    errs = np.concatenate(errs)
    spread = g["cpu_spread"]                   # the generator's conditioning measurement: a quarter of the bars at most
    assert spread.shape == (5,) and spread[:4].max() < 2e-4 / 4 and 0 < spread[4] < 2.5 * lr * 3
    assert errs.max() <= 4 * spread[4]
    # the compositor-level cases carry what they claim: opaque samples, sigma <= 0 with and without the noise, a depth term
    for S_ in (32, 64):
        k = f"c{S_}_"
        den, eff = g[k + "density"][..., 0], g[k + "density"][..., 0] + g[k + "noise"] * float(g[k + "noise_std"])
        assert g[k + "z"].shape == (48, S_) and (den >= 60).any() and (den <= 0).any() and ((den <= 0) & (eff > 0)).any() and ((den > 0) & (eff <= 0)).any()
        assert np.all(g[k + "d_density"][eff <= 0] == 0) and g[k + "losses"][2] > 0
        w_rgb, w_depth, w_reg = (float(x) for x in g[k + "weights"])
        tot, l_rgb, l_dep, l_reg = (float(x) for x in g[k + "losses"])
        assert abs(tot - (w_rgb * l_rgb + w_depth * l_dep + w_reg * l_reg)) <= 1e-6 * tot
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "multiscale_step.npz")) < 1 << 20
