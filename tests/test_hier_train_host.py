"""Host-side checks of the hierarchical training step (no GPU): the new struct and entries against their ctypes declarations, every
refusal of nrf_composite_hier_loss_backward answered before any launch, FusedStep's ValueErrors that are decided without a device,
train_cli's --n-importance / --coarse-weight refusals, and the new unit's resource figures -- built into a sub-directory of the
object directory with a census of its own (tests/golden/kernel_resources_hier_train.json), beside the closed one of the main directory."""
import ctypes as C
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "nrf_composite_hier_loss_backward"


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def test_header_and_ctypes_agree(L):
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    lib = L.lib()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in ((ENTRY, 5), ("nrf_hier_train_workspace_bytes", 3)):
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)
    body = re.search(r"typedef struct nrf_hier_loss \{(.*?)\} nrf_hier_loss;", code, re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    fields = [re.search(r"(\w+)\s*$", d).group(1) for d in decls]
    T = L.nrf_hier_loss
    assert fields == [f for f, _ in T._fields_]
    # every field's C type against its ctypes one
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    for d, (f, t) in zip(decls, T._fields_):
        ctype = d[: d.rindex(f)].strip()
        assert (t is C.c_void_p) if ctype.endswith("*") else (t is kinds[ctype]), (d, t)
    assert C.sizeof(T) == 200 and T.rgb_coarse.offset == 16 and T.w_coarse.offset == 80 and T.w_fine.offset == 84
    assert T.d_rgb_coarse.offset == 88 and T.zero_n.offset == 176 and T.workspace_bytes.offset == 192
    assert L.hier_loss().struct_bytes == 200
    with pytest.raises(TypeError):
        L.hier_loss(no_such_field=1)
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(5) == -1
    doc = " ".join(w for w in header[header.index("The hierarchical training step"):header.index(ENTRY + "(const")].split() if w != "*")
    for word in ("coarse depth goes in front of an equal new one", "equal new depths keep their order", "1e10 |d|", "No gradient reaches the depths",
                 "one fp32 addition", "no atomics", "n_rays == 0 is NRF_OK"):
        assert word in doc, word


def test_workspace_bytes(L):
    lib = L.lib()
    for bad in ((-1, 8, 8), (4, 0, 8), (4, 8, 0), (4, 4000, 97)):
        assert lib.nrf_hier_train_workspace_bytes(*bad) == -1, bad
    assert lib.nrf_hier_train_workspace_bytes(0, 8, 8) == 0
    for R, S, Ni in ((1, 1, 1), (5, 70, 61), (2048, 128, 64), (3, 4000, 96)):
        b = lib.nrf_hier_train_workspace_bytes(R, S, Ni)
        need = 4 * (10 * R * (S + Ni) + 5 * R)             # 40 B per sample: rows, d rows, depth, rank; 20 B per ray
        assert need <= b < need + 16 and b % 16 == 0, (R, S, Ni, b)


def test_refusals_before_any_launch(L):
    """Every refusal the header lists, with its message; nothing here owns device memory: a launch would fault."""
    lib = L.lib()
    R, S, Ni = 8, 16, 8
    ws_bytes = lib.nrf_hier_train_workspace_bytes(R, S, Ni)
    good = dict(white_bkgd=0, rgb_stride=3, sigma_stride=1, rgb_coarse=0x1000, sigma_coarse=0x2000, rgb_new=0x3000, sigma_new=0x4000,
                z_coarse=0x5000, z_new=0x6000, rays_d=0x7000, target=0x8000, w_coarse=1.0, w_fine=1.0, d_rgb_coarse=0x9000,
                d_sigma_coarse=0xA000, d_rgb_new=0xB000, d_sigma_new=0xC000, pred_coarse=0xD000, pred_fine=0xE000, ray_loss=0xF000,
                ray_parts=0x10000, z_union=0x11000, weights_fine=0x12000, zero_buf=None, zero_n=0, workspace=0x20000, workspace_bytes=ws_bytes)

    def call(a="good", n_rays=R, n_samples=S, n_importance=Ni, **kw):
        a = L.hier_loss(**{**good, **kw}) if a == "good" else a
        return lib.nrf_composite_hier_loss_backward(None if a is None else C.byref(a), n_rays, n_samples, n_importance, None)

    def refused(word, **kw):
        assert call(**kw) == -1, (word, kw)                                   # NRF_EINVAL
        assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())

    refused("a is NULL", a=None)
    short = L.hier_loss(**good)
    short.struct_bytes -= 8
    refused("struct_bytes", a=short)
    refused("n_rays < 0", n_rays=-1)
    refused("n_samples < 1", n_samples=0)
    refused("n_importance < 1", n_importance=0)
    refused("n_importance < 1", n_importance=-3)
    refused("> 4096", n_samples=4000, n_importance=97, workspace_bytes=1 << 40)
    refused("> 4096", n_samples=4096, n_importance=1, workspace_bytes=1 << 40)
    refused("bad strides", rgb_stride=2)
    refused("bad strides", sigma_stride=0)
    refused(">= 0", w_coarse=-0.5)
    refused(">= 0", w_fine=-1e-3)
    refused(">= 0", w_fine=float("nan"))
    refused(">= 0", w_coarse=float("inf"))
    for k in ("rgb_coarse", "sigma_coarse", "rgb_new", "sigma_new", "z_coarse", "z_new", "rays_d", "target", "d_rgb_coarse", "d_sigma_coarse",
              "d_rgb_new", "d_sigma_new"):
        refused("null pointer", **{k: None})
    refused("ray_loss is NULL", ray_loss=None)
    for k in ("rgb_coarse", "sigma_new", "z_coarse", "z_new", "rays_d", "target", "d_rgb_coarse", "d_sigma_new", "pred_coarse", "pred_fine", "ray_loss",
              "ray_parts", "z_union", "weights_fine"):
        refused("4-byte aligned", **{k: good[k] + 2})
    refused("4-byte aligned", zero_buf=0x30002, zero_n=4)
    refused("zero_buf is NULL", zero_n=5)
    refused("zero_buf is NULL", zero_buf=0x30000, zero_n=-1)
    refused("workspace is NULL", workspace=None)
    refused("16-byte aligned", workspace=0x20004)
    refused("workspace smaller", workspace_bytes=ws_bytes - 1)
    refused("workspace smaller", workspace_bytes=0)
    # the optional outputs may all be missing, the weights may be zero: with no rays that is NRF_OK and nothing is launched
    assert call(n_rays=0) == 0
    assert call(n_rays=0, pred_coarse=None, pred_fine=None, ray_parts=None, z_union=None, weights_fine=None, w_coarse=0.0, w_fine=0.0,
                workspace_bytes=0) == 0
    assert call(n_rays=0, n_samples=1, n_importance=1) == 0
    assert call(n_rays=0, n_samples=4000, n_importance=96) == 0
    assert call(n_rays=0, zero_buf=0x30000, zero_n=64) == 0


def _model():
    import nerf_few_shot_limitations_amd as N
    return N.NeRFMLP(pos_dim=63, hidden_dim=64, n_layers=2, mma_mode="f32")


def test_fused_step_refusals_need_no_device():
    from nerf_few_shot_limitations_amd.training import FusedStep
    for fn in (FusedStep.step_rays_hierarchical, FusedStep.step_view_hierarchical):
        p = inspect.signature(fn).parameters
        assert p["coarse_weight"].default == 1.0 and p["u"].default is None and p["perturb"].default is True
        assert list(p)[list(p).index("n_samples") + 1] == "n_importance"
        assert "no gradient reaches the depths" in " ".join(FusedStep.step_rays_hierarchical.__doc__.split()).lower()
    m = _model()
    rays = ([[0.0, 0.0, 4.0]], [[0.0, 0.0, -1.0]], [[0.5, 0.5, 0.5]])          # plain lists: nothing here may reach a device
    view = (None, None, 4, 4, 5.0, None)

    def both(step, word, S=16, Ni=8, **kw):
        with pytest.raises(ValueError, match=word):
            step.step_rays_hierarchical(*rays, 2.0, 6.0, S, Ni, **kw)
        with pytest.raises(ValueError, match=word):
            step.step_view_hierarchical(*view, 2.0, 6.0, S, Ni, **kw)

    for kw in (dict(reg_weight=1e-4), dict(depth_weight=0.1), dict(noise_std=0.5)):
        both(FusedStep(m, **kw), "reg_weight, depth_weight or noise_std")
    step = FusedStep(m, max_grad_norm=1.0, decoupled_weight_decay=True)          # these two keep working: they act behind the gradient
    both(step, "occupancy", occupancy=object())
    both(step, "d_dino_out", d_dino_out=object())
    both(step, "points_out", points_out=object())
    both(step, "n_importance must be >= 1", Ni=0)
    both(step, "n_importance must be >= 1", Ni=-4)
    both(step, "<= 4096", S=4000, Ni=97)
    both(step, "coarse_weight", coarse_weight=-0.25)
    both(step, "coarse_weight", coarse_weight=float("nan"))
    # the weights: w_fine = rgb_weight, w_coarse = rgb_weight * coarse_weight as ONE fp32 product
    import numpy as np
    step = FusedStep(m, rgb_weight=0.7)
    S, Ni, wc, wf = step._hier_check(16, 8, 0.35)
    assert (S, Ni) == (16, 8) and np.float32(wf) == np.float32(0.7) and np.float32(wc) == np.float32(0.7) * np.float32(0.35)
    assert step._hier_check(16, 8, 0.0)[2] == 0.0
    assert step.last_losses is None


_CFG = ("experiment: {{name: t}}\ndata: {{near: 2.0, far: 6.0, resolution: 16}}\nmodel: {{use_dino: {dino}}}\n"
        "nerf_model: {{pos_freq: 10, dir_freq: 4, hidden_dim: 256, num_layers: 8}}\n"
        "optimizer: {{lr: 1.0e-3, weight_decay: 0.0, lr_milestones: [2], lr_gamma: 0.5}}\n"
        "dino_model: {{name: facebook/dinov2-small, lora_rank: 4, lora_alpha: 8, use_lora: true}}\n")


@pytest.mark.parametrize("dino,flags,word", [
    ("false", ["--n-importance", "8", "--recipe", "multiscale"], "--recipe multiscale"),
    ("false", ["--n-importance", "8", "--occupancy-res", "64"], "--occupancy-"),
    ("false", ["--n-importance", "8", "--occupancy-box", "-1", "1"], "--occupancy-"),
    ("false", ["--n-importance", "8", "--occupancy-warmup", "4"], "--occupancy-"),
    ("true", ["--n-importance", "8", "--occupancy-res", "64", "--occupancy-per-view", "--dino-random-init"], "--occupancy-"),
    ("true", ["--n-importance", "8", "--train-extractor", "--dino-random-init"], "--train-extractor"),
    ("false", ["--n-importance", "-1"], "--n-importance must be >= 0"),
    ("false", ["--n-importance", "8", "--coarse-weight", "-0.5"], "--coarse-weight must be >= 0"),
    ("false", ["--coarse-weight", "0.5"], "--coarse-weight needs --n-importance"),
])
def test_train_cli_argument_refusals(tmp_path, dino, flags, word):
    from nerf_few_shot_limitations_amd import train_cli
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino=dino))
    with pytest.raises(SystemExit) as e:                         # decided before the data set is read or a device is touched
        train_cli.main(["--config", str(cfg), "--data", str(tmp_path / "nowhere"), *flags])
    assert word in str(e.value), e.value


def test_train_cli_carries_the_feature():
    import argparse
    from nerf_few_shot_limitations_amd import train_cli
    ok = argparse.Namespace(n_importance=8, coarse_weight=0.0, recipe="train", occupancy_res=0, train_extractor=False)
    assert train_cli.hierarchical_args_error(ok) is None
    assert train_cli.hierarchical_args_error(argparse.Namespace()) is None                   # neither flag: today's run
    p = inspect.signature(train_cli.train_epoch).parameters
    assert p["n_importance"].default == 0 and p["coarse_weight"].default == 1.0
    doc = " ".join(train_cli.__doc__.split())
    for word in ("--n-importance N", "--coarse-weight", "step_view_hierarchical", "evaluate_views(N_importance=N)", "implies the --fused-inputs route"):
        assert word in doc, word


# ---------------------------------------------------------------------------------------------
# the new unit's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from nerf_few_shot_limitations_amd import build as B
    sub = os.path.join(B.OBJ, B.HIER_TRAIN_DIR)
    if not os.path.isdir(sub) or not any(f.endswith(".o.remarks") for f in os.listdir(sub)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B


NEW = ("merge_gather_kernel", "scatter_add_kernel")


def test_new_kernels_match_their_census_and_spill_nothing(B):
    res = B.kernel_resources(os.path.join(B.OBJ, B.HIER_TRAIN_DIR))
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources_hier_train.json")))
    fields = gold["fields"]
    assert set(res) == set(gold["kernels"]) and len(res) == len(NEW), sorted(res)
    for kernel in NEW:
        (name, r), = [(k, v) for k, v in res.items() if "::" + kernel + "(" in k]
        print(kernel, r)
        assert r["tu"] == "hier_train"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["agprs"] == 0 and r.get("lds", 0) == 0 and r["occupancy"] >= 6, (name, r)
        assert [r.get(f, 0) for f in fields] == gold["kernels"][name], (name, dict(zip(fields, gold["kernels"][name])), r)


def test_the_sub_directory_stays_out_of_the_main_census(B):
    main = B.kernel_resources()
    assert not any(k.startswith("hier_train:") or any(n in k for n in NEW) for k in main), [k for k in main if "hier_train" in k]
    assert all(len(item) == 3 for item in B.SOURCES) and not any(src == "hier_train.hip" for src, _, _ in B.SOURCES)
    assert [(src, name, sub) for src, name, _, sub in B.SUBDIR_SOURCES] == [("hier_train.hip", "hier_train", B.HIER_TRAIN_DIR)]
    # the object is part of the library: the entry that launches the unit's kernels is exported
    from nerf_few_shot_limitations_amd import _lib
    assert hasattr(_lib.lib(), ENTRY)
