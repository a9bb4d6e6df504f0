"""Host-side checks of training under an occupancy grid (no GPU): the two new structs and three entry points against their ctypes
declarations, every refusal that answers before any launch, train_cli's --occupancy-* argument checks, and the build's resource
figures -- the new kernels use no scratch and spill nothing, and every kernel the library had before keeps its figures
(tests/golden/kernel_resources.json: the parent build's remarks)."""
import ctypes as C
import inspect
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda a: a


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def _opts(L, **kw):
    o = L.nrf_render_opts()
    o.near, o.far, o.n_samples, o.mma_mode = 2.0, 6.0, 16, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_header_and_ctypes_agree(L):
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    lib = L.lib()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("nrf_occupancy_compact_workspace_bytes", 1), ("nrf_occupancy_compact_rays", 6), ("nrf_composite_loss_backward_indexed", 21)):
        decl = re.search(r"\b" + name + r"\s*\((.*?)\);", code, re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name)
    # the indexed entry is nrf_composite_loss_backward's argument list with `slot` behind `loss`
    plain = [a.strip() for a in re.search(r"\bnrf_composite_loss_backward\s*\((.*?)\);", code, re.S).group(1).split(",")]
    idx = [a.strip() for a in re.search(r"\bnrf_composite_loss_backward_indexed\s*\((.*?)\);", code, re.S).group(1).split(",")]
    k = idx.index("const int32_t* slot")
    assert idx[:k] + idx[k + 1:] == plain and idx[k - 1] == "const nrf_loss_opts* loss"
    body = re.search(r"typedef struct nrf_compact \{(.*?)\} nrf_compact;", code, re.S).group(1)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f for f, _ in L.nrf_compact._fields_]
    assert fields == ["struct_bytes", "reserved", "capacity", "index", "slot", "positions", "directions", "count", "workspace", "workspace_bytes"]
    T = L.nrf_compact
    assert C.sizeof(T) == 72 and T.capacity.offset == 8 and T.index.offset == 16 and T.count.offset == 48 and T.workspace_bytes.offset == 64
    assert L.compact().struct_bytes == 72
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(5) == -1
    # the semantics are written down next to the declarations
    doc = header[header.index("Training under an occupancy grid"):header.index("nrf_composite_loss_backward_indexed(")]
    for word in ("-inf", "behind the density noise", "strictly ascending", "counter_uniform(rng_seed, r, s)", "no workgroup waits", "next ladder sample"):
        assert word in doc, word


def test_workspace_bytes(L):
    lib = L.lib()
    assert lib.nrf_occupancy_compact_workspace_bytes(-1) == -1
    assert lib.nrf_occupancy_compact_workspace_bytes(0) == 16
    for n in (1, 4, 5, 37, 2048, 1 << 20):
        b = lib.nrf_occupancy_compact_workspace_bytes(n)
        assert b >= 4 * n and b % 16 == 0 and b < 4 * n + 16, n


def test_compaction_refusals_before_any_launch(L):
    """Every refusal the header lists, with its message; nothing here owns device memory: a launch would fault."""
    lib = L.lib()
    R, S = 8, 16
    good_rays = dict(rays_o=P(0x1000), rays_d=P(0x2000), z_vals=P(0x3000))
    pix = dict(pixels=P(0x1000), H=8, W=8, focal=10.0, c2w=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], z_vals=P(0x3000), rays_d_out=P(0x4000))
    good_occ = dict(bits=0x9000, res=(32, 8, 8), lo=(-1.0, -1.0, -1.0), scale=(16.0, 4.0, 4.0))
    good_out = dict(capacity=R * S, index=0x10000, slot=0x20000, positions=0x30000, directions=0x40000, count=0x50000, workspace=0x60000,
                    workspace_bytes=lib.nrf_occupancy_compact_workspace_bytes(R))

    def call(rays=good_rays, opts=None, occ=good_occ, out=good_out, n_rays=R, **opt_kw):
        rays = rays if rays is None or isinstance(rays, L.nrf_train_rays) else L.train_rays(**rays)
        occ = occ if occ is None or isinstance(occ, L.nrf_occupancy) else L.occupancy(**occ)
        out = out if out is None or isinstance(out, L.nrf_compact) else L.compact(**out)
        opts = _opts(L, **opt_kw) if opts is None else opts
        ref = lambda s: None if s is None else C.byref(s)
        return lib.nrf_occupancy_compact_rays(ref(rays), n_rays, ref(opts) if opts != "null" else None, ref(occ), ref(out), None)

    def refused(word, **kw):
        assert call(**kw) == -1, (word, kw)                                   # NRF_EINVAL
        assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())

    # the structs
    refused("rays is NULL", rays=None)
    short = L.train_rays(**good_rays)
    short.struct_bytes = 112
    refused("nrf_train_rays: struct_bytes", rays=short)
    refused("opts is NULL", opts="null")
    refused("occ is NULL", occ=None)
    wrong = L.occupancy(**good_occ)
    wrong.struct_bytes -= 8
    refused("nrf_occupancy: struct_bytes", occ=wrong)
    refused("out is NULL", out=None)
    wrong = L.compact(**good_out)
    wrong.struct_bytes += 8
    refused("nrf_compact: struct_bytes", out=wrong)
    # the ray source and the options, as nrf_mlp_forward_train_rays reads them
    refused("n_rays < 0", n_rays=-1)
    refused("ert_eps", ert_eps=0.01)
    refused("n_samples", n_samples=0)
    refused("not both and not neither", rays=dict(z_vals=P(0x3000)))
    refused("not both and not neither", rays={**good_rays, "pixels": P(0x8000)})
    refused("come together", rays=dict(rays_o=P(0x1000), z_vals=P(0x3000)))
    refused("camera", rays={**pix, "focal": 0.0})
    # a missing required output
    refused("z_vals is required", rays=dict(rays_o=P(0x1000), rays_d=P(0x2000)))
    refused("rays_d_out is required", rays={**pix, "rays_d_out": None})
    for k in ("index", "slot", "positions", "count"):
        refused("are required", out={**good_out, k: None})
    assert call(out={**good_out, "directions": None}, n_rays=0) == 0          # directions may be NULL (V1)
    # sizes
    refused("capacity", out={**good_out, "capacity": R * S - 1})
    refused("too large", n_rays=1 << 20, n_samples=4096, out={**good_out, "capacity": 1 << 40, "workspace_bytes": 1 << 30})
    assert call(n_rays=(1 << 31) // 16 - 1, out={**good_out, "capacity": 1 << 31, "workspace_bytes": 1 << 30, "index": None}) == -1
    assert b"are required" in lib.nrf_last_error()                            # R * S = 2^31 - 16 passes the size check
    # alignment
    for k in ("index", "slot", "positions", "directions", "workspace"):
        refused("4-byte aligned", out={**good_out, k: good_out[k] + 2})
    refused("4-byte aligned", rays={**good_rays, "z_vals": 0x3002})
    refused("8-byte aligned", out={**good_out, "count": 0x50004})
    # the workspace
    refused("workspace is NULL", out={**good_out, "workspace": None})
    refused("workspace smaller", out={**good_out, "workspace_bytes": good_out["workspace_bytes"] - 1})
    refused("workspace smaller", out={**good_out, "workspace_bytes": 0})
    # every condition nrf_occupancy already refuses
    refused("outside must be", occ={**good_occ, "outside": 2})
    refused("bits is NULL", occ={**good_occ, "bits": None})
    refused("bits is NULL or not 4-byte aligned", occ={**good_occ, "bits": 0x9002})
    refused("res must be in 1..512", occ={**good_occ, "res": (32, 0, 8)})
    refused("res must be in 1..512", occ={**good_occ, "res": (32, 8, 513)})
    refused("multiple of 32", occ={**good_occ, "res": (48, 8, 8)})
    refused("lo must be finite", occ={**good_occ, "lo": (float("nan"), 0.0, 0.0)})
    refused("scale must be finite and > 0", occ={**good_occ, "scale": (0.0, 1.0, 1.0)})
    refused("scale must be finite and > 0", occ={**good_occ, "scale": (1.0, float("inf"), 1.0)})
    # n_rays == 0 is NRF_OK and launches nothing, in both modes
    assert call(n_rays=0) == 0
    assert call(rays=pix, n_rays=0) == 0
    assert call(n_rays=0, out={**good_out, "capacity": 0, "workspace_bytes": 16}) == 0


def test_indexed_compositor_refusals_before_any_launch(L):
    lib = L.lib()
    lo = L.loss_opts()
    good = dict(rgb=0x1000, rs=3, sigma=0x2000, ss=1, z=0x3000, d=0x4000, R=8, S=16, white=0, tgt=0x5000, loss=lo, slot=0x6000, pred=0x7000,
                d_rgb=0x8000, drs=3, d_sigma=0x9000, dss=1, terms=0xA000, zero=None, zero_n=0)

    def call(**kw):
        a = {**good, **kw}
        return lib.nrf_composite_loss_backward_indexed(a["rgb"], a["rs"], a["sigma"], a["ss"], a["z"], a["d"], a["R"], a["S"], a["white"], a["tgt"],
                                                       None if a["loss"] is None else C.byref(a["loss"]), a["slot"], a["pred"], a["d_rgb"],
                                                       a["drs"], a["d_sigma"], a["dss"], a["terms"], a["zero"], a["zero_n"], None)

    def refused(word, **kw):
        assert call(**kw) == -1, (word, kw)
        assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())

    refused("slot is NULL", slot=None)
    refused("slot must be 4-byte aligned", slot=0x6002)
    refused("loss is NULL", loss=None)
    bad = L.loss_opts()
    bad.struct_bytes -= 4
    refused("struct_bytes", loss=bad)
    refused("noise_std", loss=L.loss_opts(noise_std=-1.0))
    refused("loss weights", loss=L.loss_opts(reg_weight=-1.0))
    refused("bad sizes", R=0)
    refused("bad sizes", S=4097)
    refused("bad strides", rs=2)
    refused("bad strides", dss=0)
    for k in ("rgb", "sigma", "z", "d", "tgt", "d_rgb", "d_sigma", "terms"):
        refused("null pointer", **{k: None})
    refused("zero_buf is NULL", zero_n=5)


def test_fused_step_and_grid_carry_the_feature():
    from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
    from nerf_few_shot_limitations_amd.training import FusedStep
    for fn in (FusedStep.step_rays, FusedStep.step_view):
        assert inspect.signature(fn).parameters["occupancy"].default is None
    assert "occupancy" not in inspect.signature(FusedStep.__call__).parameters          # the staged-points step stays without a grid
    p = inspect.signature(OccupancyGrid.refresh).parameters
    assert p["decay"].default == 0.95 and {"model", "threshold", "samples_per_cell", "cells", "seed", "dino"} <= set(p)
    assert "starved of gradient" in " ".join(OccupancyGrid.refresh.__doc__.split())
    g = OccupancyGrid.full((32, 4, 4), -1.0, 1.0)
    assert g.res == (32, 4, 4) and g.occupied_fraction == 1.0 and bool(g.to_mask().all()) and g.bits.numel() == 16
    assert OccupancyGrid.full(32, 0.0, (1.0, 2.0, 3.0)).res == (32, 32, 32)
    with pytest.raises(ValueError):
        OccupancyGrid.full((48, 4, 4), -1.0, 1.0)


_CFG = ("experiment: {{name: t}}\ndata: {{near: 2.0, far: 6.0, resolution: 16}}\nmodel: {{use_dino: {dino}}}\n"
        "nerf_model: {{pos_freq: 10, dir_freq: 4, hidden_dim: 256, num_layers: 8}}\n"
        "optimizer: {{lr: 1.0e-3, weight_decay: 0.0, lr_milestones: [2], lr_gamma: 0.5}}\n"
        "dino_model: {{name: facebook/dinov2-small, lora_rank: 4, lora_alpha: 8, use_lora: true}}\n")


@pytest.mark.parametrize("dino,flags,word", [
    ("true", ["--occupancy-res", "64", "--dino-random-init"], "use_dino"),
    ("true", ["--occupancy-res", "64", "--dino-random-init", "--train-extractor"], "use_dino"),
    ("false", ["--occupancy-box", "-1", "1"], "--occupancy-box needs --occupancy-res"),
    ("false", ["--occupancy-threshold", "0.5"], "--occupancy-threshold needs --occupancy-res"),
    ("false", ["--occupancy-decay", "0.9"], "--occupancy-decay needs --occupancy-res"),
    ("false", ["--occupancy-refresh-every", "4"], "--occupancy-refresh-every needs --occupancy-res"),
    ("false", ["--occupancy-cells-per-refresh", "64"], "--occupancy-cells-per-refresh needs --occupancy-res"),
    ("false", ["--occupancy-warmup", "0"], "--occupancy-warmup needs --occupancy-res"),
    ("false", ["--occupancy-res", "0", "--occupancy-warmup", "10"], "--occupancy-warmup needs --occupancy-res"),
    ("false", ["--occupancy-res", "48"], "multiple of 32"),
    ("false", ["--occupancy-res", "64", "--occupancy-box", "1", "1"], "LO < HI"),
    ("false", ["--occupancy-res", "64", "--occupancy-decay", "1.5"], "--occupancy-decay"),
    ("false", ["--occupancy-res", "64", "--occupancy-refresh-every", "0"], "--occupancy-refresh-every"),
    ("false", ["--occupancy-res", "64", "--occupancy-cells-per-refresh", "40"], "multiple of 32"),
    ("false", ["--occupancy-res", "64", "--occupancy-warmup", "-1"], "--occupancy-warmup"),
])
def test_train_cli_argument_refusals(tmp_path, dino, flags, word):
    from nerf_few_shot_limitations_amd import train_cli
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino=dino))
    with pytest.raises(SystemExit) as e:                         # decided before the data set is read or a device is touched
        train_cli.main(["--config", str(cfg), "--data", str(tmp_path / "nowhere"), *flags])
    assert word in str(e.value), e.value


def test_train_cli_refuses_the_extractor_under_a_grid():
    """--train-extractor needs a use_dino config, which a grid refuses first: the combination is checked on the function itself."""
    import argparse
    from nerf_few_shot_limitations_amd import train_cli
    args = argparse.Namespace(occupancy_res=64, train_extractor=True, **{f: None for f in train_cli.OCCUPANCY_FLAGS})
    assert "--train-extractor" in train_cli.occupancy_args_error(args, {"model": {"use_dino": False}})
    args.train_extractor = False
    assert train_cli.occupancy_args_error(args, {"model": {"use_dino": False}}) is None
    assert inspect.signature(train_cli.train_epoch).parameters["occupancy"].default is None
    doc = " ".join(train_cli.__doc__.split())
    assert "all-ones" in doc and "resumed run starts again" in doc


# ---------------------------------------------------------------------------------------------
# the build's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res():
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B.kernel_resources()


NEW = ("occupancy_compact_count_kernel", "occupancy_compact_scan_kernel", "occupancy_compact_write_kernel",
       "indexed_loss_backward_kernel")


def test_new_kernels_use_no_scratch_and_spill_nothing(res):
    for kernel in NEW:
        ks = {k: v for k, v in res.items() if "::" + kernel + "(" in k}
        assert len(ks) == 1, (kernel, sorted(ks))
        (name, r), = ks.items()
        print(kernel, r)
        assert r["tu"] == "staged_kernels"
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["agprs"] == 0 and r["occupancy"] >= 6, (name, r)


def test_every_existing_kernel_keeps_its_figures(res):
    """tests/golden/kernel_resources.json is the complete census of the library's kernels, by unit and demangled name, taken from the
    build of the commit before the instantiation units became one source: every one of those kernels is still built, under its name and in
    its unit, with the same registers, scratch, spills, occupancy and LDS, and no kernel is built beside them."""
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))
    fields = gold["fields"]
    assert len(gold["kernels"]) == 228
    assert set(res) == set(gold["kernels"]), (sorted(set(gold["kernels"]) - set(res)), sorted(set(res) - set(gold["kernels"])))
    for name, want in gold["kernels"].items():
        now = res[name]
        assert [now.get(f, 0) for f in fields] == want, (name, dict(zip(fields, want)), now)
