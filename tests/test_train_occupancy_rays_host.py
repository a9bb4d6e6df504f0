"""Host-side checks of the ray route under an occupancy grid (no GPU): nrf_mlp_forward_train_rays_indexed against its ctypes
declaration, every refusal it answers before any launch, the resource figures of its kernels against their *_rays_kernel siblings,
train_cli's --occupancy-per-view argument checks, the per-view grid state's checkpoint round trip, and FusedStep's new keyword."""
import argparse
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nrf_mlp_forward_train_rays_indexed"


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
    args = [a.strip() for a in re.search(r"\b" + NAME + r"\s*\((.*?)\);", code, re.S).group(1).split(",")]
    restype, argtypes = L.SIGNATURES[NAME]
    assert len(args) == len(argtypes) == 11 and restype is C.c_int and hasattr(lib, NAME)
    # nrf_mlp_forward_train_rays' argument list with the row list behind the options
    plain = [a.strip() for a in re.search(r"\bnrf_mlp_forward_train_rays\s*\((.*?)\);", code, re.S).group(1).split(",")]
    k = args.index("const int32_t* index")
    assert args[k + 1] == "int64_t n_rows" and args[:k] + args[k + 2:] == plain and args[k - 1] == "const nrf_render_opts* opts"
    assert argtypes[:k] + argtypes[k + 2:] == L.SIGNATURES["nrf_mlp_forward_train_rays"][1]
    assert argtypes[k] is C.c_void_p and argtypes[k + 1] is C.c_int64
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(5) == -1
    doc = " ".join(header[header.index("nrf_mlp_forward_train_rays on a compacted sample list"):header.index(NAME + "(")].split())
    for word in ("index[j] = r*S + s", "READ from rays->z_vals", "writes none of the nrf_train_rays outputs", "undefined",
                 "n_rows == 0 succeeds", "nrf_train_context_bytes(m, mode, n_rows)"):
        assert word in doc, word


def test_refusals_before_any_launch(L):
    """Every refusal the header lists that needs no model, with its message, in the pattern of test_compaction_refusals_before_any_launch:
    nothing here owns device memory, a launch would fault.  (A context too small for n_rows reads the model: the GPU suite has it.)"""
    lib = L.lib()
    R, S = 8, 16
    good_rays = dict(rays_o=0x1000, rays_d=0x2000, z_vals=0x3000)
    pix = dict(pixels=0x1000, H=8, W=8, focal=10.0, c2w=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], z_vals=0x3000, rays_d_out=0x4000)
    model = C.c_void_p(0)                                         # no model: every refusal below comes before the model is read

    def call(rays=good_rays, opts=None, index=0x10000, n_rows=R * S, n_rays=R, **opt_kw):
        rays = rays if rays is None or isinstance(rays, L.nrf_train_rays) else L.train_rays(**rays)
        opts = _opts(L, **opt_kw) if opts is None else opts
        ref = lambda s: None if s is None else C.byref(s)
        return lib.nrf_mlp_forward_train_rays_indexed(model, ref(rays), n_rays, ref(opts) if opts != "null" else None, index, n_rows, 0x5000, 0x6000,
                                                      0x7000, 1 << 40, None)

    def refused(word, **kw):
        assert call(**kw) == -1, (word, kw)                                   # NRF_EINVAL
        assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())

    # the row list
    refused("index is NULL", index=None)
    refused("index must be 4-byte aligned", index=0x10002)
    refused("n_rows < 0", n_rows=-1)
    refused("n_rows exceeds n_rays * n_samples", n_rows=R * S + 1)
    refused("n_rows exceeds n_rays * n_samples", n_rows=1, n_rays=0)
    # the depths the compaction left
    refused("rays->z_vals is required", rays=dict(rays_o=0x1000, rays_d=0x2000))
    # everything nrf_mlp_forward_train_rays refuses
    refused("rays is NULL", rays=None)
    short = L.train_rays(**good_rays)
    short.struct_bytes = 112
    refused("nrf_train_rays: struct_bytes", rays=short)
    refused("opts is NULL", opts="null")
    refused("n_rays < 0", n_rays=-1)
    refused("ert_eps", ert_eps=0.01)
    refused("n_samples", n_samples=0)
    refused("not both and not neither", rays=dict(z_vals=0x3000))
    refused("not both and not neither", rays={**good_rays, "pixels": 0x8000})
    refused("come together", rays=dict(rays_o=0x1000, z_vals=0x3000))
    refused("camera", rays={**pix, "focal": 0.0})
    refused("rays_d_out is required", rays={**pix, "rays_d_out": None})
    refused("too large", n_rays=1 << 20, n_samples=4096)
    # with everything above in order the model is looked at next -- also for no rows at all
    refused("model is NULL")
    refused("model is NULL", rays=pix)
    refused("model is NULL", n_rows=0)
    refused("model is NULL", n_rows=R * S, index=0x10004)


# ---------------------------------------------------------------------------------------------
# the build's resource figures
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def res():
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    # the indexed kernels by kernel name, and everything else
    every = B.kernel_resources()
    new = {n: r for n, r in every.items() if "_rays_indexed_kernel<" in n}
    return new, {n: r for n, r in every.items() if n not in new}


def _kernel(name):
    """'tu: void nrf::kernel<args>(params)' -> 'kernel<args>'"""
    return name.split(": ", 1)[1].split("(")[0].split("nrf::", 1)[1]


# (scratch bytes per lane, VGPRs spilled) where an indexed kernel does not meet its sibling, which stands beside it.  All are 8-wave
# workgroups at the 256-VGPR ceiling with no AGPR half to park in (the row's sample id arrives from a load the
# sibling computes, so the allocator sees one more value live across the first layer and spills one or two more registers); their
# SGPR spills are all below the siblings'.
OWN = {
    "train_forward_v2_rays_indexed_kernel<nrf::ModeBF16, 8, 10, 4>": ((20, 4), (12, 2)),
    "train_forward_v2_rays_indexed_kernel<nrf::ModeF16, 8, 10, 4>": ((20, 4), (12, 2)),
    "train_forward_v3_rays_indexed_kernel<nrf::ModeBF16, 8, 12, 4, 2>": ((140, 30), (132, 28)),
    "train_forward_v3_rays_indexed_kernel<nrf::ModeF16, 8, 12, 4, 2>": ((136, 29), (132, 28)),
    "train_forward_v3_rays_indexed_kernel<nrf::ModeBF16, 8, 12, 4, 4>": ((140, 30), (132, 28)),
    "train_forward_v3_rays_indexed_kernel<nrf::ModeF16, 8, 12, 4, 4>": ((136, 29), (132, 28)),
}


def test_indexed_kernels_meet_their_siblings(res):
    new, main = res
    want = {f"train_forward_rays_indexed_kernel<nrf::Mode{m}, {w}, 10>" for m, w in (("BF16", 4), ("BF16", 8), ("F16", 4), ("F16", 8), ("F32", 4))}
    want |= {f"train_forward_v2_rays_indexed_kernel<nrf::Mode{m}, {w}, 10, 4>" for m, w in (("BF16", 4), ("BF16", 8), ("F16", 4), ("F16", 8), ("F32", 4))}
    want |= {f"train_forward_v3_rays_indexed_kernel<nrf::Mode{m}, {w}, 12, 4, {dt}>" for dt in (2, 4)
             for m, w in (("BF16", 4), ("BF16", 8), ("F16", 4), ("F16", 8), ("F32", 4))}
    assert {_kernel(n) for n in new} == want                                  # V1, V2, V3 at dino_dim 64 / 128, three modes, both geometries
    siblings = {_kernel(n): r for n, r in main.items() if "_rays_kernel<" in n}
    for name, r in sorted(new.items()):
        k = _kernel(name)
        s = siblings[k.replace("_rays_indexed_kernel", "_rays_kernel")]
        print(k, {f: (r[f], s[f]) for f in ("vgprs", "agprs", "sgprs", "scratch", "vgpr_spill", "sgpr_spill", "occupancy")})
        assert r["tu"].startswith("train_rays_indexed_")
        assert r["occupancy"] == s["occupancy"] and r["lds"] == s["lds"], k
        assert r["sgpr_spill"] <= s["sgpr_spill"], k
        if k in OWN:
            own, sib = OWN[k]
            assert (s["scratch"], s["vgpr_spill"]) == sib, (k, s)
            assert r["scratch"] <= own[0] and r["vgpr_spill"] <= own[1], (k, r)
        else:
            assert r["scratch"] <= s["scratch"] and r["vgpr_spill"] <= s["vgpr_spill"], (k, r, s)


# ---------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------
def _args(**kw):
    from nerf_few_shot_limitations_amd import train_cli
    base = dict(occupancy_res=0, occupancy_per_view=False, train_extractor=False, **{f: None for f in train_cli.OCCUPANCY_FLAGS})
    return argparse.Namespace(**{**base, **kw})


def test_occupancy_args_error_with_and_without_the_flag():
    from nerf_few_shot_limitations_amd import train_cli
    err = train_cli.occupancy_args_error
    dino, plain = {"model": {"use_dino": True}}, {"model": {"use_dino": False}}
    # with the flag: a use_dino config is accepted, with and without a trained extractor
    assert err(_args(occupancy_res=64, occupancy_per_view=True), dino) is None
    assert err(_args(occupancy_res=64, occupancy_per_view=True, train_extractor=True), dino) is None
    assert err(_args(occupancy_res=64, occupancy_per_view=True), {}) is None              # use_dino defaults to true
    # ... refused without a grid and for a field that does not depend on the view
    assert "--occupancy-per-view needs --occupancy-res" in err(_args(occupancy_per_view=True), dino)
    assert "--occupancy-per-view needs --occupancy-res" in err(_args(occupancy_per_view=True), plain)
    msg = err(_args(occupancy_res=64, occupancy_per_view=True), plain)
    assert "--occupancy-per-view" in msg and "use_dino: false" in msg
    # ... and the other checks still apply
    assert "multiple of 32" in err(_args(occupancy_res=48, occupancy_per_view=True), dino)
    assert "--occupancy-decay" in err(_args(occupancy_res=64, occupancy_per_view=True, occupancy_decay=1.5), dino)
    # without the flag: the old answers
    old = err(_args(occupancy_res=64), dino)
    assert old.startswith("--occupancy-res: this config has use_dino: true") and "ONE source view" in old
    assert err(_args(occupancy_res=64, train_extractor=True), dino) == old
    assert "--train-extractor" in err(_args(occupancy_res=64, train_extractor=True), plain)
    assert err(_args(occupancy_res=64), plain) is None and err(_args(), dino) is None
    assert "--occupancy-warmup needs --occupancy-res" in err(_args(occupancy_warmup=3), plain)
    ns = argparse.Namespace(occupancy_res=64, train_extractor=False, **{f: None for f in train_cli.OCCUPANCY_FLAGS})   # a caller from before the flag
    assert err(ns, plain) is None and err(ns, dino) == old
    doc = " ".join(train_cli.__doc__.split())
    assert "--occupancy-per-view" in doc and "occupancy_per_view_state" in doc
    assert "The grid is not part of a checkpoint: a resumed run starts again" in doc       # the single grid stays out, as documented


def test_train_cli_refuses_the_flag_on_the_command_line(tmp_path):
    from nerf_few_shot_limitations_amd import train_cli
    from tests.test_train_occupancy_host import _CFG
    for dino, flags, word in (("true", ["--occupancy-per-view", "--dino-random-init"], "--occupancy-per-view needs --occupancy-res"),
                              ("false", ["--occupancy-per-view", "--occupancy-res", "32"], "use_dino: false")):
        cfg = tmp_path / f"cfg_{dino}.yaml"
        cfg.write_text(_CFG.format(dino=dino))
        with pytest.raises(SystemExit) as e:                     # decided before the data set is read or a device is touched
            train_cli.main(["--config", str(cfg), "--data", str(tmp_path / "nowhere"), *flags])
        assert word in str(e.value), e.value


def test_per_view_state_survives_a_checkpoint_round_trip(tmp_path):
    from nerf_few_shot_limitations_amd import train_cli
    kw = dict(box=(-2.0, 2.0), threshold=0.25, decay=0.5, refresh_every=3, cells_per_refresh=64, warmup=5)
    a = train_cli.PerViewOccupancy(3, 32, **kw)
    assert len(a.views) == 3 and a.view(1) is a.views[1] and a.views[0].grid is not a.views[1].grid
    g = torch.Generator().manual_seed(1)
    for v, s in enumerate(a.views):                               # what refreshes and steps would have left, different per view
        s.grid.bits.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, s.grid.bits.shape, generator=g, dtype=torch.int64).to(torch.int32))
        if v != 2:                                                # view 2: never refreshed, no per-cell values yet
            s.grid.ema = torch.rand(s.grid.n_cells, generator=g)
            s.grid._cursor, s.grid._refreshes = 64 * (v + 1), 7 + v
        s.steps = 11 * v + 2
    assert a.view(0).current() is a.view(0).full and a.view(1).current() is a.view(1).grid        # warm-up 5: 2 steps, 13 steps
    path = str(tmp_path / "ckpt.pth")
    torch.save({"occupancy_per_view_state": a.state_dict()}, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)["occupancy_per_view_state"]       # as train_cli.main loads a checkpoint
    b = train_cli.PerViewOccupancy(3, 32, **kw)
    b.load_state_dict(sd)
    for v, (sa, sb) in enumerate(zip(a.views, b.views)):
        assert torch.equal(sa.grid.bits, sb.grid.bits) and sb.grid.bits.dtype == torch.int32, v
        ea, eb = getattr(sa.grid, "ema", None), getattr(sb.grid, "ema", None)
        assert (ea is None and eb is None) if v == 2 else torch.equal(ea, eb), v
        assert getattr(sa.grid, "_cursor", 0) == getattr(sb.grid, "_cursor", 0) and getattr(sa.grid, "_refreshes", 0) == getattr(sb.grid, "_refreshes", 0)
        assert sa.steps == sb.steps == 11 * v + 2
        assert (sb.current() is sb.full) == (sa.current() is sa.full)
    assert bool(b.views[0].full.to_mask().all())                                  # the warm-up's all-ones grid is not part of the state
    assert a.occupied_fraction == b.occupied_fraction
    with pytest.raises(ValueError):
        train_cli.PerViewOccupancy(2, 32, **kw).load_state_dict(sd)               # another number of views
    with pytest.raises(ValueError):
        train_cli.PerViewOccupancy(3, 64, **kw).load_state_dict(sd)               # another resolution
    # the single grid's schedule keeps its constructor and its steps
    s = train_cli.OccupancySchedule(32, warmup=1)
    assert s.current() is s.full and "dino" in inspect.signature(s.after_step).parameters
    assert inspect.signature(train_cli.save_checkpoint).parameters["occupancy"].default is None


def test_signatures():
    from nerf_few_shot_limitations_amd.training import FusedStep
    for fn in (FusedStep.step_rays, FusedStep.step_view):
        assert inspect.signature(fn).parameters["grid_inputs"].default == "staged"
    assert "grid_inputs" not in inspect.signature(FusedStep.__call__).parameters
