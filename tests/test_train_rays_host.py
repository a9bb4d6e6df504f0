"""Host-side checks of the training forward that takes rays (no GPU): the new C ABI struct and entry point against their ctypes
declarations, the refusals that answer before any launch, train_cli's --fused-inputs, and the build's resource figures of the
ray-input forward kernels next to their staged-input siblings.

Three of the refusals of nrf_mlp_forward_train_rays read the model (a V3 model without `dino`, `dino->C != dino_dim`, a context
that is too small) and a model cannot be created without a device: they are in tests/test_gpu_train_rays.py."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "nrf_mlp_forward_train_rays"


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def test_header_and_ctypes_agree_on_the_struct_and_the_entry_point(L):
    header = open(os.path.join(ROOT, "include", "nerfhip.h")).read()
    lib = L.lib()
    assert re.search(r"\b" + NAME + r"\s*\(", header)
    assert NAME in L.SIGNATURES and hasattr(lib, NAME)
    body = re.search(r"typedef struct nrf_train_rays \{(.*?)\} nrf_train_rays;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            names = decl.strip().split(None, 1)[1] if not decl.strip().startswith("const") else decl.strip().split(None, 2)[2]
            fields += [re.match(r"\*?\s*(\w+)", n.strip()).group(1) for n in names.split(",")]
    assert fields == [f for f, _ in L.nrf_train_rays._fields_]
    assert fields == ["struct_bytes", "reserved", "rays_o", "rays_d", "pixels", "H", "W", "focal", "c2w", "z_vals", "rays_d_out", "points_out"]
    T = L.nrf_train_rays
    assert C.sizeof(T) == 120 and T.rays_o.offset == 8 and T.pixels.offset == 24 and T.H.offset == 32 and T.c2w.offset == 44
    assert T.z_vals.offset == 96 and T.points_out.offset == 112
    assert L.train_rays().struct_bytes == 120
    # additive: the ABI version and the size table are what they were
    assert lib.nrf_abi_version() == 5 and lib.nrf_abi_sizeof(5) == -1 and lib.nrf_abi_sizeof(99) == -1
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\b" + NAME + r"\s*\((.*?)\);", code, re.S).group(1)
    assert len(decl.split(",")) == len(L.SIGNATURES[NAME][1]) == 9
    assert "train.py:188-229" in header                       # the header cites what the entry point replaces


def _opts(L, **kw):
    o = L.nrf_render_opts()
    o.near, o.far, o.n_samples, o.mma_mode = 2.0, 6.0, 16, 0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_refusals_before_any_launch(L):
    lib = L.lib()
    P = lambda a: a
    good = dict(rays_o=P(0x1000), rays_d=P(0x2000), z_vals=P(0x3000))
    pix = dict(pixels=P(0x1000), H=8, W=8, focal=10.0, c2w=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], z_vals=P(0x3000), rays_d_out=P(0x4000))

    def call(rays, opts, n_rays=8, model=None, out_a=P(0x5000), out_b=P(0x6000), ctx=P(0x7000), nbytes=1 << 30):
        return lib.nrf_mlp_forward_train_rays(model, None if rays is None else C.byref(rays), n_rays, None if opts is None else C.byref(opts),
                                              out_a, out_b, ctx, nbytes, None)

    def refused(word, *a, **kw):
        assert call(*a, **kw) == -1, (word, a, kw)                          # NRF_EINVAL
        assert word.encode() in lib.nrf_last_error(), (word, lib.nrf_last_error())

    refused("rays is NULL", None, _opts(L))
    short = L.train_rays(**good)
    short.struct_bytes = 112
    refused("struct_bytes", short, _opts(L))
    refused("opts is NULL", L.train_rays(**good), None)
    refused("ert_eps", L.train_rays(**good), _opts(L, ert_eps=0.01))
    refused("n_samples", L.train_rays(**good), _opts(L, n_samples=0))
    refused("n_rays < 0", L.train_rays(**good), _opts(L), n_rays=-1)
    refused("not both and not neither", L.train_rays(z_vals=P(0x3000)), _opts(L))                                   # neither
    refused("not both and not neither", L.train_rays(**{**good, "pixels": P(0x8000)}), _opts(L))                    # both
    refused("come together", L.train_rays(rays_o=P(0x1000), z_vals=P(0x3000)), _opts(L))
    refused("z_vals", L.train_rays(rays_o=P(0x1000), rays_d=P(0x2000)), _opts(L))
    refused("rays_d_out", L.train_rays(**{**pix, "rays_d_out": None}), _opts(L))
    refused("camera", L.train_rays(**{**pix, "focal": 0.0}), _opts(L))
    refused("too large", L.train_rays(**good), _opts(L, n_samples=4096), n_rays=1 << 20)
    # everything the arguments alone decide is in order: the next thing looked at is the model
    refused("model is NULL", L.train_rays(**good), _opts(L))
    refused("model is NULL", L.train_rays(**pix), _opts(L))
    refused("model is NULL", L.train_rays(**good), _opts(L), n_rays=0)


def test_train_cli_carries_the_flag():
    from nerf_few_shot_limitations_amd import train_cli
    sig = inspect.signature(train_cli.train_epoch)
    assert sig.parameters["fused_inputs"].default is False
    # parses: with the flag the command gets as far as reading the (missing) config, without it too
    for extra in ([], ["--fused-inputs"]):
        with pytest.raises((FileNotFoundError, OSError)):
            train_cli.main(["--config", os.path.join(ROOT, "no_such_config.yaml"), "--data", "y", *extra])
    with pytest.raises(SystemExit):
        train_cli.main(["--config", "x", "--data", "y", "--fused-inputs=maybe"])


def test_fused_step_has_the_ray_entry_points():
    from nerf_few_shot_limitations_amd.training import FusedStep
    p = inspect.signature(FusedStep.step_rays).parameters
    assert list(p)[:7] == ["self", "rays_o", "rays_d", "target", "near", "far", "n_samples"]
    assert p["perturb"].default is True and all(p[k].default is None for k in ("t_rand", "seed", "z_in", "dino", "target_depth", "noise", "d_dino_out",
                                                                               "points_out"))
    q = inspect.signature(FusedStep.step_view).parameters
    assert list(q)[:10] == ["self", "image", "pose", "H", "W", "focal", "pixels", "near", "far", "n_samples"] and q["target"].default is None


# ---------------------------------------------------------------------------------------------
# the build's resource figures
# ---------------------------------------------------------------------------------------------
MODES = ("ModeBF16", "ModeF16", "ModeF32")


@pytest.fixture(scope="module")
def res():
    from nerf_few_shot_limitations_amd import build as B
    if not os.path.isdir(B.OBJ) or not any(f.endswith(".o.remarks") for f in os.listdir(B.OBJ)):
        pytest.skip("no object directory (the library was built elsewhere), as in tests/test_kernel_resources.py")
    return B.kernel_resources()


def _forward_kernels(res, kernel, tail=""):
    """{(mode, waves): figures} of the instantiations of `kernel` whose template arguments end in `tail`."""
    out = {}
    for name, r in res.items():
        m = re.search(r"nrf::" + kernel + r"<nrf::(Mode\w+), (\d+), ([^>]*)>\(", name)
        if m and m.group(3).endswith(tail):
            out[(m.group(1), int(m.group(2)))] = r
    return out


def test_a_ray_input_forward_kernel_is_built_for_every_family_and_mode(res):
    for kernel, tail in (("train_forward_rays_kernel", ""), ("train_forward_v2_rays_kernel", ""),
                         ("train_forward_v3_rays_kernel", ", 2"), ("train_forward_v3_rays_kernel", ", 4")):               # dino_dim / 32
        ks = _forward_kernels(res, kernel, tail)
        # both geometries of the 16-bit modes, the one of fp32 (train_impl.hpp:dispatch_chain)
        assert set(ks) == {("ModeBF16", 4), ("ModeBF16", 8), ("ModeF16", 4), ("ModeF16", 8), ("ModeF32", 4)}, (kernel, tail, sorted(ks))
        assert {m for m, _ in ks} == set(MODES)


@pytest.mark.parametrize("kernel", ["train_forward_kernel", "train_forward_v2_kernel"])
def test_v1_and_v2_ray_kernels_spill_no_more_than_their_staged_siblings(res, kernel):
    rays, staged = _forward_kernels(res, kernel.replace("_kernel", "_rays_kernel")), _forward_kernels(res, kernel)
    assert set(rays) == set(staged) and len(rays) == 5
    for key in sorted(rays):
        r, s = rays[key], staged[key]
        print(kernel, key, "rays", r["vgpr_spill"], r["scratch"], "staged", s["vgpr_spill"], s["scratch"])
        assert r["vgpr_spill"] <= s["vgpr_spill"] and r["scratch"] <= s["scratch"], (kernel, key, r, s)
