"""What the C API refuses, as a whole: return code and exact nrf_last_error() text of every refusal that csrc/api.cpp can give
before it needs a model or a device, the order in which two faults in one call are reported, and the bytes the seven debug
entries write.  tests/golden/api_refusals.json holds what the library answered before the checks of api.cpp were each written
once, every message once and per entry one line of `label:message index`; `python -m tests.test_api_refusals_host` prints the same
form for the library it runs on (sections `host` and `debug`, and under `uncovered` every string literal of api.cpp that no
recorded message contains).

A case is a call with good arguments and one fault (`entry/label`) or two faults that are neighbours in the order of the entry's
checks (`entry/first+second`: the first is the one reported).  Everything the host code reads is real host memory (structs, c2w,
res / lo / scale, the Linears of the debug entries); every other pointer is an aligned integer that nothing dereferences, because
every case is refused, or returns NRF_OK early, in front of the first launch.  For an early NRF_OK the code alone is recorded:
the last error is stale by design.  The cases behind a model check run in tests/test_gpu_api_refusals.py from the same tables."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

from nerf_few_shot_limitations_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_refusals.json")
API_CPP = os.path.join(ROOT, "nerf_few_shot_limitations_amd", "csrc", "api.cpp")
P = 0x7f0000001000          # a pointer nothing reads: 16-byte aligned
OFF16, OFF8, OFF4 = P + 4, P + 4, P + 2
MODEL = object()            # the model argument: NULL on the host, the family's model on the GPU
N_GPU = 64                  # samples of the cases that run with a model


class Late:
    """A value that needs the finished argument list (and, with a model, the library): fn(api, args)."""
    def __init__(self, fn):
        self.fn = fn


class F:
    """One fault: the arguments it overrides (`a__b` = field b of argument a, through pointers; an integer part indexes an array).
    alt: a second way to trip the check of the fault before it, outside the order chain.  final: part of the last gate in front of
    the launch, which the cases with a model keep shut unless they are about that gate."""
    def __init__(self, label, alt=False, final=False, **ov):
        self.label, self.alt, self.final, self.ov = label, alt, final, ov


class Spec:
    def __init__(self, entry, names, good, chain, fam=None, tag="", safe=None, host_tag=None):
        self.entry, self.names, self.good, self.chain, self.fam, self.tag, self.safe = entry, names.split(), good, chain, fam, tag, safe
        self.host_tag = tag if host_tag is None else host_tag          # (False: the host cases are those of another family's spec)
        assert len(self.names) == len(L.SIGNATURES[entry][1]), entry
        labels = [f.label for f in chain]
        assert len(labels) == len(set(labels)), (entry, labels)

    def title(self, with_model):
        tag = self.tag if with_model else self.host_tag
        return self.entry + (f"[{tag}]" if tag else "")


def api():
    """The library through a handle of its own: array parameters (c2w, res, lo, scale) are plain pointers here, so that NULL can be
    passed for them."""
    L.lib()
    h = C.CDLL(L.LIB_PATH)
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype = res
        fn.argtypes = [C.c_void_p if isinstance(a, type) and issubclass(a, C.Array) else a for a in args]
    return h


def set_path(args, path, value):
    parts = path.split("__")
    if len(parts) == 1:
        args[path] = value
        return
    obj = args[parts[0]]
    for p in parts[1:-1]:
        obj = getattr(obj, p)
        if isinstance(obj, C._Pointer):
            obj = obj.contents
    if isinstance(obj, C._Pointer):
        obj = obj.contents
    if parts[-1].isdigit():
        obj[int(parts[-1])] = value
    else:
        setattr(obj, parts[-1], value)


def conflict(a, b):
    """Two faults that cannot stand in one call: they override the same argument or field, or one removes what the other edits."""
    return any(x == y or x.startswith(y + "__") or y.startswith(x + "__") for x in a.ov for y in b.ov)


def call(h, spec, faults, model=None, dry=False):
    args = spec.good()
    for k, v in list(args.items()):
        if v is MODEL:
            args[k] = model
    todo = list(faults)
    if model is not None and spec.safe and not any(f.final for f in faults):
        todo.insert(0, next(f for f in spec.chain if f.label == spec.safe))
    for f in todo:
        for path, v in f.ov.items():
            set_path(args, path, v)
    for k, v in list(args.items()):
        if isinstance(v, Late):
            args[k] = v.fn(h, args)
    argv = [C.byref(args[n]) if isinstance(args[n], (C.Structure, C._SimpleCData)) else args[n] for n in spec.names]
    if dry:
        return argv
    rc = getattr(h, spec.entry)(*argv)
    return {"rc": rc, "error": h.nrf_last_error().decode()} if rc < 0 else {"rc": rc}


def cases(spec, with_model):
    """(name, faults) of a spec.  Without a model: the chain up to the model check; with one: what lies behind it."""
    chain = [f for f in spec.chain if not f.alt]
    cut = next((i for i, f in enumerate(chain) if f.label == "model"), None)
    if with_model:
        if cut is None or spec.fam is None:
            return
        first = cut + 1
        keep = lambda f: spec.chain.index(f) > spec.chain.index(chain[cut])
    else:
        if spec.host_tag is False:
            return
        first, chain = 0, chain if cut is None else chain[:cut + 1]
        keep = lambda f: cut is None or spec.chain.index(f) < spec.chain.index(chain[cut])
    for f in spec.chain:
        if (f in chain and chain.index(f) >= first) or (f.alt and keep(f)):
            yield f"{spec.title(with_model)}/{f.label}", [f]
    for a, b in zip(chain[first:], chain[first + 1:]):
        if not conflict(a, b):
            yield f"{spec.title(with_model)}/{a.label}+{b.label}", [a, b]


# ------------------------------------------------------------------------------------------------------------------------------
# the three small networks, and arguments that are in order
# ------------------------------------------------------------------------------------------------------------------------------
def net(fam):
    """The smallest network of a family the plans accept (hidden 256, one trunk layer, one frequency, dino_dim 64): arch, Linears,
    their count, and the arrays to keep alive.  Small-integer weights, exact in every mode."""
    pe, de, H, dd = 9, 9, 256, 64
    tail = [(1, H), (H, H), (H // 2, H + de), (H // 4, H // 2), (3, H // 4)]
    shapes = {"v1": [(H, pe), (1, H), (3, H)], "v2": [(H, pe)] + tail,
              "v3": [(H, pe + dd), (H, H), (H // 4, H), (2, H // 4), (H, H), (H, H)] + tail}[fam]
    arr, keep = (L.nrf_linear * len(shapes))(), []
    for i, (o, k) in enumerate(shapes):
        r, c = np.meshgrid(np.arange(o), np.arange(k), indexing="ij")
        w = np.ascontiguousarray(((((3 * r + 5 * c + i) % 7) - 3) / 16).astype(np.float32))
        b = np.ascontiguousarray((((np.arange(o) + i) % 5 - 2) / 4).astype(np.float32))
        keep += [w, b]
        arr[i] = L.nrf_linear(w.ctypes.data_as(L.c_float_p), b.ctypes.data_as(L.c_float_p), o, k)
    arch = L.nrf_arch({"v1": 1, "v2": 2, "v3": 3}[fam], 1, 0 if fam == "v1" else 1, H, 1, dd if fam == "v3" else 0)
    return arch, arr, len(shapes), keep


NETS = {fam: net(fam) for fam in ("v1", "v2", "v3")}


def bad_linears(fam):
    """The family's Linears with a non-positive shape in the second one."""
    _, arr, n, _ = NETS[fam]
    out = (L.nrf_linear * n)(*arr)
    out[1].out_f = 0
    return out


def fa(*v):
    return (C.c_float * len(v))(*v)


def ia(*v):
    return (C.c_int32 * len(v))(*v)


def c2w(n=1):
    return fa(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4] * n))


def dino(**kw):
    d = L.nrf_dino(features=P, Hp=4, Wp=4, C=64, focal=4.0, H=4, W=4)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def opts(with_dino=False, **kw):
    o = L.nrf_render_opts(near=2.0, far=6.0, n_samples=4, mma_mode=0)
    if with_dino:
        o.dino = C.pointer(dino())
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def occ(**kw):
    return L.occupancy(bits=P, res=(32, 8, 8), **kw)


OPTS_F = [F("opts", opts=None), F("n_samples", opts__n_samples=0), F("near_far", opts__near=0.0), F("mma_mode", opts__mma_mode=4),
          F("ert_range", opts__ert_eps=1.0)]
BOX_F = lambda p: [F("res", **{p + "res__1": 0}), F("res_high", alt=True, **{p + "res__2": 513}), F("lo", **{p + "lo__1": float("inf")}),
                   F("scale", **{p + "scale__2": 0.0}), F("res0", **{p + "res__0": 48})]
OCC_F = [F("occ", occ=None), F("occ_struct", occ__struct_bytes=8), F("outside", occ__outside=2), F("bits", occ__bits=None),
         F("bits_align", alt=True, occ__bits=OFF4), *BOX_F("occ__")]
RGBD_F = [F("rgbd", opts__out_rgbd=1, rgb=OFF16)]
DINO_F = [F("dino_missing", final=True, opts__dino=None), F("dino_size", final=True, opts__dino__Hp=0),
          F("dino_channels", final=True, opts__dino__C=32)]
TAIL_F = [F("tail", tail=None), F("tail_mode", tail__mode=0), F("tail_base", opts__mma_mode=2), F("tail_ert", opts__ert_eps=0.5),
          F("tail_ws", tail__workspace=None), F("tail_ws_align", tail__workspace=OFF16), F("tail_ws_bytes", tail__workspace_bytes=15)]
EMIT_F = [F("raw4", raw4=None), F("raw4_align", alt=True, raw4=OFF16), F("emit_ert", opts__ert_eps=0.5)]
OUT4 = dict(rgb=P, depth=P, weights=None, z_vals=None, stream=None)


def tail():
    return L.nrf_tail(3, P, 1 << 40)


def render_specs():
    """The three renders in their plain, _tail, _emit and _occ forms.  With a model they run on the V3 one with `dino` missing: the
    last gate in front of the launch stays shut."""
    out = []
    for form in ("", "_tail", "_emit", "_occ"):
        extra = {"": "", "_tail": " tail", "_occ": " occ", "_emit": ""}[form]
        last = " raw4 raw_only stream" if form == "_emit" else " stream"
        more = {"": {}, "_tail": {"tail": tail}, "_occ": {"occ": occ}, "_emit": {"raw4": lambda: P, "raw_only": lambda: 0}}[form]
        mid_tail = TAIL_F if form == "_tail" else []
        mid_emit = EMIT_F if form == "_emit" else []
        fill = lambda d, more=more: {**d, **{k: v() for k, v in more.items()}}

        head = (OCC_F + [F("occ_rays", n_rays=1 << 31)] if form == "_occ" else [])
        out.append(Spec("nrf_render_rays" + form, "m rays_o rays_d n_rays opts" + extra + " rgb depth weights z_vals" + last,
                        lambda fill=fill: fill(dict(m=MODEL, rays_o=P, rays_d=P, n_rays=N_GPU, opts=opts(True), **OUT4)),
                        head + RGBD_F + [F("model", m=None), F("n_rays", n_rays=-1), F("zero", n_rays=0), *OPTS_F, *mid_emit,
                                         F("null", rays_o=None), F("null_out", alt=True, rgb=None), F("large", opts__n_samples=4096, n_rays=1 << 29),
                                         *mid_tail, *DINO_F], fam="v3", safe="dino_missing"))
        head = (OCC_F + [F("occ_rays", H=1 << 16, W=1 << 16, ray_end=1 << 31)] if form == "_occ" else [])
        out.append(Spec("nrf_render_camera" + form, "m H W focal c2w ray_begin ray_end opts" + extra + " rgb depth weights z_vals" + last,
                        lambda fill=fill: fill(dict(m=MODEL, H=8, W=8, focal=8.0, c2w=c2w(), ray_begin=0, ray_end=N_GPU, opts=opts(True), **OUT4)),
                        head + RGBD_F + [F("model", m=None), F("camera", focal=0.0), F("camera_c2w", alt=True, c2w=None), F("range", ray_begin=-1),
                                         F("zero", ray_end=0), *OPTS_F, *mid_emit, F("null_out", rgb=None), *mid_tail, *DINO_F],
                        fam="v3", safe="dino_missing"))
        if form == "_emit":
            continue
        head = (OCC_F + [F("occ_rays", n_tiles=1 << 20, tile_rays=1 << 11)] if form == "_occ" else [])
        out.append(Spec("nrf_render_cameras_tiles" + form,
                        "m H W focal c2w n_cams tile_rays first_tile tile_step n_tiles opts" + extra + " rgb depth weights z_vals stream",
                        lambda fill=fill: fill(dict(m=MODEL, H=8, W=8, focal=8.0, c2w=c2w(2), n_cams=2, tile_rays=8, first_tile=0, tile_step=1, n_tiles=4,
                                                    opts=opts(True), **OUT4)),
                        head + RGBD_F + [F("model", m=None), F("camera", H=0), F("n_cams", n_cams=9), F("tiles", tile_step=0), F("zero", n_tiles=0),
                                         F("first_tile", first_tile=8), *OPTS_F, F("null_out", rgb=None), F("per_ray", opts__z_in=P), *mid_tail,
                                         *DINO_F], fam="v3", safe="dino_missing"))
    return out


# ---- the ray source of the training entries -------------------------------------------------------------------------------
def by_rays():
    return L.train_rays(rays_o=P, rays_d=P, z_vals=P)


def by_pixels():
    return L.train_rays(pixels=P, H=8, W=8, focal=8.0, c2w=[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 4], z_vals=P, rays_d_out=P)


SRC_HEAD = [F("rays", rays=None), F("rays_struct", rays__struct_bytes=112), F("n_rays", n_rays=-1), *OPTS_F, F("ert", opts__ert_eps=0.5)]
SRC_RAYS = SRC_HEAD + [F("both", rays__pixels=P), F("neither", alt=True, rays__rays_o=None, rays__rays_d=None), F("together", rays__rays_d=None),
                       F("z_vals", rays__z_vals=None), F("large", n_rays=1 << 20, opts__n_samples=4096)]
SRC_PIXELS = SRC_HEAD + [F("neither", rays__pixels=None), F("camera", rays__focal=0.0), F("camera_H", alt=True, rays__H=0), F("z_vals", rays__z_vals=None),
                         F("rays_d_out", rays__rays_d_out=None), F("large", n_rays=1 << 20, opts__n_samples=4096)]
TRAIN_DINO_F = [F(f.label, final=True, **f.ov) for f in DINO_F]


def ctx_below(n_of):
    return Late(lambda h, a: h.nrf_train_context_bytes(a["m"], 2 if a["opts"].mma_mode == 3 else a["opts"].mma_mode, n_of(a)) - 1)


def ray_source_specs():
    out = []
    for tag, src, rays in (("rays", SRC_RAYS, by_rays), ("pixels", SRC_PIXELS, by_pixels)):
        for fam in ("v1", "v2", "v3"):
            v1 = fam == "v1"
            fam_f = (TRAIN_DINO_F if fam == "v3" else []) + [F("zero", n_rays=0)] + \
                    [F("null", out_a=None), F("null_ctx", alt=True, ctx=None)] + ([F("out_b", out_b=P)] if v1 else [F("null_b", alt=True, out_b=None)])
            out.append(Spec("nrf_mlp_forward_train_rays", "m rays n_rays opts out_a out_b ctx ctx_bytes stream",
                            lambda rays=rays, fam=fam, v1=v1: dict(m=MODEL, rays=rays(), n_rays=N_GPU // 4, opts=opts(fam == "v3"), out_a=P,
                                                                   out_b=None if v1 else P, ctx=P, ctx_bytes=1 << 40, stream=None),
                            src + [F("model", m=None)] + fam_f +
                            [F("ctx", final=True, ctx_bytes=ctx_below(lambda a: a["n_rays"] * a["opts"].n_samples))],
                            fam=fam, tag=f"{tag},{fam}", safe="ctx", host_tag=tag if v1 else False))
            fam_f = (TRAIN_DINO_F if fam == "v3" else []) + [F("zero", n_rows=0)] + \
                    [F("null", out_a=None)] + ([F("out_b", out_b=P)] if v1 else [F("null_b", alt=True, out_b=None)])
            out.append(Spec("nrf_mlp_forward_train_rays_indexed", "m rays n_rays opts index n_rows out_a out_b ctx ctx_bytes stream",
                            lambda rays=rays, fam=fam, v1=v1: dict(m=MODEL, rays=rays(), n_rays=N_GPU // 4, opts=opts(fam == "v3"), index=P, n_rows=N_GPU // 2,
                                                                   out_a=P, out_b=None if v1 else P, ctx=P, ctx_bytes=1 << 40, stream=None),
                            src + [F("index", index=None), F("index_align", index=OFF4), F("n_rows", n_rows=-1), F("n_rows_high", n_rows=N_GPU + 1),
                                   F("model", m=None)] + fam_f + [F("ctx", final=True, ctx_bytes=ctx_below(lambda a: a["n_rows"]))],
                            fam=fam, tag=f"{tag},{fam}", safe="ctx", host_tag=tag if v1 else False))
        out.append(Spec("nrf_occupancy_compact_rays", "rays n_rays opts occ out stream",
                        lambda rays=rays: dict(rays=rays(), n_rays=16, opts=opts(), occ=occ(),
                                               out=L.compact(64, P, P, P, P, P, P, 1 << 20), stream=None),
                        src + OCC_F + [F("out", out=None), F("out_struct", out__struct_bytes=8), F("outputs", out__count=None),
                                       F("outputs_index", alt=True, out__index=None), F("capacity", out__capacity=63), F("align4", out__directions=OFF4),
                                       F("align4_z", alt=True, rays__z_vals=OFF4), F("count_align", out__count=OFF8), F("workspace", out__workspace=None),
                                       F("workspace_bytes", out__workspace_bytes=15), F("zero", n_rays=0)], tag=tag))
    return out


# ---- the training entries on staged inputs: everything lies behind the model -----------------------------------------------
def train_specs():
    def ctx1(h, a):
        return h.nrf_train_context_bytes(a["m"], a["mma_mode"], a["n"]) - 1
    head = [F("model", m=None), F("n_mode", mma_mode=3), F("n_neg", alt=True, n=-1), F("zero", n=0)]
    ctx = [F("ctx", final=True, ctx_bytes=Late(ctx1))]
    base = dict(m=MODEL, mma_mode=1, n=N_GPU, ctx=P, ctx_bytes=1 << 40, stream=None)
    S = lambda entry, names, extra, chain, fam: Spec(entry, names, lambda: {**base, **extra}, head + chain + ctx, fam=fam, tag=fam, safe="ctx")
    out = [S("nrf_mlp_forward_train_v1", "m mma_mode x_enc n out4 ctx ctx_bytes stream", dict(x_enc=P, out4=P), [F("null", out4=None)], "v1"),
           S("nrf_mlp_backward_v1", "m mma_mode out4 g_out4 n ctx ctx_bytes flat_grad stream", dict(out4=P, g_out4=P, flat_grad=P),
             [F("null", flat_grad=None)], "v1")]
    fwd = "m mma_mode positions directions dino n rgb density ctx ctx_bytes stream"
    bwd = "m mma_mode rgb density g_rgb g_density n ctx ctx_bytes flat_grad stream"
    io = dict(positions=P, directions=P, dino=P, rgb=P, density=P)
    g = dict(rgb=P, density=P, g_rgb=P, g_density=P, flat_grad=P)
    out += [S("nrf_mlp_forward_train", fwd, io, [F("null", rgb=None), F("family", )], "v1"),
            S("nrf_mlp_forward_train", fwd, io, [F("null", ctx=None)], "v2"),
            S("nrf_mlp_forward_train", fwd, io, [F("null", positions=None), F("dino", dino=None)], "v3"),
            S("nrf_mlp_backward", bwd, g, [F("null", g_rgb=None), F("family")], "v1"),
            S("nrf_mlp_backward", bwd, g, [F("null", ctx=None)], "v3")]
    dn = "m mma_mode n ctx ctx_bytes d_dino stream"
    out += [S("nrf_mlp_backward_dino", dn, dict(d_dino=P), [F("null", d_dino=None), F("family")], "v2"),
            S("nrf_mlp_backward_dino", dn, dict(d_dino=P), [F("null", ctx=None), F("align", d_dino=OFF16)], "v3")]
    inp = "m mma_mode n ctx ctx_bytes positions directions d_x_enc d_positions d_directions stream"
    pd = dict(positions=P, directions=P, d_x_enc=None, d_positions=P, d_directions=P)
    out += [S("nrf_mlp_backward_inputs", inp, pd, [F("null", ctx=None), F("family")], "v3"),
            S("nrf_mlp_backward_inputs", inp, {**pd, "d_directions": None},
              [F("null", ctx=None), F("no_output", d_positions=None), F("v1_directions", d_directions=P), F("positions", positions=None),
               F("align", d_x_enc=OFF4)], "v1"),
            S("nrf_mlp_backward_inputs", inp, pd,
              [F("null", ctx=None), F("no_output", d_positions=None, d_directions=None), F("v2_x_enc", d_x_enc=P), F("positions", positions=None),
               F("directions", directions=None), F("align", d_directions=OFF4)], "v2")]
    inp3 = "m mma_mode n ctx ctx_bytes positions directions d_positions d_directions stream"
    pd3 = dict(positions=P, directions=P, d_positions=P, d_directions=P)
    out += [S("nrf_mlp_backward_inputs_v3", inp3, pd3, [F("null", ctx=None), F("family")], "v2"),
            S("nrf_mlp_backward_inputs_v3", inp3, pd3,
              [F("null", ctx=None), F("no_output", d_positions=None, d_directions=None), F("positions", positions=None), F("directions", directions=None),
               F("align", positions=OFF4)], "v3")]
    plain = lambda entry, names, extra, chain, fam: Spec(entry, names, lambda: dict(extra), chain, fam=fam, tag=fam)
    out += [plain("nrf_mlp_forward_v1", "m mma_mode x_enc n out4 stream", dict(m=MODEL, mma_mode=1, x_enc=P, n=N_GPU, out4=P, stream=None),
                  [F("model", m=None), F("n", n=-1), F("zero", n=0), F("null", final=True, out4=None)], "v1"),
            plain("nrf_mlp_forward", "m mma_mode positions directions dino n rgb density stream",
                  dict(m=MODEL, mma_mode=1, positions=P, directions=P, dino=None, n=N_GPU, rgb=P, density=P, stream=None),
                  [F("model", m=None), F("n", n=-1), F("zero", n=0), F("null", rgb=None), F("dino", final=True)], "v3")]
    return out


# ---- entries that take no model: every check is on the host ----------------------------------------------------------------
def loss_chain(who):
    return [F("loss", loss=None), F("loss_struct", loss__struct_bytes=8), F("loss_weights", loss__reg_weight=-1.0)] + \
           ([F("noise_std", loss__noise_std=-1.0)] if who == "launch" else [])


REG_F = [F("reg", reg=None), F("reg_struct", reg__struct_bytes=8), F("reg_weights", reg__occ_weight=float("inf")), F("dist_span", reg__dist_inv_span=0.0),
         F("occ_samples", reg__occ_samples=0)]
PATCH_F = [F("patch", patch=None), F("patch_struct", patch__struct_bytes=8), F("smooth_weight", patch__depth_smooth_weight=-1.0),
           F("patch_size", patch__patch_size=17), F("n_patches", patch__n_patches=-1), F("patch_rays", n_rays=8)]
INFO_F = [F("info", info=None), F("info_struct", info__struct_bytes=8), F("info_weights", info__ent_threshold=-1.0),
          F("kl_patches", patch__n_patches=0), F("kl_lds", patch__patch_size=16, n_rays=1 << 12, n_samples=49)]
LAUNCH_F = lambda **sizes: loss_chain("launch") + [F("sizes", **(sizes or dict(n_samples=4097))), F("strides", d_sigma_stride=0), F("null", ray_terms=None),
                                   F("zero_buf", zero_n=-1), F("zero_buf_null", alt=True, zero_n=4, zero_buf=None)]
TOO_MANY_RAYS = dict(n_rays=(1 << 30) + 1)       # (with the KL term on, n_samples > 4096 is refused earlier: the patch's LDS rows)
COMP = "rgb rgb_stride sigma sigma_stride z_vals rays_d n_rays n_samples white_bkgd"
COMP_GOOD = dict(rgb=P, rgb_stride=3, sigma=P, sigma_stride=1, z_vals=P, rays_d=P, n_rays=64, n_samples=8, white_bkgd=0)
DOUT = "d_rgb d_rgb_stride d_sigma d_sigma_stride"
DOUT_GOOD = dict(d_rgb=P, d_rgb_stride=3, d_sigma=P, d_sigma_stride=1)
ADAM = "params grads exp_avg exp_avg_sq n lr beta1 beta2 eps weight_decay step"
ADAM_GOOD = dict(params=P, grads=P, exp_avg=P, exp_avg_sq=P, n=64, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
MARK_F = lambda who: [F("n_samples", n_samples=0), F("box_null", res=None), F("lo_null", alt=True, lo=None), *BOX_F(""),
                      F("threshold", weight_threshold=-1.0), F("threshold_nan", alt=True, weight_threshold=float("nan")), F("seen_eps", seen_eps=1.0),
                      F("no_bits", hit_bits=None, seen_bits=None), F("bits_align", seen_bits=OFF4), F("z_vals", z_vals=None)]
BOX_GOOD = lambda: dict(res=ia(32, 8, 8), lo=fa(0, 0, 0), scale=fa(1, 1, 1), weight_threshold=0.01, seen_eps=1e-4, hit_bits=P, seen_bits=P, stream=None)
CAM_F = [F("camera", W=0), F("camera_focal", alt=True, focal=float("nan")), F("camera_c2w", alt=True, c2w=None), F("range", ray_end=65),
         F("range_order", alt=True, ray_begin=9, ray_end=8)]
MERGE_F = [F("sizes", n_samples=0), F("mma_mode", mma_mode=4)]
MERGE_TAIL_F = [F("null", z_coarse=None), F("null_new", alt=True, z_new=None), F("raw_align", raw_new=OFF16), F("rgbd", out_rgbd=1, rgb=OFF16)]
MERGE_GOOD = dict(z_coarse=P, raw_coarse=P, z_new=P, raw_new=P, n_samples=8, n_importance=4, mma_mode=0, white_bkgd=0, out_rgbd=0, rgb=P, depth=P,
                  weights=None, z_union=None, stream=None)
FETCH_F = [F("d_map", d_map=None), F("nothing", n=0, accumulate=1), F("null", points=None), F("ws", ws=None), F("ws_align", ws=OFF4),
           F("ws_bytes", ws_bytes=15)]


def hier_good():
    ptrs = {f: P for f, t in L.nrf_hier_loss._fields_ if t is C.c_void_p}
    return dict(a=L.hier_loss(rgb_stride=3, sigma_stride=1, w_coarse=1.0, w_fine=1.0, zero_n=4, workspace_bytes=1 << 40, **ptrs), n_rays=16, n_samples=8,
                n_importance=4, stream=None)


def debug_good(fam, **extra):
    arch, arr, n, _ = NETS[fam]
    return dict(arch=L.nrf_arch.from_buffer_copy(arch), linears=arr, n_linear=n, **extra)


PACK = "arch linears n_linear mma_mode stream_out stream_cap stream_bytes"
PACKERS = {"nrf_debug_pack": ("v1", "v2", "v3"), "nrf_debug_pack_dino_grad": ("v3",), "nrf_debug_pack_input_grad": ("v1", "v2"),
           "nrf_debug_pack_input_grad_v3": ("v3",), "nrf_debug_pack_backward": ("v1", "v2", "v3")}
LISTERS = {"nrf_debug_train_plan": "out cap n_ints", "nrf_debug_freq_mask_ids": "out cap n_ids"}
OTHER_FAMILY = {"nrf_debug_pack_dino_grad": "v2", "nrf_debug_pack_input_grad": "v3", "nrf_debug_pack_input_grad_v3": "v1"}


def debug_specs():
    out = []
    for entry, fams in PACKERS.items():
        full = entry == "nrf_debug_pack"
        names = PACK + (" bias_out bias_cap n_bias" if full else "")
        for fam in fams:
            good = lambda fam=fam, full=full: debug_good(fam, mma_mode=1, stream_out=P, stream_cap=0, stream_bytes=None,
                                                         **(dict(bias_out=P, bias_cap=0, n_bias=None) if full else {}))
            chain = [F("null", arch=None), F("null_count", alt=True, n_linear=0), F("mma_mode", mma_mode=4 if full else 3),
                     F("linears", linears=bad_linears(fam)), F("plan", arch__hidden=128), F("stream_cap", stream_cap=0)]
            out.append(Spec(entry, names, good, chain, tag=fam))
        if entry in OTHER_FAMILY:
            fam = OTHER_FAMILY[entry]
            out.append(Spec(entry, names, lambda fam=fam: debug_good(fam, mma_mode=1, stream_out=P, stream_cap=0, stream_bytes=None),
                            [F("family")], tag=fam))
    for entry, names in LISTERS.items():
        for fam in ("v1", "v2", "v3"):
            out.append(Spec(entry, "arch linears n_linear " + names,
                            lambda fam=fam, names=names: debug_good(fam, **dict(zip(names.split(), (P, 0, None)))),
                            [F("null", linears=None), F("linears", linears=bad_linears(fam)), F("plan", arch__n_layers=17), F("cap", cap=0)], tag=fam))
    return out


def host_specs():
    S = Spec
    cam = lambda **kw: dict(H=8, W=8, focal=8.0, c2w=c2w(), ray_begin=0, ray_end=64, **kw)
    loss4 = lambda: dict(loss=L.loss_opts(1.0, 1e-4, 0.0, None, 0.1, P, 3))
    reg = lambda: dict(reg=L.ray_reg(0.1, 0.25, 0.1, 4))
    patch = lambda: dict(patch=L.patch_reg(0.1, 4, 2), patch_terms=P)
    info = lambda: dict(info=L.info_reg(0.1, 0.01, 0.1), info_terms=P)
    lb_tail = dict(pred=P, **DOUT_GOOD, ray_terms=P, zero_buf=P, zero_n=4, stream=None)
    LB = COMP + " target loss"
    LBT = " pred " + DOUT + " ray_terms zero_buf zero_n stream"
    arch1, arr1, n1, _ = NETS["v1"]
    out = [
        S("nrf_model_create", "out device arch linears n_linear",
          lambda: dict(out=C.c_void_p(), device=0, arch=L.nrf_arch.from_buffer_copy(arch1), linears=arr1, n_linear=n1),
          [F("null", out=None), F("null_count", alt=True, n_linear=0), F("linears", linears=bad_linears("v1")), F("plan", arch__pos_freq=16)]),
        S("nrf_model_update", "m linears n_linear stream", lambda: dict(m=MODEL, linears=arr1, n_linear=n1, stream=None), [F("model", m=None)]),
        S("nrf_model_flops_per_sample", "m", lambda: dict(m=MODEL), [F("model", m=None)]),
        S("nrf_param_count", "m", lambda: dict(m=MODEL), [F("model", m=None)]),
        S("nrf_model_update_device", "m flat_params mode_mask stream", lambda: dict(m=MODEL, flat_params=P, mode_mask=1, stream=None),
          [F("model", m=None), F("params", flat_params=None), F("mode_mask", final=True, mode_mask=0), F("mode_mask_high", alt=True, final=True, mode_mask=16)],
          fam="v2", tag="v2", safe="mode_mask"),
        S("nrf_model_set_freq_mask", "m pos_scale dir_scale", lambda: dict(m=MODEL, pos_scale=fa(*[1.0] * 9), dir_scale=None),
          [F("model", m=None), F("v1_dir", dir_scale=fa(*[1.0] * 9)), F("scales", final=True, pos_scale__3=1.5),
           F("scales_nan", alt=True, final=True, pos_scale__0=float("nan"))], fam="v1", tag="v1", safe="scales"),
        S("nrf_model_get_freq_mask", "m pos_scale dir_scale active", lambda: dict(m=MODEL, pos_scale=None, dir_scale=None, active=None),
          [F("model", m=None)]),
        S("nrf_train_context_bytes", "m mma_mode n", lambda: dict(m=MODEL, mma_mode=1, n=64),
          [F("model", m=None), F("mode", final=True, mma_mode=3), F("n", alt=True, final=True, n=-1)], fam="v1", tag="v1", safe="mode"),
        S("nrf_render_tail_bytes", "n_rays", lambda: dict(n_rays=64), [F("n_rays", n_rays=-1)]),
        S("nrf_occupancy_pack", "density n_cells k threshold bits stream", lambda: dict(density=P, n_cells=64, k=2, threshold=0.5, bits=P, stream=None),
          [F("sizes", k=0), F("cells", alt=True, n_cells=33), F("zero", n_cells=0), F("null", bits=None)]),
        S("nrf_occupancy_dilate", "bits_in res bits_out stream", lambda: dict(bits_in=P, res=ia(32, 8, 8), bits_out=P + 64, stream=None),
          [F("null", bits_in=None), F("same", alt=True, bits_out=P), F("null_res", alt=True, res=None), F("res", res__2=513), F("res0", res__0=16)]),
        S("nrf_occupancy_mark_rays", "rays_o rays_d n_rays n_samples z_vals weights res lo scale weight_threshold seen_eps hit_bits seen_bits stream",
          lambda: dict(rays_o=P, rays_d=P, n_rays=16, n_samples=4, z_vals=P, weights=P, **BOX_GOOD()),
          [F("n_rays", n_rays=-1), F("large", n_rays=1 << 31), *MARK_F("rays"), F("null_rays", rays_d=None), F("zero", n_rays=0)]),
        S("nrf_occupancy_mark_camera", "H W focal c2w ray_begin ray_end n_samples z_vals weights res lo scale weight_threshold seen_eps hit_bits seen_bits stream",
          lambda: dict(**cam(), n_samples=4, z_vals=P, weights=P, **BOX_GOOD()),
          [*CAM_F, F("large", H=1 << 16, W=1 << 16, ray_end=1 << 31), *MARK_F("camera"), F("zero", ray_end=0)]),
        S("nrf_get_rays", "H W focal c2w ray_begin ray_end rays_o rays_d stream", lambda: cam(rays_o=P, rays_d=P, stream=None),
          [*CAM_F, F("null", rays_o=None)]),
        S("nrf_sample_along_rays", "rays_o rays_d n_rays near far n_samples lindisp perturb t_rand z_ladder rng_seed pts z_vals stream",
          lambda: dict(rays_o=P, rays_d=P, n_rays=16, near=2.0, far=6.0, n_samples=4, lindisp=0, perturb=0, t_rand=None, z_ladder=None, rng_seed=1, pts=P,
                       z_vals=P, stream=None),
          [F("sizes", n_samples=0), F("zero", n_rays=0), F("null", pts=None, z_vals=None)]),
        S("nrf_encode", "x n dim num_freqs include_input freq_bands out stream",
          lambda: dict(x=P, n=16, dim=3, num_freqs=4, include_input=1, freq_bands=None, out=P, stream=None),
          [F("sizes", num_freqs=32), F("zero", n=0), F("null", out=None)]),
        S("nrf_composite", COMP + " out_rgb out_depth out_weights stream", lambda: dict(**COMP_GOOD, out_rgb=P, out_depth=None, out_weights=None, stream=None),
          [F("sizes", n_samples=0), F("strides", rgb_stride=2), F("zero", n_rays=0), F("null", out_rgb=None)]),
        S("nrf_composite_backward", COMP + " g_rgb g_depth g_weights " + DOUT + " stream",
          lambda: dict(**COMP_GOOD, g_rgb=P, g_depth=None, g_weights=None, **DOUT_GOOD, stream=None),
          [F("sizes", n_samples=4097), F("strides", d_rgb_stride=2), F("zero", n_rays=0), F("null", d_sigma=None), F("no_gradient", g_rgb=None)]),
        S("nrf_composite_backward_geom", COMP + " g_rgb g_depth g_weights " + DOUT + " d_z d_rays_d stream",
          lambda: dict(**COMP_GOOD, g_rgb=P, g_depth=None, g_weights=None, **DOUT_GOOD, d_z=P, d_rays_d=P, stream=None),
          [F("sizes", n_rays=-1), F("strides", sigma_stride=0), F("zero", n_rays=0), F("null", d_z=None), F("no_gradient", g_rgb=None)]),
        S("nrf_ray_grad", "d_points d_dirs z_vals rays_d d_z_in d_rays_d_in n_rays n_samples d_rays_o d_rays_d d_z_out stream",
          lambda: dict(d_points=P, d_dirs=None, z_vals=P, rays_d=P, d_z_in=None, d_rays_d_in=None, n_rays=16, n_samples=4, d_rays_o=P, d_rays_d=None,
                       d_z_out=None, stream=None),
          [F("sizes", n_samples=0), F("zero", n_rays=0), F("null", d_points=None), F("no_output", d_rays_o=None)]),
        S("nrf_mse_grad", "pred target n weight g_pred loss stream", lambda: dict(pred=P, target=P, n=64, weight=1.0, g_pred=P, loss=P, stream=None),
          [F("n", n=0), F("n_high", alt=True, n=(1 << 22) + 1), F("null", loss=None)]),
        S("nrf_composite_mse_backward", COMP + " target weight pred " + DOUT + " ray_loss zero_buf zero_n stream",
          lambda: dict(**COMP_GOOD, target=P, weight=1.0, pred=None, **DOUT_GOOD, ray_loss=P, zero_buf=P, zero_n=4, stream=None),
          [F("sizes", n_rays=0), F("strides", rgb_stride=2), F("null", target=None), F("zero_buf", zero_buf=None), F("zero_n", alt=True, zero_n=-1)]),
        S("nrf_adam_step", ADAM + " stream", lambda: dict(**ADAM_GOOD, stream=None),
          [F("n_step", step=0), F("zero", n=0), F("null", grads=None), F("constants", beta1=1.0), F("constants_eps", alt=True, eps=float("nan"))]),
        S("nrf_adam_step_loss", ADAM + " ray_loss n_rays loss_weight loss stream",
          lambda: dict(**ADAM_GOOD, ray_loss=P, n_rays=16, loss_weight=1.0, loss=P, stream=None),
          [F("n_step", n=0), F("null", exp_avg=None), F("constants", beta2=-0.5), F("ray_loss", n_rays=0)]),
        S("nrf_adamw_step_loss", ADAM + " decoupled max_norm sqnorm_partials grad_norm ray_terms n_rays n_samples rgb_weight depth_weight reg_weight losses stream",
          lambda: dict(**ADAM_GOOD, decoupled=1, max_norm=0.0, sqnorm_partials=None, grad_norm=None, ray_terms=P, n_rays=16, n_samples=4, rgb_weight=1.0,
                       depth_weight=0.0, reg_weight=0.0, losses=P, stream=None),
          [F("n_step", step=0), F("null", params=None), F("constants", eps=-1.0), F("max_norm_nan", alt=True, max_norm=float("nan")),
           F("max_norm", max_norm=1.0), F("grad_norm", grad_norm=P), F("together", losses=None), F("rays", n_samples=0), F("weights", depth_weight=-1.0)]),
        S("nrf_composite_loss_backward", LB + LBT, lambda: dict(**COMP_GOOD, target=P, **loss4(), **lb_tail), LAUNCH_F()),
        S("nrf_composite_loss_backward_indexed", LB + " slot" + LBT, lambda: dict(**COMP_GOOD, target=P, **loss4(), slot=P, **lb_tail),
          [F("slot", slot=None), F("slot_align", slot=OFF4), *LAUNCH_F()]),
        S("nrf_composite_reg_loss_backward", LB + " reg slot" + LBT, lambda: dict(**COMP_GOOD, target=P, **loss4(), **reg(), slot=None, **lb_tail),
          [*REG_F, F("slot_align", slot=OFF4), *LAUNCH_F()]),
        S("nrf_ray_terms_finish", "ray_terms n_rays reg losses4 losses6 stream", lambda: dict(ray_terms=P, n_rays=16, **reg(), losses4=P, losses6=P, stream=None),
          [*REG_F, F("sizes", n_rays=0), F("null", losses6=None)]),
        S("nrf_composite_patch_loss_backward", LB + " reg slot" + LBT + " patch patch_terms patch_depth",
          lambda: dict(**COMP_GOOD, target=P, **loss4(), **reg(), slot=None, **lb_tail, **patch(), patch_depth=None),
          [*REG_F, *PATCH_F, F("patch_terms", patch_terms=None), F("slot_align", slot=OFF4), *LAUNCH_F()]),
        S("nrf_patch_terms_finish", "ray_terms n_rays n_samples loss reg patch patch_terms losses7 stream",
          lambda: dict(ray_terms=P, n_rays=64, n_samples=8, **loss4(), **reg(), **patch(), losses7=P, stream=None),
          [*REG_F, *PATCH_F, *loss_chain("finish"), F("sizes", n_samples=0), F("null", losses7=None), F("null_patch_terms", alt=True, patch_terms=None)]),
        S("nrf_composite_info_loss_backward", LB + " reg slot" + LBT + " patch patch_terms patch_depth info info_terms patch_kl",
          lambda: dict(**COMP_GOOD, target=P, **loss4(), **reg(), slot=None, **lb_tail, **patch(), patch_depth=None, **info(), patch_kl=P),
          [*REG_F, *PATCH_F, *INFO_F, F("patch_terms", patch_terms=None), F("info_terms", info_terms=None), F("patch_kl", patch_kl=None),
           F("slot_align", slot=OFF4), *LAUNCH_F(**TOO_MANY_RAYS)]),
        S("nrf_info_terms_finish", "ray_terms n_rays n_samples loss reg patch patch_terms info info_terms patch_kl losses9 stream",
          lambda: dict(ray_terms=P, n_rays=64, n_samples=8, **loss4(), **reg(), **patch(), **info(), patch_kl=P, losses9=P, stream=None),
          [*REG_F, *PATCH_F, *INFO_F, *loss_chain("finish"), F("sizes", **TOO_MANY_RAYS), F("null", patch_kl=None), F("null_info_terms", alt=True, info_terms=None)]),
        S("nrf_hier_train_workspace_bytes", "n_rays n_samples n_importance", lambda: dict(n_rays=16, n_samples=8, n_importance=4),
          [F("sizes", n_samples=4000, n_importance=97)]),
        S("nrf_composite_hier_loss_backward", "a n_rays n_samples n_importance stream", hier_good,
          [F("a", a=None), F("struct", a__struct_bytes=8), F("n_rays", n_rays=-1), F("n_samples", n_samples=0), F("n_importance", n_importance=0),
           F("sum", n_samples=4093), F("strides", a__rgb_stride=2), F("weights", a__w_fine=float("nan")), F("null", a__target=None),
           F("ray_loss", a__ray_loss=None), F("align", a__z_union=OFF4), F("zero_buf", a__zero_buf=None), F("workspace", a__workspace=None),
           F("workspace_align", a__workspace=OFF16), F("workspace_bytes", a__workspace_bytes=-1), F("zero", n_rays=0)]),
        S("nrf_occupancy_compact_workspace_bytes", "n_rays", lambda: dict(n_rays=16), [F("n_rays", n_rays=-1)]),
        S("nrf_grad_sqnorm_workspace_bytes", "n", lambda: dict(n=16), [F("n", n=0)]),
        S("nrf_grad_sqnorm_partials", "grads n workspace workspace_bytes stream", lambda: dict(grads=P, n=1000, workspace=P, workspace_bytes=1 << 30, stream=None),
          [F("n", n=0), F("null", grads=None), F("workspace", workspace=None), F("workspace_align", workspace=OFF4), F("workspace_bytes", workspace_bytes=3)]),
        S("nrf_hier_workspace_bytes", "n_rays n_samples n_importance", lambda: dict(n_rays=16, n_samples=8, n_importance=4), [F("sizes", n_importance=-1)]),
        S("nrf_composite_merge", "z_coarse raw_coarse z_new raw_new rays_d n_rays n_samples n_importance mma_mode white_bkgd out_rgbd rgb depth weights z_union stream",
          lambda: dict(**MERGE_GOOD, rays_d=P, n_rays=16),
          [F("rays_d", rays_d=None), *MERGE_F, F("zero", n_rays=0), *MERGE_TAIL_F]),
        S("nrf_composite_merge_camera",
          "z_coarse raw_coarse z_new raw_new H W focal c2w ray_begin ray_end n_samples n_importance mma_mode white_bkgd out_rgbd rgb depth weights z_union stream",
          lambda: dict(**MERGE_GOOD, **cam()), [*CAM_F, *MERGE_F, F("zero", ray_end=0), *MERGE_TAIL_F]),
        S("nrf_debug_ray_deal", "n_rays n_samples cols_per_wave n_cu head items cap n_items",
          lambda: dict(n_rays=1000, n_samples=8, cols_per_wave=64, n_cu=8, head=(C.c_int64 * 4)(), items=(C.c_int64 * 4)(), cap=1, n_items=C.c_int64()),
          [F("argument", cols_per_wave=48), F("head", alt=True, head=None), F("items", )]),
        S("nrf_sample_features", "features Hp Wp C points_2d n feats stream", lambda: dict(features=P, Hp=4, Wp=4, C=8, points_2d=P, n=16, feats=P, stream=None),
          [F("sizes", C=0), F("zero", n=0), F("null", feats=None)]),
        S("nrf_fetch_backward_workspace_bytes", "Hp Wp C n", lambda: dict(Hp=4, Wp=4, C=8, n=16), [F("sizes", Wp=0)]),
        S("nrf_project_fetch_backward", "dino points n d_feats d_map accumulate ws ws_bytes stream",
          lambda: dict(dino=dino(), points=P, n=16, d_feats=P, d_map=P, accumulate=0, ws=P, ws_bytes=1 << 40, stream=None),
          [F("dino", dino=None), F("dino_size", dino__W=0), F("sizes", n=-1), *FETCH_F]),
        S("nrf_sample_features_backward", "Hp Wp C points_2d n d_feats d_map accumulate ws ws_bytes stream",
          lambda: dict(Hp=4, Wp=4, C=8, points=P, points_2d=P, n=16, d_feats=P, d_map=P, accumulate=0, ws=P, ws_bytes=1 << 40, stream=None),
          [F("sizes", Hp=0), *[F(f.label, f.alt, f.final, **{k.replace("points", "points_2d"): v for k, v in f.ov.items()}) for f in FETCH_F]]),
        S("nrf_project_fetch_backward_points", "dino points n d_feats d_points accumulate stream",
          lambda: dict(dino=dino(), points=P, n=16, d_feats=P, d_points=P, accumulate=0, stream=None),
          [F("n", n=-1), F("zero", n=0), F("null", d_feats=None), F("align", d_points=OFF4), F("dino", dino=None), F("dino_features", alt=True, dino__features=None),
           F("dino_size", dino__C=0), F("features_align", dino__features=OFF4)]),
        S("nrf_sample_features_backward_points", "features Hp Wp C points_2d n d_feats d_xy stream",
          lambda: dict(features=P, Hp=4, Wp=4, C=8, points_2d=P, n=16, d_feats=P, d_xy=P, stream=None),
          [F("sizes", n=-1), F("zero", n=0), F("null", d_xy=None), F("align", features=OFF4)]),
        S("nrf_project_fetch", "dino points n feats xy stream", lambda: dict(dino=dino(), points=P, n=16, feats=P, xy=None, stream=None),
          [F("n", n=-1), F("zero", n=0), F("null", points=None), F("dino", dino=None), F("dino_size", dino__Hp=0)]),
    ]
    for sorted_ in (False, True):
        names = "z_vals weights n_rays n_samples n_importance u u_ray_stride samples " + ("samples_sorted " if sorted_ else "") + "z_union stream"
        out.append(S("nrf_sample_pdf" + ("_sorted" if sorted_ else ""), names,
                     lambda s=sorted_: dict(z_vals=P, weights=P, n_rays=16, n_samples=8, n_importance=4, u=P, u_ray_stride=4, samples=None, z_union=P, stream=None,
                                            **(dict(samples_sorted=None) if s else {})),
                     [F("sizes", n_samples=1), F("zero", n_rays=0), F("null", z_union=None), F("u_stride", u_ray_stride=3),
                      F("lds_row", n_samples=4096, n_importance=4096, u_ray_stride=4096)]))
    return out


def all_specs():
    return host_specs() + render_specs() + ray_source_specs() + train_specs() + debug_specs()


def record_host(h):
    out = {}
    for spec in all_specs():
        for name, faults in cases(spec, False):
            assert name not in out, name
            out[name] = call(h, spec, faults)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# what the debug entries write
# ------------------------------------------------------------------------------------------------------------------------------
def record_debug(h):
    """Per entry, family and mode: the sizes reported with NULL outputs, the SHA-256 of what is written, and the refusal at one
    element below the size."""
    out = {}
    sha = lambda buf: hashlib.sha256(bytes(buf)).hexdigest()
    err = lambda rc: {"rc": rc, "error": h.nrf_last_error().decode()}
    for entry, fams in PACKERS.items():
        full = entry == "nrf_debug_pack"
        for fam in fams:
            arch, arr, n, _ = NETS[fam]
            for mode in range(4 if full else 3):
                nb, nbias = C.c_int64(-1), C.c_int64(-1)
                more = lambda bo, bc, nbp: (bo, bc, nbp) if full else ()
                assert getattr(h, entry)(C.byref(arch), arr, n, mode, None, 0, C.byref(nb), *more(None, 0, C.byref(nbias))) == 0, (entry, fam, mode)
                raw, bias = (C.c_uint8 * nb.value)(), (C.c_float * max(nbias.value, 1))()
                assert getattr(h, entry)(C.byref(arch), arr, n, mode, raw, nb.value, None, *more(bias, nbias.value, None)) == 0
                rec = {"stream_bytes": nb.value, "stream": sha(raw)}
                rec["stream_short"] = err(getattr(h, entry)(C.byref(arch), arr, n, mode, raw, nb.value - 1, None, *more(None, 0, None)))
                if full:
                    rec.update(n_bias=nbias.value, bias=sha(bias), bias_short=err(h.nrf_debug_pack(C.byref(arch), arr, n, mode, None, 0, None, bias,
                                                                                                    nbias.value - 1, None)))
                out[f"{entry}[{fam},{mode}]"] = rec
    for entry, ctype in (("nrf_debug_train_plan", C.c_int32), ("nrf_debug_freq_mask_ids", C.c_int8)):
        for fam in ("v1", "v2", "v3"):
            arch, arr, n, _ = NETS[fam]
            cnt = C.c_int64(-1)
            assert getattr(h, entry)(C.byref(arch), arr, n, None, 0, C.byref(cnt)) == 0, (entry, fam)
            buf = (ctype * cnt.value)()
            assert getattr(h, entry)(C.byref(arch), arr, n, buf, cnt.value, None) == 0
            out[f"{entry}[{fam}]"] = {"count": cnt.value, "out": sha(buf), "short": err(getattr(h, entry)(C.byref(arch), arr, n, buf, cnt.value - 1, None))}
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# the golden file: every message once, and per spec one line of `label:message index` (`label:ok` for an early NRF_OK)
# ------------------------------------------------------------------------------------------------------------------------------
def pack(answers, messages):
    out = {}
    for name, rec in answers.items():
        title, label = name.split("/")
        assert rec["rc"] in (0, -1), name
        out[title] = (out[title] + " " if title in out else "") + label + ":" + ("ok" if rec["rc"] == 0 else str(messages.index(rec["error"])))
    return out


def unpack(section, messages):
    return {f"{title}/{item.split(':')[0]}": {"rc": 0} if item.endswith(":ok") else {"rc": -1, "error": messages[int(item.split(":")[1])]}
            for title, line in section.items() for item in line.split()}


def messages_of(*answer_sets):
    return sorted({rec["error"] for a in answer_sets for rec in a.values() if "error" in rec})


def dump(obj, f):
    """JSON with one line per item of each section."""
    f.write("{\n")
    for i, (key, sec) in enumerate(obj.items()):
        items = [json.dumps(v) for v in sec] if isinstance(sec, list) else [json.dumps(k) + ": " + json.dumps(v, sort_keys=True) for k, v in sec.items()]
        f.write(json.dumps(key) + ": " + "[{"[isinstance(sec, dict)] + "\n" + ",\n".join(items) + "\n" + "]}"[isinstance(sec, dict)] + ("," if i + 1 < len(obj) else "") + "\n")
    f.write("}\n")


def load_golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {"host": unpack(g["host"], g["messages"]), "gpu": unpack(g["gpu"], g["messages"]), "debug": g["debug"],
            "uncovered_at_parent": g["uncovered_at_parent"]}


def uncovered(messages):
    """The string literals of api.cpp that no recorded message contains."""
    src = open(API_CPP).read()
    src = re.sub(r"//[^\n]*", "", src)
    lits = []
    for line in src.splitlines():
        if line.lstrip().startswith("#include") or line.lstrip().startswith("extern"):
            continue
        lits += [m.encode().decode("unicode_escape") for m in re.findall(r'"((?:[^"\\]|\\.)*)"', line)]
    return sorted({s for s in lits if len(s) > 2 and not any(s in m for m in messages)})


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def lib():
    return api()


def test_every_host_case_is_the_recorded_answer(lib, golden):
    got = record_host(lib)
    assert sorted(got) == sorted(golden["host"])
    wrong = {k: (v, golden["host"][k]) for k, v in got.items() if v != golden["host"][k]}
    assert not wrong, wrong


def test_no_host_case_reached_a_launch_or_the_device(golden):
    for name, rec in golden["host"].items():
        assert rec["rc"] in (0, -1) or name.split("/")[0].endswith("_bytes") or name.startswith("nrf_model_flops") or name.startswith("nrf_param_count"), name
        assert "launch failed" not in rec.get("error", "") and "cannot select" not in rec.get("error", ""), name


def test_the_debug_entries_write_the_recorded_bytes(lib, golden):
    got = record_debug(lib)
    assert sorted(got) == sorted(golden["debug"])
    wrong = {k: (v, golden["debug"][k]) for k, v in got.items() if v != golden["debug"][k]}
    assert not wrong, wrong


def test_what_stayed_uncovered_at_the_parent_has_a_reason(golden):
    assert all(isinstance(r, str) and r for r in golden["uncovered_at_parent"].values())


if __name__ == "__main__":
    h = api()
    host, debug = record_host(h), record_debug(h)
    msgs = [r["error"] for r in host.values() if "error" in r] + [r["error"] for d in debug.values() for r in d.values() if isinstance(r, dict)]
    if os.path.exists(GOLDEN):
        msgs += [r["error"] for r in load_golden()["gpu"].values() if "error" in r]
    table = messages_of(host)
    dump({"messages": table, "host": pack(host, table), "debug": debug, "uncovered": uncovered(msgs)}, sys.stdout)
