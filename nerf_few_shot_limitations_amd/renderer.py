"""The fused render call surface: sample -> encode -> MLP -> composite in ONE
kernel launch (nrf_render_rays / nrf_render_camera).

`render_rays` replaces NeRFDINOTrainer.render_rays (src/training/train.py:188-242);
`render_full_image` replaces NeRFDINOEvaluator.render_full_image
(src/training/evaluate.py:65-81) and the eval chunk loop (train.py:305-319);
`NeRFRenderer` carries the trainer-side state those methods read from `self`
(config near/far, the model, the precomputed DINO map of view 0).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L
from .nerf_model import NeRFMLP
from .occupancy import occupancy_arg
from .ray_sampler import _c2w12


def make_dino(features, pose, focal, H, W):
    """Pack the V3 side channel: feature map (1,Hp,Wp,C) of the source view + its camera (train.py:203-214).
    Returns (nrf_dino struct, tensors that must stay alive)."""
    fm = L.dev_f32(features)
    if fm.dim() != 4 or fm.shape[0] != 1:
        raise ValueError("features must be (1,Hp,Wp,C)")
    inv = torch.inverse(torch.as_tensor(pose).detach().to("cpu", torch.float32))      # ray_utils.py:191
    d = L.nrf_dino()
    d.features = fm.data_ptr()
    d.Hp, d.Wp, d.C = int(fm.shape[1]), int(fm.shape[2]), int(fm.shape[3])
    d.inv_pose = (C.c_float * 16)(*inv.reshape(-1).tolist())
    d.focal, d.H, d.W = float(focal), int(H), int(W)
    return d, fm


def _opts(near, far, n_samples, perturb, t_rand, seed, lindisp, ert_eps, white_bkgd, mma_mode, dino, device, z_in=None):
    o = L.nrf_render_opts()
    o.near, o.far, o.n_samples, o.lindisp = float(near), float(far), int(n_samples), int(bool(lindisp))
    o.perturb = int(bool(perturb) or t_rand is not None)
    o.t_rand = t_rand.data_ptr() if t_rand is not None else None
    o.z_ladder = L.z_ladder(near, far, n_samples, lindisp, device).data_ptr()     # cached per (near, far, S, device)
    o.z_in = z_in.data_ptr() if z_in is not None else None
    if seed is None:                 # a new jitter pattern per call (ray_utils.py:78 draws torch.rand per call); repeats under torch.manual_seed
        seed = L.fresh_seed() if (o.perturb and t_rand is None) else 0
    o.rng_seed = int(seed)
    o.ert_eps, o.white_bkgd, o.mma_mode = float(ert_eps), int(bool(white_bkgd)), L.MMA_MODES[mma_mode]
    o.dino = C.pointer(dino) if dino is not None else None
    return o


def _handle(model, device, mma_mode, tail_mode):
    """The model's handle with the streams a render in `mma_mode` (+ `tail_mode`) reads brought up to date: a tail render reads
    the base mode's AND the split-f16 stream, and after a device-side re-pack only the modes asked for are current."""
    return model.handle(device, mma_mode, also=tail_mode)


def render_rays(model: NeRFMLP, rays_o, rays_d, near, far, N_samples=64, perturb=False, t_rand=None, seed=None, lindisp=False,
                ert_eps=0.0, white_bkgd=False, mma_mode: Optional[str] = None, dino=None, return_weights=True, return_z=False,
                z_in=None, tail_mode: Optional[str] = None, occupancy=None, return_stats=False):
    """Render explicit rays (R,3)/(H,W,3) -> {'rgb' (R,3), 'depth' (R,), 'weights' (R,S)[, 'z_vals' (R,S)]}.
    Under torch.no_grad() or with the model in eval() mode (evaluate, train.py:294-296) this is ONE fused kernel launch.  With
    grad enabled and the model in train() mode (train_step, train.py:245,280-287) the same call returns tensors with a grad_fn:
    the staged training kernels behind one autograd node (training.render_rays_train), so `loss.backward(); optimizer.step()`
    work on the drop-in unchanged.  (`mma_mode` selects the arithmetic on both routes; the split mode trains in exact fp32.)
    `tail_mode="f16x3"` (with a 16-bit mma_mode): every ray's last sample -- the one composited with dist = 1e10, whose opacity
    is a step function of its density -- is evaluated in split-f16; two launches.  Refused under grad (ValueError): the training
    kernels have no split mode.
    `occupancy=` (an occupancy.OccupancyGrid): samples in empty cells are stepped over and composited as density 0, on the ray-queue
    kernel (ert_eps >= 0).  `return_stats=True` adds 'stats', an int64 device tensor [evaluated (ray, sample) pairs, MLP passes of
    waves that held a live ray].  Refused with tail_mode and under grad (ValueError)."""
    L.require_gpu()
    if (model.training and model._wants_grad()) or model._wants_input_grad(rays_o, rays_d, z_in):
        if occupancy is not None:
            raise ValueError("occupancy is for inference: the differentiable route (a model in train() mode under grad) evaluates every sample")
        from .training import render_rays_train
        out = render_rays_train(model, rays_o, rays_d, near, far, N_samples, perturb=perturb, t_rand=t_rand, seed=seed, lindisp=lindisp,
                                white_bkgd=white_bkgd, dino=dino, z_in=z_in, mma_mode=mma_mode, tail_mode=tail_mode)
        if not return_weights:
            out.pop("weights")
        if not return_z:
            out.pop("z_vals")
        return out
    o = L.dev_f32(rays_o).reshape(-1, 3)
    d = L.dev_f32(rays_d, o.device).reshape(-1, 3)
    R, S = o.shape[0], int(N_samples)
    tr = L.dev_f32(t_rand, o.device).reshape(R, S) if t_rand is not None else None
    zin = L.dev_f32(z_in, o.device).reshape(R, S) if z_in is not None else None
    keep = None
    dn = None
    if model.net == L.NRF_NET_V3:
        if dino is None:
            raise ValueError("a use_dino model needs dino=dict(features=, pose=, focal=, H=, W=)")
        dn, keep = make_dino(**dino)
    opts = _opts(near, far, S, perturb, tr, seed, lindisp, ert_eps, white_bkgd, mma_mode or model.mma_mode, dn, o.device, zin)
    h = _handle(model, o.device, mma_mode or model.mma_mode, tail_mode)
    with torch.cuda.device(o.device):
        rgb = torch.empty((R, 3), dtype=torch.float32, device=o.device)
        depth = torch.empty((R,), dtype=torch.float32, device=o.device)
        w = torch.empty((R, S), dtype=torch.float32, device=o.device) if return_weights else None
        z = torch.empty((R, S), dtype=torch.float32, device=o.device) if return_z else None
        occ, stats, occ_keep = occupancy_arg(occupancy, return_stats, tail_mode, o.device)
        tail, ws = L.tail_arg(tail_mode, mma_mode or model.mma_mode, R, o.device)
        if occ is not None:
            L.check(L.lib().nrf_render_rays_occ(h, L.ptr(o), L.ptr(d), R, C.byref(opts), C.byref(occ), L.ptr(rgb), L.ptr(depth), L.ptr(w), L.ptr(z),
                                                L.stream_ptr()))
        elif tail is None:
            L.check(L.lib().nrf_render_rays(h, L.ptr(o), L.ptr(d), R, C.byref(opts), L.ptr(rgb), L.ptr(depth), L.ptr(w), L.ptr(z), L.stream_ptr()))
        else:
            L.check(L.lib().nrf_render_rays_tail(h, L.ptr(o), L.ptr(d), R, C.byref(opts), C.byref(tail), L.ptr(rgb), L.ptr(depth), L.ptr(w),
                                                 L.ptr(z), L.stream_ptr()))
    del keep
    out = {"rgb": rgb, "depth": depth}
    if w is not None:
        out["weights"] = w
    if z is not None:
        out["z_vals"] = z
    if stats is not None:
        out["stats"] = stats
    return out


def render_camera(model: NeRFMLP, H, W, focal, c2w, near, far, N_samples=64, ray_begin=0, ray_end=None, perturb=False, seed=None,
                  lindisp=False, ert_eps=0.0, white_bkgd=False, mma_mode: Optional[str] = None, dino=None, device=None,
                  out_rgb=None, out_depth=None, tail_mode: Optional[str] = None, occupancy=None, return_stats=False):
    """Render rays [ray_begin, ray_end) of an HxW pinhole camera with in-kernel ray generation
    (get_rays + render_rays of the reference, train.py:179,305-319) -> (rgb (n,3), depth (n,)).  `tail_mode`, `occupancy`: see render_rays; with
    return_stats=True the result is (rgb, depth, stats)."""
    L.require_gpu()
    H, W = int(H), int(W)
    ray_end = H * W if ray_end is None else int(ray_end)
    n = ray_end - int(ray_begin)
    if device is None:
        p = next(model.parameters())
        device = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    keep = None
    dn = None
    if model.net == L.NRF_NET_V3:
        if dino is None:
            raise ValueError("a use_dino model needs dino=...")
        dn, keep = make_dino(**dino)
    opts = _opts(near, far, N_samples, perturb, None, seed, lindisp, ert_eps, white_bkgd, mma_mode or model.mma_mode, dn, device)
    h = _handle(model, device, mma_mode or model.mma_mode, tail_mode)
    with torch.cuda.device(device):
        rgb = out_rgb if out_rgb is not None else torch.empty((n, 3), dtype=torch.float32, device=device)
        depth = out_depth if out_depth is not None else torch.empty((n,), dtype=torch.float32, device=device)
        occ, stats, occ_keep = occupancy_arg(occupancy, return_stats, tail_mode, device)
        tail, ws = L.tail_arg(tail_mode, mma_mode or model.mma_mode, n, device)
        if occ is not None:
            L.check(L.lib().nrf_render_camera_occ(h, H, W, float(focal), _c2w12(c2w), int(ray_begin), ray_end, C.byref(opts), C.byref(occ),
                                                  L.ptr(rgb), L.ptr(depth), None, None, L.stream_ptr()))
        elif tail is None:
            L.check(L.lib().nrf_render_camera(h, H, W, float(focal), _c2w12(c2w), int(ray_begin), ray_end, C.byref(opts),
                                              L.ptr(rgb), L.ptr(depth), None, None, L.stream_ptr()))
        else:
            L.check(L.lib().nrf_render_camera_tail(h, H, W, float(focal), _c2w12(c2w), int(ray_begin), ray_end, C.byref(opts), C.byref(tail),
                                                   L.ptr(rgb), L.ptr(depth), None, None, L.stream_ptr()))
    del keep
    return (rgb, depth, stats) if stats is not None else (rgb, depth)


def render_hierarchical(model: NeRFMLP, rays_o, rays_d, near, far, N_samples=128, N_importance=64, perturb=False, u=None, reuse_coarse=False,
                        **kw):
    """Coarse pass -> inverse-cdf resampling of its weights -> fine pass on the sorted union of S+Ni depths
    (BASELINE.json config 3: 128 coarse + 64 fine).  Mirrors the intent of ray_utils.py:86-143, which the
    reference never calls and which raises on every input: parity of the resampling step is
    unpinned, the two render passes are the same kernel as `render_rays`.
    Returns the fine pass' dict plus 'coarse' (the coarse pass' dict) and 'z_vals' (R, S+Ni).  A `tail_mode` applies to both
    passes (the fine pass marches its explicit depths, z_in, with the same split), and so do `occupancy` / `return_stats`.
    `reuse_coarse=True`: the fine pass evaluates the network on the Ni new depths only and composites them merged with the S
    coarse samples, whose raw network outputs the coarse pass kept (nerfhip.h: nrf_render_rays_emit, nrf_composite_merge) -- S + Ni
    network evaluations per ray instead of 2 S + Ni, the same dict bit for bit.  Inference only: with tail_mode, occupancy,
    return_stats or ert_eps > 0, or on the differentiable route (a model in train() mode under grad), it raises ValueError."""
    if reuse_coarse:
        return _render_hierarchical_reuse(model, rays_o, rays_d, near, far, N_samples, N_importance, perturb, u, **kw)
    from .ray_sampler import sample_pdf
    coarse = render_rays(model, rays_o, rays_d, near, far, N_samples, perturb=perturb, return_weights=True, return_z=True, **kw)
    if u is None and perturb:
        u = torch.rand((coarse["weights"].shape[0], int(N_importance)), device=coarse["weights"].device)
    _, union = sample_pdf(coarse["z_vals"], coarse["weights"], N_importance, u=u)
    kw.pop("t_rand", None)
    fine = render_rays(model, rays_o, rays_d, near, far, N_samples + int(N_importance), z_in=union, return_weights=True, **kw)
    fine["coarse"] = coarse
    fine["z_vals"] = union
    return fine


def _refuse_reuse(tail_mode, occupancy, return_stats, ert_eps):
    """What the coarse-reusing hierarchical routes do not take (there is no silent fallback to the three-call route)."""
    for name, on in (("tail_mode", tail_mode is not None), ("occupancy", occupancy is not None), ("return_stats", bool(return_stats)),
                     ("ert_eps > 0", float(ert_eps) > 0.0)):
        if on:
            raise ValueError(f"the coarse-reusing hierarchical render takes no {name}: every sample of both passes is evaluated once, by the "
                             "plain march (use render_hierarchical without reuse_coarse)")


def render_rays_emit(model: NeRFMLP, rays_o, rays_d, near, far, N_samples=64, perturb=False, t_rand=None, seed=None, lindisp=False,
                     white_bkgd=False, mma_mode: Optional[str] = None, dino=None, z_in=None, raw_only=False):
    """render_rays' fused launch (inference, ert_eps = 0) that also keeps every sample's raw head outputs: the same 'rgb', 'depth',
    'weights', 'z_vals' bits plus 'raw4' (R,S,4) = [r, g, b before the sigmoid, density before the ReLU] (nerfhip.h:
    nrf_render_rays_emit).  raw_only=True: {'raw4'} alone -- the fine stage of the coarse-reusing hierarchical render."""
    L.require_gpu()
    o = L.dev_f32(rays_o).reshape(-1, 3)
    d = L.dev_f32(rays_d, o.device).reshape(-1, 3)
    R, S, dev = o.shape[0], int(N_samples), o.device
    mode = mma_mode or model.mma_mode
    tr = L.dev_f32(t_rand, dev).reshape(R, S) if t_rand is not None else None
    zin = L.dev_f32(z_in, dev).reshape(R, S) if z_in is not None else None
    keep = dn = None
    if model.net == L.NRF_NET_V3:
        if dino is None:
            raise ValueError("a use_dino model needs dino=dict(features=, pose=, focal=, H=, W=)")
        dn, keep = make_dino(**dino)
    opts = _opts(near, far, S, perturb, tr, seed, lindisp, 0.0, white_bkgd, mode, dn, dev, zin)
    h = _handle(model, dev, mode, None)
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        out = {} if raw_only else {"rgb": torch.empty((R, 3), **f32), "depth": torch.empty((R,), **f32), "weights": torch.empty((R, S), **f32),
                                   "z_vals": torch.empty((R, S), **f32)}
        raw4 = torch.empty((R, S, 4), **f32)
        L.check(L.lib().nrf_render_rays_emit(h, L.ptr(o), L.ptr(d), R, C.byref(opts), L.ptr(out.get("rgb")), L.ptr(out.get("depth")),
                                             L.ptr(out.get("weights")), L.ptr(out.get("z_vals")), L.ptr(raw4), int(bool(raw_only)), L.stream_ptr()))
    del keep
    out["raw4"] = raw4
    return out


def composite_merge(z_coarse, raw_coarse, rays_d, z_new=None, raw_new=None, mma_mode="f32", white_bkgd=False):
    """The merging compositor (nerfhip.h: nrf_composite_merge) on kept rows: z_coarse (R,S) and raw_coarse (R,S,4) of an emitting
    render, optionally the ascending new depths z_new (R,Ni) and their rows, rays_d (R,3) -> {'rgb', 'depth', 'weights' (R,S+Ni),
    'z_vals' (R,S+Ni)}.  `mma_mode`: the mode that emitted the rows.  Without new samples it composites the coarse rows alone."""
    L.require_gpu()
    zc = L.dev_f32(z_coarse)
    dev = zc.device
    R, S = zc.shape
    rc = L.dev_f32(raw_coarse, dev).reshape(R, S, 4)
    d = L.dev_f32(rays_d, dev).reshape(R, 3)
    Ni = 0 if z_new is None else int(z_new.shape[-1])
    zn = L.dev_f32(z_new, dev).reshape(R, Ni) if Ni else None
    rn = L.dev_f32(raw_new, dev).reshape(R, Ni, 4) if Ni else None
    with torch.cuda.device(dev):
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"rgb": torch.empty((R, 3), **f32), "depth": torch.empty((R,), **f32), "weights": torch.empty((R, S + Ni), **f32),
               "z_vals": torch.empty((R, S + Ni), **f32)}
        L.check(L.lib().nrf_composite_merge(L.ptr(zc), L.ptr(rc), L.ptr(zn), L.ptr(rn), L.ptr(d), R, S, Ni, L.MMA_MODES[mma_mode],
                                            int(bool(white_bkgd)), 0, L.ptr(out["rgb"]), L.ptr(out["depth"]), L.ptr(out["weights"]),
                                            L.ptr(out["z_vals"]), L.stream_ptr()))
    return out


def _render_hierarchical_reuse(model, rays_o, rays_d, near, far, N_samples, N_importance, perturb, u, t_rand=None, seed=None, lindisp=False,
                               ert_eps=0.0, white_bkgd=False, mma_mode=None, dino=None, tail_mode=None, occupancy=None, return_stats=False):
    from .ray_sampler import sample_pdf_sorted
    L.require_gpu()
    _refuse_reuse(tail_mode, occupancy, return_stats, ert_eps)
    if (model.training and model._wants_grad()) or model._wants_input_grad(rays_o, rays_d):
        raise ValueError("reuse_coarse=True is for inference: the differentiable route (a model in train() mode under grad) renders both passes whole")
    Ni = int(N_importance)
    if Ni < 1:
        raise ValueError("N_importance must be >= 1")
    o = L.dev_f32(rays_o).reshape(-1, 3)
    d = L.dev_f32(rays_d, o.device).reshape(-1, 3)
    mode = mma_mode or model.mma_mode
    kw = dict(lindisp=lindisp, white_bkgd=white_bkgd, mma_mode=mode, dino=dino)
    coarse = render_rays_emit(model, o, d, near, far, N_samples, perturb=perturb, t_rand=t_rand, seed=seed, **kw)
    raw_c = coarse.pop("raw4")
    if u is None and perturb:
        u = torch.rand((o.shape[0], Ni), device=o.device)
    z_new = sample_pdf_sorted(coarse["z_vals"], coarse["weights"], Ni, u=u)
    raw_n = render_rays_emit(model, o, d, near, far, Ni, z_in=z_new, raw_only=True, **kw)["raw4"]
    fine = composite_merge(coarse["z_vals"], raw_c, d, z_new, raw_n, mma_mode=mode, white_bkgd=white_bkgd)
    fine["coarse"] = coarse
    return fine


def render_camera_hierarchical(model: NeRFMLP, H, W, focal, c2w, near, far, N_samples=128, N_importance=64, ray_begin=0, ray_end=None,
                               chunk_rays=1 << 15, perturb=False, seed=None, lindisp=False, white_bkgd=False, mma_mode: Optional[str] = None,
                               dino=None, out_rgb=None, out_depth=None):
    """Hierarchical render (coarse pass -> inverse-cdf resampling -> fine pass on the sorted union) of rays [ray_begin, ray_end) of an
    HxW pinhole camera -> (rgb (n,3), depth (n,)): the fine image of render_hierarchical(reuse_coarse=True) on get_rays of the camera,
    bit for bit, with the rays generated in-kernel and nothing of frame x samples size held.  The frame is marched in ray ranges of
    `chunk_rays`; each range is four launches (emitting coarse render, resampling, emitting render of the Ni new depths, merging
    compositor) through ONE workspace, cached on the model's device and reused by every range:
        bytes per ray = S * (4 + 4 + 16) + Ni * (4 + 16)      (coarse depths, weights, raw rows; new depths, raw rows)
    i.e. 4 352 B at 128 + 64, 143 MB at the default range of 32 768 rays.  The inverse-cdf arguments `u` are the shared
    linspace(0, 1, Ni) row.  `perturb=True` jitters the coarse ladder through the counter RNG, keyed by the global ray id: the image
    does not depend on the cut into ranges (seed=None: a fresh seed per call).  No tail_mode, occupancy or early termination."""
    from .ray_sampler import sample_pdf_sorted
    L.require_gpu()
    H, W, S, Ni = int(H), int(W), int(N_samples), int(N_importance)
    if Ni < 1:
        raise ValueError("N_importance must be >= 1")
    chunk = int(chunk_rays)
    if chunk < 1:
        raise ValueError("chunk_rays must be >= 1")
    ray_begin = int(ray_begin)
    ray_end = H * W if ray_end is None else int(ray_end)
    n = ray_end - ray_begin
    p = next(model.parameters())
    dev = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
    mode = mma_mode or model.mma_mode
    keep = dn = None
    if model.net == L.NRF_NET_V3:
        if dino is None:
            raise ValueError("a use_dino model needs dino=...")
        dn, keep = make_dino(**dino)
    if seed is None:                     # ONE jitter pattern for the frame, not one per range
        seed = L.fresh_seed() if perturb else 0
    h = _handle(model, dev, mode, None)
    c2w12 = _c2w12(c2w)
    with torch.cuda.device(dev):
        rgb = out_rgb if out_rgb is not None else torch.empty((n, 3), dtype=torch.float32, device=dev)
        depth = out_depth if out_depth is not None else torch.empty((n,), dtype=torch.float32, device=dev)
        ws = L.hier_workspace(min(chunk, max(n, 1)), S, Ni, dev)
        lib, st = L.lib(), L.stream_ptr()
        for b in range(ray_begin, ray_end, chunk):
            e = min(b + chunk, ray_end)
            m = e - b
            # the 16-byte rows first: every piece starts 16-byte aligned
            cut = [0, 4 * m * S, 4 * m * Ni, m * S, m * S, m * Ni]
            for i in range(1, len(cut)):
                cut[i] += cut[i - 1]
            raw_c, raw_n, z_c, w_c, z_n = (ws[cut[i]:cut[i + 1]] for i in range(5))
            z_c, w_c, z_n = z_c.view(m, S), w_c.view(m, S), z_n.view(m, Ni)
            o_rgb, o_depth = rgb[b - ray_begin:e - ray_begin], depth[b - ray_begin:e - ray_begin]
            opts = _opts(near, far, S, perturb, None, seed, lindisp, 0.0, white_bkgd, mode, dn, dev)
            # (the coarse image lands in the output rows and is overwritten by the merge)
            L.check(lib.nrf_render_camera_emit(h, H, W, float(focal), c2w12, b, e, C.byref(opts), L.ptr(o_rgb), L.ptr(o_depth), L.ptr(w_c),
                                               L.ptr(z_c), L.ptr(raw_c), 0, st))
            sample_pdf_sorted(z_c, w_c, Ni, out=z_n)
            opts_n = _opts(near, far, Ni, False, None, seed, lindisp, 0.0, white_bkgd, mode, dn, dev, z_n)
            L.check(lib.nrf_render_camera_emit(h, H, W, float(focal), c2w12, b, e, C.byref(opts_n), None, None, None, None, L.ptr(raw_n), 1, st))
            L.check(lib.nrf_composite_merge_camera(L.ptr(z_c), L.ptr(raw_c), L.ptr(z_n), L.ptr(raw_n), H, W, float(focal), c2w12, b, e, S, Ni,
                                                   L.MMA_MODES[mode], int(bool(white_bkgd)), 0, L.ptr(o_rgb), L.ptr(o_depth), None, None, st))
    del keep
    return rgb, depth


class NeRFRenderer:
    """Trainer-shaped wrapper: `render_rays(rays_o, rays_d, view_idx, N_samples=64)` and
    `render_full_image(rays_o, rays_d, closest_view_idx, chunk_size=1024)` with the
    signatures of train.py:188 and evaluate.py:65.  `chunk_size` is accepted and
    ignored: the fused kernel never materialises (rays x samples) intermediates."""

    def __init__(self, model: NeRFMLP, near, far, white_bkgd=False, mma_mode=None, ert_eps=0.0,
                 dino_features=None, poses=None, focal=None, H=None, W=None, tail_mode=None, occupancy=None):
        self.nerf_model, self.near, self.far = model, float(near), float(far)
        self.white_bkgd, self.mma_mode, self.ert_eps, self.tail_mode = white_bkgd, mma_mode, ert_eps, tail_mode
        self.occupancy = occupancy           # an OccupancyGrid (V3: of the source view evaluation renders from, view 0); used outside training only
        self.dino_features_precomputed, self.poses, self.focal, self.H, self.W = dino_features, poses, focal, H, W

    def _dino(self, view_idx):
        if self.nerf_model.net != L.NRF_NET_V3:
            return None
        idx = view_idx if self.nerf_model.training else 0          # train.py:203-208
        return dict(features=self.dino_features_precomputed[idx], pose=self.poses[idx], focal=self.focal, H=self.H, W=self.W)

    def render_rays(self, rays_o, rays_d, view_idx=0, N_samples=64):
        """train.py:188: differentiable under grad mode (train_step), the fused kernel under torch.no_grad() (evaluate)."""
        return render_rays(self.nerf_model, rays_o, rays_d, self.near, self.far, N_samples,
                           perturb=self.nerf_model.training, white_bkgd=self.white_bkgd, mma_mode=self.mma_mode,
                           ert_eps=self.ert_eps, dino=self._dino(view_idx), tail_mode=self.tail_mode,
                           occupancy=None if ((self.nerf_model.training and self.nerf_model._wants_grad())
                                              or self.nerf_model._wants_input_grad(rays_o, rays_d)) else self.occupancy)

    @torch.no_grad()
    def render_full_image(self, rays_o, rays_d, closest_view_idx=0, chunk_size=1024, N_samples=64):
        H, W = rays_o.shape[:2]
        out = self.render_rays(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), closest_view_idx, N_samples)
        return out["rgb"].reshape(H, W, 3).cpu().numpy()
