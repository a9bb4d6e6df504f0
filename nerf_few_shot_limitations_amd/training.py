"""The training path: what `loss.backward()` / `optimizer.step()` of the reference's loops
(src/training/train_minimal.py:80-127, src/training/train.py:244-292) run through on the GPU.

  * `mlp_v1_train`, `mlp_v2_train`   NeRFMLP.forward with grad enabled: libnerfhip's forward that saves
                     every layer's operand tiles, and a backward made of the transposed weight-stream
                     chain + MFMA weight-gradient kernel (csrc/train_impl.hpp);
  * `composite`      nerf_mlp.VolumeRenderer / volume_render_radiance with grad enabled;
  * `FlatParams`     the module's parameters as views into one flat fp32 vector, so that an
                     optimizer step is visible to the kernels without leaving the device;
  * `Adam`           torch.optim.Adam's update as one kernel on the flat vectors (train.py:113-118); optionally torch.optim.AdamW's
                     decoupled decay and clip_grad_norm_ without its host read-back (train_multiscale.py:259-266);
  * `FusedStep`      the whole optimisation step of the reference's loop as a fixed sequence of library calls: train.py's
                     (rgb_weight * mse, Adam) or train_multiscale.py's (density noise, nerf_mlp.NeRFLoss, clipping, AdamW);
  * `all_reduce_gradients`   data-parallel training: ONE collective per step on the flat gradient vector.

Each launch sequence is written once: module-level helpers (_context .. _render_backward) and FusedStep's _launch_loss / _finish.

There is no PyTorch fallback: without libnerfhip.so / a gfx950 GPU every call raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import torch

from . import _lib as L


# ---------------------------------------------------------------------------------------------
# flat parameter storage
# ---------------------------------------------------------------------------------------------
class FlatParams:
    """Parameters of `module.linears()` (weight, bias per Linear, state_dict order == include/nerfhip.h's flat
    layout) re-homed as views into one contiguous fp32 device vector.  The nn.Parameter objects stay the same
    (optimizers keep working); only their storage moves."""

    def __init__(self, module):
        self.module = module
        self.flat = None
        self.offsets = []

    def params(self):
        # looked up on every call: Module.to() across device types REPLACES the nn.Parameter objects (a cached list would keep
        # feeding the old ones to autograd); the registry dicts are read directly, nn.Module.__getattr__ is the slow path
        return [m._parameters[k] for m in self.module.linears() for k in ("weight", "bias")]

    def ensure(self):
        ps = self.params()
        dev = ps[0].device
        if not ps[0].is_cuda:
            raise RuntimeError("training runs on the GPU: move the module with .to('cuda') first")
        if self.flat is not None and self.flat.device == dev:
            base = self.flat.data_ptr()
            if all(p.data_ptr() == base + 4 * off and p.dtype == torch.float32 for p, off in zip(ps, self.offsets)):
                return self.flat
        total = sum(p.numel() for p in ps)
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        offsets, off = [], 0
        with torch.no_grad():
            for p in ps:
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1).to(torch.float32))
                p.data = flat[off:off + n].view(p.shape)
                offsets.append(off)
                off += n
        self.flat, self.offsets = flat, offsets
        return flat

    def views(self, vec):
        """Per-parameter views of another flat vector of the same layout (gradients, Adam moments)."""
        return [vec[off:off + p.numel()].view(p.shape) for p, off in zip(self.params(), self.offsets)]


def _grad_target(module):
    """Where a backward should accumulate: (flat vector, attach).  The gradients live in ONE persistent flat vector whose
    per-parameter views are the parameters' .grad, so the kernels add into it directly and autograd's per-parameter
    AccumulateGrad (20+ tensors cloned and added per step) is bypassed.  Cases:
      * every .grad is None (after zero_grad(set_to_none=True)): zero the vector, attach the views;
      * every .grad already is our view: accumulate (two backward calls before a step add up, as in torch);
      * anything else (someone else produced some .grad): return None -- the caller falls back to handing autograd
        ordinary gradient tensors."""
    fp = module.flat_params()
    ps = fp.params()
    flat = fp.flat
    fg = getattr(module, "_flat_grad", None)
    if fg is None or fg.shape != flat.shape or fg.device != flat.device:
        fg = module._flat_grad = torch.zeros_like(flat)
        module._flat_grad_views = fp.views(fg)
    grads = [p.grad for p in ps]
    base = fg.data_ptr()
    if all(g is None for g in grads):
        fg.zero_()
        # the view objects handed out earlier ARE the old .grad tensors: Module.to() re-homes a parameter's .grad in place
        # (same Python object, new storage), after which they no longer alias the flat vector -- check before re-use
        views = module._flat_grad_views
        if any(v.data_ptr() != base + 4 * off for v, off in zip(views, fp.offsets)):
            views = module._flat_grad_views = fp.views(fg)
        for p, v in zip(ps, views):
            p.grad = v
        return fg
    if all(g is not None and g.data_ptr() == base + 4 * off and g.shape == p.shape for g, p, off in zip(grads, ps, fp.offsets)):
        return fg
    return None


def _context_bytes(h, mode, n):
    """Bytes of the context a saving forward over n rows fills (call with the device current)."""
    nbytes = L.lib().nrf_train_context_bytes(h, mode, n)
    if nbytes < 0:
        raise L.NrfError(-2, L.lib().nrf_last_error().decode("utf-8", "replace"))
    return nbytes


def _context(h, mode, n, dev):
    """(buffer, nbytes): the context of a saving forward over n rows, allocated (call with the device current)."""
    nbytes = _context_bytes(h, mode, n)
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev), nbytes


def _heads(o4, n, v1):
    """The two heads inside an (n,4) buffer of network outputs (or of their gradients) and the compositor's (ptr, stride, ptr, stride)
    for them.  V1: [r,g,b,sigma] rows, read strided -- (o4, None, args).  V2/V3: rgb (n,3) | density (n,1) packed in the same storage,
    which is not strided: two plain tensors as views -- (rgb, density, args)."""
    if v1:
        return o4, None, (L.ptr(o4), 4, C.c_void_p(o4.data_ptr() + 12), 4)
    rgb, den = o4.view(-1)[:3 * n].view(n, 3), o4.view(-1)[3 * n:].view(n, 1)
    return rgb, den, (L.ptr(rgb), 3, L.ptr(den), 1)


def _addr(p):
    """A device address as an int: _heads hands the V1 density pointer out as a c_void_p, a ctypes struct field takes an int."""
    return p.value if isinstance(p, C.c_void_p) else p


def _prep(g):
    """An incoming gradient as the kernels read it; None (an unused output) stays None."""
    return None if g is None else g.to(torch.float32).contiguous()


def _param_grad_target(module, wanted=True):
    """(the flat vector a backward's weight-gradient kernels add into, what that backward returns for its *params slots).
    wanted=False (frozen parameters: an input-gradient backward) and a module whose .grad tensors are not ours (_grad_target: None)
    get a zeroed scratch vector; only the latter hands its per-parameter views to autograd.  Otherwise the kernels accumulate
    into the parameters' .grad directly and autograd is handed nothing."""
    fp = module.flat_params()
    direct = _grad_target(module) if wanted else None
    if direct is not None:
        return direct, (None,) * len(fp.offsets)           # already accumulated into the parameters' .grad
    grad = torch.zeros_like(fp.flat)
    return grad, (tuple(fp.views(grad)) if wanted else (None,) * len(fp.offsets))


def _train_handle(module, dev, mma_mode=None):
    """nrf_model* with forward AND backward streams matching the current parameter values."""
    module.flat_params().ensure()
    train_mode = L.TRAIN_MODE[mma_mode or module.mma_mode]
    h = module.handle(dev, train_mode)
    mode = L.MMA_MODES[train_mode]
    if not module._train_ready:
        # first use: build the backward plan, then pack both directions from the flat vector
        with torch.cuda.device(dev):
            _context_bytes(h, mode, 1)
            L.check(L.lib().nrf_model_update_device(h, L.ptr(module.flat_params().flat), 1 << mode, L.stream_ptr()))
        module._train_ready = True
        module._packed, module._packed_modes = module._versions(), {mode}
        module._bwd_modes = {mode}       # (nerf_model.handle: the modes whose backward weights a later re-pack must not leave stale)
    return h, mode


def _dino_grad(module, mode, n, buf, nbytes, dev, out=None):
    """dL/d (per-sample DINO features) (n, C) of a V3 module, from the context of a finished nrf_mlp_backward (one launch)."""
    d_dino = out if out is not None else torch.empty((n, module.dino_dim), dtype=torch.float32, device=dev)
    L.check(L.lib().nrf_mlp_backward_dino(module._handle, mode, n, C.c_void_p(buf.data_ptr()), nbytes, L.ptr(d_dino), L.stream_ptr()))
    return d_dino


def _live_input(module, t, what, device=None):
    """An input of the field as the kernels read it.  A tensor that requires grad stays in the graph on a module built with
    input_grad=True (use_dino form: point_grad=True) and is refused otherwise (_lib.refuse_grad)."""
    if (torch.is_grad_enabled() and isinstance(t, torch.Tensor) and t.requires_grad
            and (getattr(module, "input_grad", False) or getattr(module, "point_grad", False))):
        if device is None:
            device = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return t.to(device=device, dtype=torch.float32).contiguous()
    return L.dev_f32(L.refuse_grad(t, what), device)


def _input_grad(module, mode, n, buf, nbytes, dev, positions=None, directions=None, want_x=False, want_p=False, want_d=False):
    """(d_x_enc, d_positions, d_directions) -- None where not asked for -- of a module, from the context of a finished
    nrf_mlp_backward_v1 / nrf_mlp_backward (one launch).  V3: through the positional encodings; there is no d_x_enc, and the share of
    d_positions through the fetched features is not in it (points_fetch_backward)."""
    v3 = module.net == L.NRF_NET_V3
    want_x = want_x and not v3
    if not (want_x or want_p or want_d):
        return None, None, None
    d_x = torch.empty((n, 3 * (2 * module.pos_freq + 1)), dtype=torch.float32, device=dev) if want_x else None
    d_p = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_p else None
    d_d = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_d else None
    saved = (module._handle, mode, n, C.c_void_p(buf.data_ptr()), nbytes, L.ptr(positions) if want_p else None, L.ptr(directions) if want_d else None)
    if v3:
        L.check(L.lib().nrf_mlp_backward_inputs_v3(*saved, L.ptr(d_p), L.ptr(d_d), L.stream_ptr()))
    else:
        L.check(L.lib().nrf_mlp_backward_inputs(*saved, L.ptr(d_x), L.ptr(d_p), L.ptr(d_d), L.stream_ptr()))
    return d_x, d_p, d_d


def points_fetch_backward(dino, points, d_feats, d_points=None):
    """d_points (n,3) [+]= the adjoint of nrf_project_fetch with respect to `points` (n,3) applied to d_feats (n,C), for the source
    view dino = dict(features= (1,Hp,Wp,C), pose=, focal=, H=, W=).  With d_points given the result is added onto it (the V3 input
    gradient: onto the share through the positional encoding); otherwise a new tensor is returned.  Bit-reproducible."""
    from .renderer import make_dino
    dn, keep = make_dino(**dino)
    dev = keep.device
    pts = L.dev_f32(points, dev).reshape(-1, 3)
    g = L.dev_f32(d_feats, dev).reshape(pts.shape[0], -1)
    if g.shape[1] != dn.C:
        raise ValueError("d_feats must hold one row of C channels per point")
    acc = d_points is not None
    if not acc:
        d_points = torch.empty((pts.shape[0], 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().nrf_project_fetch_backward_points(C.byref(dn), L.ptr(pts), pts.shape[0], L.ptr(g), L.ptr(d_points), int(acc), L.stream_ptr()))
    del keep
    return d_points


_fetch_ws = {}


def fetch_backward_workspace(Hp, Wp, Cc, n, device):
    """The workspace of nrf_project_fetch_backward / nrf_sample_features_backward for these sizes, cached per (device, stream)
    and grown on demand: the launches that use it are ordered on that stream.  Call with `device` current."""
    nbytes = L.lib().nrf_fetch_backward_workspace_bytes(int(Hp), int(Wp), int(Cc), int(n))
    if nbytes < 0:
        raise L.NrfError(-1, L.lib().nrf_last_error().decode("utf-8", "replace"))
    key = (str(device), L.stream_ptr())
    ws = _fetch_ws.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        if len(_fetch_ws) > 16:
            _fetch_ws.clear()
        ws = _fetch_ws[key] = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=device)
    return ws


def project_fetch_backward(dino, points, d_feats, d_map, accumulate=True):
    """d_map (1,Hp,Wp,C) [+]= the adjoint of nrf_project_fetch at `points` (n,3) applied to d_feats (n,C), for the source view
    dino = dict(features= (only its shape is used), pose=, focal=, H=, W=): what a trainer that lets FusedStep write
    `d_dino_out` calls per batch before map.backward(d_map).  Bit-reproducible (no atomics)."""
    from .renderer import make_dino
    dev = d_map.device
    pts = L.dev_f32(points, dev).reshape(-1, 3)
    g = L.dev_f32(d_feats, dev).reshape(pts.shape[0], -1)
    dn, keep = make_dino(**{**dino, "features": d_map.detach()})
    with torch.cuda.device(dev):
        ws = fetch_backward_workspace(dn.Hp, dn.Wp, dn.C, pts.shape[0], dev)
        L.check(L.lib().nrf_project_fetch_backward(C.byref(dn), L.ptr(pts), pts.shape[0], L.ptr(g), L.ptr(d_map), int(bool(accumulate)),
                                                   L.ptr(ws), ws.numel() * 4, L.stream_ptr()))
    del keep
    return d_map


class _ProjectFetchFn(torch.autograd.Function):
    """train.py:203-217 with a live feature map: (1,Hp,Wp,C) map, (n,3) points -> (n,C) features; gradient for the map only."""

    @staticmethod
    def forward(ctx, fmap, pts, dino):
        from .renderer import make_dino
        dev = pts.device
        fm = fmap.contiguous()
        dn, keep = make_dino(**{**dino, "features": fm})
        n = pts.shape[0]
        feats = torch.empty((n, dn.C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().nrf_project_fetch(C.byref(dn), L.ptr(pts), n, L.ptr(feats), None, L.stream_ptr()))
        del keep
        ctx.dino, ctx.shape = dino, tuple(fm.shape)
        ctx.save_for_backward(pts)
        return feats

    @staticmethod
    def backward(ctx, g):
        (pts,) = ctx.saved_tensors
        d_map = torch.empty(ctx.shape, dtype=torch.float32, device=pts.device)
        project_fetch_backward(ctx.dino, pts, g.to(torch.float32).contiguous(), d_map, accumulate=False)
        return d_map, None, None


class _MLPV1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x_enc, points, *params):
        dev = x_enc.device
        h, mode = _train_handle(module, dev)
        n = x_enc.shape[0]
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            buf, nbytes = _context(h, mode, n, dev)
            L.check(L.lib().nrf_mlp_forward_train_v1(h, mode, L.ptr(x_enc), n, L.ptr(out), C.c_void_p(buf.data_ptr()), nbytes, L.stream_ptr()))
        ctx.module, ctx.buf, ctx.nbytes, ctx.n, ctx.mode = module, buf, nbytes, n, mode
        ctx.versions = module._versions()
        ctx.save_for_backward(out, points)
        return out

    @staticmethod
    def backward(ctx, g_out):
        module = ctx.module
        if module._versions() != ctx.versions:
            raise RuntimeError("NeRFMLP parameters were modified between forward and backward: the saved activations "
                               "no longer match the packed weights")
        out, points = ctx.saved_tensors
        dev = out.device
        g = _prep(g_out)
        grad, d_params = _param_grad_target(module, any(ctx.needs_input_grad[3:]))
        with torch.cuda.device(dev):
            L.check(L.lib().nrf_mlp_backward_v1(module._handle, ctx.mode, L.ptr(out), L.ptr(g), ctx.n, C.c_void_p(ctx.buf.data_ptr()), ctx.nbytes,
                                                L.ptr(grad), L.stream_ptr()))
            # input_grad modules with inputs that require grad: one more launch over what the backward saved
            d_x, d_p, _ = _input_grad(module, ctx.mode, ctx.n, ctx.buf, ctx.nbytes, dev, positions=points,
                                      want_x=ctx.needs_input_grad[1], want_p=ctx.needs_input_grad[2])
        ctx.buf = None
        return (None, d_x, d_p) + d_params


class _MLPV2Fn(torch.autograd.Function):
    """nerf_mlp.py:134-158: (positions, directions[, dino features]) -> (rgb, density); V2 and V3 models."""

    @staticmethod
    def forward(ctx, module, pos, dirs, dino, *params):
        dev = pos.device
        h, mode = _train_handle(module, dev)
        n = pos.shape[0]
        rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
        dens = torch.empty((n, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            buf, nbytes = _context(h, mode, n, dev)
            L.check(L.lib().nrf_mlp_forward_train(h, mode, L.ptr(pos), L.ptr(dirs), L.ptr(dino), n, L.ptr(rgb), L.ptr(dens),
                                                  C.c_void_p(buf.data_ptr()), nbytes, L.stream_ptr()))
        ctx.module, ctx.buf, ctx.nbytes, ctx.n, ctx.mode = module, buf, nbytes, n, mode
        ctx.versions = module._versions()
        ctx.save_for_backward(rgb, dens, pos, dirs)
        return rgb, dens

    @staticmethod
    def backward(ctx, g_rgb, g_dens):
        module = ctx.module
        if module._versions() != ctx.versions:
            raise RuntimeError("NeRFMLP parameters were modified between forward and backward: the saved activations "
                               "no longer match the packed weights")
        rgb, dens, pos, dirs = ctx.saved_tensors
        dev = rgb.device
        g_rgb, g_dens = _prep(g_rgb), _prep(g_dens)
        grad, d_params = _param_grad_target(module, any(ctx.needs_input_grad[4:]))
        with torch.cuda.device(dev):
            L.check(L.lib().nrf_mlp_backward(module._handle, ctx.mode, L.ptr(rgb), L.ptr(dens), L.ptr(g_rgb), L.ptr(g_dens), ctx.n,
                                             C.c_void_p(ctx.buf.data_ptr()), ctx.nbytes, L.ptr(grad), L.stream_ptr()))
            # dino_grad modules with features that require grad: one more launch over what the backward saved
            d_dino = _dino_grad(module, ctx.mode, ctx.n, ctx.buf, ctx.nbytes, dev) if ctx.needs_input_grad[3] else None
            # input_grad / point_grad modules with positions / directions that require grad: likewise
            _, d_p, d_d = _input_grad(module, ctx.mode, ctx.n, ctx.buf, ctx.nbytes, dev, positions=pos, directions=dirs,
                                      want_p=ctx.needs_input_grad[1], want_d=ctx.needs_input_grad[2])
        ctx.buf = None
        return (None, d_p, d_d, d_dino) + d_params


def mlp_v2_train(module, positions, directions, dino_features=None):
    """(P,3) positions, (P,3) directions [, (P,C) DINO features for the use_dino=True form] -> rgb (P,3), density (P,1),
    differentiable with respect to the parameters, -- for a module built with dino_grad=True -- the DINO features and -- for a
    module built with input_grad=True -- the positions and directions (without the switch a tensor that requires grad is refused)."""
    pos = _live_input(module, positions, "NeRFMLP.forward(positions)").reshape(-1, 3)
    dirs = _live_input(module, directions, "NeRFMLP.forward(directions)", pos.device).reshape(-1, 3)
    dino = None
    if module.net == L.NRF_NET_V3:
        if dino_features is None:
            raise ValueError("use_dino=True needs dino_features")
        if torch.is_grad_enabled() and getattr(dino_features, "requires_grad", False):
            if not (getattr(module, "dino_grad", False) or getattr(module, "point_grad", False)):
                raise NotImplementedError("no gradient with respect to the DINO features is produced by default (the reference computes "
                                          "its maps under no_grad: SURVEY.md section 8 f4); detach them, or build the module with "
                                          "NeRFMLP(..., dino_grad=True)")
            dino = dino_features.to(device=pos.device, dtype=torch.float32).reshape(-1, module.dino_dim).contiguous()      # stays in the graph
        else:
            dino = L.dev_f32(dino_features, pos.device).reshape(-1, module.dino_dim)
    return _MLPV2Fn.apply(module, pos, dirs, dino, *module.flat_params().params())


def mlp_v1_train(module, x_enc, points=None):
    """(P, 63) encoded points -> (P, 4) = [sigmoid rgb, raw sigma], differentiable with respect to the parameters and -- for a
    module built with input_grad=True -- x_enc and `points`, the (P,3) positions x_enc encodes."""
    x = _live_input(module, x_enc, "NeRFMLP.forward(x_encoded)")
    pe = 3 * (2 * module.pos_freq + 1)
    flat_in = x.reshape(-1, pe)
    pts = None
    if points is not None:
        pts = _live_input(module, points, "NeRFMLP.forward(points)", x.device).reshape(-1, 3)
        if pts.shape[0] != flat_in.shape[0]:
            raise ValueError("points must hold one (x,y,z) row per row of x_encoded")
    out = _MLPV1Fn.apply(module, flat_in, pts, *module.flat_params().params())
    return out.reshape(*x.shape[:-1], 4)


def field_input_grad(module, points, dino=None):
    """nerf_model.density_normals: one saving forward, the dZ chain with dL/d sigma = 1 (its parameter gradients go to a scratch
    vector) and the input-gradient kernel.  A point_grad (V3) module with its source view `dino`: the fetch in front, and behind the
    chain dL/d features and the adjoint of the fetch added onto the input-gradient kernel's result."""
    pts = L.dev_f32(points).reshape(-1, 3)
    dev, n = pts.device, pts.shape[0]
    h, mode = _train_handle(module, dev)
    lib = L.lib()
    v3 = module.net == L.NRF_NET_V3
    dn = keep = None
    if v3:
        from .renderer import make_dino
        dn, keep = make_dino(**{**dino, "features": L.dev_f32(dino["features"], dev)})
        if dn.C != module.dino_dim:
            raise ValueError("features must be (1,Hp,Wp,dino_dim)")
    with torch.cuda.device(dev):
        buf, nbytes = _context(h, mode, n, dev)
        scratch = torch.zeros_like(module.flat_params().flat)
        st, cb = L.stream_ptr(), C.c_void_p(buf.data_ptr())
        if module.net == L.NRF_NET_V1:
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
            g = torch.zeros_like(out)
            g[:, 3] = 1.0
            L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(_encoder(module.pos_freq)(pts)), n, L.ptr(out), cb, nbytes, st))
            L.check(lib.nrf_mlp_backward_v1(h, mode, L.ptr(out), L.ptr(g), n, cb, nbytes, L.ptr(scratch), st))
            sigma = out[:, 3:4].contiguous()
        else:
            feats = None
            if v3:
                feats = torch.empty((n, dn.C), dtype=torch.float32, device=dev)
                L.check(lib.nrf_project_fetch(C.byref(dn), L.ptr(pts), n, L.ptr(feats), None, st))
            dirs = torch.zeros_like(pts)                 # the density does not depend on the view direction
            rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
            sigma = torch.empty((n, 1), dtype=torch.float32, device=dev)
            L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(pts), L.ptr(dirs), L.ptr(feats), n, L.ptr(rgb), L.ptr(sigma), cb, nbytes, st))
            g_rgb, g_den = torch.zeros_like(rgb), torch.ones_like(sigma)          # (named: they must outlive the launch's pointers)
            L.check(lib.nrf_mlp_backward(h, mode, L.ptr(rgb), L.ptr(sigma), L.ptr(g_rgb), L.ptr(g_den), n, cb, nbytes, L.ptr(scratch), st))
        d_feats = _dino_grad(module, mode, n, buf, nbytes, dev) if v3 else None
        _, g, _ = _input_grad(module, mode, n, buf, nbytes, dev, positions=pts, want_p=True)
        if v3:
            L.check(lib.nrf_project_fetch_backward_points(C.byref(dn), L.ptr(pts), n, L.ptr(d_feats), L.ptr(g), 1, st))
    del keep
    norm = g.norm(dim=-1, keepdim=True)
    normals = torch.where(norm > 0, -g / norm.clamp_min(1e-30), torch.zeros_like(g))
    return sigma, normals


# ---------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------
class _CompositeFn(torch.autograd.Function):
    """rgb (R,S,Cs>=3 strided), sigma (R,S strided) -> rgb_map, depth, weights; gradients for rgb and sigma only
    (the reference never differentiates the sample depths or ray directions) unless `geom`: then also for z and d
    (nrf_composite_backward_geom)."""

    @staticmethod
    def forward(ctx, packed, z, d, white_bkgd, geom=False):
        R, S = z.shape
        dev = z.device
        out_rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
        out_depth = torch.empty((R,), dtype=torch.float32, device=dev)
        out_w = torch.empty((R, S), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().nrf_composite(*_heads(packed, R * S, True)[2], L.ptr(z), L.ptr(d), R, S,
                                          int(bool(white_bkgd)), L.ptr(out_rgb), L.ptr(out_depth), L.ptr(out_w), L.stream_ptr()))
        ctx.save_for_backward(packed, z, d)
        ctx.white, ctx.geom = int(bool(white_bkgd)), bool(geom)
        ctx.set_materialize_grads(False)      # unused outputs arrive as None, not as zero tensors
        return out_rgb, out_depth, out_w

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_w):
        packed, z, d = ctx.saved_tensors
        R, S = z.shape
        dev = z.device
        g_rgb, g_depth, g_w = _prep(g_rgb), _prep(g_depth), _prep(g_w)
        d_packed = torch.empty_like(packed)
        if g_rgb is None and g_depth is None and g_w is None:
            return None, None, None, None, None
        heads, d_heads = _heads(packed, R * S, True)[2], _heads(d_packed, R * S, True)[2]
        with torch.cuda.device(dev):
            if ctx.geom:
                d_z, d_d = torch.empty_like(z), torch.empty_like(d)
                L.check(L.lib().nrf_composite_backward_geom(*heads, L.ptr(z), L.ptr(d), R, S, ctx.white, L.ptr(g_rgb), L.ptr(g_depth), L.ptr(g_w),
                                                            *d_heads, L.ptr(d_z), L.ptr(d_d), L.stream_ptr()))
                return d_packed, d_z, d_d, None, None
            L.check(L.lib().nrf_composite_backward(*heads, L.ptr(z), L.ptr(d), R, S, ctx.white, L.ptr(g_rgb), L.ptr(g_depth), L.ptr(g_w),
                                                   *d_heads, L.stream_ptr()))
        return d_packed, None, None, None, None


def composite(rgb_sigma, z, d, white_bkgd=False, geom_grad=False):
    """Differentiable alpha compositing of (R,S,4) [r,g,b,sigma] rows.  geom_grad=True: z (R,S) and d (R,3) that require grad
    receive dL/d z_vals and dL/d rays_d (through |rays_d|) as well."""
    if geom_grad:
        return _CompositeFn.apply(rgb_sigma.contiguous(), z.to(torch.float32).contiguous(), d.to(torch.float32).contiguous(), white_bkgd, True)
    return _CompositeFn.apply(rgb_sigma.contiguous(), z, d, white_bkgd, False)


# ---------------------------------------------------------------------------------------------
# render_rays with grad enabled: the trainer-shaped entry point (train.py:188-242 inside train_step, :280-287)
# ---------------------------------------------------------------------------------------------
def _render_forward(ctx, module, inputs, z, d, white, mma_mode):
    """The forward the render nodes share: context, o4 (V1: [r,g,b,sigma] rows; V2/V3: rgb (n,3) | density (n,1)) and the three
    outputs, the family's saving forward, the compositor.  inputs(stream) -> (x, dirs, dino) as the saving forward reads them: a
    node that derives them (encoding, fetch) launches that here, behind the context query, where it has always run.  Leaves on
    ctx what _render_backward reads; returns (o4, (rgb, depth, weights))."""
    dev = z.device
    R, S = z.shape
    n = R * S
    h, mode = _train_handle(module, dev, mma_mode)
    v1 = module.net == L.NRF_NET_V1
    lib = L.lib()
    with torch.cuda.device(dev):
        buf, nbytes = _context(h, mode, n, dev)
        o4 = torch.empty((n, 4), dtype=torch.float32, device=dev)
        out_rgb = torch.empty((R, 3), dtype=torch.float32, device=dev)
        out_depth = torch.empty((R,), dtype=torch.float32, device=dev)
        out_w = torch.empty((R, S), dtype=torch.float32, device=dev)
        st, cb = L.stream_ptr(), C.c_void_p(buf.data_ptr())
        x, dirs, dino = inputs(st)
        rgb, den, heads = _heads(o4, n, v1)
        if v1:
            L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(x), n, L.ptr(o4), cb, nbytes, st))
        else:
            L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(x), L.ptr(dirs), L.ptr(dino), n, L.ptr(rgb), L.ptr(den), cb, nbytes, st))
        L.check(lib.nrf_composite(*heads, L.ptr(z), L.ptr(d), R, S, white, L.ptr(out_rgb), L.ptr(out_depth), L.ptr(out_w), st))
    ctx.module, ctx.buf, ctx.nbytes, ctx.mode, ctx.white, ctx.v1, ctx.dev = module, buf, nbytes, mode, white, v1, dev
    ctx.versions = module._packed                    # the versions handle() just packed (== module._versions(), not recomputed)
    ctx.set_materialize_grads(False)
    return o4, (out_rgb, out_depth, out_w)


# what _render_backward leaves for the launches a node adds behind it: the saved tensors, rows, stream, what the node returns for
# its *params slots, and (geom) the compositor's own dL/d z and dL/d rays_d
_Backward = collections.namedtuple("_Backward", "saved n st d_params d_zc d_dc")


def _no_grads(ctx, n_in):
    """What a render node returns when none of its outputs was used."""
    return (None,) * (n_in + len(ctx.module.flat_params().offsets))


def _render_backward(ctx, g_rgb, g_depth, g_w, n_in, geom):
    """The opening the render nodes' backwards share (call with ctx.dev current): version check, gradient prep, the gradient
    target, compositor backward (geom: nrf_composite_backward_geom), network backward.  Returns a _Backward, or None when no
    output was used: nothing is launched then and the node returns _no_grads."""
    module = ctx.module
    if module._versions() != ctx.versions:
        raise RuntimeError("NeRFMLP parameters were modified between render_rays and backward: the saved activations "
                           "no longer match the packed weights")
    saved = ctx.saved_tensors
    o4, z, d = saved[:3]
    R, S = z.shape
    n = R * S
    lib = L.lib()
    g_rgb, g_depth, g_w = _prep(g_rgb), _prep(g_depth), _prep(g_w)
    if g_rgb is None and g_depth is None and g_w is None:
        return None
    # geom nodes exist for their input gradients: frozen parameters get a scratch vector.  _RenderFn does not consult
    # needs_input_grad for the parameters (it always accumulates into their .grad): kept as it is
    grad, d_params = _param_grad_target(module, not geom or any(ctx.needs_input_grad[n_in:]))
    d4 = torch.empty_like(o4)
    d_zc, d_dc = (torch.empty_like(z), torch.empty_like(d)) if geom else (None, None)
    st, cb = L.stream_ptr(), C.c_void_p(ctx.buf.data_ptr())
    rgb, den, heads = _heads(o4, n, ctx.v1)
    d_rgb, d_den, d_heads = _heads(d4, n, ctx.v1)
    if geom:
        L.check(lib.nrf_composite_backward_geom(*heads, L.ptr(z), L.ptr(d), R, S, ctx.white, L.ptr(g_rgb), L.ptr(g_depth), L.ptr(g_w),
                                                *d_heads, L.ptr(d_zc), L.ptr(d_dc), st))
    else:
        L.check(lib.nrf_composite_backward(*heads, L.ptr(z), L.ptr(d), R, S, ctx.white, L.ptr(g_rgb), L.ptr(g_depth), L.ptr(g_w),
                                           *d_heads, st))
    if ctx.v1:
        L.check(lib.nrf_mlp_backward_v1(module._handle, ctx.mode, L.ptr(o4), L.ptr(d4), n, cb, ctx.nbytes, L.ptr(grad), st))
    else:
        L.check(lib.nrf_mlp_backward(module._handle, ctx.mode, L.ptr(rgb), L.ptr(den), L.ptr(d_rgb), L.ptr(d_den), n, cb, ctx.nbytes,
                                     L.ptr(grad), st))
    return _Backward(saved, n, st, d_params, d_zc, d_dc)


def _ray_grad(d_p, d_dirs, z, d, d_zc, d_dc, z_live, st):
    """(d_rays_o, d_rays_d, d_z or None): the adjoint of the points and per-sample directions of rays, added to the compositor's own
    dL/d z and dL/d rays_d (one launch; call with the device current)."""
    R, S = z.shape
    d_o, d_d = torch.empty_like(d), torch.empty_like(d)
    d_z = torch.empty_like(z) if z_live else None
    L.check(L.lib().nrf_ray_grad(L.ptr(d_p), L.ptr(d_dirs), L.ptr(z), L.ptr(d), L.ptr(d_zc), L.ptr(d_dc), R, S, L.ptr(d_o), L.ptr(d_d),
                                 L.ptr(d_z), st))
    return d_o, d_d, d_z


class _RenderFn(torch.autograd.Function):
    """Per-sample network inputs + depths + rays -> (rgb (R,3), depth (R,), weights (R,S)), differentiable with respect to the
    parameters: ONE autograd node over the kernels FusedStep runs (saving forward -> composite | composite backward -> dZ
    chain + weight gradients), so `loss.backward()` of the reference's unmodified train_step body lands in the parameters'
    .grad (views of the module's flat gradient vector)."""

    @staticmethod
    def forward(ctx, module, x, dirs, dino, z, d, white, mma_mode, *params):
        o4, outs = _render_forward(ctx, module, lambda st: (x, dirs, dino), z, d, white, mma_mode)
        ctx.save_for_backward(o4, z, d)
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_w):
        with torch.cuda.device(ctx.dev):
            b = _render_backward(ctx, g_rgb, g_depth, g_w, 8, False)
            if b is None:
                return _no_grads(ctx, 8)
            d_dino = _dino_grad(ctx.module, ctx.mode, b.n, ctx.buf, ctx.nbytes, ctx.dev) if ctx.needs_input_grad[3] else None      # a live feature map
        ctx.buf = None
        return (None, None, None, d_dino) + (None,) * 4 + b.d_params


_encoders = {}


def _encoder(pos_freq):
    from .positional_encoding import PositionalEncoding
    enc = _encoders.get(pos_freq)
    if enc is None:
        enc = _encoders[pos_freq] = PositionalEncoding(pos_freq)
    return enc


class _RenderGeomFn(torch.autograd.Function):
    """_RenderFn of a V1 / V2 module built with input_grad=True whose rays or depths require grad: the same forward launches, and a
    backward that also runs the geometric compositor backward, the input-gradient kernel and the adjoint of the points:
    gradients for rays_o, rays_d and explicit depths as well as the parameters."""

    @staticmethod
    def forward(ctx, module, o, d, z, z_live, pts, white, mma_mode, *params):
        R, S = z.shape
        v1 = module.net == L.NRF_NET_V1
        dirs = None if v1 else d[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()

        def inputs(st):
            return (_encoder(module.pos_freq)(pts), None, None) if v1 else (pts, dirs, None)
        o4, outs = _render_forward(ctx, module, inputs, z, d, white, mma_mode)
        ctx.z_live = bool(z_live)
        ctx.save_for_backward(o4, z, d, pts, dirs)
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_w):
        with torch.cuda.device(ctx.dev):
            b = _render_backward(ctx, g_rgb, g_depth, g_w, 8, True)
            if b is None:
                return _no_grads(ctx, 8)
            _, z, d, pts, dirs = b.saved
            _, d_p, d_dirs = _input_grad(ctx.module, ctx.mode, b.n, ctx.buf, ctx.nbytes, ctx.dev, positions=pts, directions=dirs, want_p=True,
                                         want_d=not ctx.v1)
            d_o, d_d, d_z = _ray_grad(d_p, d_dirs, z, d, b.d_zc, b.d_dc, ctx.z_live, b.st)
        ctx.buf = None
        return (None, d_o, d_d, d_z) + (None,) * 4 + b.d_params


class _RenderPointFn(torch.autograd.Function):
    """_RenderGeomFn of a V3 module built with point_grad=True whose rays or depths require grad.  Forward: project + fetch, the
    saving forward, the compositor.  Backward, one node: the geometric compositor backward, the V3 dZ chain, dino_grad_kernel into a
    scratch d_feats, input_grad_v3_kernel, fetch_points_backward_kernel adding onto its d_positions, the adjoint of the points; a
    live feature map (a dino_grad module) receives d_map from the same d_feats."""

    @staticmethod
    def forward(ctx, module, o, d, z, z_live, pts, fmap, dino, white, mma_mode, *params):
        from .renderer import make_dino
        R, S = z.shape
        dirs = d[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
        fm = fmap.detach().contiguous()
        dn, keep = make_dino(**{**dino, "features": fm})

        def fetched(st):
            feats = torch.empty((R * S, dn.C), dtype=torch.float32, device=z.device)
            L.check(L.lib().nrf_project_fetch(C.byref(dn), L.ptr(pts), R * S, L.ptr(feats), None, st))
            return pts, dirs, feats
        o4, outs = _render_forward(ctx, module, fetched, z, d, white, mma_mode)
        del keep
        ctx.z_live, ctx.dino = bool(z_live), dino
        ctx.save_for_backward(o4, z, d, pts, dirs, fm)
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_w):
        from .renderer import make_dino
        module, dev = ctx.module, ctx.dev
        with torch.cuda.device(dev):
            b = _render_backward(ctx, g_rgb, g_depth, g_w, 10, True)
            if b is None:
                return _no_grads(ctx, 10)
            (_, z, d, pts, dirs, fm), n, st = b.saved, b.n, b.st
            dn, keep = make_dino(**{**ctx.dino, "features": fm})
            d_map = None
            d_feats = _dino_grad(module, ctx.mode, n, ctx.buf, ctx.nbytes, dev)
            _, d_p, d_dirs = _input_grad(module, ctx.mode, n, ctx.buf, ctx.nbytes, dev, positions=pts, directions=dirs, want_p=True, want_d=True)
            L.check(L.lib().nrf_project_fetch_backward_points(C.byref(dn), L.ptr(pts), n, L.ptr(d_feats), L.ptr(d_p), 1, st))
            if ctx.needs_input_grad[6]:                  # a live feature map
                d_map = torch.empty_like(fm)
                ws = fetch_backward_workspace(dn.Hp, dn.Wp, dn.C, n, dev)
                L.check(L.lib().nrf_project_fetch_backward(C.byref(dn), L.ptr(pts), n, L.ptr(d_feats), L.ptr(d_map), 0, L.ptr(ws), ws.numel() * 4, st))
            d_o, d_d, d_z = _ray_grad(d_p, d_dirs, z, d, b.d_zc, b.d_dc, ctx.z_live, st)
        del keep
        ctx.buf = None
        return (None, d_o, d_d, d_z, None, None, d_map) + (None,) * 3 + b.d_params


def render_rays_train(module, rays_o, rays_d, near, far, n_samples, perturb=True, t_rand=None, seed=None, lindisp=False,
                      white_bkgd=False, dino=None, z_in=None, mma_mode=None, tail_mode=None):
    """renderer.render_rays when grad is enabled: the reference's own sequence (train.py:188-242) -- stratified samples,
    [project + fetch DINO features,] NeRFMLP, VolumeRenderer -- returning {'rgb','depth','weights','z_vals'} that carry a grad_fn.
    Gradients reach the parameters and, for a module built with dino_grad=True, a dino['features'] map that requires grad (through
    the adjoint of the bilinear fetch, nrf_project_fetch_backward); rays and depths are data: a tensor that requires grad is refused,
    unless the module was built with input_grad=True (use_dino form: point_grad=True): then rays_o, rays_d and z_in that require grad
    receive gradients (the ladder's own depths are constants) -- for the use_dino form through the positional encodings and through
    the features fetched at the points' projections into the source view (whose own pose and intrinsics are data).
    The arithmetic mode is `mma_mode` (default: the module's own) mapped to a training mode (_lib.TRAIN_MODE: the split mode
    trains in exact fp32); early ray termination does not apply.  A `tail_mode` (renderer.render_rays) is refused: the training
    kernels have no split-f16 mode, and a silently different forward would be worse than a refusal."""
    if tail_mode is not None:
        raise ValueError("tail_mode is an inference option: the training kernels have no split-f16 mode (render under "
                         "torch.no_grad() or model.eval())")
    from .ray_sampler import sample_points_along_rays
    live_in = module._wants_input_grad(rays_o, rays_d, z_in)
    if live_in:
        o_live = _live_input(module, rays_o, "render_rays(rays_o)").reshape(-1, 3)
        d_live = _live_input(module, rays_d, "render_rays(rays_d)", o_live.device).reshape(-1, 3)
        o, d = o_live.detach(), d_live.detach()
    else:
        o = L.dev_f32(L.refuse_grad(rays_o, "render_rays(rays_o)")).reshape(-1, 3)
        d = L.dev_f32(L.refuse_grad(rays_d, "render_rays(rays_d)"), o.device).reshape(-1, 3)
    R, S = o.shape[0], int(n_samples)
    z_live = None
    if z_in is not None:
        if live_in:
            z_live = _live_input(module, z_in, "render_rays(z_in)", o.device).reshape(R, S)
            z = z_live.detach()
        else:
            z = L.dev_f32(z_in, o.device).reshape(R, S)
        pts = o[:, None, :] + d[:, None, :] * z[:, :, None]
    else:
        pts, z = sample_points_along_rays(o, d, near, far, S, perturb=perturb, lindisp=lindisp, t_rand=t_rand, seed=seed)
    pts = pts.reshape(-1, 3)
    v3 = module.net == L.NRF_NET_V3
    fmap = view = None
    if v3:
        if dino is None:
            raise ValueError("a use_dino model needs dino=dict(features=, pose=, focal=, H=, W=)")
        fmap = dino.get("features")
        map_live = torch.is_grad_enabled() and getattr(fmap, "requires_grad", False)
        if map_live and not getattr(module, "dino_grad", False):
            raise NotImplementedError("no gradient with respect to the DINO feature map is produced by default; detach it, or "
                                      "build the module with NeRFMLP(..., dino_grad=True)")
        if live_in or map_live:           # the map enters an autograd node; a map that is data goes through make_dino, unchecked here
            if live_in:
                fmap = torch.as_tensor(fmap)
            if fmap.dim() != 4 or fmap.shape[0] != 1 or fmap.shape[3] != module.dino_dim:
                raise ValueError("features must be (1,Hp,Wp,dino_dim)")
            fmap = fmap.to(device=o.device, dtype=torch.float32)
            view = {k: v for k, v in dino.items() if k != "features"}
    white, params = int(bool(white_bkgd)), module.flat_params().params()
    if live_in:
        live = z_live is not None and z_live.requires_grad
        zz = z_live if live else z
        if v3:
            rgb, depth, w = _RenderPointFn.apply(module, o_live, d_live, zz, live, pts.contiguous(), fmap, view, white, mma_mode, *params)
        else:
            rgb, depth, w = _RenderGeomFn.apply(module, o_live, d_live, zz, live, pts.contiguous(), white, mma_mode, *params)
        return {"rgb": rgb, "depth": depth, "weights": w, "z_vals": zz}
    dirs = feats = None
    if module.net == L.NRF_NET_V1:
        x = _encoder(module.pos_freq)(pts)                               # train_minimal.py:101
    else:
        x = pts
        dirs = d[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()          # train.py:225: raw ray directions per sample
        if v3 and view is not None:
            feats = _ProjectFetchFn.apply(fmap, pts.contiguous(), view)
        elif v3:
            from .renderer import make_dino
            dn, keep = make_dino(**dino)
            feats = torch.empty((R * S, module.dino_dim), dtype=torch.float32, device=o.device)
            with torch.cuda.device(o.device):
                L.check(L.lib().nrf_project_fetch(C.byref(dn), L.ptr(pts), R * S, L.ptr(feats), None, L.stream_ptr()))   # train.py:203-217
            del keep
    rgb, depth, w = _RenderFn.apply(module, x, dirs, feats, z, d, white, mma_mode, *params)
    return {"rgb": rgb, "depth": depth, "weights": w, "z_vals": z}


# ---------------------------------------------------------------------------------------------
# optimizer
# ---------------------------------------------------------------------------------------------
class Adam:
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) for a NeRFMLP whose parameters live in a FlatParams
    vector: one kernel per step.  Same update rule and defaults as the reference's optimizer (train.py:113-118).
    decoupled=True is torch.optim.AdamW's rule (p *= 1 - lr * weight_decay in front of the moment update); max_grad_norm=c
    clips the gradients as torch.nn.utils.clip_grad_norm_(params, c) in front of the step would, on the device: one small
    launch leaves partial sums of squares, the update kernel forms the coefficient -- no read-back, no sync.  The pre-clip
    norm of the last step stays in `last_grad_norm` (a device scalar)."""

    def __init__(self, module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None):
        self.module = module
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.decoupled = bool(decoupled)
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None: no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._norm_ws = None
        self.step_count = 0
        self.exp_avg = None
        self.exp_avg_sq = None
        self.grad = None

    def _buffers(self):
        fp = self.module.flat_params()
        flat = fp.ensure()
        if self.exp_avg is None or self.exp_avg.shape != flat.shape or self.exp_avg.device != flat.device:
            self.exp_avg = torch.zeros_like(flat)
            self.exp_avg_sq = torch.zeros_like(flat)
        return fp, flat

    @property
    def extended(self):
        """True when the step needs the clipped / decoupled kernel (nrf_adamw_step_loss) instead of nrf_adam_step[_loss]."""
        return self.decoupled or self.max_grad_norm is not None

    def _update(self, flat, g, terms=None, R=0, S=1, weights=(0.0, 0.0, 0.0), losses=None):
        """The extended update on the flat vectors (call with the device current): [norm partials ->] clipped Adam / AdamW,
        with the loss side job when `terms` (3,R) / `losses` (4) are given."""
        lib, st, n = L.lib(), L.stream_ptr(), flat.numel()
        ws = norm = None
        if self.max_grad_norm is not None:
            ws = self._norm_ws
            if ws is None or ws.device != flat.device or ws.numel() * 4 < lib.nrf_grad_sqnorm_workspace_bytes(n):
                ws = self._norm_ws = torch.empty(lib.nrf_grad_sqnorm_workspace_bytes(n) // 4, dtype=torch.float32, device=flat.device)
            norm = torch.empty((), dtype=torch.float32, device=flat.device)
            L.check(lib.nrf_grad_sqnorm_partials(L.ptr(g), n, L.ptr(ws), ws.numel() * 4, st))
        L.check(lib.nrf_adamw_step_loss(L.ptr(flat), L.ptr(g), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), n, self.lr, self.betas[0],
                                        self.betas[1], self.eps, self.weight_decay, self.step_count, int(self.decoupled),
                                        self.max_grad_norm or 0.0, L.ptr(ws), L.ptr(norm), L.ptr(terms), R, S, *weights, L.ptr(losses), st))
        self.last_grad_norm = norm

    @staticmethod
    def _flat_grad_of(ps, fp, flat):
        """The one vector all .grad tensors are views of, if they are (the backward of training.py hands out views of its
        flat gradient in exactly this layout and autograd keeps them when nothing else accumulated)."""
        g0 = ps[0].grad
        base = getattr(g0, "_base", None) if g0 is not None else None
        if base is not None and base.dim() != 1:
            base = None
        if base is None or base.shape != flat.shape or base.dtype != torch.float32 or base.device != flat.device or not base.is_contiguous():
            return None
        b = base.data_ptr()
        for p, off in zip(ps, fp.offsets):
            if p.grad is None or p.grad.data_ptr() != b + 4 * off:
                return None
        return base

    def zero_grad(self, set_to_none=True):
        for p in self.module.flat_params().params():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def step(self):
        fp, flat = self._buffers()
        ps = fp.params()
        g = self._flat_grad_of(ps, fp, flat)
        if g is None:
            # gather the gradients autograd left on the parameters into the flat layout
            g = self.grad if self.grad is not None and self.grad.shape == flat.shape and self.grad.device == flat.device else torch.empty_like(flat)
            self.grad = g
            with torch.no_grad():
                for p, v in zip(ps, fp.views(g)):
                    if p.grad is None:
                        v.zero_()
                    elif p.grad.data_ptr() != v.data_ptr():
                        v.copy_(p.grad)
        self.step_count += 1
        with torch.no_grad(), torch.cuda.device(flat.device):
            if self.extended:
                self._update(flat, g)
            else:
                L.check(L.lib().nrf_adam_step(L.ptr(flat), L.ptr(g), L.ptr(self.exp_avg), L.ptr(self.exp_avg_sq), flat.numel(), self.lr,
                                              self.betas[0], self.betas[1], self.eps, self.weight_decay, self.step_count, L.stream_ptr()))
        self.module._gen += 1            # the packed streams are now older than the parameters


# ---------------------------------------------------------------------------------------------
# data-parallel training: one collective per step
# ---------------------------------------------------------------------------------------------
def _all_reduce_mean(t, group, average=True):
    """In-place all-reduce of a device vector.  RCCL (backend "nccl") reduces device memory directly; under gloo (CPU
    rehearsals, one-GPU test boxes) the vector takes the host round trip gloo needs."""
    import torch.distributed as dist
    if dist.get_backend(group) == "gloo":
        h = t.cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    if average:
        t.div_(dist.get_world_size(group))
    return t


def all_reduce_gradients(model, group=None, average=True):
    """Sum (or average) the gradients of all ranks before optimizer.step().  The gradients of a NeRFMLP live in ONE flat
    vector (see _grad_target), so data-parallel training costs a single all-reduce of nrf_param_count floats
    (1.9 MB for the 8x256 network: one RCCL ring step over xGMI) instead of one per parameter.  Rays shard over the ranks
    (every rank renders its own rays of the batch: no exchange inside the path); call between backward() and step()."""
    fp = model.flat_params()
    fg = getattr(model, "_flat_grad", None)
    ps = fp.params()
    if fg is None or any(p.grad is None for p in ps) or any(p.grad.data_ptr() != fg.data_ptr() + 4 * off for p, off in zip(ps, fp.offsets)):
        raise RuntimeError("all_reduce_gradients: the parameters' .grad are not the flat gradient vector of this module "
                           "(call it right after loss.backward())")
    return _all_reduce_mean(fg, group, average)


# ---------------------------------------------------------------------------------------------
# one optimisation step without autograd in between
# ---------------------------------------------------------------------------------------------
_FOUR = ("total", "rgb", "depth", "reg")
# The loss launch of a FusedStep by kind: (entry, entry behind the multi-term optimiser that completes the loss vector, names of
# last_losses, rows of ray_loss).  mse and indexed may run in front of the plain optimiser, which leaves the first value alone.
_LOSS_KINDS = {
    "mse": ("nrf_composite_mse_backward", None, _FOUR, 3),
    "multi": ("nrf_composite_loss_backward", None, _FOUR, 3),
    "indexed": ("nrf_composite_loss_backward_indexed", None, _FOUR, 3),         # the step under a grid, plain or multi-term
    "reg": ("nrf_composite_reg_loss_backward", "nrf_ray_terms_finish", _FOUR + ("dist", "occ"), 5),
    "patch": ("nrf_composite_patch_loss_backward", "nrf_patch_terms_finish", _FOUR + ("dist", "occ", "smooth"), 5),
    "info": ("nrf_composite_info_loss_backward", "nrf_info_terms_finish", _FOUR + ("dist", "occ", "smooth", "entropy", "kl"), 5),
    "hier": ("nrf_composite_hier_loss_backward", None, ("total", "coarse", "fine"), 3),
}


class _LossPlan:
    """One step's loss launch, decided once (FusedStep._loss_plan): the entry that runs, the structs and term buffers it is handed,
    the launch behind the optimiser that completes the loss vector, and the names of that vector's values."""

    def __init__(self, kind, multi):
        self.kind, self.multi = kind, multi                 # multi: the clipped optimiser with the four loss values runs behind it
        self.entry, self.finish_entry, names, _ = _LOSS_KINDS[kind]
        self.names = names if multi or kind == "hier" else names[:1]
        self.lo = self.reg = None           # nrf_loss_opts (every kind but mse), nrf_ray_reg (reg, patch, info)
        self.tail = self.finish_tail = ()   # what the patch and information entries take behind the common arguments
        self.keep = None                    # tensors whose pointers the launch reads: alive until it is enqueued
        self.depth = False                  # target_depth was passed: the depth term is on
        self.parts = None                   # hier: ((2,R) squared errors coarse | fine, R)

    def launch(self, step, heads, d_heads, z, d, tgt, R, S, slot, st):
        """The kind's entry on the step's buffers: the arguments all six share, written once, and the kind's own between and behind
        them -- rgb_weight or the loss options, the ray regularisers, the slot map (None: dense), the patch and information tail."""
        a = [*heads, L.ptr(z), L.ptr(d), R, S, step.white, L.ptr(tgt), step.rgb_weight if self.lo is None else C.byref(self.lo)]
        if self.reg is not None:
            a.append(C.byref(self.reg))
        if self.kind not in ("mse", "multi"):               # dense or indexed
            a.append(None if slot is None else slot.data_ptr())
        L.check(getattr(L.lib(), self.entry)(*a, L.ptr(step.pred), *d_heads, L.ptr(step.ray_loss), L.ptr(step.grad), step.grad.numel(), st,
                                             *self.tail))
        self.keep = None

    def finish(self, step, R, S, loss4, st):
        """Behind the multi-term optimiser, which left loss4: one small launch more where the kind has terms of its own; returns the
        step's loss vector, one value per name."""
        if self.finish_entry is None:
            return loss4
        loss = torch.empty((len(self.names),), dtype=torch.float32, device=loss4.device)
        if self.kind == "reg":              # the two new terms summed in a fixed order and appended to the four
            a = (R, C.byref(self.reg), L.ptr(loss4))
        else:                               # every value with the divisors of the batch layout (the optimiser's four divide by R);
            a = (R, S, C.byref(self.lo), C.byref(self.reg), *self.finish_tail)      # loss_opts.target_depth: a flag here, not read
        L.check(getattr(L.lib(), self.finish_entry)(L.ptr(step.ray_loss), *a, L.ptr(loss), st))
        return loss

    def losses(self, vec):
        v = vec.reshape(-1)
        if self.parts is None:
            return dict(zip(self.names, v))
        parts, R = self.parts
        mse = parts.sum(dim=1) / (3.0 * R)                  # formed when asked for (torch reductions on the stream: no sync), from the step's buffer
        return dict(zip(self.names, (v[0], mse[0], mse[1])))


class FusedStep:
    """The body of the reference's inner loop -- render a batch of rays, `rgb_weight * mse(pred['rgb'], target)`
    (train.py:36-44,280-288; train_minimal.py:102-123), backward, Adam -- as a fixed sequence of libnerfhip calls on
    preallocated buffers: saving forward -> [composite, mse and its gradient, composite backward: one launch] -> dZ chain +
    weight gradients -> Adam -> (next step) device re-pack.  Same kernels and the same numbers as the autograd route; what it saves is the
    autograd graph, the per-parameter gradient tensors and the Python between the launches, which at the reference's batch
    sizes (1-2 k rays x 32-64 samples) cost more than the kernels.

        step = FusedStep(model, lr=5e-4, weight_decay=1e-6)
        loss = step(points, z_vals, rays_d, target)               # V1: points = encoded (R*S, 63)
        loss = step(points, z_vals, rays_d, target, dirs=dirs)    # V2: points (R*S, 3), dirs (R*S, 3)
        loss = step(points, z_vals, rays_d, target, dirs=dirs, dino=feats)    # V3: + per-sample DINO features (R*S, C)

    The multiscale trainer's step (train_multiscale.py:207-211,249-266) is the same sequence with its options switched on --
    density noise in front of the compositor's ReLU, nerf_mlp.NeRFLoss (rgb_weight * mse + depth_weight * l1(depth,
    target_depth) + reg_weight * mean(weights^2)), clip_grad_norm_, AdamW:

        step = FusedStep(model, lr=2e-4, weight_decay=1e-6, reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0,
                         decoupled_weight_decay=True)

    The general compositor/loss kernel stands in for the mse one and the clipped optimiser for Adam; the only additional launch
    is the norm's partial sums (with max_grad_norm).  The returned value is the total loss; `last_losses` holds the components
    ({'total', 'rgb', 'depth', 'reg'}: device scalars, the reference's `losses` dict) and `last_grad_norm` the pre-clip norm
    (device scalar, None without clipping).  Nothing synchronises.

    Few-shot ray regularisers (nerfhip.h: nrf_ray_reg), on __call__, step_rays and step_view, with or without occupancy=:

        step = FusedStep(model, lr=5e-4, dist_weight=1e-2, occ_weight=1e-2, occ_samples=4)

    dist_weight * mean_r D_r is mip-NeRF 360's distortion loss on the weights and the interval midpoints scaled by 1 / dist_span
    (None: far - near of the step), occ_weight * mean_r O_r FreeNeRF's penalty on the density of every ray's first occ_samples
    samples.  With either weight on the step is the multi-term one with nrf_composite_reg_loss_backward as its loss launch and
    one small launch (nrf_ray_terms_finish) behind the optimiser; `last_losses` gains 'dist' and 'occ' (unweighted; 0 for a term
    whose weight is 0), 'total' and the returned loss include both.  With both weights 0 (the default) nothing changes.

    Patch regulariser (RegNeRF's depth-smoothness loss on patches of unseen views; nerfhip.h: nrf_patch_reg), on __call__ and
    step_rays, with or without occupancy=:

        step = FusedStep(model, lr=5e-4, depth_smooth_weight=0.1, patch_size=8)
        o_p, d_p = patch_rays(H, W, focal, sample_patch_poses(train_poses, 16), 8)                   # ray_sampler
        loss = step.step_rays(torch.cat([rays_o, o_p]), torch.cat([rays_d, d_p]), target, near, far, 64, n_patches=16)

    The last n_patches * patch_size^2 rays of the batch are patch rays -- patch-major, row-major inside a patch -- and `target`
    (and target_depth) hold the rows of the R_s rays in front of them.  A patch ray has no colour term; it takes reg_weight,
    dist_weight and occ_weight like any ray, and depth_smooth_weight * mean over patches and anchors of the squared depth
    differences to its right and lower neighbour.  The step is the multi-term one with nrf_composite_patch_loss_backward as its
    loss launch -- a workgroup owns a patch and its rays' depths meet in LDS between the compositor forward and its backward -- and
    nrf_patch_terms_finish behind the optimiser: as many launches as a step with dist_weight > 0.  `last_losses` gains 'smooth'
    (seven keys; rgb and depth are means over the R_s supervised rays), `last_patch_depth` is the (n_patches, P, P) view of a
    buffer of this object with the rendered depths.  step_view and the hierarchical steps refuse such a step object.  With
    depth_smooth_weight = 0 (the default) nothing changes, launch for launch.

    Information regularisers (InfoNeRF's ray entropy and its KL between neighbouring rays; nerfhip.h: nrf_info_reg):

        step = FusedStep(model, lr=5e-4, ent_weight=1e-3, ent_threshold=0.01, kl_weight=1e-5, patch_size=8)
        loss = step.step_rays(torch.cat([rays_o, o_p]), torch.cat([rays_d, d_p]), target, near, far, 64, n_patches=16)

    Both act on a ray's distribution p_i = a_i / sum a over its S - 1 finite intervals, a_i = 1 - exp(-relu(sigma_i) dist_i): ent_weight
    times the mean over ALL rays of the batch (patch rays included) of the entropy of p, for rays whose sum a exceeds ent_threshold;
    kl_weight times the mean over patches and anchors of KL(p_anchor || p_right) + KL(p_anchor || p_below), both rays above the
    threshold, the gradient into both arguments.  ent_weight goes wherever dist_weight does (__call__, step_rays with or without
    occupancy=, step_view); kl_weight wherever depth_smooth_weight does, on the patch rays behind n_patches= (patch_size^2 *
    n_samples <= 12288: the patch's distributions meet in LDS); n_patches > 0 is accepted with any of the three weights.  The step is
    the patch step with nrf_composite_info_loss_backward as its loss launch and nrf_info_terms_finish behind the optimiser: the same
    launch count.  `last_losses` gains 'entropy' and 'kl' (nine keys, unweighted).  The hierarchical steps refuse both weights.  With
    both 0 (the default) nothing changes, launch for launch and bit for bit.

    Frequency regularisation (FreeNeRF's coarse-to-fine mask on the positional encodings), on every step method:

        step = FusedStep(model, lr=5e-4, freq_reg_end=9000)

    Step t (opt.step_count before the step) runs under model.set_freq_mask(freq_mask_columns(pos_freq, freq_mask_visible(t,
    freq_reg_end, pos_freq))), and the same on the direction encoding unless freq_reg_dirs=False, set before anything of the step
    is packed.  The mask costs no launch: it rides in the re-pack and in the weight gradients' second stage.  Hidden columns
    receive gradient exactly 0 (with weight_decay = 0 their weights keep their bits; under decay they decay like any weight).
    Once all bands are visible the mask is cleared and the step is the plain one, launch for launch and bit for bit.  The mask is
    a function of the step count alone, so data_parallel ranks agree on it.
    """

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, rgb_weight=1.0, white_bkgd=False,
                 process_group=None, data_parallel=False, reg_weight=0.0, depth_weight=0.0, noise_std=0.0, max_grad_norm=None,
                 decoupled_weight_decay=False, seed=None, dist_weight=0.0, occ_weight=0.0, occ_samples=0, dist_span=None,
                 freq_reg_end=0, freq_reg_dirs=True, depth_smooth_weight=0.0, patch_size=8, ent_weight=0.0, ent_threshold=0.01,
                 kl_weight=0.0):
        """data_parallel=True (inside an initialised torch.distributed job): every rank passes ITS shard of the ray batch
        (equal sizes), the flat gradient vector is averaged over the ranks with one all-reduce before Adam (the norm of
        max_grad_norm is taken behind it, so all ranks clip alike), and the returned loss is this rank's.
        seed: of the in-kernel density noise (noise_std > 0 and no `noise` tensor passed to the call); step t draws from
        seed + t, a ray's draw is keyed by its index in the call.  Default: drawn from torch's CPU generator when first needed."""
        if model.net not in (L.NRF_NET_V1, L.NRF_NET_V2, L.NRF_NET_V3):
            raise NotImplementedError("FusedStep: unknown network family")
        if min(float(rgb_weight), float(reg_weight), float(depth_weight), float(noise_std)) < 0.0:
            raise ValueError("FusedStep: loss weights and noise_std must be >= 0")
        for names, values in (("dist_weight and occ_weight", (dist_weight, occ_weight)), ("depth_smooth_weight", (depth_smooth_weight,)),
                              ("ent_weight", (ent_weight,)), ("ent_threshold", (ent_threshold,)), ("kl_weight", (kl_weight,))):
            if not all(float(v) >= 0.0 and math.isfinite(float(v)) for v in values):
                raise ValueError(f"FusedStep: {names} must be finite and >= 0")
        if int(occ_samples) < 0 or (float(occ_weight) > 0.0 and int(occ_samples) < 1):
            raise ValueError("FusedStep: occ_samples must be >= 1 with occ_weight > 0 (and never negative)")
        if dist_span is not None and not (math.isfinite(float(dist_span)) and float(dist_span) > 0.0):
            raise ValueError("FusedStep: dist_span must be finite and > 0 (None: far - near of the step)")
        if int(freq_reg_end) < 0:
            raise ValueError("FusedStep: freq_reg_end must be >= 0 (0: no frequency regularisation)")
        if int(patch_size) != patch_size or not 2 <= int(patch_size) <= 16:
            raise ValueError("FusedStep: patch_size must be an integer in 2 ... 16")
        self.model = model
        self.freq_reg_end, self.freq_reg_dirs = int(freq_reg_end), bool(freq_reg_dirs)
        self.data_parallel = bool(data_parallel)
        self.group = process_group
        self.opt = Adam(model, lr, betas, eps, weight_decay, decoupled=decoupled_weight_decay, max_grad_norm=max_grad_norm)
        self.rgb_weight = float(rgb_weight)
        self.reg_weight, self.depth_weight, self.noise_std = float(reg_weight), float(depth_weight), float(noise_std)
        self.dist_weight, self.occ_weight, self.occ_samples = float(dist_weight), float(occ_weight), int(occ_samples)
        self.dist_span = None if dist_span is None else float(dist_span)
        self.ray_reg = self.dist_weight > 0.0 or self.occ_weight > 0.0        # the step with the two few-shot terms
        self.depth_smooth_weight, self.patch_size = float(depth_smooth_weight), int(patch_size)
        self.patch_reg = self.depth_smooth_weight > 0.0                       # the step with the patch-based depth-smoothness term
        self.ent_weight, self.ent_threshold, self.kl_weight = float(ent_weight), float(ent_threshold), float(kl_weight)
        self.info_reg = self.ent_weight > 0.0 or self.kl_weight > 0.0         # the step with InfoNeRF's ray entropy and / or patch KL term
        self._reg_kind = "info" if self.info_reg else "patch" if self.patch_reg else "reg" if self.ray_reg else None
        self.seed = None if seed is None else int(seed)
        self.white = int(bool(white_bkgd))
        self._plan, self._loss_vec, self.last_grad_norm = None, None, None     # the last step's _LossPlan and what its optimiser launch left
        self.last_count = None              # M of the last step under an occupancy grid (step_rays / step_view with occupancy=)
        self.last_patch_depth = None        # (n_patches, P, P) view of a buffer of this object: the last patch step's rendered depths
        # The buffer sets, {name: (key, {buffer name: tensor})}; each is built when first needed and again when its key changes (_set):
        #   plain  every step but the hierarchical one    ctx nbytes out4 d_out4 pred ray_loss grad
        #   ray    step_rays / step_view, beside plain     last_z rays_d
        #   grid   a step with occupancy=, beside ray      index slot pos count cws [dirs enc feats: the staged route's inputs]
        #   patch, info   the term buffers of a step with the patch / information terms
        #   hier   the hierarchical steps                  grad pred pred_coarse ray_loss last_z last_weights last_z_new + its own
        # _PUBLIC names the buffers a caller reads: a step points them at the sets it ran on.  A hierarchical step drops plain and ray,
        # so the plain step that follows it builds its own again; hier itself survives plain steps.
        self._sets = {}
        self.ctx = self.nbytes = self.out4 = self.d_out4 = self.pred = self.pred_coarse = self.ray_loss = self.grad = None
        self.last_z = self.last_weights = self.last_z_new = None

    _PUBLIC ={"plain": ("ctx", "nbytes", "out4", "d_out4", "pred", "ray_loss", "grad"), "ray": ("last_z",),
               "hier": ("grad", "pred", "pred_coarse", "ray_loss", "last_z", "last_weights", "last_z_new")}

    def _set(self, name, key, make):
        """These tensors for this key: buffer set `name`, built by make() when its key changes; its public names pointed at it."""
        s = self._sets.get(name)
        if s is None or s[0] != key:
            s = self._sets[name] = (key, make())
        b = s[1]
        for k in self._PUBLIC.get(name, ()):
            setattr(self, k, b[k])
        return b

    def _freq_reg(self):
        """The frequency mask of the step about to run, set on the model before anything of the step is packed."""
        if self.freq_reg_end <= 0:
            return
        from .positional_encoding import freq_mask_columns, freq_mask_visible
        m, t = self.model, self.opt.step_count
        pos = freq_mask_columns(m.pos_freq, freq_mask_visible(t, self.freq_reg_end, m.pos_freq))
        dirs = None
        if self.freq_reg_dirs and m.net != L.NRF_NET_V1:
            dirs = freq_mask_columns(m.dir_freq, freq_mask_visible(t, self.freq_reg_end, m.dir_freq))
        m.set_freq_mask(pos, dirs)

    @property
    def last_losses(self):
        """The last step's loss terms as device scalars (no sync): {'total'} of the plain step, {'total', 'rgb', 'depth', 'reg'}
        (nerf_mlp.NeRFLoss's dict, unweighted components) of the multi-term one, and 'dist', 'occ' behind them of the step with the
        few-shot ray regularisers, and 'smooth' behind those of the step with the patch term, and 'entropy' and 'kl' behind that of
        the step with ent_weight or kl_weight > 0; None before the first step."""
        return None if self._plan is None else self._plan.losses(self._loss_vec)

    def _buffers(self, n, R, S, dev, h, mode):
        """The plain step's buffers for n = R * S rows; returns their key, which the ray and the grid set share."""
        key = (n, R, S, str(dev), mode)

        def make():
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            ctx, nbytes = _context(h, mode, n, dev)
            # out4: V1: [rgb, sigma] rows; V2: rgb | density packed in the same rows
            # ray_loss row 0: squared rgb errors; rows 1, 2 (multi-term loss): sum of w^2, |depth error|; rows 3, 4 (ray regularisers): D_r, O_r
            return dict(ctx=ctx, nbytes=nbytes, out4=f(n, 4), d_out4=f(n, 4), pred=f(R, 3), ray_loss=f(_LOSS_KINDS[self._reg_kind or "mse"][3], R),
                        grad=torch.zeros(self.model.flat_params().flat.numel(), dtype=torch.float32, device=dev))
        self._set("plain", key, make)
        return key

    def _check_outputs(self, n, d_dino_out, points_out=None):
        """The refusals of the per-sample outputs a step over n = R * S samples can be handed."""
        m = self.model
        if d_dino_out is not None:
            if m.net != L.NRF_NET_V3 or not getattr(m, "dino_grad", False):
                raise ValueError("d_dino_out needs a use_dino model built with dino_grad=True")
            if (not d_dino_out.is_cuda or d_dino_out.dtype != torch.float32 or not d_dino_out.is_contiguous()
                    or d_dino_out.numel() != n * m.dino_dim):
                raise ValueError("d_dino_out must be a contiguous float32 (R*S, dino_dim) tensor on the GPU")
        if points_out is not None and (not points_out.is_cuda or points_out.dtype != torch.float32 or not points_out.is_contiguous()
                                       or points_out.numel() != n * 3):
            raise ValueError("points_out must be a contiguous float32 (R*S, 3) tensor on the GPU")

    def _loss_plan(self, R, S, dev, target_depth, noise, slot=None, span=None, n_patches=0):
        """The step's _LossPlan.  The multi-term step runs the general compositor/loss kernel and the clipped optimiser; its
        nrf_loss_opts is also built for the step under a grid (slot), whose one indexed kernel takes it either way -- with every option
        off its bits are the mse kernel's.  The noise seed of step t is seed + t: step_count is read before the step increments it.
        span: the depth range the distortion term's midpoints are scaled by."""
        opt, kind, f32 = self.opt, self._reg_kind, dict(dtype=torch.float32, device=dev)
        multi = (self.reg_weight > 0.0 or self.depth_weight > 0.0 or self.noise_std > 0.0 or opt.extended or target_depth is not None
                 or noise is not None or kind is not None)
        plan = _LossPlan(kind or ("indexed" if slot is not None else "multi" if multi else "mse"), multi)
        if plan.kind != "mse":
            td = None if target_depth is None else L.dev_f32(target_depth, dev).reshape(R - n_patches * self.patch_size ** 2)
            nz = None if noise is None or self.noise_std == 0.0 else L.dev_f32(noise, dev).reshape(R, S)
            seed = 0
            if self.noise_std > 0.0 and nz is None:
                if self.seed is None:
                    self.seed = L.fresh_seed()
                seed = self.seed + opt.step_count
            plan.lo = L.loss_opts(self.rgb_weight, self.reg_weight, self.depth_weight, L.ptr(td), self.noise_std, L.ptr(nz), seed)
            plan.keep, plan.depth = (td, nz), td is not None
        if kind is not None:
            span = self.dist_span if self.dist_span is not None else span
            if self.dist_weight > 0.0 and not (span is not None and math.isfinite(span) and span > 0.0):
                raise ValueError("dist_weight > 0 needs a depth range: pass dist_span= to FusedStep (__call__ has no near / far), "
                                 "or step with far > near")
            plan.reg = L.ray_reg(self.dist_weight, 1.0 / span if self.dist_weight > 0.0 else 0.0, self.occ_weight, self.occ_samples)
        if kind in ("patch", "info"):       # the rays' depths (and distributions) meet in LDS between the entry's forward and its backward
            P, n1 = self.patch_size, max(n_patches, 1)
            if self.kl_weight > 0.0 and P * P * S > L.INFO_KL_MAX_LDS_FLOATS:
                raise ValueError(f"kl_weight > 0 keeps a patch's distributions in LDS: patch_size^2 * n_samples = {P * P * S} exceeds "
                                 f"{L.INFO_KL_MAX_LDS_FLOATS}")
            t = self._set("patch", (n1, dev), lambda: dict(terms=torch.zeros((n1,), **f32), depth=torch.zeros((n1 * P * P,), **f32)))
            self.last_patch_depth = t["depth"][: n_patches * P * P].view(n_patches, P, P)
            plan.finish_tail = (C.byref(L.patch_reg(self.depth_smooth_weight, P, n_patches)), L.ptr(t["terms"]))
            plan.tail = plan.finish_tail + (L.ptr(t["depth"]),)
            if kind == "info":
                t = self._set("info", (R, n1, dev), lambda: dict(terms=torch.zeros((R,), **f32), kl=torch.zeros((n1,), **f32)))
                more = (C.byref(L.info_reg(self.ent_weight, self.ent_threshold, self.kl_weight)), L.ptr(t["terms"]), L.ptr(t["kl"]))
                plan.tail, plan.finish_tail = plan.tail + more, plan.finish_tail + more
        return plan

    def _patch_check(self, R, n_patches):
        """The refusals of n_patches on a batch of R rays; returns R_s, the number of supervised rays in front of the patch rays."""
        n_patches = int(n_patches)
        if n_patches < 0:
            raise ValueError("n_patches must be >= 0")
        if n_patches > 0 and not (self.patch_reg or self.info_reg):
            raise ValueError("n_patches > 0 needs a FusedStep built with depth_smooth_weight, kl_weight or ent_weight > 0")
        if n_patches == 0 and self.kl_weight > 0.0:
            raise ValueError("kl_weight > 0 acts on patch rays: pass n_patches > 0")
        Rs = R - n_patches * self.patch_size ** 2
        if Rs < 1:
            raise ValueError("the last n_patches * patch_size^2 rays of the batch are patch rays: at least one supervised ray must stand in front of them")
        return Rs

    def _launch_loss(self, heads, d_heads, z, d, tgt, R, S, dev, target_depth, noise, st, slot=None, span=None, n_patches=0):
        """compositor -> d loss / d pred = 2 w (pred - target) / (3 R) -> compositor backward, and the flat gradient vector cleared:
        one launch (a ray's loss gradient needs only its own prediction); the rays' squared errors stay in ray_loss.  slot (the step
        under a grid): the indexed kernel, or the regularised entry run indexed.  Returns the step's _LossPlan."""
        plan = self._loss_plan(R, S, dev, target_depth, noise, slot, span, n_patches)
        plan.launch(self, heads, d_heads, z, d, tgt, R, S, slot, st)
        return plan

    def _network_backward(self, h, mode, rows, out, d_out, ctx, st, d_dino_out=None, nbytes=None):
        """dZ chain + weight gradients over the first `rows` rows, added into the flat gradient vector [-> dL/d dino].  nbytes: of a
        context other than the plain step's (the hierarchical step holds two)."""
        lib = L.lib()
        nbytes = self.nbytes if nbytes is None else nbytes
        if self.model.net == L.NRF_NET_V1:
            L.check(lib.nrf_mlp_backward_v1(h, mode, L.ptr(out[0]), L.ptr(d_out[0]), rows, ctx, nbytes, L.ptr(self.grad), st))
        else:
            L.check(lib.nrf_mlp_backward(h, mode, L.ptr(out[0]), L.ptr(out[1]), L.ptr(d_out[0]), L.ptr(d_out[1]), rows, ctx, nbytes,
                                         L.ptr(self.grad), st))
            if d_dino_out is not None:
                _dino_grad(self.model, mode, rows, self.ctx, self.nbytes, d_dino_out.device, out=d_dino_out)

    def _finish(self, plan, R, S, dev, st, loss_weight=None):
        """[all-reduce ->] the optimiser's launch with the loss as its side job [-> the plan's launch behind it], the bookkeeping, and
        the parameters marked newer than the packed streams (call with the device current).  Returns the step's total loss (a device
        scalar).  loss_weight: the factor on sum(ray_loss[0]) / (3 R) when it is not rgb_weight (the hierarchical step's ray_loss
        carries its two weights already)."""
        opt = self.opt
        loss_weight = self.rgb_weight if loss_weight is None else loss_weight
        if self.data_parallel:
            _all_reduce_mean(self.grad, self.group)
        fp, flat = opt._buffers()
        opt.step_count += 1
        if plan.multi:
            # [norm partials ->] clipped Adam / AdamW, and as a side job of its launch the loss terms summed in a fixed order
            loss = torch.empty((4,), dtype=torch.float32, device=dev)
            opt._update(flat, self.grad, self.ray_loss, R, S, (loss_weight, self.depth_weight if plan.depth else 0.0, self.reg_weight), loss)
            loss = plan.finish(self, R, S, loss, st)
            self.last_grad_norm, total = opt.last_grad_norm, loss[0]
        else:
            # Adam, and as a side job of its launch the loss value: rgb_weight * sum(ray_loss) / (3 R) in a fixed order
            loss = total = torch.empty((), dtype=torch.float32, device=dev)
            L.check(L.lib().nrf_adam_step_loss(L.ptr(flat), L.ptr(self.grad), L.ptr(opt.exp_avg), L.ptr(opt.exp_avg_sq), flat.numel(), opt.lr,
                                               opt.betas[0], opt.betas[1], opt.eps, opt.weight_decay, opt.step_count, L.ptr(self.ray_loss), R,
                                               loss_weight, L.ptr(loss), st))
            self.last_grad_norm = None
        self._plan, self._loss_vec = plan, loss
        self.model._gen += 1
        return total

    @torch.no_grad()
    def __call__(self, points, z_vals, rays_d, target, dirs=None, dino=None, target_depth=None, noise=None, d_dino_out=None, n_patches=0):
        """target_depth (R): switches the depth term on (with depth_weight); noise (R,S): the standard normals of the density noise
        (with noise_std) instead of the in-kernel RNG -- what torch.randn_like would have drawn, for parity runs.
        d_dino_out: a preallocated (R*S, dino_dim) fp32 tensor that receives dL/d dino of this step (V3 with model.dino_grad: one
        more launch behind the weight gradients; project_fetch_backward turns it into the feature map's gradient).
        n_patches (a step built with depth_smooth_weight > 0): the last n_patches * patch_size^2 rays of the batch are patch rays
        (patch-major, row-major inside a patch); target and target_depth hold the rows of the other rays."""
        m = self.model
        if self.dist_weight > 0.0 and self.dist_span is None:
            raise ValueError("dist_weight > 0 needs dist_span= on a FusedStep that is called with depths: there is no near / far to take it from")
        if d_dino_out is not None:                  # (z_vals may still be a list when there is nothing to check)
            self._check_outputs(z_vals.numel(), d_dino_out)
        pts = L.dev_f32(points)
        dev = pts.device
        z = L.dev_f32(z_vals, dev)
        R, S = z.shape
        d = L.dev_f32(rays_d, dev).reshape(R, 3)
        n_patches = int(n_patches)
        tgt = L.dev_f32(target, dev).reshape(self._patch_check(R, n_patches), 3)
        v1 = m.net == L.NRF_NET_V1                                   # otherwise the trainer forms: positions + directions (+ DINO features)
        pts = pts.reshape(R * S, 3 * (2 * m.pos_freq + 1) if v1 else 3)
        n = R * S
        lib = L.lib()
        self._freq_reg()
        h, mode = _train_handle(m, dev)
        with torch.cuda.device(dev):
            self._buffers(n, R, S, dev, h, mode)
            st = L.stream_ptr()
            ctx = C.c_void_p(self.ctx.data_ptr())
            *out, heads = _heads(self.out4, n, v1)
            *d_out, d_heads = _heads(self.d_out4, n, v1)
            if v1:
                L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(pts), n, L.ptr(out[0]), ctx, self.nbytes, st))
            else:
                dirs_d = L.dev_f32(dirs, dev).reshape(n, 3)
                dino_d = L.dev_f32(dino, dev).reshape(n, m.dino_dim) if m.net == L.NRF_NET_V3 else None
                L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(pts), L.ptr(dirs_d), L.ptr(dino_d), n, L.ptr(out[0]), L.ptr(out[1]), ctx, self.nbytes, st))
            plan = self._launch_loss(heads, d_heads, z, d, tgt, R, S, dev, target_depth, noise, st, n_patches=n_patches)
            self._network_backward(h, mode, n, out, d_out, ctx, st, d_dino_out)
            return self._finish(plan, R, S, dev, st)

    # ---- the same step from rays: sampling, encoding and the feature fetch happen inside the saving forward ----------------
    @staticmethod
    def _rays_source(rays_o, rays_d, target):
        """Rays given by origin and direction, as the ray steps take them: (R, device, make_rays(z, d_out, p_out) -> nrf_train_rays, the
        (R,3) directions the compositor reads, target)."""
        o = L.dev_f32(rays_o).reshape(-1, 3)
        d = L.dev_f32(rays_d, o.device).reshape(-1, 3)
        if d.shape != o.shape:
            raise ValueError("rays_o and rays_d must both be (R,3)")
        return o.shape[0], o.device, lambda z, d_out, p_out=None: L.train_rays(rays_o=L.ptr(o), rays_d=L.ptr(d), z_vals=z, points_out=p_out), d, target

    @staticmethod
    def _view_source(image, pose, H, W, focal, pixels, target):
        """Pixels of a pinhole view, in the same form; the directions are None: the kernel writes them (d_out) for the compositor."""
        if not (isinstance(pixels, torch.Tensor) and pixels.is_cuda and pixels.dtype == torch.int64 and pixels.dim() == 1):
            raise ValueError("pixels must be a 1-d int64 tensor of ray ids on the GPU")
        pix = pixels.contiguous()
        H, W = int(H), int(W)
        if target is None:
            img = L.dev_f32(image, pix.device)
            if img.numel() != H * W * 3:
                raise ValueError("image must be (H,W,3) (or pass target=)")
            target = img.reshape(-1, 3)[pix]
        from .ray_sampler import _c2w12
        c2w = pose if isinstance(pose, C.Array) else _c2w12(pose)
        return (pix.shape[0], pix.device,
                lambda z, d_out, p_out=None: L.train_rays(pixels=pix.data_ptr(), H=H, W=W, focal=focal, c2w=c2w, z_vals=z, rays_d_out=d_out, points_out=p_out),
                None, target)

    def _prologue(self, R, S, dev, target, t_rand, dino, z_in=None, d_dino_out=None, points_out=None, n_patches=0):
        """What every ray step does before its buffers: the refusals of the batch, target, jitter and depths on the device, the DINO
        struct (V3), the frequency mask and the packed handle.  Returns (tgt, t_rand, z_in, nrf_dino, its tensors, handle, mode)."""
        if R < 1:
            raise ValueError("a step needs at least one ray")
        self._check_outputs(R * S, d_dino_out, points_out)
        tgt = L.dev_f32(target, dev).reshape(self._patch_check(R, n_patches), 3)
        tr = L.dev_f32(t_rand, dev).reshape(R, S) if t_rand is not None else None
        zin = L.dev_f32(z_in, dev).reshape(R, S) if z_in is not None else None
        dn = keep = None
        if self.model.net == L.NRF_NET_V3:
            if dino is None:
                raise ValueError("a use_dino model needs dino=dict(features=, pose=, focal=, H=, W=)")
            from .renderer import make_dino
            dn, keep = make_dino(**dino) if isinstance(dino, dict) else dino
        self._freq_reg()
        return (tgt, tr, zin, dn, keep) + _train_handle(self.model, dev)

    @torch.no_grad()
    def step_rays(self, rays_o, rays_d, target, near, far, n_samples, perturb=True, t_rand=None, seed=None, lindisp=False, z_in=None,
                  dino=None, target_depth=None, noise=None, d_dino_out=None, points_out=None, occupancy=None, grid_inputs="staged", n_patches=0):
        """One step on rays (R,3) and their target (R,3): what train.py:188-229 builds in front of the network -- stratified
        samples, per-sample directions, projected DINO features, encodings -- is derived inside the forward kernel
        (nrf_mlp_forward_train_rays), so no per-sample input tensor exists.  Depths, points and therefore (V2) every bit of the step
        are those of `self(points, z_vals, rays_d, target, dirs=...)` on `sample_points_along_rays(rays_o, rays_d, near, far,
        n_samples, perturb, lindisp, t_rand, seed)`.

            step = FusedStep(model, lr=5e-4)
            loss = step.step_rays(rays_o, rays_d, target, near=2.0, far=6.0, n_samples=64)                       # V1, V2
            loss = step.step_rays(rays_o, rays_d, target, 2.0, 6.0, 64, dino=dict(features=fmap, pose=pose, focal=f, H=H, W=W))   # V3

        t_rand (R,S): the jitter's uniforms instead of the counter RNG; z_in (R,S): explicit depths; dino: the renderer's dict of the
        source view (V3); points_out: a preallocated (R*S,3) tensor that receives the sample positions (what
        project_fetch_backward needs next to d_dino_out); target_depth, noise, d_dino_out, the returned loss, `last_losses` and
        `last_grad_norm` as in __call__.  `last_z` holds the step's (R,S) depths: a buffer of this object that the next ray step
        of the same shape overwrites -- clone it to keep it.  `dino` may also be the (struct, tensors) pair `renderer.make_dino`
        returned, for a caller that steps many batches on one source view.

        occupancy (an occupancy.OccupancyGrid): the step under the grid -- the plain step with every sample in an empty cell
        composited as colour 0 and effective density -inf (behind the density noise), and the network, its backward and the weight
        gradients run on the M occupied samples alone (_grid_forward).  UNLIKE THE PLAIN STEP IT SYNCHRONISES ONCE: the 8 bytes of
        M are read back between the compaction and the network.  `last_count` holds M.  Not combined with d_dino_out / points_out
        on the default route.

        grid_inputs (only with occupancy=): "staged" (default) feeds the M compacted points to the staged saving forward (V1:
        through nrf_encode, V3: through nrf_project_fetch); "rays" keeps the ray route's front end under the grid
        (nrf_mlp_forward_train_rays_indexed: ray, position, encoding and feature gather derived in the kernel for row index[j]).
        With "rays" d_dino_out and points_out are accepted: rows [0, M) of both hold the compacted samples in ascending flat-id
        order (the compaction writes its positions straight into points_out), rows >= M are not written.

        n_patches: as in __call__ -- the last n_patches * patch_size^2 rays are patch rays (ray_sampler.patch_rays writes them), target
        (R_s,3) and target_depth (R_s) belong to the rays in front of them; with or without occupancy=, on both grid_inputs routes."""
        return self._ray_step(*self._rays_source(rays_o, rays_d, target), near, far, n_samples, perturb, t_rand, seed, lindisp, z_in, dino,
                              target_depth, noise, d_dino_out, points_out, occupancy, grid_inputs, n_patches)

    @torch.no_grad()
    def step_view(self, image, pose, H, W, focal, pixels, near, far, n_samples, perturb=True, t_rand=None, seed=None, lindisp=False,
                  z_in=None, dino=None, target_depth=None, noise=None, d_dino_out=None, points_out=None, target=None, occupancy=None,
                  grid_inputs="staged"):
        """step_rays on pixels of a pinhole view: `pixels` is an int64 device tensor of ray ids y*W+x of get_rays(H, W, focal, pose),
        whose origins and directions the kernel computes itself.  The target is `target` (R,3) if given, otherwise
        image.reshape(-1,3)[pixels] of the (H,W,3) image: one torch gather.  The jitter of a ray is keyed by its position in
        `pixels`, not by the pixel id: the step equals step_rays on the gathered rays to the bit.  `pose` may also be the 12 floats
        `ray_sampler._c2w12` made of it (as `dino` may be `make_dino`'s pair): nothing is converted per batch then.  occupancy: as in
        step_rays (one 8-byte read-back per step), and so is grid_inputs.  A step built with depth_smooth_weight > 0 is refused: a
        view has one pose, and the patches come from poses of their own (step_rays)."""
        if self.patch_reg or self.kl_weight > 0.0:
            raise ValueError("step_view takes one pose per call: a FusedStep with depth_smooth_weight or kl_weight > 0 steps through step_rays or __call__")
        return self._ray_step(*self._view_source(image, pose, H, W, focal, pixels, target), near, far, n_samples, perturb, t_rand, seed, lindisp,
                              z_in, dino, target_depth, noise, d_dino_out, points_out, occupancy, grid_inputs)

    # ---- the hierarchical step: a coarse and a fine image of one network, every sample evaluated once --------------------------
    def _hier_check(self, n_samples, n_importance, coarse_weight, occupancy=None, d_dino_out=None, points_out=None):
        """The refusals of the hierarchical step, all decided on the host before a device is touched; returns (S, Ni, w_coarse,
        w_fine) with w_coarse = rgb_weight * coarse_weight formed as one fp32 product."""
        if self.reg_weight > 0.0 or self.depth_weight > 0.0 or self.noise_std > 0.0:
            raise ValueError("the hierarchical step takes the plain rgb loss: a FusedStep with reg_weight, depth_weight or noise_std > 0 is refused")
        if self.ray_reg:
            raise ValueError("the hierarchical step takes the plain rgb loss: a FusedStep with dist_weight or occ_weight > 0 is refused")
        if self.patch_reg:
            raise ValueError("the hierarchical step takes the plain rgb loss: a FusedStep with depth_smooth_weight > 0 is refused")
        if self.info_reg:
            raise ValueError("the hierarchical step takes the plain rgb loss: a FusedStep with ent_weight or kl_weight > 0 is refused")
        if occupancy is not None:
            raise ValueError("the hierarchical step is not combined with occupancy=")
        if d_dino_out is not None or points_out is not None:
            raise ValueError("the hierarchical step hands out no per-sample gradients: d_dino_out / points_out are refused")
        S, Ni = int(n_samples), int(n_importance)
        if Ni < 1:
            raise ValueError("n_importance must be >= 1 (step_rays / step_view are the step without resampling)")
        if S < 2:
            raise ValueError("n_samples must be >= 2: the resampling needs a bin")
        if S + Ni > 4096:
            raise ValueError("n_samples + n_importance must be <= 4096")
        cw = float(coarse_weight)
        if not cw >= 0.0:
            raise ValueError("coarse_weight must be >= 0")
        f32 = lambda x: C.c_float(x).value
        return S, Ni, f32(f32(self.rgb_weight) * f32(cw)), f32(self.rgb_weight)      # (the product of two fp32 values is exact in double)

    @torch.no_grad()
    def step_rays_hierarchical(self, rays_o, rays_d, target, near, far, n_samples, n_importance, perturb=True, t_rand=None, seed=None,
                               lindisp=False, u=None, dino=None, coarse_weight=1.0, occupancy=None, d_dino_out=None, points_out=None):
        """One step of NeRF's coarse-to-fine training on ONE network: the loss is

            rgb_weight * (coarse_weight * mse(pred_coarse, target) + mse(pred_fine, target))

        where pred_coarse composites the n_samples ladder samples and pred_fine the sorted union of those and n_importance depths
        drawn from the coarse weights by inverse-cdf resampling (render_hierarchical's fine pass).  Every sample is evaluated once,
        forward and backward -- n_samples + n_importance network rows per ray -- and the coarse rows receive the gradient of both
        images.  No gradient reaches the depths: the resampling is a constant, as in NeRF.  One fixed launch sequence on
        preallocated buffers, nothing synchronises:

            saving forward on the ladder -> nrf_composite (the coarse weights) -> nrf_sample_pdf_sorted -> saving forward on the
            new depths (a context of its own) -> nrf_composite_hier_loss_backward (both images, both losses, d rows of both row
            sets; clears the gradient vector) -> backward on the coarse context -> backward on the new one -> [all-reduce ->]
            the optimiser

        u: the resampling's uniforms, (R, n_importance) or one shared row (n_importance); default torch.rand on the device with
        perturb=True, the shared linspace(0, 1, n_importance) row with perturb=False (render_camera_hierarchical's).  t_rand, seed,
        lindisp, dino as in step_rays.  coarse_weight = 0 is allowed: the coarse rows then learn through the fine image alone.
        Kept for the caller, as buffers of this object like `last_z`: last_z (R,S), last_weights (R,S: what the resampling read),
        last_z_new (R,Ni), pred (the fine image), pred_coarse, grad.  `last_losses` = {'total', 'coarse', 'fine'}: the step's loss
        and the two unweighted mse terms, device scalars (the two terms are summed from the step's buffer when asked for: read them
        before the next hierarchical step).  max_grad_norm and decoupled_weight_decay act behind the gradient as in
        the plain step.  Refused with ValueError: a step object with reg_weight, depth_weight or noise_std > 0, occupancy=,
        d_dino_out=, points_out=, n_importance < 1, n_samples + n_importance > 4096, coarse_weight < 0."""
        chk = self._hier_check(n_samples, n_importance, coarse_weight, occupancy, d_dino_out, points_out)
        return self._hier_step(*self._rays_source(rays_o, rays_d, target), near, far, chk, perturb, t_rand, seed, lindisp, u, dino)

    @torch.no_grad()
    def step_view_hierarchical(self, image, pose, H, W, focal, pixels, near, far, n_samples, n_importance, perturb=True, t_rand=None,
                               seed=None, lindisp=False, u=None, dino=None, coarse_weight=1.0, target=None, occupancy=None, d_dino_out=None,
                               points_out=None):
        """step_rays_hierarchical on pixels of a pinhole view, as step_view is step_rays on them: `pixels` an int64 device tensor of
        ray ids, the target `target` (R,3) or image.reshape(-1,3)[pixels]; jitter and uniforms are keyed by the position in `pixels`,
        so the step equals step_rays_hierarchical on the gathered rays to the bit."""
        chk = self._hier_check(n_samples, n_importance, coarse_weight, occupancy, d_dino_out, points_out)
        return self._hier_step(*self._view_source(image, pose, H, W, focal, pixels, target), near, far, chk, perturb, t_rand, seed, lindisp, u, dino)

    def _hier_buffers(self, R, S, Ni, dev, h, mode):
        """The hierarchical step's buffers, kept apart from the plain step's (a FusedStep may take both kinds of step)."""
        def make():
            f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            b = {}
            b["ctx_c"], b["nbytes_c"] = _context(h, mode, R * S, dev)
            b["ctx_n"], b["nbytes_n"] = _context(h, mode, R * Ni, dev)
            for k, rows in (("c", R * S), ("n", R * Ni)):
                b["out4_" + k], b["d_out4_" + k] = f(rows, 4), f(rows, 4)
            b["pred"], b["pred_coarse"], b["rays_d"] = f(R, 3), f(R, 3), f(R, 3)
            b["ray_loss"] = torch.zeros((3, R), dtype=torch.float32, device=dev)     # row 0: w_c se_c + w_f se_f; rows 1, 2 stay 0 (the clipped optimiser's side job reads three rows)
            b["parts"] = f(2, R)
            b["last_z"], b["last_weights"], b["last_z_new"], b["z_new_out"] = f(R, S), f(R, S), f(R, Ni), f(R, Ni)
            b["ws"] = torch.empty((max(int(L.lib().nrf_hier_train_workspace_bytes(R, S, Ni)), 16) // 4,), dtype=torch.float32, device=dev)
            b["grad"] = torch.zeros(self.model.flat_params().flat.numel(), dtype=torch.float32, device=dev)
            return b
        self._sets.pop("plain", None)       # grad, pred, ray_loss and last_z leave the plain step's buffers: it takes its own again
        self._sets.pop("ray", None)
        return self._set("hier", (R, S, Ni, str(dev), mode), make)

    def _hier_step(self, R, dev, make_rays, d, target, near, far, chk, perturb, t_rand, seed, lindisp, u, dino):
        """The launch sequence of step_rays_hierarchical; d is the caller's (R,3) directions or None (pixel mode)."""
        from .renderer import _opts
        S, Ni, w_coarse, w_fine = chk
        m, lib = self.model, L.lib()
        v1 = m.net == L.NRF_NET_V1
        tgt, tr, _, dn, keep, h, mode = self._prologue(R, S, dev, target, t_rand, dino)
        with torch.cuda.device(dev):
            if u is None:
                uu, stride = (torch.rand((R, Ni), dtype=torch.float32, device=dev), Ni) if perturb else (L.u_row(Ni, dev), 0)
            else:
                uu = L.dev_f32(u, dev)
                if uu.numel() == Ni:
                    uu, stride = uu.reshape(Ni), 0
                elif uu.numel() == R * Ni:
                    uu, stride = uu.reshape(R, Ni), Ni
                else:
                    raise ValueError("u must be (R, n_importance) or one shared row (n_importance)")
            b = self._hier_buffers(R, S, Ni, dev, h, mode)
            z, w, z_new = b["last_z"], b["last_weights"], b["last_z_new"]
            if d is None:
                d = b["rays_d"]
            st = L.stream_ptr()
            train_mode = L.TRAIN_MODE[m.mma_mode]
            ctx_c, ctx_n = C.c_void_p(b["ctx_c"].data_ptr()), C.c_void_p(b["ctx_n"].data_ptr())
            *out_c, heads_c = _heads(b["out4_c"], R * S, v1)
            *d_out_c, d_heads_c = _heads(b["d_out4_c"], R * S, v1)
            *out_n, heads_n = _heads(b["out4_n"], R * Ni, v1)
            *d_out_n, d_heads_n = _heads(b["d_out4_n"], R * Ni, v1)
            # the coarse samples, their weights, the new depths, the new samples
            opts = _opts(near, far, S, perturb, tr, seed, lindisp, 0.0, self.white, train_mode, dn, dev)
            rays = make_rays(L.ptr(z), L.ptr(b["rays_d"]))
            L.check(lib.nrf_mlp_forward_train_rays(h, C.byref(rays), R, C.byref(opts), L.ptr(out_c[0]), L.ptr(out_c[1]), ctx_c, b["nbytes_c"], st))
            L.check(lib.nrf_composite(*heads_c, L.ptr(z), L.ptr(d), R, S, self.white, L.ptr(self.pred_coarse), None, L.ptr(w), st))
            L.check(lib.nrf_sample_pdf_sorted(L.ptr(z), L.ptr(w), R, S, Ni, L.ptr(uu), stride, None, L.ptr(z_new), None, st))
            opts_n = _opts(near, far, Ni, False, None, 0, lindisp, 0.0, self.white, train_mode, dn, dev, z_new)
            rays_n = make_rays(L.ptr(b["z_new_out"]), L.ptr(b["rays_d"]))
            L.check(lib.nrf_mlp_forward_train_rays(h, C.byref(rays_n), R, C.byref(opts_n), L.ptr(out_n[0]), L.ptr(out_n[1]), ctx_n, b["nbytes_n"], st))
            del keep, uu
            # both images, both losses, the d rows of both row sets (the coarse ones: both terms); the gradient vector cleared
            a = L.hier_loss(white_bkgd=self.white, rgb_stride=heads_c[1], sigma_stride=heads_c[3],
                            rgb_coarse=heads_c[0], sigma_coarse=_addr(heads_c[2]), rgb_new=heads_n[0], sigma_new=_addr(heads_n[2]),
                            z_coarse=L.ptr(z), z_new=L.ptr(z_new), rays_d=L.ptr(d), target=L.ptr(tgt), w_coarse=w_coarse, w_fine=w_fine,
                            d_rgb_coarse=d_heads_c[0], d_sigma_coarse=_addr(d_heads_c[2]), d_rgb_new=d_heads_n[0], d_sigma_new=_addr(d_heads_n[2]),
                            pred_coarse=L.ptr(self.pred_coarse), pred_fine=L.ptr(self.pred), ray_loss=L.ptr(self.ray_loss), ray_parts=L.ptr(b["parts"]),
                            zero_buf=L.ptr(self.grad), zero_n=self.grad.numel(), workspace=b["ws"].data_ptr(), workspace_bytes=b["ws"].numel() * 4)
            plan = _LossPlan("hier", self.opt.extended)
            plan.parts = (b["parts"], R)
            L.check(getattr(lib, plan.entry)(C.byref(a), R, S, Ni, st))
            self._network_backward(h, mode, R * S, out_c, d_out_c, ctx_c, st, nbytes=b["nbytes_c"])
            self._network_backward(h, mode, R * Ni, out_n, d_out_n, ctx_n, st, nbytes=b["nbytes_n"])
            return self._finish(plan, R, S + Ni, dev, st, loss_weight=1.0)

    def _ray_step(self, R, dev, make_rays, d, target, near, far, n_samples, perturb, t_rand, seed, lindisp, z_in, dino, target_depth, noise,
                  d_dino_out, points_out, occupancy=None, grid_inputs="staged", n_patches=0):
        """__call__'s sequence with nrf_mlp_forward_train_rays in front -- or, under an occupancy grid, _grid_forward; d is the
        caller's (R,3) directions or None (pixel mode: the kernel writes them for the compositor)."""
        from .renderer import _opts
        if grid_inputs not in ("staged", "rays"):
            raise ValueError('grid_inputs must be "staged" or "rays"')
        if occupancy is None and grid_inputs != "staged":
            raise ValueError("grid_inputs chooses the route of a step under a grid: pass occupancy= with it")
        by_rays = grid_inputs == "rays"
        if occupancy is not None:
            from .occupancy import OccupancyGrid
            if not by_rays and (d_dino_out is not None or points_out is not None):
                raise ValueError("occupancy is not combined with d_dino_out / points_out: the step under a grid hands out no per-sample gradients")
            if not isinstance(occupancy, OccupancyGrid):
                raise TypeError("occupancy must be an occupancy.OccupancyGrid")
        m, lib = self.model, L.lib()
        S, n_patches = int(n_samples), int(n_patches)
        n = R * S
        v1 = m.net == L.NRF_NET_V1
        tgt, tr, zin, dn, keep, h, mode = self._prologue(R, S, dev, target, t_rand, dino, z_in, d_dino_out, points_out, n_patches)
        with torch.cuda.device(dev):
            key = self._buffers(n, R, S, dev, h, mode)
            rb = self._set("ray", key, lambda: dict(last_z=torch.empty((R, S), dtype=torch.float32, device=dev),
                                                    rays_d=torch.empty((R, 3), dtype=torch.float32, device=dev)))
            z = self.last_z
            opts = _opts(near, far, S, perturb, tr, seed, lindisp, 0.0, self.white, L.TRAIN_MODE[m.mma_mode], dn, dev, zin)
            rays = make_rays(L.ptr(z), L.ptr(rb["rays_d"]), L.ptr(points_out))
            if d is None:
                d = rb["rays_d"]
            st = L.stream_ptr()
            ctx = C.c_void_p(self.ctx.data_ptr())
            *out, heads = _heads(self.out4, n, v1)
            *d_out, d_heads = _heads(self.d_out4, n, v1)
            if occupancy is not None:
                rows, slot = self._grid_forward(key, rays, R, S, dev, opts, occupancy, dn, h, mode, out, ctx, st, by_rays, points_out)
            else:
                L.check(lib.nrf_mlp_forward_train_rays(h, C.byref(rays), R, C.byref(opts), L.ptr(out[0]), L.ptr(out[1]), ctx, self.nbytes, st))
                rows, slot = n, None
            del keep
            plan = self._launch_loss(heads, d_heads, z, d, tgt, R, S, dev, target_depth, noise, st, slot, span=float(far) - float(near), n_patches=n_patches)
            if occupancy is None or rows:
                self._network_backward(h, mode, rows, out, d_out, ctx, st, d_dino_out)
            return self._finish(plan, R, S, dev, st)

    def _grid_forward(self, key, rays, R, S, dev, opts, occupancy, dn, h, mode, out, ctx, st, by_rays=False, points_out=None):
        """The saving forward of the step under an occupancy grid (nerfhip.h: nrf_occupancy_compact_rays); returns (M, the slot map of
        the indexed loss launch).  key: of the plain step's buffers, which the grid's share.  The step:

            compact -> read M back -> [V1: encode | V3: project + fetch] of the M points -> saving forward on M rows
            -> indexed compositor, loss and backward (clears the gradient vector) -> dZ chain + weight gradients on M rows
            -> [all-reduce] -> the plain step's optimiser launch

        The context and every buffer are sized once for R * S rows (the library accepts a larger context than M needs), so no
        step allocates.  The read-back of M (8 bytes) is the step's ONLY synchronisation and the one thing the plain step does not
        have: the launches behind it are sized by M on the host.  M == 0 is a valid step: the network launches nothing, the
        prediction is the background, the gradient is zero and the optimiser still steps.  With an all-ones grid every bit of the
        step is the plain step's (V2), or __call__'s on the staged points (V1: nrf_encode; V3: nrf_project_fetch).

        by_rays (grid_inputs="rays"): the bracket is gone -- the saving forward is nrf_mlp_forward_train_rays_indexed on the M rows of
        `index`, which derives every row from the ray source as the plain ray step does and reads neither the compacted positions
        nor directions.  The compaction still has to leave its positions somewhere: in points_out when the caller passed one.  With
        an all-ones grid every bit of the step is the plain ray step's, for all three families."""
        m, lib, n = self.model, L.lib(), R * S
        v1, v3 = m.net == L.NRF_NET_V1, m.net == L.NRF_NET_V3
        g = self._set("grid", key, lambda: dict(
            index=torch.empty((n,), dtype=torch.int32, device=dev), slot=torch.empty((n,), dtype=torch.int32, device=dev),
            pos=torch.empty((n, 3), dtype=torch.float32, device=dev), dirs=None, enc=None, feats=None,
            count=torch.zeros((1,), dtype=torch.int64, device=dev),
            cws=torch.empty((int(lib.nrf_occupancy_compact_workspace_bytes(R)),), dtype=torch.uint8, device=dev)))
        if not by_rays and g["dirs"] is None and g["enc"] is None:      # the staged route's per-sample inputs, on its first step
            g["dirs"] = None if v1 else torch.empty((n, 3), dtype=torch.float32, device=dev)
            g["enc"] = torch.empty((n, 3 * (2 * m.pos_freq + 1)), dtype=torch.float32, device=dev) if v1 else None
            g["feats"] = torch.empty((n, m.dino_dim), dtype=torch.float32, device=dev) if v3 else None
        occ, occ_keep = occupancy.struct(dev)
        pos = points_out if by_rays and points_out is not None else g["pos"]
        cp = L.compact(n, g["index"].data_ptr(), g["slot"].data_ptr(), L.ptr(pos), None if by_rays else L.ptr(g["dirs"]), g["count"].data_ptr(),
                       g["cws"].data_ptr(), g["cws"].numel())
        L.check(lib.nrf_occupancy_compact_rays(C.byref(rays), R, C.byref(opts), C.byref(occ), C.byref(cp), st))
        M = int(g["count"].item())         # the step's only synchronisation: 8 bytes
        self.last_count = M
        if M and by_rays:
            L.check(lib.nrf_mlp_forward_train_rays_indexed(h, C.byref(rays), R, C.byref(opts), g["index"].data_ptr(), M, L.ptr(out[0]), L.ptr(out[1]),
                                                           ctx, self.nbytes, st))
        elif M:
            if v1:
                L.check(lib.nrf_encode(L.ptr(g["pos"]), M, 3, m.pos_freq, 1, None, L.ptr(g["enc"]), st))
                L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(g["enc"]), M, L.ptr(out[0]), ctx, self.nbytes, st))
            else:
                if v3:
                    L.check(lib.nrf_project_fetch(C.byref(dn), L.ptr(g["pos"]), M, L.ptr(g["feats"]), None, st))
                L.check(lib.nrf_mlp_forward_train(h, mode, L.ptr(g["pos"]), L.ptr(g["dirs"]), L.ptr(g["feats"]), M, L.ptr(out[0]), L.ptr(out[1]),
                                                  ctx, self.nbytes, st))
        del occ_keep
        return M, g["slot"]
