"""The DINO side channel as the reference's trainer calls it (src/training/train.py:203-214): project the sampled points
into the source view, then fetch that view's feature map at the projections.  Drop-ins for
`utils.ray_utils.project_points_to_image` (ray_utils.py:176-210) and
`SpatialDINOFeatures.sample_features_at_points` (dino_feature_model.py:114-148 == lora_dino.py:110-144 ==
multi_scale_dino.py:156-183) on libnerfhip's staged kernel; the fused renderer does both inside the kernel, the training
path (where the features are an input of NeRFMLP.forward) needs them as tensors.  The feature map itself comes from the
DINOv2 extractor (dino_feature_model.py); with `feature_grad=True` the fetch is differentiable with respect to the map, so
that the extractor in front of it trains; with `point_grad=True` both functions are differentiable with respect to the points
(fetch_points_backward_kernel), which is what carries a loss back to rays, depths and a pose through the DINO features."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .renderer import make_dino


class _ProjectFn(torch.autograd.Function):
    """nrf_project_fetch's projection with a backward: (N,3) points -> (N,2) normalised image points.  The adjoint is a handful of
    elementwise torch operations in the order fetch_points_backward_kernel (staged_kernels.hip) applies them -- one rounding per
    operation there (-ffp-contract=off) and here -- so that the route through the public pieces and render_rays' one node agree
    bit for bit."""

    @staticmethod
    def forward(ctx, pts, inv, focal, H, W):
        dev = pts.device
        n = pts.shape[0]
        dummy = torch.zeros((1, 1, 1, 1), dtype=torch.float32, device=dev)
        d = L.nrf_dino()
        d.features = dummy.data_ptr()
        d.Hp = d.Wp = d.C = 1
        d.inv_pose = (C.c_float * 16)(*inv)
        d.focal, d.H, d.W = float(focal), int(H), int(W)
        xy = torch.empty((n, 2), dtype=torch.float32, device=dev)
        feats = torch.empty((n, 1), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(pts), n, L.ptr(feats), L.ptr(xy), L.stream_ptr()))
        ctx.inv = [float(v) for v in d.inv_pose]                       # as the kernel reads them: fp32
        ctx.sx = float(np.float32(2.0) * np.float32(d.focal) / np.float32(W))
        ctx.sy = float(np.float32(2.0) * np.float32(d.focal) / np.float32(H))
        ctx.save_for_backward(pts)
        return xy

    @staticmethod
    def backward(ctx, g):
        (pts,) = ctx.saved_tensors
        inv = ctx.inv
        g = g.to(torch.float32)
        p0, p1, p2 = pts[:, 0], pts[:, 1], pts[:, 2]
        pc = [inv[4 * i] * p0 + inv[4 * i + 1] * p1 + inv[4 * i + 2] * p2 + inv[4 * i + 3] for i in range(3)]
        zi = pc[2] + 1e-8
        ax, ay = g[:, 0] * ctx.sx, g[:, 1] * ctx.sy
        dpc = [ax / zi, ay / zi, -(ax * pc[0] + ay * pc[1]) / (zi * zi)]
        d_pts = torch.stack([inv[j] * dpc[0] + inv[4 + j] * dpc[1] + inv[8 + j] * dpc[2] for j in range(3)], dim=-1)
        return d_pts, None, None, None, None


def project_points_to_image(points_3d, pose, focal, H, W, point_grad=False):
    """(N,3) world points -> (points_2d (N,2) in [-1,1], depths (N,), valid_mask (N,)) for the (4,4) camera-to-world `pose`.
    point_grad=True with points that require grad: points_2d and depths carry the points' gradient (none with respect to the
    pose or the intrinsics of the source view); default: the points are data."""
    L.require_gpu()
    if point_grad and torch.is_grad_enabled() and getattr(points_3d, "requires_grad", False):
        dev = points_3d.device if points_3d.is_cuda else torch.device("cuda", torch.cuda.current_device())
        live = points_3d.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
        inv = torch.inverse(torch.as_tensor(pose).detach().to("cpu", torch.float32))      # ray_utils.py:191, as renderer.make_dino
        xy = _ProjectFn.apply(live, inv.reshape(-1).tolist(), focal, H, W)
        invd = inv.to(dev)
        depths = live @ invd[2, :3] + invd[2, 3]
        return xy, depths, depths.detach() > 0
    pts = L.dev_f32(points_3d).reshape(-1, 3)
    n = pts.shape[0]
    dev = pts.device
    dummy = torch.zeros((1, 1, 1, 1), dtype=torch.float32, device=dev)               # the kernel fetches as it projects: a 1x1x1 map
    d, keep = make_dino(dummy, pose, focal, H, W)
    with torch.cuda.device(dev):
        xy = torch.empty((n, 2), dtype=torch.float32, device=dev)
        feats = torch.empty((n, 1), dtype=torch.float32, device=dev)
        L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(pts), n, L.ptr(feats), L.ptr(xy), L.stream_ptr()))
    # depth and the in-front mask are by-products the trainer discards (train.py:212 keeps the first output only)
    inv = torch.inverse(torch.as_tensor(pose).detach().to("cpu", torch.float32)).to(dev)
    depths = pts @ inv[2, :3] + inv[2, 3]
    return xy, depths, depths > 0


class _SampleFeaturesFn(torch.autograd.Function):
    """nrf_sample_features / nrf_sample_features_backward: (B,Hp,Wp,C) map, (N,2) points -> (B,N,C); gradient for the map only."""

    @staticmethod
    def forward(ctx, fm, xy):
        fm = fm.contiguous()
        B, Hp, Wp, Cc = (int(v) for v in fm.shape)
        n = xy.shape[0]
        out = torch.empty((B, n, Cc), dtype=torch.float32, device=fm.device)
        with torch.cuda.device(fm.device):
            for b in range(B):
                L.check(L.lib().nrf_sample_features(L.ptr(fm[b]), Hp, Wp, Cc, L.ptr(xy), n, L.ptr(out[b]), L.stream_ptr()))
        ctx.shape = (B, Hp, Wp, Cc)
        ctx.save_for_backward(xy)
        return out

    @staticmethod
    def backward(ctx, g):
        from .training import fetch_backward_workspace
        (xy,) = ctx.saved_tensors
        B, Hp, Wp, Cc = ctx.shape
        n = xy.shape[0]
        g = g.to(torch.float32).contiguous()
        d_map = torch.empty(ctx.shape, dtype=torch.float32, device=xy.device)
        with torch.cuda.device(xy.device):
            ws = fetch_backward_workspace(Hp, Wp, Cc, n, xy.device)
            for b in range(B):
                L.check(L.lib().nrf_sample_features_backward(Hp, Wp, Cc, L.ptr(xy), n, L.ptr(g[b]), L.ptr(d_map[b]), 0, L.ptr(ws), ws.numel() * 4,
                                                             L.stream_ptr()))
        return d_map, None


class _SampleFeaturesPointFn(torch.autograd.Function):
    """_SampleFeaturesFn that also returns d_xy (N,2), the adjoint of the fetch with respect to the points
    (nrf_sample_features_backward_points); d_map only when asked for."""

    @staticmethod
    def forward(ctx, fm, xy, want_map):
        fm = fm.contiguous()
        B, Hp, Wp, Cc = (int(v) for v in fm.shape)
        n = xy.shape[0]
        out = torch.empty((B, n, Cc), dtype=torch.float32, device=fm.device)
        with torch.cuda.device(fm.device):
            for b in range(B):
                L.check(L.lib().nrf_sample_features(L.ptr(fm[b]), Hp, Wp, Cc, L.ptr(xy), n, L.ptr(out[b]), L.stream_ptr()))
        ctx.shape, ctx.want_map = (B, Hp, Wp, Cc), bool(want_map)
        ctx.save_for_backward(fm, xy)
        return out

    @staticmethod
    def backward(ctx, g):
        from .training import fetch_backward_workspace
        fm, xy = ctx.saved_tensors
        B, Hp, Wp, Cc = ctx.shape
        n = xy.shape[0]
        g = g.to(torch.float32).contiguous()
        d_map = d_xy = None
        with torch.cuda.device(xy.device):
            if ctx.needs_input_grad[1]:
                for b in range(B):
                    d_b = torch.empty((n, 2), dtype=torch.float32, device=xy.device)
                    L.check(L.lib().nrf_sample_features_backward_points(L.ptr(fm[b]), Hp, Wp, Cc, L.ptr(xy), n, L.ptr(g[b]), L.ptr(d_b),
                                                                        L.stream_ptr()))
                    d_xy = d_b if d_xy is None else d_xy + d_b
            if ctx.want_map and ctx.needs_input_grad[0]:
                d_map = torch.empty(ctx.shape, dtype=torch.float32, device=xy.device)
                ws = fetch_backward_workspace(Hp, Wp, Cc, n, xy.device)
                for b in range(B):
                    L.check(L.lib().nrf_sample_features_backward(Hp, Wp, Cc, L.ptr(xy), n, L.ptr(g[b]), L.ptr(d_map[b]), 0, L.ptr(ws),
                                                                 ws.numel() * 4, L.stream_ptr()))
        return d_map, d_xy, None


def sample_features_at_points(features, points_2d, feature_grad=False, point_grad=False):
    """features (B,Hp,Wp,C) channel-last, points_2d (N,2) in [-1,1] -> (N,C) (B == 1) or (B,N,C): bilinear, zeros padding,
    align_corners=False.  feature_grad=True with a map that requires grad: the result carries the map's gradient (the adjoint
    kernel; none with respect to the points); default: a detached read, as the reference's precomputed maps are used.
    point_grad=True with points that require grad: the result carries the points' gradient too (piecewise: the fetch has a kink
    at every texel edge), and the map's when it is live and feature_grad=True."""
    L.require_gpu()
    if point_grad and torch.is_grad_enabled() and getattr(points_2d, "requires_grad", False):
        if features.dim() != 4:
            raise ValueError("features must be (B,Hp,Wp,C)")
        dev = points_2d.device if points_2d.is_cuda else torch.device("cuda", torch.cuda.current_device())
        xy = points_2d.to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous()
        want_map = bool(feature_grad and getattr(features, "requires_grad", False))
        fm = features.to(device=dev, dtype=torch.float32) if want_map else L.dev_f32(features, dev)
        out = _SampleFeaturesPointFn.apply(fm, xy, want_map)
        return out[0] if out.shape[0] == 1 else out
    if feature_grad and torch.is_grad_enabled() and getattr(features, "requires_grad", False):
        if features.dim() != 4:
            raise ValueError("features must be (B,Hp,Wp,C)")
        dev = features.device if features.is_cuda else torch.device("cuda", torch.cuda.current_device())
        xy = L.dev_f32(points_2d, dev).reshape(-1, 2)
        out = _SampleFeaturesFn.apply(features.to(device=dev, dtype=torch.float32), xy)
        return out[0] if out.shape[0] == 1 else out
    fm = L.dev_f32(features)
    if fm.dim() != 4:
        raise ValueError("features must be (B,Hp,Wp,C)")
    xy = L.dev_f32(points_2d, fm.device).reshape(-1, 2)
    n = xy.shape[0]
    B, Hp, Wp, Cc = (int(v) for v in fm.shape)
    out = torch.empty((B, n, Cc), dtype=torch.float32, device=fm.device)
    with torch.cuda.device(fm.device):
        for b in range(B):
            L.check(L.lib().nrf_sample_features(L.ptr(fm[b]), Hp, Wp, Cc, L.ptr(xy), n, L.ptr(out[b]), L.stream_ptr()))
    return out[0] if B == 1 else out
