"""The DINO side channel as the reference's trainer calls it (src/training/train.py:203-214): project the sampled points
into the source view, then fetch that view's feature map at the projections.  Drop-ins for
`utils.ray_utils.project_points_to_image` (ray_utils.py:176-210) and
`SpatialDINOFeatures.sample_features_at_points` (dino_feature_model.py:114-148 == lora_dino.py:110-144 ==
multi_scale_dino.py:156-183) on libnerfhip's staged kernel; the fused renderer does both inside the kernel, the training
path (where the features are an input of NeRFMLP.forward) needs them as tensors.  The feature map itself comes from the
DINOv2 extractor (dino_feature_model.py); with `feature_grad=True` the fetch is differentiable with respect to the map, so
that the extractor in front of it trains."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .renderer import make_dino


def project_points_to_image(points_3d, pose, focal, H, W):
    """(N,3) world points -> (points_2d (N,2) in [-1,1], depths (N,), valid_mask (N,)) for the (4,4) camera-to-world `pose`."""
    L.require_gpu()
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


def sample_features_at_points(features, points_2d, feature_grad=False):
    """features (B,Hp,Wp,C) channel-last, points_2d (N,2) in [-1,1] -> (N,C) (B == 1) or (B,N,C): bilinear, zeros padding,
    align_corners=False.  feature_grad=True with a map that requires grad: the result carries the map's gradient (the adjoint
    kernel; none with respect to the points); default: a detached read, as the reference's precomputed maps are used."""
    L.require_gpu()
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
