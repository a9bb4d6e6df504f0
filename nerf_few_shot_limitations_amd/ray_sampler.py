"""Rays and stratified samples on the GPU (drop-in for the reference's
src/models/ray_sampler.py and src/utils/ray_utils.py:4-143).

Same names, argument order and shapes as the reference; the work is done by
libnerfhip.so (nrf_get_rays / nrf_sample_along_rays / nrf_sample_pdf).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L


def _c2w12(c2w) -> "C.Array":
    m = torch.as_tensor(c2w).detach().to("cpu", torch.float32)
    if m.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"c2w must be (4,4) or (3,4), got {tuple(m.shape)}")
    return (C.c_float * 12)(*m[:3, :4].reshape(-1).tolist())


class _GetRaysFn(torch.autograd.Function):
    """get_rays with a pose that requires grad: the staged kernel forward, and in torch the adjoint of rays_d = R dirs_cam,
    rays_o = t with the camera-frame directions of ray_sampler.py:4-30."""

    @staticmethod
    def forward(ctx, c2w, H, W, focal):
        rays_o, rays_d = get_rays(H, W, focal, c2w.detach())
        ctx.H, ctx.W, ctx.focal, ctx.shape = H, W, float(focal), tuple(c2w.shape)
        ctx.set_materialize_grads(False)
        return rays_o, rays_d

    @staticmethod
    def backward(ctx, g_o, g_d):
        H, W = ctx.H, ctx.W
        g = g_o if g_o is not None else g_d
        if g is None:
            return None, None, None, None
        d_c2w = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        if g_o is not None:
            d_c2w[:3, 3] = g_o.to(torch.float32).reshape(-1, 3).sum(0)
        if g_d is not None:
            x = torch.arange(W, dtype=torch.float32, device=g.device)[None, :].expand(H, W)
            y = torch.arange(H, dtype=torch.float32, device=g.device)[:, None].expand(H, W)
            cam = torch.stack([(x - W * 0.5) / ctx.focal, -(y - H * 0.5) / ctx.focal, -torch.ones_like(x)], -1).reshape(-1, 3)
            d_c2w[:3, :3] = g_d.to(torch.float32).reshape(-1, 3).t() @ cam
        return d_c2w, None, None, None


def get_rays(H, W, focal, c2w, pose_grad=False):
    """rays_o, rays_d of shape (H,W,3); ray id y*W+x.  ray_sampler.py:4-30 == ray_utils.py:4-37.
    pose_grad=True: a (4,4) / (3,4) c2w tensor that requires grad receives dL/d c2w (camera-pose refinement); the rays are the
    same bits."""
    L.require_gpu()
    H, W = int(H), int(W)
    if pose_grad and torch.is_grad_enabled() and isinstance(c2w, torch.Tensor) and c2w.requires_grad:
        if c2w.shape not in ((4, 4), (3, 4)):
            raise ValueError(f"c2w must be (4,4) or (3,4), got {tuple(c2w.shape)}")
        return _GetRaysFn.apply(c2w, H, W, focal)
    dev = c2w.device if isinstance(c2w, torch.Tensor) and c2w.is_cuda else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        rays_o = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        rays_d = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        L.check(L.lib().nrf_get_rays(H, W, float(focal), _c2w12(c2w), 0, H * W, L.ptr(rays_o), L.ptr(rays_d), L.stream_ptr()))
    return rays_o, rays_d


class _SampleFn(torch.autograd.Function):
    """sample_points_along_rays with rays that require grad: the staged kernel forward; backward nrf_ray_grad, the adjoint of
    pts = o + d z (the depths are the ladder's: constants) and of the expansion of rays_d over the samples (`dirs`, the per-sample
    view directions of train.py:225)."""

    @staticmethod
    def forward(ctx, o, d, args):
        pts, z = sample_points_along_rays(o.detach(), d.detach(), *args)
        S = z.shape[-1]
        dirs = d.detach().reshape(-1, 1, 3).expand(-1, S, 3).reshape(*z.shape, 3).contiguous()
        ctx.save_for_backward(z.reshape(-1, S), d.detach().reshape(-1, 3).contiguous())
        ctx.shape = tuple(o.shape)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(z)
        return pts, z, dirs

    @staticmethod
    def backward(ctx, g_pts, g_z, g_dirs):
        if g_pts is None and g_dirs is None:
            return None, None, None
        z, d = ctx.saved_tensors
        R, S = z.shape
        g = L.dev_f32(g_pts, z.device).reshape(R * S, 3) if g_pts is not None else torch.zeros((R * S, 3), dtype=torch.float32, device=z.device)
        gd = L.dev_f32(g_dirs, z.device).reshape(R * S, 3) if g_dirs is not None else None
        with torch.cuda.device(z.device):
            d_o, d_d = torch.empty_like(d), torch.empty_like(d)
            L.check(L.lib().nrf_ray_grad(L.ptr(g), L.ptr(gd), L.ptr(z), L.ptr(d), None, None, R, S, L.ptr(d_o), L.ptr(d_d), None, L.stream_ptr()))
        return d_o.reshape(ctx.shape), d_d.reshape(ctx.shape), None


def sample_points_along_rays(rays_o, rays_d, near, far, N_samples, perturb=True, lindisp=False, t_rand=None, seed=None, ray_grad=False,
                             return_dirs=False):
    """pts (...,S,3), z_vals (...,S) for rays of shape (N,3) or (H,W,3).

    ray_utils.py:39-84 (flat) == ray_sampler.py:32-61 (image).  `perturb=True`
    draws the stratified jitter from the kernel's counter RNG unless `t_rand`
    (same shape as z_vals, U[0,1)) is given.  seed=None (default): a NEW seed per
    call taken from torch's CPU generator, so that, as with the reference's
    torch.rand (ray_utils.py:78), consecutive calls jitter differently and a run
    repeats under torch.manual_seed; an int pins the pattern.
    ray_grad=True: rays that require grad receive gradients through pts (same
    bits as without the flag).  return_dirs=True adds the per-sample view
    directions (...,S,3), rays_d repeated over the samples (train.py:225); with
    ray_grad their gradient flows back into rays_d in the same launch.
    """
    L.require_gpu()
    if ray_grad and torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (rays_o, rays_d)):
        # rays that require grad receive gradients through pts; the forward is this function on the detached rays: the same bits
        if seed is None:
            seed = L.fresh_seed() if (perturb and t_rand is None) else 0
        dev = rays_o.device if isinstance(rays_o, torch.Tensor) and rays_o.is_cuda else torch.device("cuda", torch.cuda.current_device())
        o = torch.as_tensor(rays_o).to(device=dev, dtype=torch.float32)
        d = torch.as_tensor(rays_d).to(device=dev, dtype=torch.float32)
        pts, z, dirs = _SampleFn.apply(o, d, (near, far, N_samples, perturb, lindisp, t_rand, seed))
        return (pts, z, dirs) if return_dirs else (pts, z)
    o = L.dev_f32(L.refuse_grad(rays_o, "sample_points_along_rays(rays_o)"))
    d = L.dev_f32(L.refuse_grad(rays_d, "sample_points_along_rays(rays_d)"), o.device)
    if seed is None:
        seed = L.fresh_seed() if (perturb and t_rand is None) else 0
    lead = tuple(o.shape[:-1])
    if o.shape[-1] != 3 or d.shape != o.shape:
        raise ValueError("rays_o and rays_d must both be (...,3)")
    o2, d2 = o.reshape(-1, 3), d.reshape(-1, 3)
    R, S = o2.shape[0], int(N_samples)
    tr = None
    if t_rand is not None:
        tr = L.dev_f32(t_rand, o.device).reshape(R, S)
    with torch.cuda.device(o.device):
        pts = torch.empty((R, S, 3), dtype=torch.float32, device=o.device)
        z = torch.empty((R, S), dtype=torch.float32, device=o.device)
        lad = L.z_ladder(near, far, S, lindisp, o.device)
        L.check(L.lib().nrf_sample_along_rays(L.ptr(o2), L.ptr(d2), R, float(near), float(far), S, int(bool(lindisp)),
                                              int(bool(perturb) or tr is not None), L.ptr(tr), L.ptr(lad), int(seed), L.ptr(pts), L.ptr(z),
                                              L.stream_ptr()))
    if return_dirs:
        return pts.reshape(*lead, S, 3), z.reshape(*lead, S), d2[:, None, :].expand(R, S, 3).reshape(*lead, S, 3).contiguous()
    return pts.reshape(*lead, S, 3), z.reshape(*lead, S)


def hierarchical_sampling(rays_o, rays_d, z_vals, weights, N_importance, perturb=True, u=None):
    """Importance resampling: returns (pts (R,S+Ni,3), z_union (R,S+Ni)) like ray_utils.py:86-143.

    The reference function raises on every input; this is its
    intent with bin EDGES (see oracle/nerf_oracle.py:sample_pdf).  `perturb`
    needs explicit `u` (R,Ni) in [0,1); otherwise u = linspace(0,1,Ni).
    """
    L.require_gpu()
    z = L.dev_f32(z_vals)
    w = L.dev_f32(weights, z.device)
    R, S = z.shape
    Ni = int(N_importance)
    if u is not None:
        uu, stride = L.dev_f32(u, z.device).reshape(R, Ni), Ni
    elif perturb:
        uu, stride = torch.rand((R, Ni), dtype=torch.float32, device=z.device), Ni
    else:
        uu, stride = L.u_row(Ni, z.device), 0                        # ray_utils.py:115-116: linspace(0,1,Ni) as this host computes it
    with torch.cuda.device(z.device):
        union = torch.empty((R, S + Ni), dtype=torch.float32, device=z.device)
        L.check(L.lib().nrf_sample_pdf(L.ptr(z), L.ptr(w), R, S, Ni, L.ptr(uu), stride, None, L.ptr(union), L.stream_ptr()))
    o = L.dev_f32(rays_o, z.device).reshape(R, 3)
    d = L.dev_f32(rays_d, z.device).reshape(R, 3)
    pts = o[:, None, :] + d[:, None, :] * union[:, :, None]
    return pts, union


def sample_pdf(z_vals, weights, N_importance, u=None):
    """(new samples (R,Ni), sorted union (R,S+Ni)) -- the staged form of hierarchical_sampling."""
    L.require_gpu()
    z = L.dev_f32(z_vals)
    w = L.dev_f32(weights, z.device)
    R, S = z.shape
    Ni = int(N_importance)
    uu, stride = (L.u_row(Ni, z.device), 0) if u is None else (L.dev_f32(u, z.device).reshape(R, Ni), Ni)
    with torch.cuda.device(z.device):
        smp = torch.empty((R, Ni), dtype=torch.float32, device=z.device)
        union = torch.empty((R, S + Ni), dtype=torch.float32, device=z.device)
        L.check(L.lib().nrf_sample_pdf(L.ptr(z), L.ptr(w), R, S, Ni, L.ptr(uu), stride, L.ptr(smp), L.ptr(union), L.stream_ptr()))
    return smp, union


def sample_pdf_sorted(z_vals, weights, N_importance, u=None, out=None):
    """The new samples (R,Ni) of sample_pdf in ascending order -- the row the kernel merges into the sorted union (equal values keep
    the order of `u`).  `out`: a contiguous (R,Ni) fp32 tensor to fill."""
    L.require_gpu()
    z = L.dev_f32(z_vals)
    w = L.dev_f32(weights, z.device)
    R, S = z.shape
    Ni = int(N_importance)
    uu, stride = (L.u_row(Ni, z.device), 0) if u is None else (L.dev_f32(u, z.device).reshape(R, Ni), Ni)
    with torch.cuda.device(z.device):
        srt = out if out is not None else torch.empty((R, Ni), dtype=torch.float32, device=z.device)
        L.check(L.lib().nrf_sample_pdf_sorted(L.ptr(z), L.ptr(w), R, S, Ni, L.ptr(uu), stride, None, L.ptr(srt), None, L.stream_ptr()))
    return srt


# ---- patches of unseen views (RegNeRF's depth-smoothness term: FusedStep(depth_smooth_weight=), n_patches=) -- plain torch ----------
def patch_pixels(H, W, patch_size, n_patches, generator=None, stride=1):
    """int64 ray ids y*W+x of n_patches random windows of patch_size x patch_size pixels that lie inside an (H,W) image, flat in the
    batch layout of the patch term: patch-major, row-major inside a patch (id k of patch p is element p*P*P + k).  stride dilates a
    window: neighbouring patch pixels are `stride` image pixels apart.  The draw comes from `generator` (a CPU torch.Generator; None:
    torch's global one), so it repeats under a seed."""
    H, W, P, n, st = int(H), int(W), int(patch_size), int(n_patches), int(stride)
    if P < 2 or P > 16:
        raise ValueError("patch_size must be in 2 ... 16")
    if n < 0 or st < 1:
        raise ValueError("n_patches must be >= 0 and stride >= 1")
    ext = (P - 1) * st + 1
    if ext > H or ext > W:
        raise ValueError(f"a {P} x {P} window of stride {st} spans {ext} pixels: it does not fit a {H} x {W} image")
    y0 = torch.randint(0, H - ext + 1, (n,), generator=generator, dtype=torch.int64)
    x0 = torch.randint(0, W - ext + 1, (n,), generator=generator, dtype=torch.int64)
    k = torch.arange(P, dtype=torch.int64) * st
    ids = (y0[:, None, None] + k[None, :, None]) * W + (x0[:, None, None] + k[None, None, :])
    return ids.reshape(-1)


def sample_patch_poses(train_poses, n, generator=None, focus_jitter=0.125):
    """n camera-to-world matrices (n,4,4) of views nobody observed, from the (V,4,4) / (V,3,4) training poses: positions uniform in
    the bounding box of the training cameras' positions and rescaled to their mean distance from the origin, every camera looking
    at the origin + N(0, focus_jitter^2), up the mean training up vector.  The columns are the camera's right, up and backward axes
    (it looks down -z, as get_rays has it): orthonormal, det = +1.  Returned on the CPU in float32."""
    p = torch.as_tensor(train_poses).detach().to("cpu", torch.float64)
    if p.dim() != 3 or tuple(p.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError("train_poses must be (V,4,4) or (V,3,4)")
    n = int(n)
    pos = p[:, :3, 3]
    lo, hi = pos.amin(dim=0), pos.amax(dim=0)
    radius = pos.norm(dim=1).mean()
    up = p[:, :3, 1].mean(dim=0)
    up = up / up.norm().clamp_min(1e-12)
    u = torch.rand((n, 3), generator=generator, dtype=torch.float64)
    c = lo + (hi - lo) * u
    c = c * (radius / c.norm(dim=1, keepdim=True).clamp_min(1e-12))
    focus = torch.randn((n, 3), generator=generator, dtype=torch.float64) * float(focus_jitter)
    zax = c - focus
    zax = zax / zax.norm(dim=1, keepdim=True).clamp_min(1e-12)
    xax = torch.linalg.cross(up.expand(n, 3), zax)
    xax = xax / xax.norm(dim=1, keepdim=True).clamp_min(1e-12)
    yax = torch.linalg.cross(zax, xax)
    out = torch.zeros((n, 4, 4), dtype=torch.float64)
    out[:, :3, 0], out[:, :3, 1], out[:, :3, 2], out[:, :3, 3] = xax, yax, zax, c
    out[:, 3, 3] = 1.0
    return out.to(torch.float32)


def patch_rays(H, W, focal, poses, patch_size, generator=None, stride=1):
    """(rays_o, rays_d), each (n * P * P, 3) in the patch term's batch layout: one window of patch_pixels per pose of `poses`
    (n,4,4) / (n,3,4), the rays written with get_rays' formula -- rays_d = R ((x - W/2) / focal, -(y - H/2) / focal, -1), rays_o = t --
    on the device of `poses`.  The windows are patch_pixels(H, W, patch_size, n, generator, stride)."""
    c2w = torch.as_tensor(poses).to(torch.float32)
    if c2w.dim() != 3 or tuple(c2w.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError("poses must be (n,4,4) or (n,3,4)")
    n, P = c2w.shape[0], int(patch_size)
    ids = patch_pixels(H, W, P, n, generator, stride).reshape(n, P * P).to(c2w.device)
    x, y = (ids % int(W)).to(torch.float32), (ids // int(W)).to(torch.float32)
    cam = torch.stack([(x - int(W) * 0.5) / float(focal), -(y - int(H) * 0.5) / float(focal), -torch.ones_like(x)], dim=-1)      # (n, P*P, 3)
    rot = c2w[:, None, :3, :3]
    rays_d = cam[..., 0:1] * rot[..., 0] + cam[..., 1:2] * rot[..., 1] + cam[..., 2:3] * rot[..., 2]
    rays_o = c2w[:, None, :3, 3].expand(n, P * P, 3)
    return rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()


def get_ray_batch(rays_o, rays_d, batch_size=1024):
    """ray_utils.py:145-174: host-side chunk generator, kept for callers that still chunk
    (the fused renderer does not need it)."""
    H, W = rays_o.shape[:2]
    n = H * W
    o, d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    idx = torch.arange(n, device=o.device)
    for i in range(0, n, batch_size):
        yield o[i:i + batch_size], d[i:i + batch_size], idx[i:i + batch_size]
