#!/usr/bin/env python3
"""Capture the golden vectors of the V3 point gradient by running the REFERENCE's own modules under autograd.

Run in the build container only (needs the reference checkout, NERF_REFERENCE, as make_golden.py does):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_point_grad.py
Writes tests/golden/point_grads.npz -- inputs and the reference's outputs, nothing else.

The chain is the trainer's (train.py:203-229,280-287) with the one thing the reference never does: the rays and an explicit,
jittered depth ladder require grad.  points = o + z d -> project_points_to_image -> SpatialDINOFeatures.sample_features_at_points
(F.grid_sample) -> NeRFWithDINO (3 density layers) -> VolumeRenderer -> mse_loss -> loss.backward().  The source view is the
`orbit` view of dino_views.npz (NOT the rendered camera: all samples of a ray would project to one pixel and the feature path
would have no component along the ray) with a random 14 x 22 x 64 map.  Stored: the inputs, loss and pred, d_rays_o, d_rays_d,
d_z, the retained d_feats and d_points, and d_points_feat = the gradient of (feats . d_feats.detach()).sum() with respect to the
points -- the feature path alone, which is 100 to 3000 times smaller than the path through the positional encoding and has to
be compared at its own scale.  The 48 rays are the first clean ones of 400 candidates: no sample within 4e-5 of a ReLU
threshold (oracle.relu_margin), none within 1e-3 texel of a texel edge (the bilinear fetch has a kink there)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NERF_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "src"))
sys.path.insert(0, os.path.join(REF, "src", "models"))

from oracle import nerf_oracle as O  # noqa: E402  (only its input generators and relu_margin are used here)

from utils.ray_utils import get_rays as ref_get_rays_flat, sample_points_along_rays as ref_sample_flat  # noqa: E402
from utils.ray_utils import project_points_to_image as ref_project  # noqa: E402
import models.nerf_mlp as ref_mlp  # noqa: E402
import models.dino_feature_model as ref_dfm  # noqa: E402

torch.set_num_threads(4)
HP, WP, CH = 14, 22, 64


def npf(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def edge_distance(xy):
    """Distance, in texels, of every sample from the nearest texel edge of the (HP, WP) map (align_corners=False)."""
    gx, gy = ((xy[:, 0] + 1) * WP - 1) / 2, ((xy[:, 1] + 1) * HP - 1) / 2
    fx, fy = gx - torch.floor(gx), gy - torch.floor(gy)
    return torch.minimum(torch.minimum(fx, 1 - fx), torch.minimum(fy, 1 - fy))


def main():
    S, cand, R = 8, 400, 48
    views = np.load(os.path.join(HERE, "dino_views.npz"))
    pose = torch.from_numpy(views["orbit_pose"].copy())
    focal, Hs, Ws = float(views["orbit_focal"]), int(views["orbit_H"]), int(views["orbit_W"])
    sample = lambda fm, xy: ref_dfm.SpatialDINOFeatures.sample_features_at_points(types.SimpleNamespace(), fm, xy)  # noqa: E731
    with torch.no_grad():
        c2w = torch.from_numpy(O.LEGO_LIKE_C2W.copy())
        ro, rd = ref_get_rays_flat(20, 20, O.focal_for(20), c2w)
        ro, rd = ro.reshape(-1, 3)[:cand], rd.reshape(-1, 3)[:cand]
        tr = torch.from_numpy(O.uniform01(401, cand * S).reshape(cand, S)).float()
        orig = torch.rand
        torch.rand = lambda *a, **k: tr.clone()
        try:
            pts, z = ref_sample_flat(ro, rd, 2.0, 6.0, S, perturb=True)
        finally:
            torch.rand = orig
        dirs = rd.unsqueeze(1).expand(-1, S, -1)
        tgt_all = torch.from_numpy(O.uniform01(402, cand * 3).reshape(cand, 3)).float()
        fmap = torch.from_numpy(O.uniform01(403, HP * WP * CH).reshape(1, HP, WP, CH) * 2 - 1).float()
        p3 = O.make_weights("v3", 1, "solid", n_layers=3)
        xy_all = ref_project(pts.reshape(-1, 3), pose, focal, Hs, Ws)[0]
        feats_all = sample(fmap, xy_all)
        margin = O.relu_margin(p3, "v3", pts.reshape(-1, 3), dirs.reshape(-1, 3), feats_all)
        relu_ok = (margin.reshape(cand, S) > 4e-5).all(dim=1)
        edge_ok = (edge_distance(xy_all).reshape(cand, S) > 1e-3).all(dim=1)
        ok = (relu_ok & edge_ok).nonzero().flatten()
        print(f"clean rays: {ok.numel() / cand:.3f} of the candidates ({float(edge_ok.float().mean()):.3f} without the ReLU condition)")
        assert ok.numel() >= R, ok.numel()
        keep = ok[:R]
    m3 = ref_mlp.NeRFWithDINO(pos_freq=12, dir_freq=4, dino_dim=CH, hidden_dim=256, num_density_layers=3)
    sd = m3.state_dict()
    for k in sd:
        if k in p3:
            sd[k] = p3[k]
    m3.load_state_dict(sd)
    vr = ref_mlp.VolumeRenderer()
    o_l = ro[keep].clone().requires_grad_(True)
    d_l = rd[keep].clone().requires_grad_(True)
    z_l = z[keep].clone().requires_grad_(True)
    P = (o_l[:, None, :] + d_l[:, None, :] * z_l[:, :, None]).reshape(-1, 3)
    P.retain_grad()
    xy = ref_project(P, pose, focal, Hs, Ws)[0]
    feats = sample(fmap, xy)
    feats.retain_grad()
    col, dn = m3(P, d_l[:, None, :].expand(-1, S, -1).reshape(-1, 3), feats)
    rgb_map, _, _ = vr(col.reshape(R, S, 3), dn.reshape(R, S, 1), z_l, d_l)
    loss = torch.nn.functional.mse_loss(rgb_map, tgt_all[keep])
    loss.backward()
    # the feature path alone: the points' gradient of (feats . d_feats) with d_feats held fixed
    P2 = P.detach().clone().requires_grad_(True)
    f2 = sample(fmap, ref_project(P2, pose, focal, Hs, Ws)[0])
    (f2 * feats.grad.detach()).sum().backward()
    gx, gy = ((xy[:, 0] + 1) * WP - 1) / 2, ((xy[:, 1] + 1) * HP - 1) / 2
    on_map = float(((gx >= 0) & (gx <= WP - 1) & (gy >= 0) & (gy <= HP - 1)).float().mean())
    print(f"samples with all four taps on the map: {on_map:.2f}; max|d_points| {float(P.grad.abs().max()):.3g}; "
          f"max|d_points_feat| {float(P2.grad.abs().max()):.3g}; max|d_feats| {float(feats.grad.abs().max()):.3g}")
    out = dict(rays_o=npf(ro[keep]), rays_d=npf(rd[keep]), z=npf(z[keep]), target=npf(tgt_all[keep]), fmap=npf(fmap), pose=npf(pose),
               focal=np.float32(focal), H=Hs, W=Ws, pred=npf(rgb_map), loss=np.float32(loss.item()), d_rays_o=npf(o_l.grad), d_rays_d=npf(d_l.grad),
               d_z=npf(z_l.grad), d_feats=npf(feats.grad), d_points=npf(P.grad), d_points_feat=npf(P2.grad))
    path = os.path.join(HERE, "point_grads.npz")
    np.savez_compressed(path, **out)
    print(f"point_grads: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
