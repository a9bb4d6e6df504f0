#!/usr/bin/env python3
"""Capture the golden vectors of the DINO feature-map gradient by running the REFERENCE's own modules under autograd.

Run in the build container only (needs the reference checkout, NERF_REFERENCE, as make_golden.py does):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dino_grad.py
Writes tests/golden/dino_grads.npz -- inputs and the reference's outputs, nothing else.

The chain is the trainer's (train.py:203-229,280-287) with the one thing the reference never does: the source view's feature
map requires grad.  project_points_to_image -> SpatialDINOFeatures.sample_features_at_points (F.grid_sample) -> NeRFWithDINO ->
VolumeRenderer -> mse_loss -> loss.backward(); stored: the inputs, the loss, d loss / d map, the retained d loss / d features and
a thinned subset of the parameter gradients.  Source view = the rendered camera's pose at 128 x 128; the rays are chosen among
candidates by oracle.relu_margin so that no ReLU sits on its threshold (make_golden.py: training())."""
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

from oracle import nerf_oracle as O  # noqa: E402  (only its input generators are used here)

from utils.ray_utils import get_rays as ref_get_rays_flat, sample_points_along_rays as ref_sample_flat  # noqa: E402
from utils.ray_utils import project_points_to_image as ref_project  # noqa: E402
import models.nerf_mlp as ref_mlp  # noqa: E402
import models.dino_feature_model as ref_dfm  # noqa: E402

torch.set_num_threads(4)


def npf(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def thin(t):
    """Large gradient matrices are stored as every 8th row (the fixture stays under 300 KB; the test slices the same way)."""
    return t[::8] if t.ndim == 2 and t.numel() > 20000 else t


# the stored subset of the parameter gradients: every bias, and the weights next to the feature input, the gate and the two ends
WEIGHTS = ("dino_fusion.fusion.0.weight", "dino_fusion.fusion.2.weight", "dino_fusion.attention.2.weight",
           "density_mlp.density_layers.0.weight", "color_mlp.color_layers.4.weight")


def main():
    S, cand, R = 8, 400, 48
    Hs = Ws = 128
    pose = torch.from_numpy(O.LEGO_LIKE_C2W.copy())
    focal = O.focal_for(Ws)
    with torch.no_grad():
        ro, rd = ref_get_rays_flat(20, 20, O.focal_for(20), pose)
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
        fmap0 = torch.from_numpy(O.uniform01(403, 81 * 64).reshape(1, 9, 9, 64) * 2 - 1).float()
        p3 = O.make_weights("v3", 1, "solid", n_layers=3)
        xy_all = ref_project(pts.reshape(-1, 3), pose, focal, Hs, Ws)[0]
        feats_all = ref_dfm.SpatialDINOFeatures.sample_features_at_points(types.SimpleNamespace(), fmap0, xy_all)
        margin = O.relu_margin(p3, "v3", pts.reshape(-1, 3), dirs.reshape(-1, 3), feats_all)
        ok = (margin.reshape(cand, S) > 4e-5).all(dim=1).nonzero().flatten()
        assert ok.numel() >= R, ok.numel()
        keep = ok[:R]
    m3 = ref_mlp.NeRFWithDINO(pos_freq=12, dir_freq=4, dino_dim=64, hidden_dim=256, num_density_layers=3)
    sd = m3.state_dict()
    for k in sd:
        if k in p3:
            sd[k] = p3[k]
    m3.load_state_dict(sd)
    vr = ref_mlp.VolumeRenderer()
    fmap = fmap0.clone().requires_grad_(True)
    P = pts[keep].reshape(-1, 3)
    xy = ref_project(P, pose, focal, Hs, Ws)[0]
    feats = ref_dfm.SpatialDINOFeatures.sample_features_at_points(types.SimpleNamespace(), fmap, xy)
    feats.retain_grad()
    col, dn = m3(P, dirs[keep].reshape(-1, 3), feats)
    rgb_map, _, _ = vr(col.reshape(R, S, 3), dn.reshape(R, S, 1), z[keep], rd[keep])
    loss = torch.nn.functional.mse_loss(rgb_map, tgt_all[keep])
    loss.backward()
    gx, gy = ((xy[:, 0] + 1) * 9 - 1) / 2, ((xy[:, 1] + 1) * 9 - 1) / 2
    on_map = float(((gx >= 0) & (gx <= 8) & (gy >= 0) & (gy <= 8)).float().mean())
    print(f"samples with all four taps on the map: {on_map:.2f} (the others exercise the zeros padding); max|d_map| {float(fmap.grad.abs().max()):.3g}; max|d_feats| {float(feats.grad.abs().max()):.3g}")
    out = dict(pts=npf(pts[keep]), dirs=npf(dirs[keep]), z=npf(z[keep]), rays_o=npf(ro[keep]), rays_d=npf(rd[keep]), target=npf(tgt_all[keep]),
               fmap=npf(fmap0), pose=npf(pose), focal=np.float32(focal), H=Hs, W=Ws, pred=npf(rgb_map),
               loss=np.float32(loss.item()), d_map=npf(fmap.grad), d_feats=npf(feats.grad))
    for k, q in m3.named_parameters():
        if k in p3 and (k.endswith(".bias") or k in WEIGHTS):
            out["grad_" + k] = npf(thin(q.grad))
    path = os.path.join(HERE, "dino_grads.npz")
    np.savez_compressed(path, **out)
    print(f"dino_grads: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
