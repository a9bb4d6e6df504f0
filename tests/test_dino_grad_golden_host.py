"""The oracle's fetch under autograd against the reference's own backward (tests/golden/dino_grads.npz, written by
tests/golden/make_golden_dino_grad.py): the GPU tests compare the adjoint kernels with this oracle on more sizes than the
fixture holds, so the oracle itself is pinned to the reference here, on the CPU."""
import numpy as np
import torch

from oracle import nerf_oracle as O


def test_oracle_fetch_gradient_matches_the_reference(golden):
    g = golden("dino_grads")
    fmap = torch.from_numpy(g["fmap"]).clone().requires_grad_(True)
    pts = torch.from_numpy(g["pts"]).reshape(-1, 3)
    xy = O.project_points_to_image(pts, torch.from_numpy(g["pose"]), float(g["focal"]), int(g["H"]), int(g["W"]))[0]
    feats = O.sample_features_at_points(fmap, xy)
    (feats * torch.from_numpy(g["d_feats"])).sum().backward()
    err = np.abs(fmap.grad.numpy() - g["d_map"]).max() / np.abs(g["d_map"]).max()
    assert err <= 5e-6, err
    assert g["d_map"].shape == (1, 9, 9, 64) and np.abs(g["d_map"]).max() > 0 and np.abs(g["d_feats"]).max() > 0


def test_fixture_holds_arrays_only(golden):
    g = golden("dino_grads")
    for k in g.files if hasattr(g, "files") else g:
        assert np.asarray(g[k]).dtype.kind in "fiub", k
