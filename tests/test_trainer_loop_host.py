"""Host side of the trainer-loop pin: tests/golden/trainer_loop.npz was recorded by the REFERENCE's own `NeRFDINOTrainer`
(src/training/train.py: get_rays_for_view, render_rays, train_step, evaluate, train; SURVEY.md D1-D4 repaired from outside by
tests/golden/make_golden_trainer.py).  Here: the oracle's reading of render_rays, and the host pieces of our loop that need no GPU
(`schedule_for`, `view_target`, `lr_at`) against what the trainer did.  The GPU side is tests/test_gpu_trainer_loop.py, which also
takes this module's fixture helpers.
"""
import json

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from nerf_few_shot_limitations_amd import train_cli

EPOCHS = (0, 50, 100)
RENDER_CASES = [("v2", "eval", 0), ("v2", "train", 0), ("v3", "eval", 1), ("v3", "train", 0), ("v3", "train", 1)]
NEAR, FAR = 2.0, 6.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def g(golden):
    return golden("trainer_loop")


def weights(variant):
    return O.make_weights("v2", 1, "fog") if variant == "v2" else O.make_weights("v3", 2, "fog")


def scene(g):
    """(training images (2,16,16,4) float, test images, poses, test poses, maps (2,4,4,64), H, W, focal) as CPU tensors."""
    img = T(g["images"].astype(np.float32) / 255.0)
    return img[:2], img[2:], T(g["poses"]), T(g["test_poses"]), T(g["maps"]), int(g["H"]), int(g["W"]), float(g["focal"])


def jitter(seed, n, S):
    return T(O.uniform01(int(seed), n * S).reshape(n, S))


class RecordedDraws:
    """The draws of one recorded epoch, in the order the reference's train_step made them: per view torch.randperm, then per batch
    torch.rand((n,S)) -- the `draws=` of train_cli.train_epoch.  A call out of that order is a difference in the loop."""

    def __init__(self, g, epoch):
        e = f"epoch{epoch}"
        self.kind, self.seed, self.n = g[e + "_draw_kind"], g[e + "_draw_seed"], g[e + "_draw_n"]
        self.k = 0

    def _take(self, is_perm, n):
        assert self.k < len(self.seed), "the loop asks for more draws than the reference made"
        assert bool(self.kind[self.k]) == is_perm and int(self.n[self.k]) == n, (self.k, bool(self.kind[self.k]), int(self.n[self.k]), is_perm, n)
        self.k += 1
        return int(self.seed[self.k - 1])

    def permutation(self, v, n):
        return T(np.argsort(O.uniform01(self._take(True, n), n), kind="stable"))

    def jitter(self, v, i, n, S):
        return jitter(self._take(False, n), n, S)

    def exhausted(self):
        return self.k == len(self.seed)


def view_permutations(g, epoch):
    """The recorded permutation of each view of an epoch."""
    e = f"epoch{epoch}"
    return [np.argsort(O.uniform01(int(s), int(n)), kind="stable")
            for kind, s, n in zip(g[e + "_draw_kind"], g[e + "_draw_seed"], g[e + "_draw_n"]) if kind]


def recorded_stage(g, epoch):
    """(H_train, W_train, scaled focal) of an epoch, as the trainer handed them to get_rays for its last cast of a view."""
    Ht, Wt, f = g[f"epoch{epoch}_cast"][-1]
    return int(Ht), int(Wt), float(f)


def param_sample(t, n):
    f = t.reshape(-1)
    return f[:: max(1, f.numel() // n)][:n]


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,mode,view", RENDER_CASES)
def test_oracle_render_rays_reproduces_the_trainers(g, variant, mode, view):
    """O.render_rays == NeRFDINOTrainer.render_rays at baseline.yaml's three stages (S = 32 / 48 / 64, 96 rays of the 32^2, 64^2, 128^2
    frames) and a ragged 37-ray call; eval mode conditions V3 on view 0's map whatever view_idx says, train mode on view_idx's."""
    p = weights(variant)
    _, _, poses, _, maps, _, _, _ = scene(g)
    feat = view if mode == "train" else 0                                                        # train.py:203-208
    dino = dict(features=maps[feat:feat + 1], pose=poses[feat], focal=float(g["render_focal"]), H=int(g["render_H"]), W=int(g["render_W"]))
    for k, (Hs, Ws, S, n) in enumerate(g["render_stages"]):
        key = f"render_{variant}_{mode}_view{view}_{k}"
        o, d = T(g[f"render_rays_o_view{view}_{k}"]), T(g[f"render_rays_d_view{view}_{k}"])
        assert o.shape == (n, 3)
        tr = jitter(g[key + "_seed"], int(n), int(S)) if mode == "train" else None
        out = O.render_rays(p, variant, o, d, NEAR, FAR, int(S), t_rand=tr, dino=dino if variant == "v3" else None)
        assert np.abs(out["rgb"].numpy() - g[key + "_rgb"]).max() <= 1e-5
        assert np.abs(out["depth"].numpy() - g[key + "_depth"]).max() <= 2e-5
        assert np.abs(out["weights"].numpy()[::4] - g[key + "_w"]).max() <= 1e-5


@pytest.mark.parametrize("variant", ["v2", "v3"])
def test_schedule_for_gives_the_recorded_stage_of_each_epoch(g, variant):
    cfg = json.loads(str(g[f"config_{variant}"]))
    for epoch in EPOCHS:
        Ht, Wt, S, batch = train_cli.schedule_for(cfg, epoch)
        assert (Ht, Wt) == recorded_stage(g, epoch)[:2]
        e = f"epoch{epoch}"
        assert (g[e + "_batch_S"] == S).all()
        sizes = [min(batch, Ht * Wt - i) for _ in range(2) for i in range(0, Ht * Wt, batch)]     # ragged last batch of each view
        assert g[e + "_batch_size"].tolist() == sizes and int(g[f"{e}_{variant}_steps"]) == len(sizes)
        assert g[e + "_batch_view"].tolist() == [v for v in range(2) for _ in range(0, Ht * Wt, batch)]


def test_view_target_focal_and_targets(g):
    """The focal the trainer cast the stage's rays with, exactly (epoch 100's 12x10 stage tells H- from W-scaling); the targets --
    alpha over white, THEN the bilinear resize with align_corners=False -- within 1e-6: four taps of values in [0,1], a few ulp of 1."""
    images, _, _, _, _, H, W, focal = scene(g)
    for epoch in EPOCHS:
        Ht, Wt, f_rec = recorded_stage(g, epoch)
        perms = view_permutations(g, epoch)
        rec = g[f"epoch{epoch}_target"]
        for v in range(2):
            tgt, f = train_cli.view_target(images[v], H, W, focal, Ht, Wt)
            assert f == f_rec, (epoch, f, f_rec)
            want = rec[v * Ht * Wt:(v + 1) * Ht * Wt]
            assert np.abs(tgt.numpy()[perms[v]] - want).max() <= 1e-6, epoch


def test_evaluation_targets_composite_over_white(g):
    """get_rays_for_view('test'): RGBA over white at the native size (what evaluate hands to its metrics, and its gt_*.png)."""
    _, test_images, _, _, _, H, W, focal = scene(g)
    for i in range(2):
        tgt, f = train_cli.view_target(test_images[i], H, W, focal, H, W)
        assert f == focal and np.abs(tgt.reshape(H, W, 3).numpy() - g[f"eval_target{i}"]).max() <= 1e-6


def test_stage_rays_equal_the_trainers_bit_for_bit(g):
    """The oracle's get_rays at the focal `view_target` returns == the rays the trainer batched, every stage, both poses (the rule of
    test_get_rays_bit_exact; the HIP get_rays is held to the same arrays in tests/test_gpu_trainer_loop.py)."""
    images, _, poses, _, _, H, W, focal = scene(g)
    for epoch in EPOCHS:
        Ht, Wt, _ = recorded_stage(g, epoch)
        perms = view_permutations(g, epoch)
        for v in range(2):
            _, f = train_cli.view_target(images[v], H, W, focal, Ht, Wt)
            ro, rd = O.get_rays(Ht, Wt, f, poses[v])
            sl = slice(v * Ht * Wt, (v + 1) * Ht * Wt)
            assert np.array_equal(rd.reshape(-1, 3).numpy()[perms[v]], g[f"epoch{epoch}_rays_d"][sl]), (epoch, v)
            assert np.array_equal(ro.reshape(-1, 3).numpy()[perms[v]], g[f"epoch{epoch}_rays_o"][sl]), (epoch, v)


@pytest.mark.parametrize("variant", ["v2", "v3"])
def test_lr_at_reproduces_the_recorded_schedule(g, variant):
    """MultiStepLR as `train` drives it: the lr in force while epoch e trained, and the one logged after its scheduler.step()."""
    cfg = json.loads(str(g[f"config_{variant}"]))
    in_force, logged = g[f"train_{variant}_step_lr"], g[f"train_{variant}_log_lr"]
    assert g[f"train_{variant}_log_epoch"].tolist() == list(range(len(logged))) and len(in_force) == len(logged) == cfg["training"]["epochs"]
    for e in range(len(logged)):
        assert train_cli.lr_at(cfg, e) == in_force[e] and train_cli.lr_at(cfg, e + 1) == logged[e]


def test_recorded_draws_are_consumed_in_the_reference_order(g):
    """RecordedDraws refuses a loop that draws in another order or another size."""
    d = RecordedDraws(g, 0)
    assert sorted(d.permutation(0, 64).tolist()) == list(range(64))
    with pytest.raises(AssertionError):
        d.permutation(0, 64)                                                                     # the trainer drew a batch's jitter next
    j = d.jitter(0, 0, 48, 8)
    assert j.shape == (48, 8) and 0 <= float(j.min()) and float(j.max()) < 1
