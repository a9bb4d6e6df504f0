"""A record of what the frequency mask (FreeNeRF's coarse-to-fine schedule on the positional encodings) does on
tools/trained_scene.py's scene trained on few views -- kept in profiles/freq_mask_few_shot.txt, quoted in DESIGN.md section 3.4.
Needs the GPU.  Not a pass / fail: the synthetic scene may show little.

    python tools/few_shot_freq_mask.py > profiles/freq_mask_few_shot.txt

One V2 field per cell of training views in {3, 8} x frequency mask {off, on} x occ_weight in {0, 1e-2} (occ_samples 4 of the first
stage's 32), each trained by trained_scene.train_field's loop (train_cli.train_epoch, the progressive schedule scaled to --epochs)
from the same seed.  "on" is `FusedStep(freq_reg_end=N)` with N = 90 % of the run's optimiser steps (counted on the cell without
the mask), on both encodings.  Reported per cell: the PSNR of the held-out views (bf16 render, 64 samples), the last epoch's loss,
the steps taken and the training time."""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import synthetic_scene  # noqa: E402
import trained_scene  # noqa: E402

NEAR, FAR = 2.0, 6.0


def cell(scene, cfg, size, epochs, freq_reg_end, occ_weight, seed):
    """trained_scene.train_field with the step's keywords switched on: (held-out PSNR, last loss, steps, seconds)."""
    import nerf_few_shot_limitations_amd as N
    opts = dict(freq_reg_end=freq_reg_end)
    if occ_weight > 0:
        opts.update(occ_weight=occ_weight, occ_samples=4)
    model, info, _ = trained_scene.train_field("v2", cfg, scene, "bf16", seed, epoch_scale=epochs / 200.0, sigma_bias=0.5, step_options=opts)
    assert model.freq_mask == (None, None) or freq_reg_end > info["steps"]        # the run ends with every band visible
    images, poses, (H, W, focal) = N.load_blender_data(scene, "test", img_size=size)
    gt = images.permute(0, 2, 3, 1).contiguous().cuda()
    with torch.no_grad():
        img = N.evaluate_views(model, poses, H, W, focal, NEAR, FAR, 64, targets=None, mma_mode="bf16")["images"]
    return N.psnr(img, gt), info["loss_last_epoch"], info["steps"], info["train_seconds"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--views", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--test-views", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("few_shot_freq_mask needs the GPU: there is no CPU path")
    print(f"frequency mask on the synthetic scene: V2, bf16, training views at {a.size} px, {a.epochs} epochs of the progressive schedule, seed {a.seed}; "
          f"held-out: {a.test_views} views, bf16 render at 64 samples; freq_reg_end = 90 % of the steps, both encodings; occ_samples 4")
    print("views  freq_reg_end  occ_weight  held-out PSNR dB  last loss   steps  train s")
    for views in a.views:
        with tempfile.TemporaryDirectory() as tmp:
            scene = os.path.join(tmp, "scene")
            synthetic_scene.write_scene(scene, size=a.size, n_train=views, n_test=a.test_views)
            cfg = trained_scene.config(a.size, views, a.epochs)
            end = 0
            for masked in (False, True):
                for ow in (0.0, 1e-2):
                    ps, loss, steps, secs = cell(scene, cfg, a.size, a.epochs, end if masked else 0, ow, a.seed)
                    print(f"{views:<5d}  {end if masked else 0:<12d}  {ow:<10g}  {ps:16.3f}  {loss:9.6f}  {steps:6d}  {secs:7.1f}", flush=True)
                    if not masked:
                        end = int(0.9 * steps)
