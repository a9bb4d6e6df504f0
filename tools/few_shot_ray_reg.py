"""A record of what the few-shot ray regularisers do on tools/trained_scene.py's scene trained on 3 views -- kept in
profiles/ray_reg_few_shot.txt, quoted in DESIGN.md section 3.4.  Needs the GPU.  Not a pass / fail: the synthetic scene may show little.

    python tools/few_shot_ray_reg.py > profiles/ray_reg_few_shot.txt

One V2 field per cell of dist_weight in {0, 1e-3, 1e-2} x occ_weight in {0, 1e-2} (occ_samples = an eighth of the stage's samples: 4 of
32), each trained by trained_scene.train_field's loop (train_cli.train_epoch, the progressive schedule scaled to --epochs) from the
same seed, through `FusedStep(dist_weight=, occ_weight=, occ_samples=, dist_span=far - near)`.  Reported per cell: the PSNR of the
held-out views (bf16 render, 64 samples), the last epoch's loss, and -- on the held-out views' rays, 64 unjittered samples, through
the drop-in modules -- the mean weight mass in the first quarter of the ray and that mass over the ray's whole mass."""
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


def front_mass(model, scene_dir, size, S=64, rays_per_view=4096):
    """(mean_r sum_{i < S/4} w_i, mean_r of that sum over sum_i w_i) on the test views' rays."""
    import nerf_few_shot_limitations_amd as N
    dev = torch.device("cuda", torch.cuda.current_device())
    _, poses, (H, W, focal) = N.load_blender_data(scene_dir, "test", img_size=size)
    vr = N.VolumeRenderer()
    front, share = [], []
    with torch.no_grad():
        for pose in poses:
            ro, rd = N.get_rays(H, W, focal, pose.float().to(dev))
            ro, rd = ro.reshape(-1, 3)[:rays_per_view].contiguous(), rd.reshape(-1, 3)[:rays_per_view].contiguous()
            pts, z = N.sample_points_along_rays(ro, rd, NEAR, FAR, S, perturb=False)
            dirs = rd[:, None, :].expand(-1, S, 3).reshape(-1, 3).contiguous()
            c, sg = model(pts.reshape(-1, 3), dirs)
            _, _, w = vr(c.view(-1, S, 3), sg.view(-1, S, 1), z, rd)
            f, t = w[:, : S // 4].sum(1), w.sum(1)
            front.append(f.mean().item())
            share.append((f / t.clamp_min(1e-6)).mean().item())
    return sum(front) / len(front), sum(share) / len(share)


def cell(scene, cfg, size, views, epochs, dist_weight, occ_weight, seed):
    """trained_scene.train_field with the step's keywords switched on."""
    import nerf_few_shot_limitations_amd as N
    opts = dict(dist_weight=dist_weight, occ_weight=occ_weight, occ_samples=4 if occ_weight > 0 else 0, dist_span=FAR - NEAR)
    model, info, _ = trained_scene.train_field("v2", cfg, scene, "bf16", seed, epoch_scale=epochs / 200.0, sigma_bias=0.5, step_options=opts)
    images, poses, (H, W, focal) = N.load_blender_data(scene, "test", img_size=size)
    gt = images.permute(0, 2, 3, 1).contiguous().cuda()
    with torch.no_grad():
        img = N.evaluate_views(model, poses, H, W, focal, NEAR, FAR, 64, targets=None, mma_mode="bf16")["images"]
    front, share = front_mass(model.eval(), scene, size)
    return N.psnr(img, gt), info["loss_last_epoch"], front, share, info["train_seconds"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--test-views", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("few_shot_ray_reg needs the GPU: there is no CPU path")
    print(f"few-shot ray regularisers on the synthetic scene: V2, bf16, {a.views} training views at {a.size} px, {a.epochs} epochs of the progressive "
          f"schedule, seed {a.seed}; held-out: {a.test_views} views, bf16 render at 64 samples; occ_samples 4; dist_span = far - near = {FAR - NEAR:g}")
    print("dist_weight  occ_weight  held-out PSNR dB  last loss   front-quarter weight mass  its share of the ray's mass  train s")
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene")
        synthetic_scene.write_scene(scene, size=a.size, n_train=a.views, n_test=a.test_views)
        cfg = trained_scene.config(a.size, a.views, a.epochs)
        for dw in (0.0, 1e-3, 1e-2):
            for ow in (0.0, 1e-2):
                ps, loss, front, share, secs = cell(scene, cfg, a.size, a.views, a.epochs, dw, ow, a.seed)
                print(f"{dw:<11g}  {ow:<10g}  {ps:16.3f}  {loss:9.6f}  {front:25.5f}  {share:27.5f}  {secs:7.1f}", flush=True)
