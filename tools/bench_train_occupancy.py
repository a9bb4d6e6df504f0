"""Measured cost and gain of training under an occupancy grid (FusedStep.step_rays with occupancy=: compaction in front of the network,
one 8-byte read-back, the network and its backward on the occupied samples alone) -- the numbers quoted in DESIGN.md sections
3.4 / 7 and kept in profiles/train_occupancy_step_time.txt.  Needs the GPU.

    python tools/bench_train_occupancy.py > profiles/train_occupancy_step_time.txt

Every row is one batch shape (2048 rays x 32 and x 64 samples, bf16) and one field; its arms take turns in ONE process:
    plain   : step_rays without a grid -- the parent's step, nothing synchronises;
    ones    : step_rays under an all-ones grid -- every sample evaluated: the difference to `plain` is what compaction, the read-back
              and the staged inputs (points and directions in memory instead of derived in the forward kernel) cost;
    grid k  : grids of falling occupied share.
The learning rate is 0, so that the field -- and with it M -- stays what it is while the arms alternate.  Two timings:
    blocks  : `--block` steps of one arm back to back, one synchronisation behind the block, wall clock / steps: how a training loop
              runs (the plain step's launches overlap the host; the grid step's read-back drains the queue once per step);
    single  : one step between two synchronisations, the arms alternating step by step: the latency of one step.
a) "solid" V1 / V2 weights (dense everywhere): plain against ones alone.
b) the V2 field fitted by tools/trained_scene.py, rays of its training views: from_model grids over [-4, 4]^3 at rising density
   thresholds.  The break-even share is where the least-squares line through the grid arms' (M / (R S), ms) meets the plain step.

    python tools/bench_train_occupancy.py --rays > profiles/train_occupancy_rays_step_time.txt

The two routes of the step under a grid against each other (grid_inputs="staged" | "rays": DESIGN.md section 3.4), for V1, V2 and V3
(dino_dim 64) "solid" weights at the same shapes: plain, and each route under the all-ones grid and under a sparse one (a ball of
cells around the ray origins that keeps about a sixth of the samples) -- five arms alternating in one process, timed as above.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import nerf_few_shot_limitations_amd as N  # noqa: E402
from nerf_few_shot_limitations_amd.training import FusedStep  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

NEAR, FAR = 2.0, 6.0


def make(net, scene, mode):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
        m.load_state_dict(O.make_weights("v1", 0, scene))
    elif net == "v3":
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=64, mma_mode=mode)
        m.load_state_dict(O.make_weights("v3", 2, scene, dino_dim=64), strict=False)
    else:
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=mode)
        m.load_state_dict(O.make_weights("v2", 1, scene), strict=False)
    return m.cuda().train()


def fmt(a):
    a = np.asarray(a)
    return f"{np.median(a):.4f} [{a.min():.4f} .. {a.max():.4f}]"


def time_arms(arms, steps, warmup, block):
    """arms: {label: callable running one step}.  Returns ({label: ms per step of each block}, {label: ms of each single step})."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    blocks, single = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(max(1, steps // block)):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) * 1e3 / block)
    for _ in range(steps):
        for k, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            single[k].append((time.perf_counter() - t0) * 1e3)
    return blocks, single


def run_row(label, model, o, d, tgt, S, grids, steps, warmup, block, dino=None):
    """grids: [(label, OccupancyGrid or None[, grid_inputs])].  One FusedStep (lr = 0) serves every arm: the buffers are sized once for
    R * S.  dino: the source view of a V3 model."""
    step = FusedStep(model, lr=0.0)
    R = o.shape[0]
    counts = {}
    routes = {g[0]: (g[2] if len(g) > 2 else "staged") for g in grids}
    grids = [(g[0], g[1]) for g in grids]

    def arm(name, grid):
        kw = {} if grid is None else dict(occupancy=grid, grid_inputs=routes[name])
        if dino is not None:
            kw["dino"] = dino

        def fn():
            step.step_rays(o, d, tgt, NEAR, FAR, S, perturb=True, seed=11, **kw)
            if grid is not None:
                counts[name] = step.last_count
        return fn

    arms = {name: arm(name, g) for name, g in grids}
    blocks, single = time_arms(arms, steps, warmup, block)
    plain = np.median(blocks["plain"])
    print(f"{label}, {R} x {S}:")
    for name, g in grids:
        share = "" if g is None else f"   M / (R S) = {counts[name] / (R * S):.4f}   occupied cells {g.occupied_fraction:.4f}"
        print(f"    {name:<12} blocks {fmt(blocks[name])} ms / step ({np.median(blocks[name]) / plain:.3f} of plain)   single {fmt(single[name])} ms{share}",
              flush=True)
    for name, g in grids:
        if g is not None and routes[name] == "rays":
            twin = name.replace("rays", "staged")
            print(f"    {name} / {twin}: {np.median(blocks[name]) / np.median(blocks[twin]):.3f} (blocks)   "
                  f"{np.median(single[name]) / np.median(single[twin]):.3f} (single)", flush=True)
    pts = [(counts[name] / (R * S), np.median(blocks[name])) for name, g in grids if g is not None and routes[name] == "staged"]
    if len(pts) >= 3:
        x, y = np.array(pts).T
        slope, icpt = np.polyfit(x, y, 1)
        be = (plain - icpt) / slope if slope > 0 else float("nan")
        print(f"    line through the grid arms: {icpt:.4f} ms + {slope:.4f} ms x share; meets the plain step ({plain:.4f} ms) at M / (R S) = {be:.3f}", flush=True)


def report(steps, warmup, block, epochs, mode="bf16", R=2048):
    import synthetic_scene
    import trained_scene
    dev = torch.device("cuda", 0)
    print(f"training step under an occupancy grid, {mode}, {R} rays; lr = 0 (the field stays put); {steps} steps per arm after {warmup} warm-up steps, blocks "
          f"of {block}; wall clock, ms = median [min .. max]")
    ones = N.OccupancyGrid.full(128, -4.0, 4.0, device=dev)
    print('a) "solid" weights, rays from around the origin: the all-ones grid against the plain step')
    o = (torch.rand(R, 3, generator=torch.Generator().manual_seed(1)) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=torch.Generator().manual_seed(2)) - 0.5, dim=-1).cuda().contiguous()
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(3)).cuda()
    for net in ("v1", "v2"):
        for S in (32, 64):
            run_row(f"  {net} solid", make(net, "solid", mode), o, d, tgt, S, [("plain", None), ("ones", ones)], steps, warmup, block)
    size, views = 128, 8
    print(f"b) the V2 field fitted by tools/trained_scene.py ({epochs} epochs, {views} views of {size} px), {R} random rays of its training views; "
          "grids: from_model, 128^3 over [-4, 4]^3, 4 probes per cell, dilate 1, at rising thresholds")
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene")
        synthetic_scene.write_scene(scene, size=size, n_train=views, n_test=1)
        model, info, _ = trained_scene.train_field("v2", trained_scene.config(size, views, epochs), scene, mode, 0, epoch_scale=epochs / 200.0, sigma_bias=0.5)
        print(f"  loss {info['loss_first_epoch']:.6f} -> {info['loss_last_epoch']:.6f}")
        images, poses, (H, W, focal) = N.load_blender_data(scene, "train", img_size=size)
        gen = torch.Generator().manual_seed(4)
        os_, ds_, ts_ = [], [], []
        for v in range(views):
            ro, rd = N.get_rays(H, W, focal, poses[v].float())
            pix = torch.randperm(H * W, generator=gen)[: R // views].cuda()
            os_.append(ro.reshape(-1, 3)[pix]); ds_.append(rd.reshape(-1, 3)[pix])
            ts_.append(images[v].permute(1, 2, 0)[..., :3].reshape(-1, 3).cuda()[pix])
        o, d, tgt = torch.cat(os_).contiguous(), torch.cat(ds_).contiguous(), torch.cat(ts_).float().contiguous()
        grids = [("plain", None), ("ones", ones)]
        for thr in (0.0, 0.5, 2.0, 8.0, 32.0):
            grids.append((f"thr {thr:g}", N.OccupancyGrid.from_model(model, -4.0, 4.0, resolution=128, threshold=thr, mma_mode=mode)))
        model.train()
        for S in (32, 64):
            run_row("  v2 fitted", model, o, d, tgt, S, grids, steps, warmup, block)


def report_rays(steps, warmup, block, mode="bf16", R=2048):
    """The staged and the ray route of the step under a grid, side by side (module docstring)."""
    dev = torch.device("cuda", 0)
    print(f"training step under an occupancy grid, grid_inputs staged against rays, {mode}, {R} rays; lr = 0; {steps} steps per arm after {warmup} "
          f"warm-up steps, blocks of {block}; wall clock, ms = median [min .. max]")
    print('"solid" weights, rays from around the origin; grids of 128^3 cells over [-8, 8]^3: all ones, and the cells whose centre lies within 2.7 '
          'of the origin (the samples run from 2 to 6 along unit directions)')
    ones = N.OccupancyGrid.full(128, -8.0, 8.0, device=dev)
    c = (torch.arange(128, dtype=torch.float32) + 0.5) / 128 * 16.0 - 8.0
    zz, yy, xx = torch.meshgrid(c, c, c, indexing="ij")
    ball = N.OccupancyGrid.from_mask((xx * xx + yy * yy + zz * zz) < 2.7 ** 2, -8.0, 8.0).to(dev)
    o = (torch.rand(R, 3, generator=torch.Generator().manual_seed(1)) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=torch.Generator().manual_seed(2)) - 0.5, dim=-1).cuda().contiguous()
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(3)).cuda()
    # V3: a 37 x 37 x 64 map (a 518-pixel view of DINOv2's 14-pixel patches) seen from the lego-like camera
    fmap = (torch.rand(1, 37, 37, 64, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    dino = dict(features=fmap, pose=torch.from_numpy(O.LEGO_LIKE_C2W), focal=O.focal_for(128), H=128, W=128)
    arms = [("plain", None), ("staged ones", ones, "staged"), ("rays ones", ones, "rays"), ("staged ball", ball, "staged"), ("rays ball", ball, "rays")]
    for net in ("v1", "v2", "v3"):
        for S in (32, 64):
            run_row(f"  {net} solid", make(net, "solid", mode), o, d, tgt, S, arms, steps, warmup, block, dino=dino if net == "v3" else None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--rays", action="store_true", help="the staged against the ray route of the step under a grid (V1, V2, V3), nothing else")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_occupancy needs the GPU: there is no CPU path")
    if a.rays:
        report_rays(a.steps, a.warmup, a.block)
    else:
        report(a.steps, a.warmup, a.block, a.epochs)
