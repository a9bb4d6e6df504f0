"""Measured cost and gain of empty-space skipping (render_rays' occupancy=: an occupancy bit grid on the ray-queue kernel) -- the
numbers quoted in DESIGN.md sections 3.1 / 7 and kept under profiles/.  Needs the GPU.

    python tools/bench_occupancy.py --cost    > profiles/occupancy_frame_time.txt
    python tools/bench_occupancy.py --fields  > profiles/occupancy_trained_fields.txt
    python tools/bench_occupancy.py --pruned  > profiles/occupancy_pruned_fields.txt

--cost  : 800 x 800 x 64, f16.  The arms of a row alternate frame by frame in one process after a warm-up, HIP events around a frame.
          a) nothing skipped: V1 / V2 / V3 "solid" with an all-ones grid against the plain render_kernel and the plain ray-queue
             kernel (ert_eps = 1e-30: the queue march without a single termination);
          b) gain on the opaque "smooth" field: a from_model grid + ert_eps = 1e-2 against ert_eps = 1e-2 alone;
          c) the time OccupancyGrid.from_model takes at 128^3 x 4 probes.
--fields: the V1 and V2 fields fitted by tools/trained_scene.py (the only scene here with real empty space): frame time at
          800 x 800 x 64 with and without a from_model grid, evaluated share stats[0] / (R S), column utilisation
          stats[0] / (stats[1] x columns per wave), and what the grid costs in image quality on the scene's test views at the
          training resolution -- max |rgb - rgb(no grid)| and the PSNR difference against the ground truth -- at dilate 1 and 0.
--pruned: the same two fields with the from_model grid (dilate 1) pruned by the weights their own training views render
          (OccupancyGrid.prune: weight_threshold x unseen, seen_eps 1e-2, dilate 1): occupied cells, evaluated share and column
          utilisation at 800 x 800 x 64, frame time against the plain ray-queue kernel, the from_model grid and render_kernel (four
          arms alternating), and PSNR difference / max |rgb - rgb(no grid)| at the training resolution, on the training views and on
          the held-out test views separately; the build time per view; the marker kernel's own time on one 800 x 800 x 64 frame.
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
from oracle import nerf_oracle as O  # noqa: E402

C2W = torch.from_numpy(np.asarray(O.LEGO_LIKE_C2W))
COLS = {"bf16": 64, "f16": 64, "f32": 32, "f16x3": 32}


def make(net, scene, mode="f16"):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
        m.load_state_dict(O.make_weights("v1", 0, scene))
    elif net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=mode)
        m.load_state_dict(O.make_weights("v2", 1, scene), strict=False)
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=64, mma_mode=mode)
        m.load_state_dict(O.make_weights("v3", 2, scene), strict=False)
    return m.cuda().eval()


def dino_for(net, H, W):
    if net != "v3":
        return {}
    fm = torch.from_numpy(O.uniform01(7, 28 * 28 * 64).reshape(1, 28, 28, 64) * 2 - 1)
    return dict(dino=dict(features=fm, pose=C2W, focal=O.focal_for(W), H=H, W=W))


def alternate(arms, frames, warmup):
    """arms: {label: callable rendering one frame}.  Returns {label: ms per frame (array)}: the arms take turns frame by frame."""
    t = {k: [] for k in arms}
    for i in range(warmup + frames):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                t[k].append(e0.elapsed_time(e1))
    return {k: np.array(v) for k, v in t.items()}


def fmt(a):
    return f"{np.median(a):.3f} [{a.min():.3f} .. {a.max():.3f}]"


def stats_of(m, H, W, focal, pose, S, mode, grid, **kw):
    """(evaluated share, column utilisation) of one frame with `grid`."""
    st = N.render_camera(m, H, W, focal, pose, 2.0, 6.0, S, mma_mode=mode, occupancy=grid, return_stats=True, **kw)[2].tolist()
    return st[0] / float(H * W * S), st[0] / max(1.0, st[1] * COLS[mode])


def cost_report(frames, warmup, H=800, S=64, mode="f16"):
    print(f"{H}x{H}x{S} {mode}; the arms of a row alternate frame by frame in one process, {frames} frames each after {warmup} warm-up frames; "
          "HIP events around a frame; ms = median [min .. max]")
    rgb = torch.empty((H * H, 3), device="cuda"); depth = torch.empty((H * H,), device="cuda")
    focal = O.focal_for(H)
    ones = N.OccupancyGrid.from_mask(torch.ones((128, 128, 128), dtype=torch.bool), -6.0, 6.0)

    def frame(m, **kw):
        return lambda: N.render_camera(m, H, H, focal, C2W, 2.0, 6.0, S, mma_mode=mode, out_rgb=rgb, out_depth=depth, **kw)

    print("a) nothing skipped (\"solid\", all-ones 128^3 grid)")
    for net in ("v1", "v2", "v3"):
        m, kw = make(net, "solid", mode), dino_for(net, H, H)
        t = alternate({"plain": frame(m, **kw), "queue": frame(m, ert_eps=1e-30, **kw), "grid": frame(m, occupancy=ones, **kw)}, frames, warmup)
        share, util = stats_of(m, H, H, focal, C2W, S, mode, ones, **kw)
        print(f"  {net}: render_kernel {fmt(t['plain'])} ms   ray queue (ert 1e-30) {fmt(t['queue'])} ms   queue + all-ones grid {fmt(t['grid'])} ms   "
              f"grid / queue = {np.median(t['grid']) / np.median(t['queue']):.4f}   grid / render_kernel = {np.median(t['grid']) / np.median(t['plain']):.4f}   "
              f"evaluated share {share:.4f} utilisation {util:.4f}", flush=True)
    print("b) the opaque \"smooth\" field: from_model grid (128^3 over [-6, 6]^3, 4 probes, dilate 1) + ert_eps 1e-2 against ert_eps 1e-2 alone")
    for net in ("v1", "v2"):
        m = make(net, "smooth", mode)
        grid = N.OccupancyGrid.from_model(m, -6.0, 6.0, resolution=128, mma_mode=mode)
        t = alternate({"ert": frame(m, ert_eps=1e-2), "grid": frame(m, ert_eps=1e-2, occupancy=grid)}, frames, warmup)
        share, util = stats_of(m, H, H, focal, C2W, S, mode, grid, ert_eps=1e-2)
        a = N.render_camera(m, H, H, focal, C2W, 2.0, 6.0, S, mma_mode=mode, ert_eps=1e-2)[0]
        b = N.render_camera(m, H, H, focal, C2W, 2.0, 6.0, S, mma_mode=mode, ert_eps=1e-2, occupancy=grid)[0]
        print(f"  {net}: ert alone {fmt(t['ert'])} ms   grid + ert {fmt(t['grid'])} ms   ratio {np.median(t['grid']) / np.median(t['ert']):.4f}   "
              f"occupied cells {grid.occupied_fraction:.4f}   evaluated share {share:.4f}   utilisation {util:.4f}   max |rgb - rgb(ert alone)| {float((a - b).abs().max()):.3e}",
              flush=True)
    print("c) OccupancyGrid.from_model at 128^3 x 4 probes, dilate 1 (wall clock around a synchronised build, second of two)")
    for net in ("v1", "v2", "v3"):
        m, kw = make(net, "solid", mode), dino_for(net, H, H)
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            N.OccupancyGrid.from_model(m, -6.0, 6.0, resolution=128, mma_mode=mode, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        print(f"  {net}: {dt * 1e3:.1f} ms", flush=True)


def fields_report(frames, warmup, epochs, mode="f16"):
    import synthetic_scene
    import trained_scene
    size, views, S = 128, 8, 64
    print(f"fields fitted by tools/trained_scene.py ({epochs} epochs, {views} views of {size} px, trained in bf16), rendered in {mode}; grid: from_model, 128^3 over "
          "[-4, 4]^3, threshold 0, 4 probes per cell")
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene")
        synthetic_scene.write_scene(scene, size=size, n_train=views, n_test=4)
        images, poses, (H, W, focal) = N.load_blender_data(scene, "test", img_size=size)
        gt = images.permute(0, 2, 3, 1).contiguous().cuda()
        for net in ("v1", "v2"):
            model, info, _ = trained_scene.train_field(net, trained_scene.config(size, views, epochs), scene, "bf16", 0, epoch_scale=epochs / 200.0, sigma_bias=0.5)
            print(f"{net}: loss {info['loss_first_epoch']} -> {info['loss_last_epoch']}")
            with torch.no_grad():
                base = N.evaluate_views(model, poses, H, W, focal, 2.0, 6.0, S, mma_mode=mode)["images"]
                ps0 = N.psnr(base, gt)
                big = 800
                rgb = torch.empty((big * big, 3), device="cuda"); depth = torch.empty((big * big,), device="cuda")
                fb = focal * big / W
                for dil in (1, 0):
                    grid = N.OccupancyGrid.from_model(model, -4.0, 4.0, resolution=128, dilate=dil, mma_mode=mode)
                    r = N.evaluate_views(model, poses, H, W, focal, 2.0, 6.0, S, mma_mode=mode, occupancy=grid, return_stats=True)
                    ps = N.psnr(r["images"], gt)
                    t = alternate({"plain": lambda: N.render_camera(model, big, big, fb, poses[0], 2.0, 6.0, S, mma_mode=mode, out_rgb=rgb, out_depth=depth),
                                   "grid": lambda: N.render_camera(model, big, big, fb, poses[0], 2.0, 6.0, S, mma_mode=mode, out_rgb=rgb, out_depth=depth,
                                                                   occupancy=grid)}, frames, warmup)
                    share, util = stats_of(model, big, big, fb, poses[0], S, mode, grid)
                    print(f"  {net} dilate {dil}: occupied cells {grid.occupied_fraction:.4f}   test views at {size} px: max |rgb - rgb(no grid)| "
                          f"{float((r['images'] - base).abs().max()):.3e}, psnr {ps:.4f} dB against {ps0:.4f} dB without (difference {ps - ps0:+.5f} dB, "
                          f"0.01 dB bar {'met' if abs(ps - ps0) <= 0.01 else 'NOT met'}), evaluated share {r['evaluated_share']:.4f}   800x800x{S}: render_kernel "
                          f"{fmt(t['plain'])} ms, with the grid {fmt(t['grid'])} ms (ratio {np.median(t['grid']) / np.median(t['plain']):.4f}), evaluated share "
                          f"{share:.4f}, utilisation {util:.4f}", flush=True)


def marker_time(model, H, S, focal, pose, mode, grid, frames, warmup):
    """ms of nrf_occupancy_mark_camera alone on one H x H x S frame of `model`: into zeroed arrays (every first mark is an atomic) and
    into arrays that already hold the frame's marks (no atomic left)."""
    import ctypes as C
    from nerf_few_shot_limitations_amd import _lib as L
    from nerf_few_shot_limitations_amd.ray_sampler import _c2w12
    ro, rd = N.get_rays(H, H, focal, pose)
    r = N.render_rays(model, ro.reshape(-1, 3), rd.reshape(-1, 3), 2.0, 6.0, S, mma_mode=mode, return_z=True)
    w, z = r["weights"], r["z_vals"]
    del ro, rd
    res, lo, scale = (C.c_int32 * 3)(*grid.res), (C.c_float * 3)(*grid.lo), (C.c_float * 3)(*grid.scale)
    c2w = _c2w12(pose)
    hit, seen = torch.zeros_like(grid.bits), torch.zeros_like(grid.bits)

    def mark():
        L.check(L.lib().nrf_occupancy_mark_camera(H, H, float(focal), c2w, 0, H * H, S, L.ptr(z), L.ptr(w), res, lo, scale, 0.0, 1e-2,
                                                  hit.data_ptr(), seen.data_ptr(), L.stream_ptr()))

    def fresh():
        hit.zero_(); seen.zero_()
        torch.cuda.synchronize()

    cold, warm = [], []
    for i in range(warmup + frames):
        for times, prepare in ((cold, fresh), (warm, lambda: None)):
            prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            mark()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                times.append(e0.elapsed_time(e1))
    return np.array(cold), np.array(warm), H * H * S * 8


def pruned_report(frames, warmup, epochs, mode="f16"):
    import synthetic_scene
    import trained_scene
    size, views, S, big = 128, 8, 64, 800
    print(f"fields fitted by tools/trained_scene.py ({epochs} epochs, {views} views of {size} px, trained in bf16), rendered in {mode}.  base grid: from_model, "
          f"128^3 over [-4, 4]^3, threshold 0, 4 probes per cell, dilate 1.  pruned grid: base.prune over the {views} training views at {size} px x {S} samples, "
          "seen_eps 1e-2, dilate 1.")
    print(f"frame time: {big}x{big}x{S}, test pose 0; the four arms of a row (render_kernel, plain ray queue at ert_eps 1e-30, base grid, pruned grid) alternate "
          f"frame by frame in one process, {frames} frames each after {warmup} warm-up frames, HIP events around a frame on the launch stream; ms = median [min .. max].")
    print(f"image: all {views} training views / all held-out test views at {size} px against the render without a grid; d psnr = PSNR(grid) - PSNR(no grid) "
          "against the ground truth; the 0.01 dB bar of BASELINE.json is |d psnr| <= 0.01.")
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene")
        synthetic_scene.write_scene(scene, size=size, n_train=views, n_test=4)
        split = {}
        for name in ("train", "test"):
            images, poses, (H, W, focal) = N.load_blender_data(scene, name, img_size=size)
            split[name] = (images.permute(0, 2, 3, 1).contiguous().cuda(), poses)
        tr_poses, te_poses = split["train"][1], split["test"][1]
        fb = focal * big / W
        rgb = torch.empty((big * big, 3), device="cuda"); depth = torch.empty((big * big,), device="cuda")
        for net in ("v1", "v2"):
            model, info, _ = trained_scene.train_field(net, trained_scene.config(size, views, epochs), scene, "bf16", 0, epoch_scale=epochs / 200.0, sigma_bias=0.5)
            print(f"{net}: loss {info['loss_first_epoch']} -> {info['loss_last_epoch']}")
            with torch.no_grad():
                ref = {}
                for name, (gt, poses) in split.items():
                    im = N.evaluate_views(model, poses, H, W, focal, 2.0, 6.0, S, mma_mode=mode)["images"]
                    ref[name] = (im, N.psnr(im, gt))
                base = N.OccupancyGrid.from_model(model, -4.0, 4.0, resolution=128, dilate=1, mma_mode=mode)

                def frame(**kw):
                    return lambda: N.render_camera(model, big, big, fb, te_poses[0], 2.0, 6.0, S, mma_mode=mode, out_rgb=rgb, out_depth=depth, **kw)

                def image(grid):
                    out = []
                    for name, (gt, poses) in split.items():
                        r = N.evaluate_views(model, poses, H, W, focal, 2.0, 6.0, S, mma_mode=mode, occupancy=grid)
                        d = N.psnr(r["images"], gt) - ref[name][1]
                        out.append(f"{name} views: d psnr {d:+.5f} dB ({'met' if abs(d) <= 0.01 else 'NOT met'}), max |d rgb| "
                                   f"{float((r['images'] - ref[name][0]).abs().max()):.3e}")
                    return "; ".join(out)

                share, util = stats_of(model, big, big, fb, te_poses[0], S, mode, base)
                print(f"  {net} base grid: occupied cells {base.occupied_fraction:.4f}, evaluated share {share:.4f}, utilisation {util:.4f}; {image(base)}")
                for tau in (0.0, 1e-4, 1e-3, 1e-2):
                    for unseen in ("keep", "drop"):
                        cfg = dict(weight_threshold=tau, seen_eps=1e-2, unseen=unseen, dilate=1, mma_mode=mode)
                        for _ in range(2):                                     # wall clock around a synchronised build, second of two
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            grid = base.prune(model, tr_poses, H, W, focal, 2.0, 6.0, S, **cfg)
                            torch.cuda.synchronize()
                            build_ms = (time.perf_counter() - t0) * 1e3
                        t = alternate({"plain": frame(), "queue": frame(ert_eps=1e-30), "base": frame(occupancy=base), "pruned": frame(occupancy=grid)},
                                      frames, warmup)
                        share, util = stats_of(model, big, big, fb, te_poses[0], S, mode, grid)
                        med = {k: np.median(v) for k, v in t.items()}
                        print(f"  {net} tau {tau:g} unseen {unseen}: occupied cells {grid.occupied_fraction:.4f}, evaluated share {share:.4f}, utilisation {util:.4f}; "
                              f"pruned {fmt(t['pruned'])} ms, base grid {fmt(t['base'])} ms, plain queue {fmt(t['queue'])} ms, render_kernel {fmt(t['plain'])} ms; "
                              f"pruned / queue {med['pruned'] / med['queue']:.4f}, pruned / base {med['pruned'] / med['base']:.4f}, pruned / render_kernel "
                              f"{med['pruned'] / med['plain']:.4f}; {image(grid)}; build {build_ms:.1f} ms = {build_ms / views:.2f} ms per view", flush=True)
                cold, warm, nbytes = marker_time(model, big, S, fb, te_poses[0], mode, base, frames, warmup)
                print(f"  {net} marker kernel alone, one {big}x{big}x{S} frame, camera rays, hit and seen, {nbytes / 1e6:.1f} MB read (8 B per sample, no ray bytes): "
                      f"into zeroed arrays {fmt(cold)} ms = {nbytes / np.median(cold) / 1e9:.3f} TB/s; into arrays that hold the marks {fmt(warm)} ms = "
                      f"{nbytes / np.median(warm) / 1e9:.3f} TB/s (composite_kernel, the comparable wave-per-ray row kernel: 2.9 TB/s, "
                      "profiles/r01_staged_kernels_bandwidth.txt)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--fields", action="store_true")
    ap.add_argument("--pruned", action="store_true")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy needs the GPU: there is no CPU path")
    if a.cost:
        cost_report(a.frames, a.warmup)
    if a.fields:
        fields_report(a.frames, a.warmup, a.epochs)
    if a.pruned:
        pruned_report(a.frames, a.warmup, a.epochs)
