"""The five workloads BASELINE.json names, timed on ONE MI355X (synthetic weights, scene "solid", camera of SURVEY.md 8d):

  C1  100 x 100 x 32, baseline model (the reference's CPU-runnable case)
  C2  400 x 400 x 64, baseline model
  C3  800 x 800, 128 coarse + 64 fine (hierarchical: coarse pass, inverse-cdf resampling, fine pass on 192 sorted depths)
  C4  400 x 400 x 64, DINO-conditioned model (feature map 28 x 28 x 64)
  C5  800 x 800 x 128, baseline model -- the whole frame on one GPU (the 8-GPU tile-sharded run is bench.py --gpus 8)

    python tools/bench_configs.py [--mode bf16] [--reps 5]
Prints one JSON line per configuration: ms per frame, M ray-samples/s, fraction of the dense MFMA peak.

    python tools/bench_configs.py --hier [--reps 7]
C3 three ways, the arms alternating frame by frame in one process (f16 and f16x3, the V2 and the V1 network): the three-call
render_hierarchical (the yardstick), render_hierarchical(reuse_coarse=True), and render_camera_hierarchical.  One JSON line per
(network, mode): ms per frame of every arm (mean, min, max) and the ratios to the three-call route.
    python tools/bench_configs.py --hier-profile [--mode f16]
ONE frame of the camera route and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nerf_few_shot_limitations_amd as N                       # noqa: E402
from oracle import nerf_oracle as O                             # noqa: E402  (synthetic weights / camera generators only)

PEAK = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "f16x3": 2500.0}


def timed(fn, reps):
    for _ in range(3):          # warm-up: the first launches of a process run at an idle chip's clocks
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def hier_models(mode, dev):
    v2 = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=mode)
    v2.load_state_dict(O.make_weights("v2", 1, "solid"), strict=False)
    v1 = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
    v1.load_state_dict(O.make_weights("v1", 0, "solid"))
    return {"v2": v2.to(dev).eval(), "v1": v1.to(dev).eval()}


def hier_arms(reps, dev, c2w):
    """C3 (800 x 800, 128 + 64) by the three routes, alternating frame by frame; the three-call route is the yardstick."""
    H, S, Ni = 800, 128, 64
    ro, rd = N.get_rays(H, H, O.focal_for(H), c2w)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    with torch.no_grad():
        for mode in ("f16", "f16x3"):
            for net, model in hier_models(mode, dev).items():
                arms = {"three_call": lambda: N.render_hierarchical(model, ro, rd, 2.0, 6.0, S, Ni),
                        "reuse_coarse": lambda: N.render_hierarchical(model, ro, rd, 2.0, 6.0, S, Ni, reuse_coarse=True),
                        "camera": lambda: N.render_camera_hierarchical(model, H, H, O.focal_for(H), c2w, 2.0, 6.0, S, Ni)}
                outs = {}
                for _ in range(2):                   # warm-up of every arm: code objects, clocks, the allocator's blocks
                    for name, fn in arms.items():
                        outs[name] = fn()
                same = (torch.equal(outs["three_call"]["rgb"], outs["reuse_coarse"]["rgb"]) and torch.equal(outs["three_call"]["rgb"], outs["camera"][0])
                        and torch.equal(outs["three_call"]["depth"], outs["camera"][1]))
                del outs
                ms = {name: [] for name in arms}
                for _ in range(reps):
                    for name, fn in arms.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                mean = {k: sum(v) / len(v) for k, v in ms.items()}
                print(json.dumps({"config": "C3 800x800 128 coarse + 64 fine", "net": net, "mode": mode, "reps": reps, "same_image_bits": same,
                                  "ms_per_frame": {k: {"mean": round(mean[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in ms.items()},
                                  "reuse_coarse_over_three_call": round(mean["reuse_coarse"] / mean["three_call"], 4),
                                  "camera_over_three_call": round(mean["camera"] / mean["three_call"], 4),
                                  "network_evaluations_per_ray": {"three_call": S + S + Ni, "reuse_coarse": S + Ni, "camera": S + Ni}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f16", "f32", "f16x3"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hier", action="store_true", help="C3 by the three hierarchical routes, alternating (f16 and f16x3, V2 and V1)")
    ap.add_argument("--hier-profile", action="store_true", help="one C3 frame of the camera route (V2, --mode) and nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    c2w = torch.from_numpy(O.LEGO_LIKE_C2W.copy())
    if args.hier:
        return hier_arms(args.reps, dev, c2w)
    if args.hier_profile:
        with torch.no_grad():
            N.render_camera_hierarchical(hier_models(args.mode, dev)["v2"], 800, 800, O.focal_for(800), c2w, 2.0, 6.0, 128, 64)
            torch.cuda.synchronize()
        return None
    v2 = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=args.mode)
    v2.load_state_dict(O.make_weights("v2", 1, "solid"), strict=False)
    v2 = v2.to(dev).eval()
    v3 = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=64, mma_mode=args.mode)
    v3.load_state_dict(O.make_weights("v3", 2, "solid"), strict=False)
    v3 = v3.to(dev).eval()
    fm = torch.from_numpy(O.uniform01(7, 28 * 28 * 64).reshape(1, 28, 28, 64) * 2 - 1)

    def camera(model, H, S, dino=None):
        return lambda: N.render_camera(model, H, H, O.focal_for(H), c2w, 2.0, 6.0, S, dino=dino)

    ro8, rd8 = N.get_rays(800, 800, O.focal_for(800), c2w)
    ro8, rd8 = ro8.reshape(-1, 3), rd8.reshape(-1, 3)
    cases = [
        ("C1 100x100x32 baseline", camera(v2, 100, 32), 100 * 100 * 32, v2),
        ("C2 400x400x64 baseline", camera(v2, 400, 64), 400 * 400 * 64, v2),
        ("C3 800x800 128 coarse + 64 fine (hierarchical)", lambda: N.render_hierarchical(v2, ro8, rd8, 2.0, 6.0, 128, 64), 800 * 800 * (128 + 192), v2),
        ("C4 400x400x64 DINO-conditioned", camera(v3, 400, 64, dict(features=fm, pose=c2w, focal=O.focal_for(400), H=400, W=400)), 400 * 400 * 64, v3),
        ("C5 800x800x128 baseline, one GPU", camera(v2, 800, 128), 800 * 800 * 128, v2),
        ("C5 shard: 100 rows (80 000 rays) x 128 of the 800x800 frame = one GPU's share of 8", lambda: N.render_camera(v2, 800, 800, O.focal_for(800), c2w, 2.0, 6.0, 128, ray_begin=0, ray_end=80000), 80000 * 128, v2),
        ("headline shape 800x800x64 baseline", camera(v2, 800, 64), 800 * 800 * 64, v2),
    ]
    with torch.no_grad():
        for _ in range(10):          # bring the chip to its working clocks: a cold first case reads 15-20 % slow
            camera(v2, 400, 64)()
        torch.cuda.synchronize()
        for name, fn, samples, model in cases:
            dt = timed(fn, args.reps)
            tflops = samples * model.flops_per_sample() / dt / 1e12
            print(json.dumps({"config": name, "mode": args.mode, "ms_per_frame": round(dt * 1e3, 3), "M_ray_samples_per_s": round(samples / dt / 1e6, 1),
                              "ray_samples": samples, "TFLOP_per_s": round(tflops, 1), "frac_of_mfma_peak": round(tflops / PEAK[args.mode], 4)}), flush=True)


if __name__ == "__main__":
    main()
