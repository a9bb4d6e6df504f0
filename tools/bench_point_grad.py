"""Cost of the V3 point gradient on one MI355X: render_rays + mse + backward on a NeRFMLP(use_dino=True, point_grad=True) whose
rays are data ("plain": the autograd step every trainer runs) against the same call with rays that require grad ("point": the
geometric compositor backward, dino_grad_kernel, input_grad_v3_kernel, fetch_points_backward_kernel and the adjoint of the
points on top).  --net v2 runs the same pair on a NeRFMLP(input_grad=True) without DINO features: there the "point" form adds the
geometric compositor backward, input_grad_kernel and the adjoint of the points.

    python tools/bench_point_grad.py [--net v3] [--mode bf16] [--rays 2048] [--samples 32]     # one JSON line
    python tools/bench_point_grad.py --trace                                         # a short run for rocprofv3 --kernel-trace --stats

The two forms alternate block by block inside one process (tools/bench_multiscale_step.py); the figure of a form is the median
over its blocks, the spread their (max - min) / median.  --trace runs 5 warm-up + 50 steps of the point form only: the
trace's call counts divide by 55."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_few_shot_limitations_amd as N                       # noqa: E402
from oracle import nerf_oracle as O                             # noqa: E402  (deterministic synthetic weights / camera only)


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="v3", choices=["v3", "v2"])
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--rays", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--dino-dim", type=int, default=64, choices=[64, 128])
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.net == "v2" and a.dino_dim != 64:
        ap.error("--dino-dim belongs to --net v3")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if a.net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=a.mode, input_grad=True)
        m.load_state_dict(O.make_weights("v2", 2, "fog"), strict=False)
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=a.dino_dim, mma_mode=a.mode,
                      point_grad=True)
        m.load_state_dict(O.make_weights("v3", 2, "fog", dino_dim=a.dino_dim), strict=False)
    m = m.to(dev).train()
    side = int(a.rays ** 0.5 + 0.999)
    o, d = O.get_rays(side, side, O.focal_for(side), torch.from_numpy(O.LEGO_LIKE_C2W.copy()))
    o, d = o.reshape(-1, 3)[:a.rays].contiguous().to(dev), d.reshape(-1, 3)[:a.rays].contiguous().to(dev)
    tgt = torch.from_numpy(O.uniform01(7, a.rays * 3).reshape(a.rays, 3)).float().to(dev)
    # another view's map: the rendered camera moved a quarter turn about the scene's axis
    pose = torch.from_numpy(O.LEGO_LIKE_C2W.copy())
    turn = torch.tensor([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    dino = None
    if a.net == "v3":
        fmap = torch.from_numpy(O.uniform01(8, 14 * 22 * a.dino_dim).reshape(1, 14, 22, a.dino_dim) * 2 - 1).float().to(dev)
        dino = dict(features=fmap, pose=turn @ pose, focal=O.focal_for(64), H=64, W=64)

    def step(live):
        m.zero_grad(set_to_none=True)
        oo, dd = (o.clone().requires_grad_(True), d.clone().requires_grad_(True)) if live else (o, d)
        out = N.render_rays(m, oo, dd, 2.0, 6.0, a.samples, perturb=True, seed=1, dino=dino)
        ((out["rgb"] - tgt) ** 2).mean().backward()

    if a.trace:
        for _ in range(55):
            step(True)
        torch.cuda.synchronize()
        return
    fns = {"plain": lambda: step(False), "point": lambda: step(True)}
    ts = {k: [] for k in fns}
    for fn in fns.values():
        block_ms(fn, 20)
    for _ in range(a.blocks):
        for k, fn in fns.items():
            ts[k].append(block_ms(fn, a.block))
    rec = {k: {"ms": round(statistics.median(v), 4), "spread": round((max(v) - min(v)) / statistics.median(v), 3)} for k, v in ts.items()}
    rec["point_minus_plain_us"] = round((rec["point"]["ms"] - rec["plain"]["ms"]) * 1e3, 1)
    print(json.dumps({"net": a.net, "dino_dim": a.dino_dim if a.net == "v3" else 0, "rays": a.rays, "samples": a.samples, "mode": a.mode, **rec}), flush=True)


if __name__ == "__main__":
    main()
