"""Host-bound step time of FusedStep as wall time per step around a synchronise -- one arm of an A/B between two trees.

    python tools/bench_fused_step.py train v2 [--root TREE]     bench.py's `training` step: __call__, 2048 rays x 32 samples, bf16
    python tools/bench_fused_step.py train v1 [--root TREE]
    python tools/bench_fused_step.py info [--root TREE]         tools/bench_info_reg.py's shape: step_rays, 3072 rays x 64, arm `both`

--root: the tree whose package (and built library) is imported; default: this file's.  Run the trees as alternating fresh processes
and hold the difference of their medians against one tree measured twice.  Prints one JSON line: the median of 7 blocks of 300
steps behind 300 warm-up steps (the first dozens of steps after a pause run faster: the chip's power state), and the blocks."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["train", "info"])
ap.add_argument("net", nargs="?", default="v2", choices=["v1", "v2"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import nerf_few_shot_limitations_amd as N  # noqa: E402
from nerf_few_shot_limitations_amd.training import FusedStep  # noqa: E402

dev = torch.device("cuda", 0)
torch.manual_seed(0)
if args.what == "train":
    R, S = 2048, 32
    if args.net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode="bf16").to(dev).train()
        pts = torch.rand(R * S, 3, device=dev) * 4 - 2
    else:
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode="bf16").to(dev).train()
        pts = torch.rand(R * S, 63, device=dev) * 2 - 1
    dirs = torch.rand(R * S, 3, device=dev) * 2 - 1
    z = torch.sort(torch.rand(R, S, device=dev) * 4 + 2, dim=-1).values.contiguous()
    d = torch.rand(R, 3, device=dev) - 0.5
    tgt = torch.rand(R, 3, device=dev)
    step = FusedStep(m, lr=5e-4, weight_decay=1e-6)
    kw = dict(dirs=dirs) if args.net != "v1" else {}
    run = lambda: step(pts, z, d, tgt, **kw)
else:
    from oracle import nerf_oracle as O
    import bench_info_reg as B
    run = B.arms_for(N, O, "bf16", 64)["both"]
for _ in range(300):
    run()
torch.cuda.synchronize()
blocks = []
for _ in range(7):
    t0 = time.perf_counter()
    for _ in range(300):
        run()
    torch.cuda.synchronize()
    blocks.append((time.perf_counter() - t0) / 300 * 1e3)
blocks.sort()
print(json.dumps({"what": args.what + (" " + args.net if args.what == "train" else ""), "package": os.path.dirname(N.__file__),
                  "ms_per_step": round(blocks[3], 5), "blocks_ms": [round(b, 5) for b in blocks]}), flush=True)
