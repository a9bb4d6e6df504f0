"""Measured cost of the hierarchical training step (FusedStep.step_rays_hierarchical) against what the library offered before it --
the numbers quoted in DESIGN.md sections 3.4 / 7 and kept in profiles/hier_train_step_time.txt.  Needs the GPU.

    python tools/bench_hier_train.py > profiles/hier_train_step_time.txt

Every row is one batch shape (2048 rays at 64 + 64 and at 128 + 64 samples: BASELINE config 3's split) and one family (V2, V1), bf16;
its three arms take turns step by step in ONE process, after warm-up:
    (a) hier     : the hierarchical step -- S + Ni network rows per ray, forward and backward;
    (b) two steps: two plain step_rays of the parent, one on the S ladder samples and one on the S + Ni union through z_in -- the only
                   way to the same gradient before: 2 S + Ni network rows per ray;
    (c) plain    : one plain step_rays at S + Ni samples -- the same network rows as (a), without the resampling and the second image.
The row counts promise (a) / (b) = (S + Ni) / (2 S + Ni): 0.67 and 0.60.  The learning rate is 0 and the jitter seed fixed, so that
every step of an arm does the same work.  Each step is timed by a pair of device events (the time from the moment the device reaches
the step to the end of its last kernel: host gaps inside a step count, as they do in a training loop); the arms alternate until each
has at least `--seconds` of device time.  The wall clock of the whole loop is printed as a cross-check.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_hier_train.py --only hier --steps 50 --shape 128 64 --net v2

runs one arm alone for a fixed number of steps: the kernel trace of that run gives the launches per step (calls / steps) and the
per-kernel shares."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nerf_few_shot_limitations_amd as N  # noqa: E402
from nerf_few_shot_limitations_amd.training import FusedStep  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

NEAR, FAR = 2.0, 6.0
# library calls of one hierarchical step, in order (each entry is one launch unless a count is given; the two network backwards launch
# what a plain step's one backward launches, each): counted from the sequence in training.py, checked against the kernel trace
SEQUENCE = ("saving forward (ladder)", "nrf_composite", "nrf_sample_pdf_sorted", "saving forward (new depths)",
            "nrf_composite_hier_loss_backward: 4 launches", "network backward (coarse context)", "network backward (new context)", "optimiser")


def make(net, mode):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
        m.load_state_dict(O.make_weights("v1", 0, "solid"))
    else:
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=mode)
        m.load_state_dict(O.make_weights("v2", 1, "solid"), strict=False)
    return m.cuda().train()


def arms_for(net, mode, R, S, Ni):
    o = (torch.rand(R, 3, generator=torch.Generator().manual_seed(1)) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=torch.Generator().manual_seed(2)) - 0.5, dim=-1).cuda().contiguous()
    tgt = torch.rand(R, 3, generator=torch.Generator().manual_seed(3)).cuda()
    u = torch.rand(R, Ni, generator=torch.Generator().manual_seed(4)).cuda()
    hier = FusedStep(make(net, mode), lr=0.0)
    first, second, plain = (FusedStep(make(net, mode), lr=0.0) for _ in range(3))
    hier.step_rays_hierarchical(o, d, tgt, NEAR, FAR, S, Ni, seed=11, u=u)
    union = torch.sort(torch.cat([hier.last_z, hier.last_z_new], 1), dim=1, stable=True).values.contiguous()      # (b)'s z_in: lr = 0, it stays valid

    def two():
        first.step_rays(o, d, tgt, NEAR, FAR, S, seed=11)
        second.step_rays(o, d, tgt, NEAR, FAR, S + Ni, perturb=False, z_in=union)

    return {"hier": lambda: hier.step_rays_hierarchical(o, d, tgt, NEAR, FAR, S, Ni, seed=11, u=u),
            "two steps": two,
            "plain": lambda: plain.step_rays(o, d, tgt, NEAR, FAR, S + Ni, seed=11)}


def time_arms(arms, seconds, warmup, max_steps=20000):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    t0 = time.perf_counter()
    while min(sum(v) for v in ms.values()) < seconds * 1e3 and len(next(iter(ms.values()))) < max_steps:
        pending = []
        for _ in range(16):                              # 16 rounds between synchronisations: the host runs ahead as in a training loop
            for k, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                pending.append((k, a, b))
        torch.cuda.synchronize()
        for k, a, b in pending:
            ms[k].append(a.elapsed_time(b))
    return ms, time.perf_counter() - t0


def fmt(a):
    a = np.asarray(a)
    return f"{np.median(a):.4f} [{np.percentile(a, 10):.4f} .. {np.percentile(a, 90):.4f}]"


def report(seconds, warmup, mode="bf16", R=2048):
    print(f"hierarchical training step, {mode}, {R} rays, 'solid' weights, lr = 0; arms alternating step by step in one process after {warmup} warm-up "
          f"rounds, until each arm has {seconds:g} s of device time; device events per step, ms = median [10th .. 90th percentile]")
    print("library calls of one hierarchical step: " + " -> ".join(SEQUENCE))
    for net in ("v2", "v1"):
        for S, Ni in ((64, 64), (128, 64)):
            ms, wall = time_arms(arms_for(net, mode, R, S, Ni), seconds, warmup)
            a, b, c = (float(np.median(ms[k])) for k in ("hier", "two steps", "plain"))
            print(f"  {net} {S} + {Ni}  ({len(ms['hier'])} steps per arm, loop wall clock {wall:.2f} s, device time {sum(sum(v) for v in ms.values()) / 1e3:.2f} s):")
            print(f"    (a) hier      {fmt(ms['hier'])} ms")
            print(f"    (b) two steps {fmt(ms['two steps'])} ms")
            print(f"    (c) plain     {fmt(ms['plain'])} ms")
            print(f"    (a) / (b) = {a / b:.3f}   (rows promise {(S + Ni) / (2 * S + Ni):.2f})      (a) / (c) = {a / c:.3f}      (a) - (c) = {a - c:.4f} ms", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm and row")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["hier", "two steps", "plain"], default=None, help="run this arm alone for --steps steps (for a kernel trace)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--shape", type=int, nargs=2, default=(128, 64), metavar=("S", "NI"))
    ap.add_argument("--net", choices=["v1", "v2"], default="v2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hier_train needs the GPU: there is no CPU path")
    if a.only:
        fn = arms_for(a.net, "bf16", 2048, *a.shape)[a.only]
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        print(f"{a.only}: {a.steps} steps of {a.net} {a.shape[0]} + {a.shape[1]} (plus the one hierarchical step that draws the union)")
    else:
        report(a.seconds, a.warmup)
