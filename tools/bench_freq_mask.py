"""Measured cost of the frequency mask in the fused training step (NeRFMLP.set_freq_mask / FusedStep(freq_reg_end=)) -- the
numbers quoted in DESIGN.md section 3.4 and kept in profiles/freq_mask_step_time.txt.  Needs the GPU.

    python tools/bench_freq_mask.py > profiles/freq_mask_step_time.txt

Every row is one batch shape (2048 rays at 32 and at 64 samples) and one family (V1, V2), bf16; its two arms take turns step by step
in ONE process, after warm-up:
    (a) plain  : the plain step -- repack3_kernel, weight_grad_reduce_kernel;
    (b) masked : the same step on a model under a fixed mask with a distinct non-dyadic value per column (0.3 + 0.006 id, both
                 encodings) -- repack3_masked_kernel, weight_grad_reduce_masked_kernel; every other launch is the same kernel.
The learning rate is 0 and the jitter seed fixed, so that every step of an arm does the same work.  Each step is timed by a pair of
device events (host gaps inside a step count, as they do in a training loop); the arms alternate until each has `--seconds` of
device time.  Every row is measured twice, with (a) first and with (b) first in the alternation: what swapping the order moves the
medians by is the resolution of the comparison, and is printed beside the ratio.

    python tools/bench_freq_mask.py --only plain --lib /path/to/another/libnerfhip.so

times arm (a) alone on another build of the library (the parent commit's: the cross-check that arm (a) of the table above, which runs
the kernels this build shares with it, is the parent's step).

The two launches that differ are best read from a kernel trace of a short run of this tool (their names above), taken in a run of its
own: a step has one re-pack and one reduce in either arm."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ray_reg import NEAR, FAR, fmt, make, rays, time_arms  # noqa: E402

NEW_ENTRIES = ("nrf_model_set_freq_mask", "nrf_model_get_freq_mask", "nrf_debug_freq_mask_ids")


def arms_for(N, O, net, mode, R, S, which=("plain", "masked")):
    from nerf_few_shot_limitations_amd.training import FusedStep
    o, d, tgt = rays(R)
    arms = {}
    for name in which:
        model = make(N, O, net, mode)
        if name == "masked":
            n_pos, n_dir = model._freq_cols()
            model.set_freq_mask((0.3 + 0.006 * torch.arange(n_pos)).float(), (0.3 + 0.006 * (n_pos + torch.arange(n_dir))).float() if n_dir else None)
        step = FusedStep(model, lr=0.0)
        arms[name] = (lambda step: lambda: step.step_rays(o, d, tgt, NEAR, FAR, S, seed=11))(step)
    return arms


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm, row and order")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["plain", "masked"], default=None, help="time this arm alone")
    ap.add_argument("--lib", default=None, help="another build of libnerfhip.so to load instead of the package's (with --only plain)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_freq_mask needs the GPU: there is no CPU path")
    from nerf_few_shot_limitations_amd import _lib as L
    if a.lib:
        if a.only != "plain":
            raise SystemExit("--lib goes with --only plain: another build need not have the new entries")
        L.LIB_PATH = os.path.abspath(a.lib)
        L.SIGNATURES = {k: v for k, v in L.SIGNATURES.items() if k not in NEW_ENTRIES}
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    R, mode = 2048, "bf16"
    which = (a.only,) if a.only else ("plain", "masked")
    lib_name = os.path.basename(L.LIB_PATH) + " given with --lib" if a.lib else "of this tree"
    print(f"frequency mask in the fused step, {mode}, {R} rays, 'solid' weights, lr = 0; library {lib_name}; arms {' / '.join(which)} alternating "
          f"step by step in one process after {a.warmup} warm-up rounds, until each has {a.seconds:g} s of device time; device events per step, "
          f"ms = median [10th .. 90th percentile]")
    for net in ("v1", "v2"):
        for S in (32, 64):
            arms = arms_for(N, O, net, mode, R, S, which)
            orders = [which] if len(which) == 1 else [which, which[::-1]]
            med = []
            for order in orders:
                ms, wall = time_arms({k: arms[k] for k in order}, a.seconds, a.warmup)
                print(f"  {net} {R} x {S}, {' then '.join(order)}  ({len(next(iter(ms.values())))} steps per arm, loop wall clock {wall:.2f} s):")
                for k in which:
                    print(f"    ({'a' if k == 'plain' else 'b'}) {k:6s} {fmt(ms[k])} ms")
                med.append({k: float(np.median(v)) for k, v in ms.items()})
            if len(which) == 2:
                r = [m["masked"] / m["plain"] for m in med]
                swap = max(abs(med[0][k] / med[1][k] - 1.0) for k in which)
                print(f"    (b) / (a) = {r[0]:.4f} (a first), {r[1]:.4f} (b first); swapping the order moves an arm's median by up to {100 * swap:.2f} %",
                      flush=True)
