"""Measured cost of the patch-based depth-smoothness term in the fused training step (FusedStep(depth_smooth_weight=, patch_size=),
n_patches=) -- the numbers quoted in DESIGN.md section 3.4 and kept in profiles/patch_reg_step_time.txt.  Needs the GPU.

    python tools/bench_patch_reg.py > profiles/patch_reg_step_time.txt

The workload is 2048 rays x 64 samples, V2, bf16.  Three arms take turns step by step in ONE process, after warm-up:
    (a) reg    : the regularised step as it was (reg_weight = 1e-4, dist_weight = 1e-2) -- nrf_composite_reg_loss_backward, the clipped
                 optimiser entry, nrf_ray_terms_finish; 2048 supervised rays;
    (b) patch0 : the same step through the new entries with n_patches = 0 (depth_smooth_weight = 0.1) --
                 nrf_composite_patch_loss_backward, the same optimiser entry, nrf_patch_terms_finish; 2048 supervised rays;
    (c) patch  : the new step on 1024 supervised rays + 16 patches of 8 x 8 rays (2048 rays).
The learning rate is 0 and the jitter seed fixed, so that every step of an arm does the same work.  Each step is timed by a pair of
device events (bench_ray_reg.time_arms); the arms alternate until each has `--seconds` of device time, and the whole comparison is
repeated `--blocks` times: the spread of an arm is the range of its block medians, the run-to-run figure (b) - (a) is held against.
Under the table, the loss launches alone on the same shapes."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ray_reg import FAR, MULTI, NEAR, fmt, make, rays, time_arms      # noqa: E402

R, S, P, NP = 2048, 64, 8, 16


def arms_for(N, O, mode):
    from nerf_few_shot_limitations_amd.training import FusedStep
    o, d, tgt = rays(R)
    R_s = R - NP * P * P
    reg = FusedStep(make(N, O, "v2", mode), lr=0.0, **MULTI, dist_weight=1e-2)
    patch0 = FusedStep(make(N, O, "v2", mode), lr=0.0, **MULTI, dist_weight=1e-2, depth_smooth_weight=0.1, patch_size=P)
    patch = FusedStep(make(N, O, "v2", mode), lr=0.0, **MULTI, dist_weight=1e-2, depth_smooth_weight=0.1, patch_size=P)
    tgt_s = tgt[:R_s].contiguous()
    return {"reg": lambda: reg.step_rays(o, d, tgt, NEAR, FAR, S, seed=11),
            "patch0": lambda: patch0.step_rays(o, d, tgt, NEAR, FAR, S, seed=11, n_patches=0),
            "patch": lambda: patch.step_rays(o, d, tgt_s, NEAR, FAR, S, seed=11, n_patches=NP)}


def loss_launches(L, launches, rounds):
    """us per launch of the loss entries alone on random rows of the shape: the parent entry, the new one without and with patches."""
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(5)
    rgb, sig = torch.rand(R * S, 3, generator=g).cuda(), (torch.rand(R * S, generator=g) * 3 - 1).cuda()
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, dim=-1).values.cuda()
    _, d, tgt = rays(R)
    pred, d_rgb, d_sig, terms, grad, pt, pd = (torch.empty(n, device="cuda") for n in (R * 3, R * S * 3, R * S, 5 * R, 600000, NP, NP * P * P))
    lo = L.loss_opts(1.0, 1e-4, 0.0, None, 0.0, None, 0)
    reg = L.ray_reg(1e-2, 1.0 / (FAR - NEAR), 0.0, 0)
    head = (L.ptr(rgb), 3, L.ptr(sig), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo), C.byref(reg), None)
    tail = (L.ptr(pred), L.ptr(d_rgb), 3, L.ptr(d_sig), 1, L.ptr(terms), L.ptr(grad), grad.numel(), st)
    p0, p1 = L.patch_reg(0.1, P, 0), L.patch_reg(0.1, P, NP)
    calls = {"reg": lambda: L.check(lib.nrf_composite_reg_loss_backward(*head, *tail)),
             "patch0": lambda: L.check(lib.nrf_composite_patch_loss_backward(*head, *tail, C.byref(p0), L.ptr(pt), L.ptr(pd))),
             "patch": lambda: L.check(lib.nrf_composite_patch_loss_backward(*head, *tail, C.byref(p1), L.ptr(pt), L.ptr(pd)))}
    us = {n: [] for n in calls}
    for r in range(rounds + 1):
        for n, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:                                        # round 0 warms up
                us[n].append(a.elapsed_time(b) * 1e3 / launches)
    return {n: float(np.median(v)) for n, v in us.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm and block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_patch_reg needs the GPU: there is no CPU path")
    from nerf_few_shot_limitations_amd import _lib as L
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    mode = "bf16"
    print(f"patch regulariser in the fused step, v2 {mode}, {R} rays x {S} samples, 'solid' weights, lr = 0; arms reg / patch0 / patch "
          f"({R - NP * P * P} supervised rays + {NP} patches of {P} x {P}) alternating step by step in one process after {a.warmup} warm-up rounds, "
          f"{a.blocks} blocks of {a.seconds:g} s of device time per arm; device events per step, ms = median [10th .. 90th percentile]")
    arms = arms_for(N, O, mode)
    med = {k: [] for k in arms}
    for b in range(a.blocks):
        ms, wall = time_arms(arms, a.seconds, a.warmup if b == 0 else 0)
        print(f"  block {b} ({len(next(iter(ms.values())))} steps per arm, loop wall clock {wall:.2f} s):")
        for tag, k in zip("abc", arms):
            print(f"    ({tag}) {k:6s} {fmt(ms[k])} ms")
            med[k].append(float(np.median(ms[k])))
    m = {k: float(np.median(v)) for k, v in med.items()}
    spread = {k: max(v) - min(v) for k, v in med.items()}
    print("  block medians, ms: " + "   ".join(f"{k} {m[k]:.4f} (range over blocks {spread[k] * 1e3:.1f} us)" for k in arms))
    print(f"  (b) - (a) = {(m['patch0'] - m['reg']) * 1e3:+.1f} us  ({m['patch0'] / m['reg']:.4f} x)   against the run-to-run range of (a): "
          f"{spread['reg'] * 1e3:.1f} us -> {'within' if abs(m['patch0'] - m['reg']) <= spread['reg'] else 'OUTSIDE'}")
    print(f"  (c) - (a) = {(m['patch'] - m['reg']) * 1e3:+.1f} us  ({m['patch'] / m['reg']:.4f} x)")
    us = loss_launches(L, a.launches, a.rounds)
    print("  loss launch alone, us: " + "   ".join(f"{n} {v:.2f}" for n, v in us.items()), flush=True)
