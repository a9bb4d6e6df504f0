"""Measured cost of InfoNeRF's ray-entropy and patch-KL terms in the fused training step (FusedStep(ent_weight=, ent_threshold=,
kl_weight=)) -- the numbers quoted in DESIGN.md section 3.4 and kept in profiles/info_reg_step_time.txt.  Needs the GPU.

    python tools/bench_info_reg.py > profiles/info_reg_step_time.txt

The workload is 2048 supervised rays + 16 patches of 8 x 8 rays (3072 rays), V2, bf16, at S = 64 and at S = 128.  Four arms take
turns step by step in ONE process, after warm-up:
    (a) patch : the patch step as it was (reg_weight = 1e-4, dist_weight = 1e-2, depth_smooth_weight = 0.1) --
                nrf_composite_patch_loss_backward, the clipped optimiser entry, nrf_patch_terms_finish;
    (b) ent   : the same step with ent_weight = 1e-3 -- nrf_composite_info_loss_backward, nrf_info_terms_finish;
    (c) kl    : the same step with kl_weight = 1e-3;
    (d) both  : the same step with both.
The learning rate is 0 and the jitter seed fixed, so that every step of an arm does the same work.  Each step is timed by a pair of
device events (bench_ray_reg.time_arms); the arms alternate until each has `--seconds` of device time, and the whole comparison is
repeated `--blocks` times: the spread of an arm is the range of its block medians.  Under each table, the loss launches alone on the
same shape."""
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

RS, P, NP = 2048, 8, 16
R = RS + NP * P * P
ARMS = {"patch": {}, "ent": dict(ent_weight=1e-3), "kl": dict(kl_weight=1e-3), "both": dict(ent_weight=1e-3, kl_weight=1e-3)}


def arms_for(N, O, mode, S):
    from nerf_few_shot_limitations_amd.training import FusedStep
    o, d, tgt = rays(R)
    tgt_s = tgt[:RS].contiguous()
    steps = {k: FusedStep(make(N, O, "v2", mode), lr=0.0, **MULTI, dist_weight=1e-2, depth_smooth_weight=0.1, patch_size=P, **kw) for k, kw in ARMS.items()}
    return {k: (lambda s=s: s.step_rays(o, d, tgt_s, NEAR, FAR, S, seed=11, n_patches=NP)) for k, s in steps.items()}


def loss_launches(L, S, launches, rounds):
    """us per launch of the loss entries alone on random rows of the shape: the patch entry, the new one with each term and with both."""
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(5)
    rgb, sig = torch.rand(R * S, 3, generator=g).cuda(), (torch.rand(R * S, generator=g) * 3 - 1).cuda()
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, dim=-1).values.cuda()
    _, d, tgt = rays(R)
    pred, d_rgb, d_sig, terms, grad, pt, pd, it, pk = (torch.empty(n, device="cuda") for n in (R * 3, R * S * 3, R * S, 5 * R, 600000, NP, NP * P * P, R, NP))
    lo = L.loss_opts(1.0, 1e-4, 0.0, None, 0.0, None, 0)
    reg = L.ray_reg(1e-2, 1.0 / (FAR - NEAR), 0.0, 0)
    patch = L.patch_reg(0.1, P, NP)
    head = (L.ptr(rgb), 3, L.ptr(sig), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo), C.byref(reg), None)
    tail = (L.ptr(pred), L.ptr(d_rgb), 3, L.ptr(d_sig), 1, L.ptr(terms), L.ptr(grad), grad.numel(), st, C.byref(patch), L.ptr(pt), L.ptr(pd))
    infos = {k: L.info_reg(kw.get("ent_weight", 0.0), 0.01, kw.get("kl_weight", 0.0)) for k, kw in ARMS.items() if kw}
    calls = {"patch": lambda: L.check(lib.nrf_composite_patch_loss_backward(*head, *tail))}
    for k, info in infos.items():
        calls[k] = lambda info=info: L.check(lib.nrf_composite_info_loss_backward(*head, *tail, C.byref(info), L.ptr(it), L.ptr(pk)))
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
        raise SystemExit("bench_info_reg needs the GPU: there is no CPU path")
    from nerf_few_shot_limitations_amd import _lib as L
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    mode = "bf16"
    for S in (64, 128):
        print(f"information regularisers in the fused step, v2 {mode}, {RS} supervised rays + {NP} patches of {P} x {P} ({R} rays) x {S} samples, "
              f"'solid' weights, lr = 0; arms {' / '.join(ARMS)} alternating step by step in one process after {a.warmup} warm-up rounds, "
              f"{a.blocks} blocks of {a.seconds:g} s of device time per arm; device events per step, ms = median [10th .. 90th percentile]")
        arms = arms_for(N, O, mode, S)
        med = {k: [] for k in arms}
        for b in range(a.blocks):
            ms, wall = time_arms(arms, a.seconds, a.warmup if b == 0 else 0)
            print(f"  block {b} ({len(next(iter(ms.values())))} steps per arm, loop wall clock {wall:.2f} s):")
            for tag, k in zip("abcd", arms):
                print(f"    ({tag}) {k:6s} {fmt(ms[k])} ms")
                med[k].append(float(np.median(ms[k])))
        m = {k: float(np.median(v)) for k, v in med.items()}
        spread = {k: max(v) - min(v) for k, v in med.items()}
        print("  block medians, ms: " + "   ".join(f"{k} {m[k]:.4f} (range over blocks {spread[k] * 1e3:.1f} us)" for k in arms))
        for tag, k in zip("bcd", list(arms)[1:]):
            print(f"  ({tag}) - (a) = {(m[k] - m['patch']) * 1e3:+.1f} us  ({m[k] / m['patch']:.4f} x)")
        us = loss_launches(L, S, a.launches, a.rounds)
        print("  loss launch alone, us: " + "   ".join(f"{n} {v:.2f}" for n, v in us.items()), flush=True)
