"""Measured cost of the few-shot ray regularisers in the fused training step (FusedStep(dist_weight=, occ_weight=, occ_samples=)) --
the numbers quoted in DESIGN.md section 3.4 and kept in profiles/ray_reg_step_time.txt.  Needs the GPU.

    python tools/bench_ray_reg.py > profiles/ray_reg_step_time.txt

Every row is one batch shape (2048 rays at 32 and at 64 samples) and one family (V1, V2), bf16; its two arms take turns step by step
in ONE process, after warm-up:
    (a) multi : the multi-term step (reg_weight = 1e-4) -- nrf_composite_loss_backward, the clipped optimiser entry;
    (b) reg   : the same step with dist_weight = 1e-2, occ_weight = 1e-2, occ_samples = S / 8 -- nrf_composite_reg_loss_backward, the
                same optimiser entry, nrf_ray_terms_finish.
The learning rate is 0 and the jitter seed fixed, so that every step of an arm does the same work.  Each step is timed by a pair of
device events (host gaps inside a step count, as they do in a training loop); the arms alternate until each has `--seconds` of
device time.  Under every row, the two loss launches alone on the row's shape: `--launches` back-to-back launches of each entry
between one pair of events, entries alternating, the median of `--rounds` rounds.

    python tools/bench_ray_reg.py --only multi --lib /path/to/another/libnerfhip.so

times arm (a) alone on another build of the library (the parent commit's: the cross-check that arm (a) of the table above, which runs
the kernels this build shares with it, is the parent's step)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEAR, FAR = 2.0, 6.0
MULTI = dict(reg_weight=1e-4)


def make(N, O, net, mode):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
        m.load_state_dict(O.make_weights("v1", 0, "solid"))
    else:
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode=mode)
        m.load_state_dict(O.make_weights("v2", 1, "solid"), strict=False)
    return m.cuda().train()


def rays(R):
    o = (torch.rand(R, 3, generator=torch.Generator().manual_seed(1)) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(torch.rand(R, 3, generator=torch.Generator().manual_seed(2)) - 0.5, dim=-1).cuda().contiguous()
    return o, d, torch.rand(R, 3, generator=torch.Generator().manual_seed(3)).cuda()


def arms_for(N, O, net, mode, R, S, which=("multi", "reg")):
    from nerf_few_shot_limitations_amd.training import FusedStep
    o, d, tgt = rays(R)
    arms = {}
    if "multi" in which:
        multi = FusedStep(make(N, O, net, mode), lr=0.0, **MULTI)
        arms["multi"] = lambda: multi.step_rays(o, d, tgt, NEAR, FAR, S, seed=11)
    if "reg" in which:
        reg = FusedStep(make(N, O, net, mode), lr=0.0, **MULTI, dist_weight=1e-2, occ_weight=1e-2, occ_samples=max(S // 8, 1))
        arms["reg"] = lambda: reg.step_rays(o, d, tgt, NEAR, FAR, S, seed=11)
    return arms


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


def loss_launches(L, R, S, launches, rounds):
    """us per launch of the two loss entries alone, on random rows of the shape: (multi, reg, reg with the distortion term alone, reg
    with the occlusion term alone)."""
    lib, st = L.lib(), L.stream_ptr()
    g = torch.Generator().manual_seed(5)
    rgb, sig = torch.rand(R * S, 3, generator=g).cuda(), (torch.rand(R * S, generator=g) * 3 - 1).cuda()
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, dim=-1).values.cuda()
    _, d, tgt = rays(R)
    pred, d_rgb, d_sig, terms, grad = (torch.empty(n, device="cuda") for n in (R * 3, R * S * 3, R * S, 5 * R, 600000))
    lo = L.loss_opts(1.0, 1e-4, 0.0, None, 0.0, None, 0)
    head = (L.ptr(rgb), 3, L.ptr(sig), 1, L.ptr(z), L.ptr(d), R, S, 0, L.ptr(tgt), C.byref(lo))
    tail = (L.ptr(pred), L.ptr(d_rgb), 3, L.ptr(d_sig), 1, L.ptr(terms), L.ptr(grad), grad.numel(), st)
    k = max(S // 8, 1)
    regs = {"reg": L.ray_reg(1e-2, 1.0 / (FAR - NEAR), 1e-2, k), "dist only": L.ray_reg(1e-2, 1.0 / (FAR - NEAR), 0.0, 0),
            "occ only": L.ray_reg(0.0, 0.0, 1e-2, k)}
    calls = {"multi": lambda: L.check(lib.nrf_composite_loss_backward(*head, *tail))}
    for name, reg in regs.items():
        calls[name] = (lambda reg: lambda: L.check(lib.nrf_composite_reg_loss_backward(*head, C.byref(reg), None, *tail)))(reg)
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


def fmt(a):
    a = np.asarray(a)
    return f"{np.median(a):.4f} [{np.percentile(a, 10):.4f} .. {np.percentile(a, 90):.4f}]"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time per arm and row")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--only", choices=["multi", "reg"], default=None, help="time this arm alone")
    ap.add_argument("--lib", default=None, help="another build of libnerfhip.so to load instead of the package's (with --only multi)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_reg needs the GPU: there is no CPU path")
    from nerf_few_shot_limitations_amd import _lib as L
    if a.lib:
        if a.only != "multi":
            raise SystemExit("--lib goes with --only multi: another build need not have the new entries")
        L.LIB_PATH = os.path.abspath(a.lib)
        L.SIGNATURES = {k: v for k, v in L.SIGNATURES.items() if k not in ("nrf_composite_reg_loss_backward", "nrf_ray_terms_finish")}
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    R, mode = 2048, "bf16"
    which = (a.only,) if a.only else ("multi", "reg")
    lib_name = os.path.basename(L.LIB_PATH) + " given with --lib" if a.lib else "of this tree"
    print(f"few-shot ray regularisers in the fused step, {mode}, {R} rays, 'solid' weights, lr = 0; library {lib_name}; arms "
          f"{' / '.join(which)} alternating step by step in one process after {a.warmup} warm-up rounds, until each has {a.seconds:g} s of device time; "
          f"device events per step, ms = median [10th .. 90th percentile]")
    for net in ("v1", "v2"):
        for S in (32, 64):
            ms, wall = time_arms(arms_for(N, O, net, mode, R, S, which), a.seconds, a.warmup)
            print(f"  {net} {R} x {S}  ({len(next(iter(ms.values())))} steps per arm, loop wall clock {wall:.2f} s):")
            for k in which:
                print(f"    ({'a' if k == 'multi' else 'b'}) {k:5s} {fmt(ms[k])} ms")
            if len(which) == 2:
                m, r = float(np.median(ms["multi"])), float(np.median(ms["reg"]))
                print(f"    (b) / (a) = {r / m:.3f}      (b) - (a) = {(r - m) * 1e3:.1f} us")
                us = loss_launches(L, R, S, a.launches, a.rounds)
                print(f"    loss launch alone, us: " + "   ".join(f"{n} {v:.2f}" for n, v in us.items()), flush=True)
