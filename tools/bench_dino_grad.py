"""Cost of the DINO feature gradient on a V3 training step -- the numbers quoted in DESIGN.md section 3.4 and kept as
profiles/dino_grad_step_time.txt.  Needs the GPU.

    python tools/bench_dino_grad.py > profiles/dino_grad_step_time.txt
    python tools/bench_dino_grad.py --trace-target      # a short run of both forms for rocprofv3 --kernel-trace --stats

Same-process A/B: a V3 FusedStep (bf16) without and with `d_dino_out` + the scatter into the feature map
(training.project_fetch_backward), alternating step by step, HIP events around each step after a warm-up; and the two new kernels on
their own with the bytes they move (dino_grad_kernel: 2 x 8 saved tiles of 1 KiB per 32 samples read + 4 C bytes per sample
written; the scatter: 4 C bytes per sample read + the slab copies written and read back).
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_few_shot_limitations_amd as N  # noqa: E402
from nerf_few_shot_limitations_amd import _lib as L  # noqa: E402
from nerf_few_shot_limitations_amd.training import FusedStep, _dino_grad, fetch_backward_workspace, project_fetch_backward  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

POSE = torch.from_numpy(np.asarray(O.LEGO_LIKE_C2W)).float()


def setup(R, S, dd, mode="bf16"):
    m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=dd, mma_mode=mode, dino_grad=True)
    m.load_state_dict(O.make_weights("v3", 4 if dd == 128 else 2, "solid", dino_dim=dd), strict=False)
    m = m.cuda().train()
    ro, rd = O.get_rays(64, 64, O.focal_for(64), POSE)
    idx = torch.arange(R) % (64 * 64)
    o, d = ro.reshape(-1, 3)[idx].cuda().contiguous(), rd.reshape(-1, 3)[idx].cuda().contiguous()
    z = torch.sort(torch.from_numpy(O.uniform01(1, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values.cuda()
    pts = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3).contiguous()
    dirs = d[:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    tgt = torch.from_numpy(O.uniform01(2, R * 3).reshape(R, 3)).float().cuda()
    fmap = torch.from_numpy(O.uniform01(3, 81 * dd).reshape(1, 9, 9, dd) * 2 - 1).float().cuda()
    cam = dict(features=fmap, pose=POSE, focal=O.focal_for(128), H=128, W=128)
    feats = torch.empty((R * S, dd), device="cuda")
    from nerf_few_shot_limitations_amd.renderer import make_dino
    dn, keep = make_dino(**cam)
    L.check(L.lib().nrf_project_fetch(C.byref(dn), L.ptr(pts), R * S, L.ptr(feats), None, L.stream_ptr()))
    return m, pts, z, d, tgt, dirs, feats, cam


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def fmt(t):
    return f"{np.median(t):8.3f} ms [{t.min():.3f} .. {t.max():.3f}]"


def step_report(steps, warmup):
    print(f"V3 FusedStep, bf16, 8 trunk layers: plain step and step + d_dino_out + scatter into a 9x9xC map, alternating step by step in one "
          f"process, {steps} steps each after {warmup} warm-up steps, HIP events around a step; median [min .. max]")
    for R, S in ((2048, 32), (512, 64)):
        for dd in (64, 128):
            m, pts, z, d, tgt, dirs, feats, cam = setup(R, S, dd)
            step = FusedStep(m, lr=1e-5)
            d_feats = torch.empty((R * S, dd), device="cuda")
            d_map = torch.zeros_like(cam["features"])

            def plain():
                step(pts, z, d, tgt, dirs=dirs, dino=feats)

            def with_grad():
                step(pts, z, d, tgt, dirs=dirs, dino=feats, d_dino_out=d_feats)
                project_fetch_backward(cam, pts, d_feats, d_map, accumulate=True)
            for f in (plain, with_grad):
                for _ in range(warmup):
                    f()
            tp, tg = [], []
            for _ in range(steps):
                tp.append(timed(plain, 1, 0)[0])
                tg.append(timed(with_grad, 1, 0)[0])
            tp, tg = np.array(tp), np.array(tg)
            print(f"{R} x {S}, dino_dim {dd:3d}: plain {fmt(tp)}   with feature gradient {fmt(tg)}   +{100 * (np.median(tg) / np.median(tp) - 1):.1f} %", flush=True)
            # the two kernels alone, on the context the last step left
            n = R * S
            h = m._handle
            mode = L.MMA_MODES["bf16"]
            t1 = timed(lambda: _dino_grad(m, mode, n, step.ctx, step.nbytes, pts.device, out=d_feats), 50, 5)
            t2 = timed(lambda: project_fetch_backward(cam, pts, d_feats, d_map, accumulate=True), 50, 5)
            b1 = n / 32 * 2 * 8 * 2048 + n * dd * 4 + n * 8
            ws = L.lib().nrf_fetch_backward_workspace_bytes(9, 9, dd, n)
            b2 = n * dd * 4 + 2 * ws + n * 12
            print(f"    dino_grad_kernel {np.median(t1) * 1e3:7.1f} us ({b1 / np.median(t1) / 1e9:.2f} TB/s of {b1 / 1e6:.1f} MB)   "
                  f"fetch backward (2 launches, host call included) {np.median(t2) * 1e3:7.1f} us ({b2 / 1e6:.1f} MB moved, workspace {ws / 1e6:.1f} MB)", flush=True)


def trace_target():
    m, pts, z, d, tgt, dirs, feats, cam = setup(2048, 32, 64)
    step = FusedStep(m, lr=1e-5)
    d_feats = torch.empty((2048 * 32, 64), device="cuda")
    d_map = torch.zeros_like(cam["features"])
    for _ in range(20):
        step(pts, z, d, tgt, dirs=dirs, dino=feats, d_dino_out=d_feats)
        project_fetch_backward(cam, pts, d_feats, d_map, accumulate=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--trace-target", action="store_true")
    a = ap.parse_args()
    if a.trace_target:
        trace_target()
    else:
        step_report(a.steps, a.warmup)
