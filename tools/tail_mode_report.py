"""Measured error and cost of the tail mode (render_rays' tail_mode="f16x3": a 16-bit render whose last sample per ray is
evaluated in split-f16) -- the numbers quoted in DESIGN.md section 3.1 and kept under profiles/.  Needs the GPU.

    python tools/tail_mode_report.py --error  > profiles/tail_mode_error_report.txt
    python tools/tail_mode_report.py --cost   > profiles/tail_mode_frame_time.txt

--error: V1 / V2 / V3 x {f16, bf16} x {plain, tail} on the "solid" and "fog" 100 x 100 x 32 frames of
         tests/test_gpu_parity.py::test_render_vs_oracle_100x100x32 and on the 16-row band of the 800 x 800 x 64 frame: max / median
         |rgb| and |depth| error over ALL rays against the CPU oracle, PSNR against it, PSNR delta against the oracle's render with
         twice the samples (the common ground truth).
--cost : same-process A/B, plain and tail alternating frame by frame, HIP events around the launch(es) of a frame, after a warm-up:
         800 x 800 x 64 and 100 x 100 x 32, V1 / V2 / V3, f16 and bf16.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_few_shot_limitations_amd as N  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

C2W = torch.from_numpy(np.asarray(O.LEGO_LIKE_C2W))


def make(net, scene):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode="f16")
        p = O.make_weights("v1", 0, scene)
        m.load_state_dict(p)
    elif net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode="f16")
        p = O.make_weights("v2", 1, scene)
        m.load_state_dict(p, strict=False)
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=64, mma_mode="f16")
        p = O.make_weights("v3", 2, scene)
        m.load_state_dict(p, strict=False)
    return m.cuda().eval(), p


def dino_for(net, H, W):
    if net != "v3":
        return None
    fm = torch.from_numpy(O.uniform01(7, 28 * 28 * 64).reshape(1, 28, 28, 64) * 2 - 1)
    return dict(features=fm, pose=C2W, focal=O.focal_for(W), H=H, W=W)


def error_report():
    frames = [("100x100x32", 100, 100, 32, 0, 100 * 100), ("800x800x64 band (rows 400-415)", 800, 800, 64, 400 * 800, 416 * 800)]
    for label, H, W, S, b0, b1 in frames:
        ro, rd = O.get_rays(H, W, O.focal_for(W), C2W)
        ro, rd = ro.reshape(-1, 3)[b0:b1], rd.reshape(-1, 3)[b0:b1]
        for net in ("v1", "v2", "v3"):
            for scene in ("solid", "fog"):
                m, p = make(net, scene)
                dino = dino_for(net, H, W)
                kw = dict(dino=dino) if dino else {}
                ref = O.render_rays(p, net, ro, rd, 2.0, 6.0, S, **kw)
                gt = O.render_rays(p, net, ro, rd, 2.0, 6.0, 2 * S, **kw)["rgb"]
                ps_ref = O.psnr(ref["rgb"], gt)
                for mode in ("f16", "bf16"):
                    for tail in (None, "f16x3"):
                        rgb, depth = N.render_camera(m, H, W, O.focal_for(W), C2W, 2.0, 6.0, S, ray_begin=b0, ray_end=b1, mma_mode=mode,
                                                     tail_mode=tail, **kw)
                        err = (rgb.cpu() - ref["rgb"]).abs().max(-1).values
                        derr = (depth.cpu() - ref["depth"]).abs()
                        print(f"{label} {net} {scene} {mode}{'+tail' if tail else '     '}: rgb max {float(err.max()):.3e} median {float(err.median()):.3e}  "
                              f"depth max {float(derr.max()):.3e} median {float(derr.median()):.3e}  psnr vs oracle {O.psnr(rgb.cpu(), ref['rgb']):.2f} dB  "
                              f"psnr-delta vs 2S ground truth {abs(O.psnr(rgb.cpu(), gt) - ps_ref):.5f} dB", flush=True)


def cost_report(frames=24, warmup=4):
    print(f"frame time, plain and tail alternating frame by frame in one process, {frames} frames each after {warmup} warm-up frames; HIP events "
          "around the launch(es) of a frame (plain: 1, tail: 2); ms = median [min .. max]")
    for label, H, S in (("800x800x64", 800, 64), ("100x100x32", 100, 32)):
        for net in ("v1", "v2", "v3"):
            m, _ = make(net, "solid")
            dino = dino_for(net, H, H)
            kw = dict(dino=dino) if dino else {}
            for mode in ("f16", "bf16"):
                rgb = torch.empty((H * H, 3), device="cuda"); depth = torch.empty((H * H,), device="cuda")
                t = {None: [], "f16x3": []}
                for i in range(warmup + frames):
                    for tail in (None, "f16x3"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        N.render_camera(m, H, H, O.focal_for(H), C2W, 2.0, 6.0, S, mma_mode=mode, tail_mode=tail, out_rgb=rgb, out_depth=depth, **kw)
                        e1.record()
                        e1.synchronize()
                        if i >= warmup:
                            t[tail].append(e0.elapsed_time(e1))
                a, b = np.array(t[None]), np.array(t["f16x3"])
                print(f"{label} {net} {mode}: plain {np.median(a):.3f} [{a.min():.3f} .. {a.max():.3f}] ms   tail {np.median(b):.3f} [{b.min():.3f} .. {b.max():.3f}] ms   "
                      f"tail / plain = {np.median(b) / np.median(a):.4f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--error", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tail_mode_report needs the GPU: there is no CPU path")
    if a.error:
        error_report()
    if a.cost:
        cost_report(a.frames)
