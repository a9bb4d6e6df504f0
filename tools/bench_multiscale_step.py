"""Step time of training.FusedStep in its two forms on one MI355X: plain (train.py's step: rgb_weight * mse, Adam) against the
multiscale trainer's (density noise from the in-kernel RNG, NeRFLoss with the weights regulariser, gradient clipping, AdamW).

    python tools/bench_multiscale_step.py                    # V1 / V2 / V3 x {2048x32, 512x64} x {bf16, f16}, one JSON line each
    python tools/bench_multiscale_step.py --plain-only --package-root DIR     # the plain step of another checkout's build
    python tools/bench_multiscale_step.py --trace V3 bf16 2048 32             # a short run for rocprofv3 --kernel-trace --stats
    python tools/bench_multiscale_step.py --autograd          # the autograd route: training.Adam(decoupled, max_grad_norm)
                                                               # against clip_grad_norm_ + torch.optim.AdamW

The two forms alternate block by block inside one process (as tools/tail_mode_report.py alternates frames): boxes differ by
+-5 %, and so do the first blocks after a pause.  A block is `--block` steps, free running, timed on the host with one
synchronisation at its end (the step is host-bound at these sizes, so wall time is what a trainer sees); the figure of a form
is the median over its blocks, the spread their (max - min) / median.  --package-root measures a different checkout with this
same script: the yardstick for "plain" is the parent commit's FusedStep on the same box, run alternately with this build's by
the caller.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

FULL = dict(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True, seed=1)      # experiments/multiscale.yaml


def make_model(N, net, mode, dev):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=mode)
    else:
        m = N.NeRFMLP(pos_freq=12 if net == "v3" else 10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=net == "v3", dino_dim=64, mma_mode=mode)
    return m.to(dev).train()


def batch(net, R, S, dev):
    n = R * S
    x = torch.rand(n, 63 if net == "v1" else 3, device=dev) * 2 - 1
    dirs = torch.rand(n, 3, device=dev) * 2 - 1 if net != "v1" else None
    dino = torch.rand(n, 64, device=dev) * 2 - 1 if net == "v3" else None
    z = torch.sort(torch.rand(R, S, device=dev) * 4 + 2, dim=-1).values.contiguous()
    return x, z, torch.rand(R, 3, device=dev) - 0.5, torch.rand(R, 3, device=dev), dirs, dino


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(ts):
    med = statistics.median(ts)
    return {"ms": round(med, 4), "spread": round((max(ts) - min(ts)) / med, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["v1", "v2", "v3"])
    ap.add_argument("--modes", nargs="+", default=["bf16", "f16"])
    ap.add_argument("--shapes", nargs="+", default=["2048x32", "512x64"])
    ap.add_argument("--block", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--trace", nargs=4, metavar=("NET", "MODE", "RAYS", "SAMPLES"), default=None)
    ap.add_argument("--autograd", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.package_root)
    import nerf_few_shot_limitations_amd as N
    from nerf_few_shot_limitations_amd.training import Adam, FusedStep
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if a.trace:
        net, mode, R, S = a.trace[0].lower(), a.trace[1], int(a.trace[2]), int(a.trace[3])
        x, z, d, tgt, dirs, dino = batch(net, R, S, dev)
        for kw in ({}, FULL):                          # 5 warm-up + 50 steps of each form: the trace's call counts divide by 55
            step = FusedStep(make_model(N, net, mode, dev), lr=2e-4, weight_decay=1e-6, **kw)
            for _ in range(55):
                step(x, z, d, tgt, dirs=dirs, dino=dino)
            torch.cuda.synchronize()
        return
    for net in a.nets:
        for shape in a.shapes:
            R, S = (int(v) for v in shape.split("x"))
            for mode in a.modes:
                x, z, d, tgt, dirs, dino = batch(net, R, S, dev)
                if a.autograd:
                    rec = autograd_route(N, Adam, net, mode, R, S, x, z, d, tgt, dirs, dino, a)
                else:
                    forms = {"plain": FusedStep(make_model(N, net, mode, dev), lr=2e-4, weight_decay=1e-6)}
                    if not a.plain_only:
                        forms["full"] = FusedStep(make_model(N, net, mode, dev), lr=2e-4, weight_decay=1e-6, **FULL)
                    fns = {k: (lambda s=s: s(x, z, d, tgt, dirs=dirs, dino=dino)) for k, s in forms.items()}
                    ts = {k: [] for k in fns}
                    for k, fn in fns.items():
                        block_ms(fn, 20)
                    for _ in range(a.blocks):
                        for k, fn in fns.items():
                            ts[k].append(block_ms(fn, a.block))
                    rec = {k: summary(v) for k, v in ts.items()}
                    if "full" in rec:
                        rec["full_minus_plain_us"] = round((rec["full"]["ms"] - rec["plain"]["ms"]) * 1e3, 1)
                print(json.dumps({"net": net, "rays": R, "samples": S, "mode": mode, **rec}), flush=True)


def autograd_route(N, Adam, net, mode, R, S, x, z, d, tgt, dirs, dino, a):
    """The reference's loop body on the drop-in modules with the multiscale trainer's optimiser: torch.nn.utils.clip_grad_norm_ +
    torch.optim.AdamW against training.Adam(decoupled=True, max_grad_norm=1.0).  Host time = the loop without synchronisation
    (what the Python costs, the clip's read-back included, which makes the host wait for the GPU)."""
    vr = N.VolumeRenderer()
    out = {}
    for name in ("torch_clip_adamw", "nrf_adam_clip"):
        m = make_model(N, net, mode, torch.device("cuda", 0))
        m.flat_params().ensure()
        params = list(m.parameters())
        opt = (torch.optim.AdamW(params, lr=2e-4, weight_decay=1e-6) if name == "torch_clip_adamw"
               else Adam(m, lr=2e-4, weight_decay=1e-6, decoupled=True, max_grad_norm=1.0))

        def step():
            opt.zero_grad()
            if net == "v1":
                o4 = m(x).view(R, S, 4)
                c, sg = o4[..., :3], o4[..., 3:4]
            else:
                c, sg = m(x, dirs, dino)
                c, sg = c.view(R, S, 3), sg.view(R, S, 1)
            pred, _, w = vr(c, sg, z, d)
            (torch.nn.functional.mse_loss(pred, tgt) + 1e-4 * torch.mean(w ** 2)).backward()
            if name == "torch_clip_adamw":
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        block_ms(step, 20)
        wall, host = [], []
        for _ in range(a.blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.block):
                step()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            host.append((t1 - t0) * 1e3 / a.block)
            wall.append((t2 - t0) * 1e3 / a.block)
        out[name] = {"wall": summary(wall), "host": summary(host)}
    return out


if __name__ == "__main__":
    main()
