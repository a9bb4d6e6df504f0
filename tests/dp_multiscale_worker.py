"""Worker of tests/test_gpu_multiscale_step.py::test_data_parallel_with_clipping_*: one rank of a 2-rank data-parallel run of
FusedStep with the multiscale trainer's options (noise as a tensor, regulariser, clipping, AdamW).  Launched with
torch.distributed.run; every rank trains on its half of a fixed ray batch and rank 0 writes the parameters after the last step
and the pre-clip norms it saw."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nerf_few_shot_limitations_amd as N                                     # noqa: E402
from nerf_few_shot_limitations_amd.training import FusedStep                   # noqa: E402
from oracle import nerf_oracle as O                                           # noqa: E402  (input generators only)

R, S = 128, 16
# reg_weight is linear in the batch mean, as the mse: the average of the two ranks' gradients is the whole batch's
OPTS = dict(reg_weight=0.05, noise_std=0.1, max_grad_norm=0.05, decoupled_weight_decay=True, weight_decay=1e-2)


def batch():
    z = torch.sort(torch.from_numpy(O.uniform01(201, R * S).reshape(R, S) * 4 + 2).float(), dim=-1).values
    rd = torch.from_numpy(O.uniform01(202, R * 3).reshape(R, 3) - 0.5).float()
    tgt = torch.from_numpy(O.uniform01(203, R * 3).reshape(R, 3)).float()
    x = O.positional_encoding(torch.from_numpy(O.uniform01(204, R * S * 3).reshape(R * S, 3) * 4 - 2).float(), 10).reshape(R, S, 63)
    u1, u2 = 1.0 - O.uniform01(205, R * S).astype(np.float64), O.uniform01(206, R * S).astype(np.float64)
    noise = torch.from_numpy((np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).astype(np.float32)).reshape(R, S)
    return x, z, rd, tgt, noise


def main():
    out_path, steps = sys.argv[1], int(sys.argv[2])
    dist.init_process_group(backend=os.environ.get("NERF_TEST_BACKEND", "gloo"))
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)                       # the test box has one GPU: both ranks share it (gloo moves the bytes)
    x, z, rd, tgt, noise = batch()
    lo, hi = rank * R // world, (rank + 1) * R // world
    cut = lambda t: t[lo:hi].contiguous().cuda()
    model = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode="f32")
    model.load_state_dict(O.make_weights("v1", 0, "solid"))
    model = model.cuda().train()
    step = FusedStep(model, lr=1e-2, data_parallel=True, **OPTS)
    norms = []
    for _ in range(steps):
        step(cut(x).reshape(-1, 63), cut(z), cut(rd), cut(tgt), noise=cut(noise))
        norms.append(step.last_grad_norm.item())
    flat = model.flat_params().flat.detach().cpu().numpy()
    gathered = [None] * world
    dist.all_gather_object(gathered, (float(np.abs(flat).sum()), norms))
    if rank == 0:
        np.save(out_path, flat)
        np.save(out_path + ".norms.npy", np.float64(norms))
        assert all(abs(g[0] - gathered[0][0]) < 1e-3 * abs(gathered[0][0]) for g in gathered), gathered
        assert all(g[1] == gathered[0][1] for g in gathered), gathered          # every rank clips by the same norm
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
