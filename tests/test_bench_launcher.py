"""CPU tests of bench.py's host logic: `python bench.py --gpus N` with no launcher starts N fresh ranks through
torch.distributed.run BEFORE torch is imported or a GPU touched, forwards every flag, and relays the children's status."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_self_launch_builds_the_torchrun_command(monkeypatch):
    import bench
    seen = {}

    def fake_run(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = list(cmd), dict(env)
        return subprocess.CompletedProcess(cmd, 7)

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1", "--rehearse", "--mode", "bf16"]
    with pytest.raises(SystemExit) as e:
        bench.main(argv)
    assert e.value.code == 7                                     # the children's status is the parent's
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == argv                              # every flag reaches the ranks unchanged
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    assert "torch" not in bench.__dict__                         # the parent never imported torch at module level


def test_launcher_environment_mismatch_is_refused(monkeypatch):
    import bench
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "4"])
    assert "WORLD_SIZE=2" in str(e.value.code)


def test_headline_mode_is_declared_once():
    import bench
    assert bench.HEADLINE_MODE in ("f16", "bf16", "f16x3", "f32")
    import __graft_entry__ as g
    assert g.HEADLINE_MODE == bench.HEADLINE_MODE


def test_dump_outputs_writes_the_frames_and_a_fixed_sample_above_the_limit(tmp_path):
    """--dump-outputs: (views, H*W, 4) [r,g,b,depth] rows -> rgb (views, H, W, 3) / depth (views, H, W) float32; above the byte
    limit the same seeded sample of rays on every call, within the limit."""
    import numpy as np
    import torch
    import bench
    H, W = 6, 5
    frames = torch.rand(2, H * W, 4)
    bench.dump_outputs(frames, H, W, str(tmp_path / "all"))
    rgb, depth = np.load(tmp_path / "all" / "rgb.npy"), np.load(tmp_path / "all" / "depth.npy")
    assert rgb.dtype == depth.dtype == np.float32
    assert np.array_equal(rgb, frames[..., :3].reshape(2, H, W, 3).numpy()) and np.array_equal(depth, frames[..., 3].reshape(2, H, W).numpy())
    limit = 1024 + 16 * 20                                       # room for 20 of the 60 rays
    for d in ("a", "b"):
        bench.dump_outputs(frames, H, W, str(tmp_path / d), limit=limit)
        assert sum(os.path.getsize(tmp_path / d / f) for f in ("rgb.npy", "depth.npy")) <= limit
    a_rgb, b_rgb = np.load(tmp_path / "a" / "rgb.npy"), np.load(tmp_path / "b" / "rgb.npy")
    a_depth = np.load(tmp_path / "a" / "depth.npy")
    assert a_rgb.shape == (20, 3) and a_depth.shape == (20,) and np.array_equal(a_rgb, b_rgb)
    rows = frames.reshape(-1, 4).numpy()
    idx = [int(np.flatnonzero((rows[:, 3] == v))[0]) for v in a_depth]
    assert idx == sorted(idx) and np.array_equal(rows[idx, :3], a_rgb)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_frame(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` (no --full): the result line holds the headline fields and none of the
    --full legs, and the dumped frame equals render_camera of the same weights bit for bit."""
    import json
    import numpy as np
    import torch
    import bench
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    H, W, S = 64, 48, 16
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--height", str(H),
           "--width", str(W), "--samples", str(S), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["dtype"] == bench.HEADLINE_MODE and out["unit"] == "M ray-samples/s" and out["higher_is_better"] is True
    assert not {"cpu_baseline", "parity", "parity_mode", "ert", "training"} & set(out)
    m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode=bench.HEADLINE_MODE)
    m.load_state_dict(O.make_weights("v1", 0, "solid"))
    m = m.cuda().eval()
    rgb, depth = N.render_camera(m, H, W, O.focal_for(W), torch.from_numpy(O.LEGO_LIKE_C2W.copy()), 2.0, 6.0, S)
    assert np.array_equal(np.load(tmp_path / "rgb.npy"), rgb.cpu().numpy().reshape(1, H, W, 3))
    assert np.array_equal(np.load(tmp_path / "depth.npy"), depth.cpu().numpy().reshape(1, H, W))
