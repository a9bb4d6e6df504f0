#!/usr/bin/env python3
"""Capture tests/golden/trainer_loop.npz by running the REFERENCE's own trainer, `NeRFDINOTrainer` of src/training/train.py:
its `get_rays_for_view`, `render_rays`, `train_step`, `evaluate` and `train`, unmodified.

Run in the build container only (needs the reference checkout):
        PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trainer.py
The fixture holds data only: inputs, the seeds of the recorded random draws and what the trainer computed.

The trainer does not run as written.  All four defects are repaired from outside, by rebinding names:
  * models.dino_feature_model / models.multi_scale_dino are imported first; then inert stand-ins for torchvision,
    torchvision.transforms, imageio, wandb, torchmetrics and lpips go into sys.modules (none is installed; installed earlier they
    break transformers' availability probes); then training.train is imported;
  * D1: the trainer is built with object.__new__ (its __init__ constructs a class that does not exist) and its attributes are set here:
    V2 = the composition of nerf_mlp.PositionalEncoding / DensityMLP / ColorMLP SURVEY.md prescribes, V3 = nerf_mlp.NeRFWithDINO;
  * D2: train.sample_points_along_rays is bound to the flat utils.ray_utils function;
  * D3: the config carries top-level near / far;   D4: device = cpu.
Every stand-in is inert or a pure recorder; none computes a value that reaches the fixture.  (The metric stand-ins return 0, so
`train` never writes a best_*.pth: only the epoch_N.pth names are recorded.)

Randomness is an input: for the duration of a trainer call torch.randperm and torch.rand return recorded draws -- draw number k of a
call comes from O.uniform01(seed0 + k, n) (a permutation is the stable argsort of its uniforms) -- so the fixture stores seeds, and a
test rebuilds every permutation and every (n,S) jitter from them.

Size: the fixture must stay under 300 KB, so (unlike make_golden.thin's every-4th-row rule) final parameters are stored as a strided
sample of PARAM_SAMPLE elements per tensor, and render weights for every 4th ray; tests slice the same way.
"""
import inspect
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NERF_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(REF, "src"))
sys.path.insert(0, os.path.join(REF, "src", "models"))

from oracle import nerf_oracle as O  # noqa: E402  (only its input generators are used here)

torch.set_num_threads(4)

PARAM_SAMPLE = 64
TOL = 1e-4
LR, WD = 5e-4, 1e-6
SEED_IMAGES, SEED_MAPS = 700, 710


def npf(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def param_sample(t):
    """At most PARAM_SAMPLE elements of a tensor, evenly strided over its flattened form."""
    f = t.reshape(-1)
    return f[:: max(1, f.numel() // PARAM_SAMPLE)][:PARAM_SAMPLE]


def orbit_pose():
    """The 'orbit' pose of make_golden.dino_views_geometry: the LEGO-like camera turned 75 degrees about the world z axis."""
    a = np.radians(75.0)
    rz = torch.eye(4)
    rz[0, 0], rz[0, 1], rz[1, 0], rz[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return rz @ torch.from_numpy(O.LEGO_LIKE_C2W.copy())


def scene_images(seed, n, size=16):
    """n RGBA images (size,size,4) as uint8: smooth bright colours plus noise; alpha 0 in one corner block, 255 in the middle,
    fractional elsewhere.  uint8 so that a PNG round trip (the Blender loader) reproduces the floats the trainer saw."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float32) / (size - 1)
    out = []
    for i in range(n):
        u = O.uniform01(seed + i, size * size * 4).reshape(size, size, 4)
        rgb = np.stack([0.5 + 0.4 * xx, 0.5 + 0.4 * yy, np.full_like(xx, 0.6 + 0.1 * i)], -1) + 0.1 * (u[..., :3] - 0.5)
        alpha = u[..., 3].copy()
        alpha[: size // 4, : size // 4] = 0.0
        alpha[size // 4: 3 * size // 4, size // 4: 3 * size // 4] = 1.0
        out.append((np.concatenate([rgb, alpha[..., None]], -1).clip(0, 1) * 255).astype(np.uint8))
    return np.stack(out)


def config(use_dino, save_dir="unused"):
    near, far = 2.0, 6.0
    return {"experiment": {"name": "tiny"}, "near": near, "far": far,
            "data": {"near": near, "far": far, "resolution": 16, "num_views": 2},
            "rendering": {"near": near, "far": far, "chunk_size": 100, "white_bkgd": False},
            "model": {"use_dino": bool(use_dino)},
            "nerf_model": {"pos_freq": 12 if use_dino else 10, "dir_freq": 4, "hidden_dim": 256, "num_layers": 8},
            "training": {"epochs": 4, "batch_size": 24,
                         "progressive_schedule": {"epochs_0_50": [8, 8, 8], "epochs_50_100": [16, 16, 12], "epochs_100_plus": [12, 10, 16]}},
            "optimizer": {"lr": LR, "weight_decay": WD, "lr_milestones": [2], "lr_gamma": 0.5},
            "loss": {"rgb_weight": 1.0, "depth_weight": 0.0, "reg_weight": 0.0},
            "output": {"save_dir": save_dir, "val_freq": 2, "save_freq": 3},
            "dino_model": {"name": "facebook/dinov2-small", "lora_rank": 4, "lora_alpha": 8, "use_lora": True}}


# ------------------------------------------------------------------------------------------------------------------
# the repairs
# ------------------------------------------------------------------------------------------------------------------
REC = types.SimpleNamespace(imwrite=[], wandb=[], get_rays=[])


def import_trainer():
    import models.dino_feature_model as ref_dfm     # first: transformers' availability probes must not meet a stand-in
    import models.multi_scale_dino  # noqa: F401

    def stand_in(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stand_in("torchvision").transforms = stand_in("torchvision.transforms")
    stand_in("imageio", imwrite=lambda path, arr: REC.imwrite.append((path, np.array(arr))))
    stand_in("wandb", init=lambda **k: None, log=lambda d: REC.wandb.append(dict(d)), finish=lambda: None)
    stand_in("torchmetrics", PeakSignalNoiseRatio=object, StructuralSimilarityIndexMeasure=object)
    stand_in("lpips", LPIPS=object)
    import training.train as T
    import utils.ray_utils as ru
    import models.nerf_mlp as ref_mlp
    T.sample_points_along_rays = ru.sample_points_along_rays                                   # D2
    ref_get_rays = T.get_rays

    def get_rays_recorded(H, W, focal, pose):                                                   # pure recorder: the scaled focal is a local of train_step
        REC.get_rays.append((int(H), int(W), float(focal)))
        return ref_get_rays(H, W, focal, pose)
    T.get_rays = get_rays_recorded
    return T, ref_mlp, ref_dfm


T, ref_mlp, ref_dfm = import_trainer()


class V2Composition(torch.nn.Module):
    """'V2 model under the train.py ctor (D1): composition of importable PositionalEncoding + DensityMLP + ColorMLP with
    shared state_dict' behind the call train.py:229 makes."""

    def __init__(self):
        super().__init__()
        self.pos_encoder, self.dir_encoder = ref_mlp.PositionalEncoding(10), ref_mlp.PositionalEncoding(4)
        self.density_mlp, self.color_mlp = ref_mlp.DensityMLP(63, 256, 8), ref_mlp.ColorMLP(256, 27, 128)

    def forward(self, positions, directions, dino_features=None):
        density, feature = self.density_mlp(self.pos_encoder(positions))
        return self.color_mlp(feature, self.dir_encoder(directions)), density


class DinoSide:
    """What the trainer touches of its extractor once the maps are precomputed: the reference's own fetch, and inert mode switches."""
    sample_features_at_points = ref_dfm.SpatialDINOFeatures.sample_features_at_points

    def train(self):
        return self

    def eval(self):
        return self

    def state_dict(self):
        return {}


def make_model(variant, dtype):
    if variant == "v2":
        m, p = V2Composition(), O.make_weights("v2", 1, "fog")
    else:
        m = ref_mlp.NeRFWithDINO(pos_freq=12, dir_freq=4, dino_dim=64, hidden_dim=256, num_density_layers=8)
        p = O.make_weights("v3", 2, "fog")
    sd = m.state_dict()
    assert all(k in sd for k in p), [k for k in p if k not in sd]
    sd.update(p)
    m.load_state_dict(sd)
    return m.to(dtype), list(p.keys())


class Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *a, **k):
        out = self.fn(*a, **k)
        sig = inspect.signature(getattr(self.fn, "forward", self.fn)).bind(*a, **k)
        sig.apply_defaults()
        self.calls.append((tuple(sig.arguments.values()), k, out))
        return out


def metric_stand_in(calls):
    def metric(a, b):
        calls.append((npf(a), npf(b)))
        return torch.tensor(0.0)
    return metric


def make_trainer(variant, H, W, focal, images, test_images, poses, test_poses, maps, dtype=torch.float32, save_dir="unused"):
    use_dino = variant == "v3"
    tr = object.__new__(T.NeRFDINOTrainer)                                                      # D1
    tr.config = config(use_dino, save_dir)                                                      # D3: near / far at top level
    tr.device = torch.device("cpu")                                                            # D4
    tr.use_dino = use_dino
    tr.nerf_model, tr.param_names = make_model(variant, dtype)
    tr.dino_model = DinoSide() if use_dino else None
    tr.dino_features_precomputed = [m.to(dtype) for m in maps]
    tr.volume_renderer = ref_mlp.VolumeRenderer()
    tr.criterion = Recorder(T.NeRFLoss(1.0, 0.0, 0.0))
    ref_render_rays = tr.render_rays
    tr.render_rays = Recorder(lambda rays_o, rays_d, view_idx, N_samples=64: ref_render_rays(rays_o, rays_d, view_idx, N_samples))
    tr.metric_calls = {"psnr": [], "ssim": [], "lpips": []}
    tr.psnr, tr.ssim, tr.lpips = (metric_stand_in(tr.metric_calls[k]) for k in ("psnr", "ssim", "lpips"))
    o = tr.config["optimizer"]
    tr.optimizer = torch.optim.Adam(list(tr.nerf_model.parameters()), lr=o["lr"], weight_decay=o["weight_decay"])       # train.py:113-118
    tr.scheduler = torch.optim.lr_scheduler.MultiStepLR(tr.optimizer, milestones=o["lr_milestones"], gamma=o["lr_gamma"])
    tr.epoch, tr.best_psnr = 0, 0.0
    tr.H, tr.W, tr.focal = H, W, focal
    tr.images = [im.to(dtype) for im in images]
    tr.poses = [p.to(dtype) for p in poses]
    tr.test_images = [im.to(dtype) for im in test_images]
    tr.test_poses = [p.to(dtype) for p in test_poses]
    return tr


class Draws:
    """torch.randperm / torch.rand for the duration of a call: draw k comes from O.uniform01(seed0 + k, n)."""

    def __init__(self, seed0, dtype=torch.float32):
        self.seed0, self.dtype, self.log = seed0, dtype, []

    def _next(self, kind, shape):
        s = self.seed0 + len(self.log)
        self.log.append((kind, s, tuple(shape)))
        return O.uniform01(s, int(np.prod(shape)))

    def __enter__(self):
        self._orig = torch.rand, torch.randperm

        def rand(*size, **kw):
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            return torch.from_numpy(self._next("rand", shape).reshape(shape)).to(self.dtype)

        def randperm(n, **kw):
            return torch.from_numpy(np.argsort(self._next("perm", (n,)), kind="stable"))
        torch.rand, torch.randperm = rand, randperm
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randperm = self._orig


# ------------------------------------------------------------------------------------------------------------------
# sections
# ------------------------------------------------------------------------------------------------------------------
def scene(dtype=torch.float32):
    img = scene_images(SEED_IMAGES, 4)
    images = [torch.from_numpy(a.astype(np.float32) / 255.0) for a in img]
    poses = [torch.from_numpy(O.LEGO_LIKE_C2W.copy()), orbit_pose()]
    t0 = poses[0].clone()
    t0[0, 3] += 0.3
    t1 = poses[1].clone()
    t1[2, 3] += 0.2
    maps = [torch.from_numpy(O.uniform01(SEED_MAPS + v, 4 * 4 * 64).reshape(1, 4, 4, 64) * 2 - 1) for v in range(2)]
    return img, images[:2], images[2:], poses, [t0, t1], maps


RENDER_STAGES = [(32, 32, 32, 96), (64, 64, 48, 96), (128, 128, 64, 96), (64, 64, 48, 37)]       # (H_train, W_train, S, rays): baseline.yaml's stages + a ragged call
RENDER_CASES = [("v2", "eval", 0), ("v2", "train", 0), ("v3", "eval", 1), ("v3", "train", 0), ("v3", "train", 1)]


def renders(out):
    """render_rays at the reference's own shapes: a 128x128 trainer, rays of the three stages' frames (focal scaled as train_step does)."""
    _, images, test_images, poses, test_poses, maps = scene()
    H = W = 128
    focal = O.focal_for(W)
    out.update(render_H=H, render_W=W, render_focal=np.float64(focal), render_stages=np.array(RENDER_STAGES))
    rays = {}
    for v in range(2):
        for k, (Hs, Ws, S, n) in enumerate(RENDER_STAGES):
            ro, rd = T.get_rays(Hs, Ws, focal * (Hs / H), poses[v])
            idx = np.sort(np.argsort(O.uniform01(720 + k, Hs * Ws), kind="stable")[:n])
            rays[v, k] = ro.reshape(-1, 3)[idx].contiguous(), rd.reshape(-1, 3)[idx].contiguous()
            out[f"render_rays_o_view{v}_{k}"], out[f"render_rays_d_view{v}_{k}"] = npf(rays[v, k][0]), npf(rays[v, k][1])
    for c, (variant, mode, view) in enumerate(RENDER_CASES):
        tr = make_trainer(variant, H, W, focal, images, test_images, poses, test_poses, maps)
        tr.nerf_model.train(mode == "train")
        for k, (Hs, Ws, S, n) in enumerate(RENDER_STAGES):
            seed0 = 1000 + 10 * c + k
            with torch.no_grad(), Draws(seed0) as d:
                r = tr.render_rays(*rays[view, k], view, S)
            assert [x[0] for x in d.log] == (["rand"] if mode == "train" else []) and all(x[2] == (n, S) for x in d.log)
            key = f"render_{variant}_{mode}_view{view}_{k}"
            out[key + "_rgb"], out[key + "_depth"], out[key + "_w"] = npf(r["rgb"]), npf(r["depth"]), npf(r["weights"][::4])
            out[key + "_seed"] = seed0 if mode == "train" else -1


EPOCHS = (0, 50, 100)


def one_epoch(variant, epoch, dtype):
    _, images, test_images, poses, test_poses, maps = scene()
    tr = make_trainer(variant, 16, 16, O.focal_for(16), images, test_images, poses, test_poses, maps, dtype)
    del REC.get_rays[:]
    torch.set_default_dtype(dtype)                      # float64 twin: what the trainer creates itself (linspace, the pixel grid) is float64 too
    try:
        with Draws(2000 + epoch, dtype) as d:
            mean = tr.train_step(epoch)
    finally:
        torch.set_default_dtype(torch.float32)
    return tr, d.log, mean, list(REC.get_rays)


def epochs(out):
    """train_step at epochs 0 / 50 / 100, each from the initial weights, in float32 and -- the reference alone -- in float64."""
    for variant in ("v2", "v3"):
        for epoch in EPOCHS:
            tr, log, mean, cast = one_epoch(variant, epoch, torch.float32)
            tw, log64, mean64, _ = one_epoch(variant, epoch, torch.float64)
            assert log == log64
            calls, crit = tr.render_rays.calls, tr.criterion.calls
            B = len(calls)
            assert B == len(crit) == sum(1 for x in log if x[0] == "rand")
            key = f"epoch{epoch}_{variant}"
            loss = np.array([float(sum(c[2].values()).detach()) for c in crit], np.float32)
            loss64 = np.array([float(sum(c[2].values()).detach()) for c in tw.criterion.calls], np.float64)
            twin = np.abs(loss.astype(np.float64) - loss64)
            base = 2e-4 * np.abs(loss.astype(np.float64)) + 1e-6                                   # rtol 2e-4, atol 1e-6
            out[key + "_loss"], out[key + "_loss_twin_diff"] = loss, twin
            out[key + "_loss_bound"] = np.where(twin > 0.5 * base, 4.0 * twin, base)
            mtwin = abs(float(mean) - float(mean64))
            mbase = 2e-4 * abs(float(mean)) + 1e-6
            out[key + "_mean"], out[key + "_mean_bound"] = np.float64(mean), np.float64(4.0 * mtwin if mtwin > 0.5 * mbase else mbase)
            out[key + "_steps"] = B
            out[key + "_pred"] = np.concatenate([npf(c[2]["rgb"]) for c in calls])
            sd, sd64 = tr.nerf_model.state_dict(), tw.nerf_model.state_dict()
            out[key + "_param_bound"] = np.array([max(2.5 * LR * B, 4.0 * float((sd[k].double() - sd64[k]).abs().max())) for k in tr.param_names])
            out[key + "_param_twin_diff"] = np.array([float((sd[k].double() - sd64[k]).abs().max()) for k in tr.param_names])
            for k in tr.param_names:
                out[f"{key}_final_{k}"] = npf(param_sample(sd[k]))
            if variant == "v2":                                                                     # the scene side is the same for both variants
                e = f"epoch{epoch}"
                out[e + "_batch_view"] = np.array([c[0][2] for c in calls])
                out[e + "_batch_S"] = np.array([c[0][3] for c in calls])
                out[e + "_batch_size"] = np.array([c[0][0].shape[0] for c in calls])
                out[e + "_rays_o"] = np.concatenate([npf(c[0][0]) for c in calls])
                out[e + "_rays_d"] = np.concatenate([npf(c[0][1]) for c in calls])
                out[e + "_target"] = np.concatenate([npf(c[0][1]["rgb"]) for c in crit])
                out[e + "_draw_kind"] = np.array([x[0] == "perm" for x in log])                     # True: a view's permutation; False: a batch's jitter
                out[e + "_draw_seed"] = np.array([x[1] for x in log])
                out[e + "_draw_n"] = np.array([x[2][0] for x in log])
                # get_rays calls of a view: the native frame (get_rays_for_view), then -- rescaled stages only -- the stage's frame
                out[e + "_cast"] = np.array(cast, np.float64)
            else:
                assert np.array_equal(out[f"epoch{epoch}_draw_seed"], np.array([x[1] for x in log]))
    out["param_names_v2"] = json.dumps(list(O.make_weights("v2", 1, "fog").keys()))
    out["param_names_v3"] = json.dumps(list(O.make_weights("v3", 2, "fog").keys()))


def evaluation(out):
    """evaluate(0) on the two test views, chunk_size 100 (100 + 100 + 56 rays), from the initial weights."""
    for variant in ("v2", "v3"):
        _, images, test_images, poses, test_poses, maps = scene()
        with tempfile.TemporaryDirectory() as tmp:
            tr = make_trainer(variant, 16, 16, O.focal_for(16), images, test_images, poses, test_poses, maps, save_dir=tmp)
            del REC.imwrite[:]
            tr.evaluate(0)
        assert [c[0][0].shape[0] for c in tr.render_rays.calls] == [100, 100, 56] * 2 and all(c[0][3] == 16 for c in tr.render_rays.calls)
        written = {os.path.basename(p): a for p, a in REC.imwrite}
        for i in range(2):
            pred, gt = tr.metric_calls["psnr"][i]
            img = pred[0].transpose(1, 2, 0)
            # (clamp(v) * 255).astype(uint8) changes where v * 255 crosses 1, 2, ..., 255 (below 0 and above 1 the clamp holds it): a pixel is
            # safe when a render within TOL of the recorded one cannot cross any of them
            y = img.astype(np.float64) * 255
            safe = np.abs(y - np.clip(np.round(y), 1, 255)) > 255 * TOL
            assert safe.mean() >= 0.90, safe.mean()
            out[f"eval_{variant}_image{i}"], out[f"eval_{variant}_png{i}"] = np.ascontiguousarray(img), written[f"render_{i}.png"]
            out[f"eval_{variant}_png_safe{i}"] = safe
            if variant == "v2":
                out[f"eval_target{i}"], out[f"eval_gt_png{i}"] = np.ascontiguousarray(gt[0].transpose(1, 2, 0)), written[f"gt_{i}.png"]


def training_run(out):
    """train(epochs=4): val_freq 2, save_freq 3, milestone at 2."""
    for variant in ("v2", "v3"):
        _, images, test_images, poses, test_poses, maps = scene()
        with tempfile.TemporaryDirectory() as tmp:
            tr = make_trainer(variant, 16, 16, O.focal_for(16), images, test_images, poses, test_poses, maps, save_dir=tmp)
            step_lr = []
            ref_step = tr.train_step

            def train_step(epoch):
                step_lr.append(tr.optimizer.param_groups[0]["lr"])
                return ref_step(epoch)
            tr.train_step = train_step
            del REC.wandb[:], REC.imwrite[:]
            with Draws(3000):
                tr.train(tr.config["training"]["epochs"])
            logs = [r for r in REC.wandb if "lr" in r]
            names = sorted(f for f in os.listdir(tmp) if f.endswith(".pth"))
            ck = {n: torch.load(os.path.join(tmp, n), map_location="cpu", weights_only=False) for n in names}
            key = f"train_{variant}"
            out[key + "_log_epoch"], out[key + "_log_lr"] = np.array([r["epoch"] for r in logs]), np.array([r["lr"] for r in logs], np.float64)
            out[key + "_step_lr"] = np.array(step_lr, np.float64)                                    # the lr in force while epoch e trained
            out[key + "_eval_epochs"] = np.array(sorted({int(os.path.basename(os.path.dirname(p)).split("_")[1]) for p, _ in REC.imwrite}))
            out[key + "_ckpt"] = json.dumps({n: {"keys": sorted(c.keys()), "epoch": int(c["epoch"]), "last_epoch": int(c["scheduler_state_dict"]["last_epoch"]),
                                                 "model_keys": sorted(c["nerf_model_state_dict"].keys())} for n, c in ck.items()})


def main():
    out = {}
    img, _, _, poses, test_poses, maps = scene()
    out.update(images=img, poses=np.stack([npf(p) for p in poses]), test_poses=np.stack([npf(p) for p in test_poses]),
               maps=np.concatenate([npf(m) for m in maps]), H=16, W=16, focal=np.float64(O.focal_for(16)),
               config_v2=json.dumps(config(False)), config_v3=json.dumps(config(True)), tol=np.float64(TOL), param_sample=PARAM_SAMPLE)
    with torch.no_grad():
        renders(out)
        evaluation(out)
    epochs(out)
    training_run(out)
    path = os.path.join(HERE, "trainer_loop.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"trainer_loop: {size / 1024:.1f} KiB, {len(out)} arrays")
    assert size < 300 * 1024, size


if __name__ == "__main__":
    main()
