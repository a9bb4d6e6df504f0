"""Records what train_cli does, for tests/test_train_cli_flags_host.py and tests/test_gpu_train_cli_transcript.py.

    python tools/record_train_cli.py flags A.json             (no GPU)
    python tools/record_train_cli.py transcript A.json        (one MI355X)
    python tools/record_train_cli.py merge A.json B.json tests/golden/train_cli_flags.json

A recording is {section: {field: value}}.  Every recording is made twice, in two processes; `merge` keeps what both agree on: a
leaf that differs becomes null and its path is listed under "dropped" (a field whose shape differs is dropped whole).  The tests call
`flags()` / `epoch_case()` / `main_case()` themselves and compare with the file, skipping nulls.  Only train_cli's public names are used
(the parser is reached through `main`, by stopping ArgumentParser.parse_args), so one script records any commit.

flags -- through `main`: argv = --config <a complete tiny config> --data <a missing directory> + one or two FRAGMENTS, against the
four CONFIGS; the outcome is the SystemExit text or the class of what the missing data set raises.  Through the functions: every
*_args_error, *_options and draws_patches on the empty namespace, on every namespace holding one attribute, on train_extractor /
occupancy_res plus one of the fields the checks read without a default (given or None), and on every fragment's parsed namespace.  The digest of --help at COLUMNS=100.  OccupancySchedule / PerViewOccupancy.from_args over a stub OccupancyGrid, and
the key set save_checkpoint writes.  Outcomes are indices into "tables": a row of `main` is one character per argv.

transcript -- train_epoch on the scene of tests/golden/trainer_loop.npz (two 16x16 views, maps (2,4,4,64), f32, oracle weights) with
a recording FusedStep, ExtractorTrainer and occupancy schedules: `calls` holds every call in order with its keyword names, tensors as
"dtype[shape]#k", ctypes arrays as "#k", scalars by value, a grid by which object it is; `digests`[k] holds the k-th digest (first 16
hex digits of SHA-256 of the bytes; a returned loss as float.hex()).  Then the raising combinations by message, and `main` end to end.
"""
import argparse
import contextlib
import ctypes as C
import hashlib
import io
import itertools
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nerf_few_shot_limitations_amd import train_cli as T                   # noqa: E402

CFG = ("experiment: {{name: tiny}}\ndata: {{near: 2.0, far: 6.0, resolution: 16, num_views: 2}}\n"
       "rendering: {{near: 2.0, far: 6.0, chunk_size: 2048, white_bkgd: false}}\nmodel: {{use_dino: {dino}{model}}}\n"
       "nerf_model: {{pos_freq: 10, dir_freq: 4, hidden_dim: 256, num_layers: 8}}\n"
       "training: {{epochs: 3, batch_size: 64, progressive_schedule: {{epochs_0_50: [16, 16, 8], epochs_50_100: [16, 16, 12], epochs_100_plus: [16, 16, 16]}}}}\n"
       "optimizer: {{lr: 2.0e-3, weight_decay: 1.0e-6, lr_milestones: [2], lr_gamma: 0.5}}\nloss: {{rgb_weight: 1.0, depth_weight: 0.0, reg_weight: 0.0}}\n"
       "output: {{save_dir: unused, val_freq: 2, save_freq: 3}}\n"
       "dino_model: {{name: facebook/dinov2-small, lora_rank: 4, lora_alpha: 8, use_lora: {lora}}}\n")
CONFIGS = {"no_dino": dict(dino="false", model="", lora="true"), "dino": dict(dino="true", model="", lora="true"),
           "multi_scale": dict(dino="true", model=", dino_model_type: multi_scale", lora="true"),
           "no_lora": dict(dino="true", model="", lora="false")}

# one good and each bad value of every flag (the bad values of the *_host.py suites of the flags)
FRAGMENTS = [f.split() for f in (
    "--n-importance 4", "--n-importance -1", "--coarse-weight 0.5", "--coarse-weight 0", "--coarse-weight -1", "--recipe multiscale",
    "--dist-weight 0.01", "--dist-weight -1", "--dist-weight nan", "--dist-weight inf", "--occ-weight 0.01", "--occ-weight -1", "--occ-weight nan",
    "--occ-samples 2", "--occ-samples 0",
    "--depth-smooth-weight 0.1", "--depth-smooth-weight -1", "--depth-smooth-weight nan", "--patch-size 4", "--patch-size 1", "--patch-size 17",
    "--patches-per-step 2", "--patches-per-step 0", "--patch-stride 2", "--patch-stride 0",
    "--entropy-weight 0.001", "--entropy-weight -1", "--entropy-weight inf", "--entropy-threshold 0.02", "--entropy-threshold -1",
    "--entropy-threshold nan", "--entropy-unseen", "--kl-weight 1e-5", "--kl-weight -1",
    "--freq-reg-end 4", "--freq-reg-end -1", "--no-freq-reg-dirs",
    "--occupancy-res 32", "--occupancy-res 48", "--occupancy-res 1024", "--occupancy-res -32", "--occupancy-box -1 1", "--occupancy-box 1 -1",
    "--occupancy-threshold 0.02", "--occupancy-decay 0.9", "--occupancy-decay 1.5", "--occupancy-refresh-every 2", "--occupancy-refresh-every 0",
    "--occupancy-cells-per-refresh 64", "--occupancy-cells-per-refresh 33", "--occupancy-cells-per-refresh 0", "--occupancy-warmup 1",
    "--occupancy-warmup -1", "--occupancy-per-view",
    "--fused-inputs", "--dino-maps maps.pt", "--dino-weights weights", "--dino-random-init", "--train-extractor",
    "--train-extractor --dino-maps maps.pt", "--train-extractor --dino-random-init", "--train-extractor --dino-random-init --data-parallel",
    "--train-extractor --dino-weights weights --occupancy-res 32 --occupancy-per-view",
    # (what the option readers make of two flags together)
    "--occ-weight 0.01 --occ-samples 2", "--kl-weight 1e-5 --patch-size 4", "--entropy-weight 0.001 --entropy-unseen --patch-size 4",
    "--depth-smooth-weight 0.1 --kl-weight 1e-5 --patch-size 4", "--entropy-weight 0.001 --entropy-threshold 0.02", "--freq-reg-end 4 --no-freq-reg-dirs")]
NAMES = [" ".join(f) for f in FRAGMENTS]
ERRORS = ("hierarchical_args_error", "ray_reg_args_error", "patch_reg_args_error", "info_reg_args_error", "freq_reg_args_error")
WITH_CFG = ("extractor_args_error", "occupancy_args_error")
OPTIONS = ("patch_reg_options", "info_reg_options", "freq_reg_options", "draws_patches")
COLUMNS = "100"


def sha16(data):
    return hashlib.sha256(data).hexdigest()[:16]


# ---- flags -------------------------------------------------------------------------------------------------------------------------
class _Parsed(Exception):
    pass


def parsed(argv):
    """The namespace `main` parses argv into: parse_args is stopped behind its return."""
    real = argparse.ArgumentParser.parse_args

    def stop(self, args=None, namespace=None):
        raise _Parsed(real(self, args, namespace))
    argparse.ArgumentParser.parse_args = stop
    try:
        T.main(list(argv))
    except _Parsed as p:
        return p.args[0]
    finally:
        argparse.ArgumentParser.parse_args = real
    raise AssertionError("main did not parse")


def outcome(argv):
    """What `main` ends in: the SystemExit text, or the class name of another exception."""
    assert "--data-parallel" not in argv or "--train-extractor" in argv          # (refused at the parent: an accepted one opens a process group)
    sink = io.StringIO()
    try:
        with contextlib.redirect_stdout(sink), contextlib.redirect_stderr(sink):
            T.main(list(argv))
    except SystemExit as e:
        return str(e.code)
    except Exception as e:
        return type(e).__name__
    return "returned"


def result(fn, *args):
    """None, the text, the dictionary / boolean, or the class name of what fn raises."""
    try:
        return fn(*args)
    except Exception as e:
        return {"raises": type(e).__name__}


class Table:
    def __init__(self):
        self.rows, self.index = [], {}

    def add(self, value):
        key = json.dumps(value, sort_keys=True)
        if key not in self.index:
            self.index[key] = len(self.rows)
            self.rows.append(value)
        return self.index[key]


FUNCTIONS = ERRORS + OPTIONS + ("patch_draw_error", "ray_reg_options") + tuple(f"{name}/{c}" for name in WITH_CFG for c in CONFIGS)


def function_results(ns, cfgs):
    """What each of FUNCTIONS gives on a namespace, in their order."""
    out = [result(getattr(T, name), ns) for name in ERRORS + OPTIONS]
    out += [result(T.patch_draw_error, ns, "--kl-weight"), result(T.ray_reg_options, ns, 2.0, 6.0)]
    return out + [result(getattr(T, name), ns, cfg) for name in WITH_CFG for cfg in cfgs.values()]


class StubGrid:
    """Stands in for occupancy.OccupancyGrid: keeps what `full` was asked for."""
    made = []

    def __init__(self, res, lo, hi, device):
        self.asked = [res, lo, hi, str(device)]
        self.n_cells = int(res) ** 3
        self.bits = torch.zeros(self.n_cells // 32, dtype=torch.int32)
        StubGrid.made.append(self)

    @classmethod
    def full(cls, res, lo, hi, outside=0, device=None):
        return cls(res, lo, hi, device)


@contextlib.contextmanager
def stub_grid():
    from nerf_few_shot_limitations_amd import occupancy
    real = occupancy.OccupancyGrid
    occupancy.OccupancyGrid = StubGrid
    try:
        yield
    finally:
        occupancy.OccupancyGrid = real


def schedule_facts(s):
    return {"full": s.full.asked, "grid": s.grid.asked, "threshold": s.threshold, "decay": s.decay, "refresh_every": s.refresh_every,
            "warmup": s.warmup, "cells": s.cells, "steps": s.steps}


def grid_pins(base):
    """Per --occupancy-* fragment: what from_args hands to the single schedule, and whether the three per-view schedules got the same
    while sharing one all-ones grid and owning their live grids."""
    out = {}
    with stub_grid():
        spaces = {name: parsed(base + ["--occupancy-res", "64"] + frag) for name, frag in zip(NAMES, FRAGMENTS)
                  if name.startswith("--occupancy-") and not name.startswith(("--occupancy-res", "--occupancy-per-view"))}
        spaces["defaults"] = parsed(base + ["--occupancy-res", "64"])
        spaces["partial namespace"] = argparse.Namespace(occupancy_res=32)
        for name, ns in spaces.items():
            def both():
                single = schedule_facts(T.OccupancySchedule.from_args(ns, "dev"))
                views = T.PerViewOccupancy.from_args(ns, 3, "dev").views
                return dict(single, per_view=[len(views), all(schedule_facts(s) == single for s in views),
                                              all(s.full is views[0].full for s in views), len({id(s.grid) for s in views})])
            out[name] = result(both)
    return out


class _Stub:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def checkpoint_pins():
    """The key set save_checkpoint writes per recipe, with and without the extractor, the grids and the mask; the rest of a checkpoint once."""
    cfg = {"optimizer": {"lr": 1e-3, "lr_milestones": [2], "lr_gamma": 0.5}}
    out, rest = {}, []
    with stub_grid(), tempfile.TemporaryDirectory() as tmp:
        occ = T.PerViewOccupancy(2, 32, device="cpu")
        single = T.OccupancySchedule(32, device="cpu")
        ext = _Stub(extractor=_Stub(state_dict=lambda: {"lora_A": torch.ones(2)}), opt=_Stub(state_dict=lambda: {"state": {}, "param_groups": []}))
        step = _Stub(opt=_Stub(step_count=3, exp_avg=torch.zeros(4), exp_avg_sq=torch.zeros(4), lr=1e-3))
        for recipe, e, o, mask in itertools.product(("train", "multiscale"), (None, ext), (None, single, occ), (False, True)):
            model = _Stub(state_dict=lambda: {"w": torch.ones(3)}, freq_mask=(torch.ones(2), None) if mask else (None, None))
            path = os.path.join(tmp, "sub", "c.pth")
            T.save_checkpoint(path, model, step, 1, 20.0, cfg, recipe, e, o)
            ck = torch.load(path, map_location="cpu", weights_only=True)
            name = f"{recipe}/extractor={e is not None}/occupancy={'none' if o is None else 'single' if o is single else 'per_view'}/mask={mask}"
            out[name] = " ".join(sorted(ck))
            rest.append({"optimizer": sorted(ck["optimizer_state_dict"]), "scheduler": ck["scheduler_state_dict"], "epoch": ck["epoch"],
                         "best_psnr": ck["best_psnr"]})
    out["(every case)"] = dict(rest[0], same_in_all=all(r == rest[0] for r in rest))
    return out


def flags():
    """The whole CPU recording."""
    old_columns = os.environ.get("COLUMNS")
    os.environ["COLUMNS"] = COLUMNS
    try:
        with tempfile.TemporaryDirectory() as tmp:
            return _flags(tmp)
    finally:
        os.environ.pop("COLUMNS")
        if old_columns is not None:
            os.environ["COLUMNS"] = old_columns


ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+-"      # an outcome of `main` is one character: its index in "texts"


def _flags(tmp):
    from nerf_few_shot_limitations_amd import load_config
    paths = {}
    for c, kw in CONFIGS.items():
        paths[c] = os.path.join(tmp, c + ".yaml")
        with open(paths[c], "w") as f:
            f.write(CFG.format(**kw))
    cfgs = {c: load_config(p) for c, p in paths.items()}
    missing = os.path.join(tmp, "no_such_scene")
    texts, results = Table(), Table()
    out = {"main": {}, "functions": {}}
    for c, p in paths.items():
        base = ["--config", p, "--data", missing]
        for i, frag in enumerate(FRAGMENTS):              # the fragment alone, then with every later one
            out["main"][f"{c}: {NAMES[i]}"] = "".join(ALPHABET[texts.add(outcome(base + frag + (FRAGMENTS[j] if j > i else [])))]
                                                      for j in range(i, len(FRAGMENTS)))
        out["main"][f"{c}: (no flag)"] = ALPHABET[texts.add(outcome(base))]
    base = ["--config", paths["dino"], "--data", missing]
    default = parsed(base)
    spaces = {"(empty)": argparse.Namespace()}
    for i, frag in enumerate(FRAGMENTS):
        ns = parsed(base + frag)
        spaces["parsed: " + NAMES[i]] = ns
        for dest, value in vars(ns).items():
            if value != getattr(default, dest):           # (nan != nan: a nan value is kept, as it should be)
                spaces[f"only: {dest}={value!r}"] = argparse.Namespace(**{dest: value})
    for dest in ("patch_size", "patches_per_step", "patch_stride", "occupancy_res", "n_importance", "seed"):     # defaults, alone in a namespace
        spaces[f"only: {dest}={getattr(default, dest)!r}"] = argparse.Namespace(**{dest: getattr(default, dest)})
    # the fields the checks read without a default, one at a time: train_extractor / occupancy_res plus ONE of them, given or None --
    # a check must return at the first fault it meets and raise only where it reads a field the namespace lacks
    bare = T.OCCUPANCY_FLAGS + ("dino_maps", "dino_weights", "dino_random_init", "data_parallel", "occupancy_per_view", "train_extractor")
    for label, ns in list(spaces.items()):
        (dest, value), = vars(ns).items() if label.startswith("only: ") else [(None, None)]
        for with_, on in (("train_extractor", True), ("occupancy_res", 32)) if dest in bare and dest != "train_extractor" else ():
            for v in (value, None):
                spaces[f"two: {with_}={on!r} {dest}={v!r}"] = argparse.Namespace(**{with_: on, dest: v})
    for label, ns in spaces.items():
        out["functions"][label] = [results.add(r) for r in function_results(ns, cfgs)]
    sink, argv0 = io.StringIO(), sys.argv[0]
    sys.argv[0] = "train_cli.py"                          # (the usage line names the program)
    try:
        with contextlib.redirect_stdout(sink), contextlib.suppress(SystemExit):
            T.main(["--help"])
    finally:
        sys.argv[0] = argv0
    out["help"] = {"columns": COLUMNS, "digest": sha16(sink.getvalue().encode()), "lines": len(sink.getvalue().splitlines())}
    out["grids"] = grid_pins(base)
    out["checkpoints"] = checkpoint_pins()
    out["tables"] = {"fragments": NAMES, "functions": list(FUNCTIONS), "texts": texts.rows, "results": results.rows}
    return json.loads(json.dumps(out))          # (tuples as lists, nan as NaN: what the file holds)




# ---- transcript --------------------------------------------------------------------------------------------------------------------
NEAR, FAR = 2.0, 6.0
OUT_BUFFERS = ("d_dino_out", "points_out")
TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, image_size=28, patch_size=14)     # tests/test_gpu_dino_grad.py's


def tensor_digest(t):
    return sha16(t.detach().to("cpu").contiguous().numpy().tobytes())


class Log:
    def __init__(self):
        self.calls, self.digests, self.grids, self.buffers, self.alive = [], [], {}, {}, []

    def digest(self, value):
        self.digests.append(value)
        return f"#{len(self.digests) - 1}"

    def buffer(self, t):
        """Which storage a tensor lives in, counted in the order they were first seen (kept alive: no address comes twice)."""
        st = t.untyped_storage()
        if st.data_ptr() not in self.buffers:
            self.buffers[st.data_ptr()] = len(self.buffers)
            self.alive.append(st)
        return f"buffer {self.buffers[st.data_ptr()]} + {t.storage_offset()}"

    def enc(self, v, where=False, values=True):
        from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, float):
            return v.hex()
        if isinstance(v, torch.Tensor):
            out = str(v.dtype).replace("torch.", "") + str(list(v.shape)).replace(" ", "")
            if values:
                out += self.digest(tensor_digest(v))
            return out + (" " + self.buffer(v) if where else "")
        if isinstance(v, OccupancyGrid):
            return ["grid", self.grids.get(id(v), "unknown"), self.digest(tensor_digest(v.bits))]
        if isinstance(v, torch.nn.Module):
            return "model"
        if isinstance(v, torch.Generator):
            return "generator"
        if isinstance(v, C.Array):
            return self.digest(sha16(bytes(v)))
        if isinstance(v, C.Structure):
            return {name: ("ptr" if getattr(v, name) else "null") if issubclass(ftype, (C.c_void_p, C._Pointer)) else self.enc(getattr(v, name))
                    for name, ftype in v._fields_}
        if isinstance(v, dict):
            return {k: self.enc(x, where, values) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self.enc(x, where, values) for x in v]
        return type(v).__name__

    def call(self, name, fn, args, kw, where=False, returns="loss"):
        entry = {"call": name, "args": [self.enc(a, where) for a in args],
                 "kw": {k: self.enc(v, True, False) if k in OUT_BUFFERS else self.enc(v) for k, v in kw.items()}}
        self.calls.append(entry)
        out = fn(*args, **kw)
        if returns == "loss":
            entry["returned"] = self.digest(float(out).hex())
        elif returns == "buffer":
            entry["returned"] = self.enc(out, True, False)
        elif returns is not None:
            entry["returned"] = self.enc(out)
        return out

    def wrap(self, obj, label, method, **how):
        real = getattr(obj, method)
        setattr(obj, method, lambda *a, **k: self.call(f"{label}.{method}", real, a, k, **how))


def recording_step(log, model, **kw):
    from nerf_few_shot_limitations_amd.training import FusedStep

    class Recording(FusedStep):
        def __call__(self, *a, **k):
            return log.call("step", super().__call__, a, k)

        def step_view(self, *a, **k):
            return log.call("step.step_view", super().step_view, a, k)

        def step_view_hierarchical(self, *a, **k):
            return log.call("step.step_view_hierarchical", super().step_view_hierarchical, a, k)
    return Recording(model, **kw)


def record_schedule(log, sched, label, full="ones"):
    log.grids[id(sched.full)], log.grids[id(sched.grid)] = full, label
    log.wrap(sched, label, "current", returns="value")
    log.wrap(sched, label, "after_step", returns=None)


def golden():
    import numpy as np
    with np.load(os.path.join(ROOT, "tests", "golden", "trainer_loop.npz")) as z:
        return {k: z[k] for k in z.files}


def make_model(net, dino_grad=False):
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    if net == "v1":
        m, w = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=8, mma_mode="f32"), O.make_weights("v1", 0, "fog")
    elif net == "v2":
        m, w = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=False, mma_mode="f32"), O.make_weights("v2", 1, "fog")
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=8, use_dino=True, dino_dim=64, mma_mode="f32")
        w = O.make_weights("v3", 2, "fog")
    m.load_state_dict(w, strict=False)
    m.dino_grad = dino_grad
    return m.cuda().train()


def make_extractor(log, images):
    """tests/test_gpu_dino_grad.py's stand-in (a 2-layer random-init backbone with LoRA) on the views enlarged to 28 x 28 (2 x 2 patches)."""
    import warnings
    from nerf_few_shot_limitations_amd import dino_feature_model as F
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ext = F.SpatialDINOFeatures(None, use_lora=True, lora_rank=4, lora_alpha=8, image_size=28, pos_embed_dim=8, config=TINY).cuda()
    rgb = torch.stack(images)[..., :3].permute(0, 3, 1, 2)
    stack = torch.nn.functional.interpolate(rgb, size=(28, 28), mode="nearest").permute(0, 2, 3, 1).contiguous()
    tr = T.ExtractorTrainer(ext, stack, lr=2e-3, weight_decay=0.0)
    log.wrap(tr, "extractor", "begin_view", returns="value")
    log.wrap(tr, "extractor", "feats_grad_buffer", returns="buffer")
    log.wrap(tr, "extractor", "add_batch", where=True, returns=None)
    log.wrap(tr, "extractor", "end_view", returns=None)
    return tr


# name -> (net, train_epoch keywords, what else the case needs)
EPOCH_CASES = {
    "staged-v1": ("v1", {}, {}), "staged-v2": ("v2", {}, {}), "staged-v3": ("v3", {}, {}),
    "staged-v2-patches": ("v2", {}, dict(patches=True)),
    "staged-v3-extractor": ("v3", {}, dict(extractor=True)),
    "fused-v2": ("v2", dict(fused_inputs=True), {}), "fused-v3": ("v3", dict(fused_inputs=True), {}),
    "fused-v3-extractor-max-batches": ("v3", dict(fused_inputs=True, max_batches=3), dict(extractor=True)),
    "grid-v2": ("v2", {}, dict(grid="single")),
    "per-view-v3": ("v3", {}, dict(grid="per_view")), "per-view-v3-extractor": ("v3", {}, dict(grid="per_view", extractor=True)),
    "hier-v2-coarse-0": ("v2", dict(n_importance=4, coarse_weight=0.0), {}), "hier-v2-coarse-1": ("v2", dict(n_importance=4, coarse_weight=1.0), {}),
    "draws-v2": ("v2", {}, dict(draws=True)), "draws-v3-fused": ("v3", dict(fused_inputs=True), dict(draws=True)),
    "world-3-rank-0": ("v2", dict(rank=0, world=3), dict(ragged=True)), "world-3-rank-2": ("v2", dict(rank=2, world=3), dict(ragged=True)),
    "world-3-rank-2-fused": ("v2", dict(rank=2, world=3, fused_inputs=True), dict(ragged=True)),
    "raises-grid-v3": ("v3", {}, dict(grid="single")), "raises-per-view-v2": ("v2", {}, dict(grid="per_view")),
    "raises-hier-grid": ("v2", dict(n_importance=4), dict(grid="single")),
    "raises-hier-extractor": ("v3", dict(n_importance=4), dict(extractor=True)),
    "raises-patches-fused": ("v2", dict(fused_inputs=True), dict(patches=True)),
    "raises-patches-draws": ("v2", {}, dict(patches=True, draws=True)),
}
GRID = dict(warmup=1, refresh_every=2)


def epoch_case(name):
    """{'calls', 'digests', 'returned' | 'raised', 'state'} of one train_epoch."""
    from tests.test_trainer_loop_host import RecordedDraws, T as tensor
    net, kw, needs = EPOCH_CASES[name]
    kw = dict(kw)
    g = golden()
    cfg = json.loads(str(g["config_v3" if net == "v3" else "config_v2"]))
    epoch = 0
    if needs.get("ragged"):                               # 8x8 rays in batches of 21: the last holds one ray, a third of it none
        cfg["training"]["batch_size"], epoch = 21, 50
        cfg["training"]["progressive_schedule"]["epochs_50_100"] = [8, 8, 8]
    import numpy as np
    img = tensor(g["images"].astype(np.float32) / 255.0)
    images, poses, maps = [im.cuda() for im in img[:2]], list(tensor(g["poses"])), tensor(g["maps"]).cuda()
    H, W, focal = int(g["H"]), int(g["W"]), float(g["focal"])
    log = Log()
    torch.manual_seed(0)
    model = make_model(net, dino_grad=bool(needs.get("extractor")))
    step = recording_step(log, model, **T.step_options(cfg), **(dict(depth_smooth_weight=0.1, patch_size=2) if needs.get("patches") else {}))
    if needs.get("extractor"):
        kw["extractor"] = make_extractor(log, images)
    if needs.get("grid") == "single":
        kw["occupancy"] = T.OccupancySchedule(32, device=torch.device("cuda"), **GRID)
        record_schedule(log, kw["occupancy"], "grid")
    elif needs.get("grid") == "per_view":
        kw["occupancy"] = T.PerViewOccupancy(2, 32, device=torch.device("cuda"), **GRID)
        for v, s in enumerate(kw["occupancy"].views):
            record_schedule(log, s, f"grid {v}")
    if needs.get("patches"):
        kw["patches"] = dict(n=2, stride=2, generator=torch.Generator().manual_seed(5))
    if needs.get("draws"):
        kw["draws"] = RecordedDraws(g, 0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    out = {}
    try:
        mean, samples = T.train_epoch(step, cfg, epoch, images, poses, H, W, focal, NEAR, FAR, gen, dino_maps=maps if net == "v3" else None, **kw)
        out["returned"] = [float(mean).hex(), samples, type(mean).__name__, type(samples).__name__]
    except ValueError as e:
        out["raised"] = f"ValueError: {e}"
    except RuntimeError as e:
        if "shape" not in str(e):                         # (anything else ends the recording: nothing more runs behind a device error)
            raise
        out["raised"] = "RuntimeError"
    torch.cuda.synchronize()
    out["calls"], out["digests"] = log.calls, log.digests
    out["state"] = sha16(b"".join(tensor_digest(v).encode() for _, v in sorted(model.state_dict().items())))
    return json.loads(json.dumps(out))


MAIN_CASES = {
    "plain": ("v2", []), "fused-inputs": ("v2", ["--fused-inputs"]), "multiscale": ("v2", ["--recipe", "multiscale"]),
    "n-importance": ("v2", ["--n-importance", "4"]), "dist-entropy": ("v2", ["--dist-weight", "0.01", "--entropy-weight", "0.001"]),
    "depth-smooth": ("v2", ["--depth-smooth-weight", "0.1", "--patches-per-step", "2", "--patch-size", "2"]),
    "freq-reg": ("v2", ["--freq-reg-end", "4"]),
    "occupancy": ("v2", ["--occupancy-res", "32", "--occupancy-warmup", "1", "--occupancy-refresh-every", "2"]),
    "per-view-maps": ("v3", ["--occupancy-res", "32", "--occupancy-warmup", "1", "--occupancy-refresh-every", "2", "--occupancy-per-view"]),
    "resume": ("v2", ["resume"]),
}


def write_scene(root, g):
    """As tests/test_gpu_trainer_loop.py writes it."""
    from PIL import Image
    from oracle import nerf_oracle as O
    for split, imgs, poses in (("train", g["images"][:2], g["poses"]), ("test", g["images"][2:], g["test_poses"])):
        os.makedirs(os.path.join(root, split))
        frames = []
        for i, (im, pose) in enumerate(zip(imgs, poses)):
            Image.fromarray(im, "RGBA").save(os.path.join(root, split, f"r_{i}.png"))
            frames.append({"file_path": f"./{split}/r_{i}", "transform_matrix": pose.tolist()})
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump({"camera_angle_x": O.CAMERA_ANGLE_X, "frames": frames}, f)


def tensor_digests(v, path=""):
    if isinstance(v, torch.Tensor):
        return {path: tensor_digest(v)}
    out = {}
    if isinstance(v, dict):
        for k, x in v.items():
            out.update(tensor_digests(x, f"{path}/{k}"))
    elif isinstance(v, (list, tuple)):
        for k, x in enumerate(v):
            out.update(tensor_digests(x, f"{path}/{k}"))
    return out


def run_main(tmp, name, variant, flags_, g, checkpoint=None, epochs=2):
    import yaml
    from oracle import nerf_oracle as O
    from tests.test_trainer_loop_host import T as tensor
    root, out = os.path.join(tmp, "scene"), os.path.join(tmp, "run_" + name)
    if not os.path.exists(root):
        write_scene(root, g)
    cfg = json.loads(str(g[f"config_{variant}"]))
    cfg_path = os.path.join(tmp, f"cfg_{variant}.yaml")
    with open(cfg_path, "w") as f:
        f.write(yaml.safe_dump(cfg))
    if checkpoint is None:
        p = dict(O.make_weights("v2", 1, "fog") if variant == "v2" else O.make_weights("v3", 2, "fog"))
        pf = cfg["nerf_model"]["pos_freq"]
        p["pos_encoder.freq_bands"] = 2.0 ** torch.linspace(0., pf - 1, pf)
        p["dir_encoder.freq_bands"] = 2.0 ** torch.linspace(0., 3, 4)
        checkpoint = os.path.join(tmp, f"init_{variant}.pth")
        torch.save({"epoch": 0, "nerf_model_state_dict": p}, checkpoint)
    argv = ["--config", cfg_path, "--data", root, "--out", out, "--mode", "f32", "--max-batches", "3", "--epochs", str(epochs), "--checkpoint", checkpoint]
    if variant == "v3":
        torch.save(tensor(g["maps"]), os.path.join(tmp, "maps.pt"))
        argv += ["--dino-maps", os.path.join(tmp, "maps.pt")]
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        log = T.main(argv + flags_)
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    res = {"log": [{k: (v.hex() if isinstance(v, float) else v) for k, v in r.items()
                                                          if k not in ("seconds", "Msamples_per_s")} for r in log],
           "files": files, "checkpoint_keys": {}, "checkpoint_digests": {}}      # (one digest per checkpoint: of its tensors' paths and digests)
    for f in files:
        if f.endswith(".pth"):
            ck = torch.load(os.path.join(out, f), map_location="cpu", weights_only=True)
            res["checkpoint_keys"][f] = " ".join(sorted(ck))
            res["checkpoint_digests"][f] = sha16(json.dumps(tensor_digests(ck), sort_keys=True).encode())
    return json.loads(json.dumps(res)), out


def main_case(name, tmp=None):
    if tmp is None:
        with tempfile.TemporaryDirectory() as t:
            return main_case(name, t)
    variant, flags_ = MAIN_CASES[name]
    g = golden()
    if name != "resume":
        return run_main(tmp, name, variant, flags_, g)[0]
    _, out = run_main(tmp, "first", variant, [], g)
    best = [f for f in sorted(os.listdir(out)) if f.startswith("best_")]
    return run_main(tmp, name, variant, [], g, checkpoint=os.path.join(out, best[0]), epochs=3)[0]


def transcript():
    out = {"epoch": {}, "main": {}}
    for name in EPOCH_CASES:
        for k, v in epoch_case(name).items():
            out["epoch"][f"{name}/{k}"] = v
        print(name, flush=True)
    for name in MAIN_CASES:
        for k, v in main_case(name).items():
            out["main"][f"{name}/{k}"] = v
        print("main", name, flush=True)
    return out


# ---- files -------------------------------------------------------------------------------------------------------------------------
def agree(a, b, path, dropped):
    """a where b agrees with it, null where it does not."""
    if isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b):
        return {k: agree(a[k], b[k], f"{path}/{k}", dropped) for k in a}
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [agree(x, y, f"{path}[{i}]", dropped) for i, (x, y) in enumerate(zip(a, b))]
    if a == b or (a != a and b != b):
        return a
    dropped.append(path)
    return None


def matches(got, want, path=""):
    """The first difference between a fresh recording and the file (None: none); nulls of the file are not compared."""
    if want is None:
        return None
    if isinstance(want, dict) and isinstance(got, dict):
        if sorted(got) != sorted(want):
            return f"{path}: keys {sorted(got)} != {sorted(want)}"
        return next((m for m in (matches(got[k], want[k], f"{path}/{k}") for k in want) if m), None)
    if isinstance(want, list) and isinstance(got, list):
        if len(got) != len(want):
            return f"{path}: {len(got)} entries != {len(want)}"
        return next((m for m in (matches(x, y, f"{path}[{i}]") for i, (x, y) in enumerate(zip(got, want))) if m), None)
    if got == want or (got != got and want != want):
        return None
    return f"{path}: {got!r} != {want!r}"


def dump(rec, path):
    """One field per line; a list of calls or of table rows one entry per line."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, (section, fields) in enumerate(rec.items()):
            f.write(f" {json.dumps(section)}: ")
            if not isinstance(fields, dict):
                f.write(json.dumps(fields))
            else:
                f.write("{\n")
                for j, (name, value) in enumerate(fields.items()):
                    if isinstance(value, list) and (name.endswith("/calls") or section == "tables"):
                        body = "[\n" + ",\n".join("   " + json.dumps(v) for v in value) + "\n  ]"
                    else:
                        body = json.dumps(value)
                    f.write(f"  {json.dumps(name)}: {body}" + (",\n" if j + 1 < len(fields) else "\n"))
                f.write(" }")
            f.write(",\n" if i + 1 < len(rec) else "\n")
        f.write("}\n")


def main(argv):
    if argv[:1] == ["flags"] and len(argv) == 2:
        dump(flags(), argv[1])
        return 0
    if argv[:1] == ["transcript"] and len(argv) == 2:
        dump(transcript(), argv[1])
        return 0
    if argv[:1] == ["merge"] and len(argv) == 4:
        with open(argv[1]) as f:
            a = json.load(f)
        with open(argv[2]) as f:
            b = json.load(f)
        dropped = []
        out = agree(a, b, "", dropped)
        out["dropped"] = dropped
        dump(out, argv[3])
        print(len(dropped), "dropped:", *dropped[:40], sep="\n ")
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
