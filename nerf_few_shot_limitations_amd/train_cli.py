"""python -m nerf_few_shot_limitations_amd.train_cli --config experiments/baseline.yaml --data data/nerf_synthetic/lego \\
        [--n-importance N [--coarse-weight W]] [--freq-reg-end N [--no-freq-reg-dirs]] [--dist-weight W] [--occ-weight W --occ-samples K] [--recipe train|multiscale] [--epochs N] [--mode bf16|f16|f32] [--eval-mode f16] [--out DIR] [--checkpoint CKPT]
        [--dino-weights DIR | --dino-maps maps.pt] [--train-extractor] [--fused-inputs] [--seed 0]
        [--occupancy-res N [--occupancy-box LO HI] [--occupancy-threshold T] [--occupancy-decay D] [--occupancy-refresh-every K]
         [--occupancy-cells-per-refresh C] [--occupancy-warmup STEPS] [--occupancy-per-view]]

The training run of `NeRFDINOTrainer` (src/training/train.py:244-292 `train_step`, :344-372 `train`) as a command on the
HIP path: the YAML loads unchanged; per epoch and training view the rays are cast at the progressive schedule's
resolution (focal scaled, target resized bilinearly: train.py:262-266), shuffled (:268) and consumed in ray batches
(:270-288), each of them one `training.FusedStep` -- stratified samples -> NeRFMLP -> VolumeRenderer ->
rgb_weight * mse -> backward -> Adam(lr, weight_decay) -- with MultiStepLR between epochs (:119-123), validation every
`output.val_freq` epochs on the fused renderer (`evaluate_views`) and checkpoints under the reference's key names
(:374-389, readable by evaluate.py:22-33 and by evaluate_cli).

Objective.  --recipe train (the default) minimises `loss.rgb_weight * mse(rgb, target)` with Adam -- exactly what train.py
does: train.py:27-44 (the `NeRFLoss` class train.py defines and uses) computes only that term; `loss.depth_weight` /
`loss.reg_weight` of the YAMLs are read into the constructor and never used there.
--recipe multiscale is the step of the reference's other trainer, src/training/train_multiscale.py:207-211,249-266 (the one
behind experiments/multiscale.yaml), still one `FusedStep`: density noise `rendering.noise_std` in front of the compositor's
ReLU, nerf_mlp.NeRFLoss = rgb_weight * mse + `loss.reg_weight` * mean(weights^2) (`loss.depth_weight` is read and inert, as
there: its targets carry no depth), clip_grad_norm_(max_norm=1.0) and optim.AdamW(lr, weight_decay); its checkpoints carry
`nerf_state_dict` (train_multiscale.py:368-376) next to `nerf_model_state_dict`.  The ray batches, schedule, validation and
LR steps stay this command's (the two trainers agree on them); the DINO-feature mean substitution of
train_multiscale.py:190-197 (its mask is always false) is not part of it, and by default the extractor receives no gradient in
either recipe.

use_dino configs condition on the DINOv2 feature map of every training view.  As in train.py:158-169 the maps are computed ONCE,
under no_grad, by the extractor the config names (config.dino_model_from_config: SpatialDINOFeatures or
MultiScaleDINOFeatures with LoRA wrappers) -- from --dino-weights (a local transformers Dinov2Model checkpoint; the weights are
not available offline) or, to exercise the pipeline without them, --dino-random-init; --dino-maps takes precomputed maps
(V,Hp,Wp,C) instead.  The features of a sample are fetched by projection into the view being trained on (:203-214).  Because the
maps are constants, no gradient reaches the extractor -- in the reference too: its LoRA matrices sit in the optimizer
(train.py:105-110) but never receive one.

--train-extractor is the intent behind those LoRA matrices, restated (the reference never re-runs its extractor, so there is
no loop to copy).  Trainable set as train.py:105-110: extractor parameters with `lora` in their name, everything else frozen, in a
torch.optim.Adam(lr, weight_decay) of the config that follows the same lr_at(epoch).  Per epoch and view the extractor runs
on that view under grad (train mode, train.py:246-247); the view's ray batches use the detached map as before, every FusedStep
also writes dL/d features (`d_dino_out`), which nrf_project_fetch_backward adds into one per-view d_map; after the view's last
batch -- also when --max-batches ends the epoch inside the view -- `map.backward(d_map)` and one extractor step.  The NeRF
parameters step per batch as before.  Validation recomputes view 0's map under no_grad first; checkpoints add
`dino_model_state_dict` (train.py:384) and --checkpoint restores it.  Needs --dino-weights or --dino-random-init; refused
with --dino-maps (nothing to train), with --data-parallel (the per-view d_map would need one more all-reduce: not built) and
for `dino_model_type: multi_scale`: MultiScaleDINOFeatures runs its backbone under no_grad (multi_scale_dino.py:87, kept), so
its LoRA matrices would still receive nothing -- refused rather than silently training nothing.

--fused-inputs: every ray batch is one `FusedStep.step_view` -- the batch's pixel ids go to the saving forward kernel, which casts
the rays, draws the stratified depths (same seed, same key), encodes and, for use_dino, gathers the features itself; no per-sample
input tensor is built.  Same shuffle, seeds and sharding as the default route, which stays the default.

--occupancy-res N (0, the default: off) trains under an occupancy grid of N^3 cells over the cube --occupancy-box LO HI (default
-1.5 1.5): every ray batch is one `FusedStep.step_view(occupancy=grid)` -- the pixel ids go to the compaction kernels, the network,
its backward and the weight gradients run on the samples in occupied cells alone, a sample in an empty cell composites as empty
space (include/nerfhip.h: nrf_occupancy_compact_rays).  The grid follows the field: every --occupancy-refresh-every steps (default
16) `OccupancyGrid.refresh` probes the network's density in the next --occupancy-cells-per-refresh cells (a multiple of 32; default:
a sixteenth of the grid), keeps max(--occupancy-decay * old, probe) per cell (default 0.95) and marks a cell occupied when that
exceeds --occupancy-threshold (default 0.01).  Until step --occupancy-warmup (default 256) the steps run under an all-ones grid --
the same launches, every sample evaluated -- while the refreshes already collect the cells' values.  Unlike the other routes such
a step reads 8 bytes back from the device.  Refused: a use_dino config (a V3 grid belongs to ONE source view, the batches of a run
condition on the view they came from), --train-extractor (no per-sample gradients are handed out under a grid), and any
--occupancy-* flag without --occupancy-res.  The grid is not part of a checkpoint: a resumed run starts again from the all-ones
grid and its warm-up.

--occupancy-per-view (with --occupancy-res, use_dino configs only) lifts the first two refusals: the trainer keeps ONE grid per
training view (`PerViewOccupancy`: an OccupancySchedule each -- bits, per-cell values, refresh cursor and count, and a step counter
with its own warm-up, counted in batches of that view).  A batch of view v is one `FusedStep.step_view(occupancy=grid v,
grid_inputs="rays")` -- the compaction, then the ray-input saving forward on the kept rows (nrf_mlp_forward_train_rays_indexed), which
gathers view v's map itself -- and after the step grid v is refreshed with `dino=` that view's current map.  With --train-extractor the
batches also take `d_dino_out` / `points_out` under the grid: their first `last_count` rows are the kept samples, which is what
`ExtractorTrainer.add_batch` receives (nothing when no sample was kept).  Refused for use_dino: false (a V1 or V2 field does not
depend on the view: the single grid serves) and without --occupancy-res.  UNLIKE the single grid, the per-view grids ARE part of a
checkpoint (`occupancy_per_view_state`) and --checkpoint restores them, warm-up counters included.  --data-parallel works as with the
single grid: every rank refreshes from the same parameters and seeds, so the grids agree; with --train-extractor it stays refused.

--n-importance N (0, the default: off, today's run) trains coarse-to-fine on the one network: every ray batch is one
`FusedStep.step_view_hierarchical` -- the S ladder samples, Ni = N depths resampled from their weights, and the loss
`rgb_weight * (W * mse(coarse image, target) + mse(fine image, target))` with W = --coarse-weight (default 1.0; 0: the coarse rows
learn through the fine image alone).  Every sample is evaluated once forward and backward; no gradient reaches the resampled
depths.  It implies the --fused-inputs route (pixel ids in, no per-sample input tensor), and validation renders hierarchically too:
`evaluate_views(N_importance=N)`.  Refused before the data set is read: --recipe multiscale (its regulariser, depth term and density
noise are not part of the hierarchical step), any --occupancy-* flag, --train-extractor (no per-sample gradients are handed out), N < 0,
W < 0, and --coarse-weight without --n-importance.

--dist-weight W / --occ-weight W --occ-samples K (0, the default: off) add the two few-shot ray regularisers to the step's loss
(`FusedStep(dist_weight=, occ_weight=, occ_samples=)`; nerfhip.h: nrf_ray_reg): W * the distortion loss of mip-NeRF 360 -- sum_ij
w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i on the weights and the interval midpoints scaled by 1 / (far - near), against
floaters -- and W * the occlusion penalty of FreeNeRF -- the mean rectified density of every ray's first K samples, against a wall
of density in front of the cameras.  Both work with either recipe, with --fused-inputs and with --occupancy-*; the step is then
the multi-term one (clipped optimiser entry) with one small launch more.  Refused before the data set is read: a negative weight,
--occ-weight > 0 without --occ-samples K >= 1, --occ-samples without --occ-weight, and either weight together with --n-importance
(the hierarchical step takes the plain rgb loss).

--depth-smooth-weight W (0, the default: off) adds RegNeRF's depth-smoothness loss on patches of unseen views
(`FusedStep(depth_smooth_weight=W, patch_size=P)`; nerfhip.h: nrf_patch_reg): every batch of the default (staged) route gets
--patches-per-step N (default 16) patches of --patch-size P x P rays (default 8; 2 ... 16) behind its supervised rays, one patch per
freshly drawn pose (`ray_sampler.sample_patch_poses`: positions in the bounding box of the training cameras at their mean radius,
looking at the jittered origin) at the epoch's schedule resolution, neighbouring patch pixels --patch-stride K (default 1) image
pixels apart.  The term is W * the mean over patches and anchors of the squared differences between a patch ray's rendered depth
and those of its right and lower neighbours; patch rays have no colour term and take the other target-free terms like any ray.
One launch sequence as with --dist-weight: the patch rays' depths meet in LDS inside the loss launch.  It goes with both recipes,
--dist-weight / --occ-weight, --freq-reg-end and --data-parallel (every rank draws its own patches).  Refused before the config or
the data set is read: --depth-smooth-weight together with --n-importance, --fused-inputs (a view step has one pose), any
--occupancy-* flag or --train-extractor; a negative weight, P outside 2 ... 16, N < 1, K < 1.

--entropy-weight W (0, the default: off) adds InfoNeRF's ray-entropy loss (`FusedStep(ent_weight=W, ent_threshold=T)`; nerfhip.h:
nrf_info_reg): W * the mean over every ray of the batch of the entropy of the ray's per-sample distribution p_i = a_i / sum a, rays
whose sum a is at most --entropy-threshold T (default 0.01) left out.  It goes wherever --dist-weight goes (the staged route,
--fused-inputs, the occupancy routes) and is refused with --n-importance.  --entropy-unseen also draws patches of unseen poses behind
every batch (--patches-per-step / --patch-size / --patch-stride, as --depth-smooth-weight does), so that the entropy acts on rays
nobody observed; it has --depth-smooth-weight's refusals.  --kl-weight W (0: off) adds InfoNeRF's information-gain loss
(`FusedStep(kl_weight=W, patch_size=P)`): W * the mean over patches and anchors of KL(p_anchor || p_right) + KL(p_anchor || p_below) on
the same patches, neighbouring rays --patch-stride K pixels apart; it draws the patches itself and has --depth-smooth-weight's
refusals: --n-importance, --fused-inputs, any --occupancy-* flag, --train-extractor, and P^2 * n_samples above 12288 (the patch's
distributions meet in LDS).  All of this is decided before the config or the data set is read, except the last, which the step
object refuses.  The launch count is --depth-smooth-weight's.

--freq-reg-end N (0, the default: off) is FreeNeRF's frequency regularisation (`FusedStep(freq_reg_end=N)`; nerfhip.h:
nrf_model_set_freq_mask): step t trains and validates the field whose positional encodings show min(L, 1 + L t / N) bands (the
direction encoding too, unless --no-freq-reg-dirs).  The mask is a column scale of the Linears that read the encodings, applied
in the re-pack and in the weight gradients: no launch more, and it goes with every recipe, route and the other flags.  Hidden
columns receive gradient exactly 0 (under weight decay they still decay).  From step N (L - 1) / L on the run is the plain one.
Checkpoints hold the raw weights and the active mask (`freq_mask_pos`, `freq_mask_dirs`); --checkpoint and evaluate_cli apply it.

--checkpoint resumes a run: weights, Adam moments and step count, epoch counter and best PSNR (the reference's train.py saves
these keys, :374-389, but has no resume path); the LR schedule is a function of the epoch.  wandb and LPIPS are not part of
this command.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import json
import math
import os
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib as L
from . import (dino_model_from_config, evaluate_views, get_rays, load_blender_data, load_checkpoint_into, load_config, model_from_config,
               precompute_dino_features, render_settings, sample_points_along_rays)
from .ray_sampler import _c2w12, patch_rays, sample_patch_poses
from .renderer import make_dino
from .training import FusedStep, project_fetch_backward


def schedule_for(cfg, epoch):
    """(H_train, W_train, N_samples, batch_size) of an epoch: train.py:249-259."""
    t = cfg["training"]
    s = t["progressive_schedule"]
    if epoch < 50:
        return (*s["epochs_0_50"], t["batch_size"] * 2)
    if epoch < 100:
        return (*s["epochs_50_100"], t["batch_size"])
    return (*s["epochs_100_plus"], t["batch_size"] // 2)


def lr_at(cfg, epoch):
    """MultiStepLR(milestones, gamma) evaluated for the epoch about to run (train.py:119-123, scheduler.step() after each epoch)."""
    o = cfg["optimizer"]
    return float(o["lr"]) * float(o["lr_gamma"]) ** sum(1 for m in o["lr_milestones"] if epoch >= m)


def view_target(image, H, W, focal, Ht, Wt):
    """Target (Ht*Wt,3) of one training view at the schedule's resolution and the focal length of its rays (train.py:262-266)."""
    tgt = image
    if tgt.shape[-1] == 4:
        tgt = tgt[..., :3] * tgt[..., 3:4] + (1.0 - tgt[..., 3:4])
    if (Ht, Wt) == (H, W):
        return tgt.reshape(-1, 3).contiguous(), focal
    tgt = F.interpolate(tgt.permute(2, 0, 1).unsqueeze(0), size=(Ht, Wt), mode="bilinear", align_corners=False).squeeze(0).permute(1, 2, 0)
    return tgt.reshape(-1, 3).contiguous(), focal * (Ht / H)


def view_rays(image, pose, H, W, focal, Ht, Wt):
    """Rays and target of one training view at the schedule's resolution (train.py:174-186,262-266)."""
    tgt, f = view_target(image, H, W, focal, Ht, Wt)
    ro, rd = get_rays(Ht, Wt, f, pose)
    return ro.reshape(-1, 3), rd.reshape(-1, 3), tgt


def fetch_features(dino_struct, pts):
    """(n,3) points -> (n,C) features of the source view (project_points_to_image + sample_features_at_points)."""
    d, fm = dino_struct
    n = pts.shape[0]
    feats = torch.empty((n, int(fm.shape[-1])), dtype=torch.float32, device=pts.device)
    L.check(L.lib().nrf_project_fetch(C.byref(d), L.ptr(pts), n, L.ptr(feats), None, L.stream_ptr()))
    return feats


# ---- the flags, read once -------------------------------------------------------------------------------------------------------
OCCUPANCY_FLAGS = ("occupancy_box", "occupancy_threshold", "occupancy_decay", "occupancy_refresh_every", "occupancy_cells_per_refresh",
                   "occupancy_warmup")
# the flags the checks and the option readers look at, with what an absent (or None) one counts as (the type is the default's), and
# those that stay None unless given, with their type
_DEFAULTS = dict(n_importance=0, recipe="train", dist_weight=0.0, occ_weight=0.0, depth_smooth_weight=0.0, patch_size=8, patches_per_step=16,
                 patch_stride=1, entropy_weight=0.0, entropy_unseen=False, kl_weight=0.0, freq_reg_end=0, no_freq_reg_dirs=False,
                 occupancy_res=0, occupancy_per_view=False, train_extractor=False, fused_inputs=False)
_OPTIONAL = dict(coarse_weight=float, occ_samples=int, entropy_threshold=float)


class Flags(SimpleNamespace):
    """What flags_of returns."""


def flags_of(args):
    """The one reading of an argparse namespace, partial or complete (a Flags passes through): every flag of _DEFAULTS and _OPTIONAL
    with its default applied and its type fixed; every other attribute as it is -- one the namespace lacks is missing here too, so the
    checks that read such fields read them one at a time, in the order they always did, and raise where they did; and the facts several checks ask for -- grid_flags (the OCCUPANCY_FLAGS that were given), grid_given (any --occupancy-*
    flag was), draws_patches (every batch gets patches of unseen poses behind its supervised rays: --depth-smooth-weight, --kl-weight,
    or --entropy-weight with --entropy-unseen) and hierarchical (--n-importance > 0)."""
    if isinstance(args, Flags):
        return args
    f = Flags(**vars(args))
    for name, default in {**_DEFAULTS, **dict.fromkeys(_OPTIONAL)}.items():
        v = getattr(args, name, None)
        setattr(f, name, default if v is None else _OPTIONAL.get(name, type(default))(v))
    f.grid_flags = [name for name in OCCUPANCY_FLAGS if vars(f).get(name) is not None]
    f.grid_given = bool(f.occupancy_res or f.occupancy_per_view or f.grid_flags)
    f.draws_patches = f.depth_smooth_weight > 0.0 or f.kl_weight > 0.0 or (f.entropy_weight > 0.0 and f.entropy_unseen)
    f.hierarchical = f.n_importance > 0
    return f


def _refusal(*checks):
    """The message of the first (fault, message) whose fault is there; None when none is.  Every fault is evaluated before the first is
    picked, so a fault here reads only fields that flags_of always sets: one that can raise is an `if` of its own, in its place."""
    return next((message for fault, message in checks if fault), None)


def _finite(*weights):
    return all(w >= 0.0 and math.isfinite(w) for w in weights)


def extractor_args_error(args, cfg):
    """Why --train-extractor cannot run with these arguments / this config (None: it can).  Decided before any GPU work."""
    f = flags_of(args)
    if not f.train_extractor:
        return None
    model_cfg = cfg.get("model", {}) or {}
    if not bool(model_cfg.get("use_dino", True)):
        return "--train-extractor: this config has use_dino: false, there is no extractor"
    if f.dino_maps:                                       # (fields without a default, read one at a time: not for _refusal)
        return "--train-extractor needs the extractor itself (--dino-weights or --dino-random-init): --dino-maps are constants"
    if not (f.dino_weights or f.dino_random_init):
        return "--train-extractor needs --dino-weights <local Dinov2Model checkpoint> or --dino-random-init"
    if f.data_parallel:
        return "--train-extractor with --data-parallel is not built (the per-view map gradient would need its own all-reduce)"
    return _refusal(
        (model_cfg.get("dino_model_type", "single_scale") == "multi_scale",
         "--train-extractor: MultiScaleDINOFeatures runs its backbone under no_grad (multi_scale_dino.py:87), its LoRA matrices would receive no gradient"),
        (not bool((cfg.get("dino_model", {}) or {}).get("use_lora", True)),
         "--train-extractor: dino_model.use_lora is false, the trainable set of train.py:105-110 is empty"))


def hierarchical_args_error(args, cfg=None):
    """Why --n-importance / --coarse-weight cannot run with these arguments (None: they can, or neither was given).  Decided before
    any GPU work, in the style of occupancy_args_error."""
    f = flags_of(args)
    n, w = f.n_importance, f.coarse_weight
    return _refusal(
        (n < 0, "--n-importance must be >= 0 (0: off)"),
        (w is not None and not w >= 0.0, "--coarse-weight must be >= 0"),
        (n == 0 and w is not None, "--coarse-weight needs --n-importance N (N > 0): without the hierarchical step the flag would be ignored"),
        (n > 0 and f.recipe == "multiscale", "--n-importance with --recipe multiscale is refused: the regulariser, the depth term and the density "
                                             "noise are not part of the hierarchical step"),
        (n > 0 and f.grid_given, "--n-importance is not combined with --occupancy-*: the hierarchical step runs under no grid"),
        (n > 0 and f.train_extractor, "--n-importance with --train-extractor is refused: the hierarchical step hands out no per-sample gradients"))


def ray_reg_args_error(args):
    """Why --dist-weight / --occ-weight / --occ-samples cannot run with these arguments (None: they can, or none was given).  Decided
    before any GPU work, like hierarchical_args_error."""
    f = flags_of(args)
    dw, ow, k = f.dist_weight, f.occ_weight, f.occ_samples
    return _refusal(
        (not _finite(dw, ow), "--dist-weight and --occ-weight must be finite and >= 0 (0: off)"),
        (ow > 0.0 and (k is None or k < 1),
         "--occ-weight needs --occ-samples K (K >= 1): the number of samples at the front of every ray the penalty covers"),
        (ow == 0.0 and k is not None, "--occ-samples needs --occ-weight W (W > 0): without the occlusion term the flag would be ignored"),
        ((dw > 0.0 or ow > 0.0) and f.hierarchical,
         "--dist-weight / --occ-weight with --n-importance is refused: the hierarchical step takes the plain rgb loss"))


def ray_reg_options(args, near, far):
    """FusedStep's keywords of --dist-weight / --occ-weight / --occ-samples ({} when both are off); dist_span = far - near, so that the
    per-sample route (`step(points, z_vals, ...)`, which has no near / far) scales the midpoints as the ray routes do."""
    f = flags_of(args)
    if f.dist_weight == 0.0 and f.occ_weight == 0.0:
        return {}
    return dict(dist_weight=f.dist_weight, occ_weight=f.occ_weight, occ_samples=f.occ_samples or 0, dist_span=float(far) - float(near))


def patch_reg_args_error(args):
    """Why --depth-smooth-weight and its companions cannot run with these arguments (None: they can, or the weight is 0).  Decided
    before a config or a data set is read, like ray_reg_args_error."""
    f = flags_of(args)
    if not _finite(f.depth_smooth_weight):
        return "--depth-smooth-weight must be finite and >= 0 (0: off)"
    return patch_draw_error(f, "--depth-smooth-weight") if f.depth_smooth_weight > 0.0 else None


def patch_draw_error(args, flag):
    """Why the trainer cannot draw patches for `flag` (--depth-smooth-weight, --kl-weight, --entropy-unseen) with these arguments."""
    f = flags_of(args)
    return _refusal(
        (not 2 <= f.patch_size <= 16, "--patch-size must be in 2 ... 16"),
        (f.patches_per_step < 1, "--patches-per-step must be >= 1"),
        (f.patch_stride < 1, "--patch-stride must be >= 1"),
        (f.hierarchical, f"{flag} with --n-importance is refused: the hierarchical step takes the plain rgb loss"),
        (f.fused_inputs, f"{flag} with --fused-inputs is refused: a view step has one pose, the patches come from poses of their own"),
        (f.grid_given, f"{flag} is not combined with --occupancy-*: the trainer's grid route steps view by view"),
        (f.train_extractor, f"{flag} with --train-extractor is refused: the patch rays belong to no view whose map could take their gradient"))


def info_reg_args_error(args):
    """Why --entropy-weight / --entropy-threshold / --entropy-unseen / --kl-weight cannot run with these arguments (None: they can, or
    none was given).  Decided before a config or a data set is read: the entropy flag has --dist-weight's refusals, the KL flag and
    --entropy-unseen, which draw patches, --depth-smooth-weight's."""
    f = flags_of(args)
    ew, kw, th, unseen = f.entropy_weight, f.kl_weight, f.entropy_threshold, f.entropy_unseen
    problem = _refusal(
        (not _finite(ew, kw), "--entropy-weight and --kl-weight must be finite and >= 0 (0: off)"),
        (th is not None and not _finite(th), "--entropy-threshold must be finite and >= 0"),
        (th is not None and ew == 0.0 and kw == 0.0,
         "--entropy-threshold needs --entropy-weight or --kl-weight: without either term the flag would be ignored"),
        (unseen and ew == 0.0, "--entropy-unseen needs --entropy-weight W (W > 0): it draws patches of unseen poses for the entropy term"),
        (ew > 0.0 and f.hierarchical, "--entropy-weight with --n-importance is refused: the hierarchical step takes the plain rgb loss"))
    if problem or not (kw > 0.0 or unseen):
        return problem
    return patch_draw_error(f, "--kl-weight" if kw > 0.0 else "--entropy-unseen")


def info_reg_options(args):
    """FusedStep's keywords of --entropy-weight / --entropy-threshold / --kl-weight ({} when both weights are 0); patch_size with them
    when the step draws patches for these terms alone (--depth-smooth-weight hands it over itself)."""
    f = flags_of(args)
    if f.entropy_weight == 0.0 and f.kl_weight == 0.0:
        return {}
    out = dict(ent_weight=f.entropy_weight, ent_threshold=0.01 if f.entropy_threshold is None else f.entropy_threshold, kl_weight=f.kl_weight)
    if f.draws_patches and not f.depth_smooth_weight > 0.0:
        out["patch_size"] = f.patch_size
    return out


def draws_patches(args):
    """Whether every batch gets patches of unseen poses behind its supervised rays: --depth-smooth-weight, --kl-weight, or
    --entropy-weight with --entropy-unseen."""
    return flags_of(args).draws_patches


def patch_reg_options(args):
    """FusedStep's keywords of --depth-smooth-weight / --patch-size ({} when off)."""
    f = flags_of(args)
    return dict(depth_smooth_weight=f.depth_smooth_weight, patch_size=f.patch_size) if f.depth_smooth_weight > 0.0 else {}


def freq_reg_args_error(args):
    """Why --freq-reg-end / --no-freq-reg-dirs cannot run with these arguments (None: they can, or neither was given).  The mask
    goes with every recipe and route: it lives in the re-pack and the weight gradients, which all of them share."""
    f = flags_of(args)
    return _refusal(
        (f.freq_reg_end < 0, "--freq-reg-end must be >= 0 (0: off)"),
        (f.freq_reg_end == 0 and f.no_freq_reg_dirs,
         "--no-freq-reg-dirs needs --freq-reg-end N (N > 0): without the frequency mask the flag would be ignored"))


def freq_reg_options(args):
    """FusedStep's keywords of --freq-reg-end / --no-freq-reg-dirs ({} when off)."""
    f = flags_of(args)
    return dict(freq_reg_end=f.freq_reg_end, freq_reg_dirs=not f.no_freq_reg_dirs) if f.freq_reg_end > 0 else {}


def occupancy_args_error(args, cfg):
    """Why the --occupancy-* arguments cannot run with these arguments / this config (None: they can, or none was given).
    Decided before any GPU work.  The values of the OCCUPANCY_FLAGS are read last, once a grid is known to be asked for and allowed."""
    f = flags_of(args)
    res, per_view = f.occupancy_res, f.occupancy_per_view
    use_dino = bool((cfg.get("model", {}) or {}).get("use_dino", True))
    problem = _refusal(
        (per_view and res == 0, "--occupancy-per-view needs --occupancy-res N (N > 0): without a grid the flag would be ignored"),
        (per_view and not use_dino, "--occupancy-per-view: this config has use_dino: false -- such a field does not depend on the view, the "
                                    "single grid of --occupancy-res serves every batch"),
        (res == 0 and f.grid_flags, "--" + "".join(f.grid_flags[:1]).replace("_", "-") + " needs --occupancy-res N (N > 0): without a grid "
                                    "the flag would be ignored"),
        (res != 0 and (res < 32 or res > 512 or res % 32), "--occupancy-res must be a multiple of 32 in 32..512 (0: off)"),
        (res != 0 and use_dino and not per_view, "--occupancy-res: this config has use_dino: true -- a grid of such a field belongs to ONE source "
                                                 "view, the batches of a run condition on the view they came from"),
        (res != 0 and f.train_extractor and not per_view,
         "--occupancy-res with --train-extractor is refused: a step under a grid hands out no per-sample gradients"))
    if problem or res == 0:
        return problem
    if f.occupancy_box is not None and not (f.occupancy_box[0] < f.occupancy_box[1]):      # (fields without a default, read one at a time: not for _refusal)
        return "--occupancy-box LO HI needs LO < HI"
    if f.occupancy_decay is not None and not (0.0 <= f.occupancy_decay <= 1.0):
        return "--occupancy-decay must be in [0, 1]"
    if f.occupancy_refresh_every is not None and f.occupancy_refresh_every < 1:
        return "--occupancy-refresh-every must be >= 1"
    c = f.occupancy_cells_per_refresh
    if c is not None and (c < 32 or c % 32):
        return "--occupancy-cells-per-refresh must be a positive multiple of 32"
    return "--occupancy-warmup must be >= 0" if f.occupancy_warmup is not None and f.occupancy_warmup < 0 else None


# main's refusals, in the order they are reported: those of the flags alone, decided before the config is read, then those that read it
FLAG_CHECKS = (hierarchical_args_error, ray_reg_args_error, patch_reg_args_error, info_reg_args_error, freq_reg_args_error)
CONFIG_CHECKS = (extractor_args_error, occupancy_args_error)


def _grid_keywords(f):
    """OccupancySchedule's keywords of the --occupancy-* flags that were given (the others keep its defaults)."""
    kw = dict(box=f.occupancy_box, threshold=f.occupancy_threshold, decay=f.occupancy_decay, refresh_every=f.occupancy_refresh_every,
              cells_per_refresh=f.occupancy_cells_per_refresh, warmup=f.occupancy_warmup)
    return {k: v for k, v in kw.items() if v is not None}


class OccupancySchedule:
    """The grid side of --occupancy-res: the all-ones grid of the warm-up, the live grid `OccupancyGrid.refresh` keeps up to date, and
    the step counter that decides between them and when to refresh."""

    def __init__(self, res, box=(-1.5, 1.5), threshold=0.01, decay=0.95, refresh_every=16, cells_per_refresh=None, warmup=256, device=None,
                 full=None):
        from .occupancy import OccupancyGrid
        self.full = full if full is not None else OccupancyGrid.full(res, box[0], box[1], device=device)      # (never written: may be shared)
        self.grid = OccupancyGrid.full(res, box[0], box[1], device=device)
        self.threshold, self.decay, self.refresh_every, self.warmup = float(threshold), float(decay), int(refresh_every), int(warmup)
        self.cells = int(cells_per_refresh) if cells_per_refresh else max(32, self.grid.n_cells // 16 // 32 * 32)
        self.steps = 0

    @classmethod
    def from_args(cls, args, device):
        f = flags_of(args)
        return cls(f.occupancy_res, device=device, **_grid_keywords(f))

    def current(self):
        """The grid of the next step: all ones until the warm-up is over."""
        return self.full if self.steps < self.warmup else self.grid

    def after_step(self, model, dino=None):
        """dino: the source view of a use_dino model's grid (OccupancyGrid.refresh)."""
        self.steps += 1
        if self.steps % self.refresh_every == 0:
            self.grid.refresh(model, decay=self.decay, threshold=self.threshold, cells=self.cells, dino=dino)

    def state_dict(self):
        """What a resumed run needs of the live grid: its bits, the per-cell values (None before the first refresh), the round-robin
        cursor, the refresh count (the seed of the next probe points) and the step counter of the warm-up."""
        g = self.grid
        ema = getattr(g, "ema", None)
        return {"bits": g.bits.detach().cpu().clone(), "ema": None if ema is None else ema.detach().cpu().clone(),
                "cursor": int(getattr(g, "_cursor", 0)), "refreshes": int(getattr(g, "_refreshes", 0)), "steps": int(self.steps)}

    def load_state_dict(self, sd):
        g = self.grid
        if sd["bits"].dtype != torch.int32 or sd["bits"].numel() != g.bits.numel():
            raise ValueError("occupancy state: the checkpoint's grid has another resolution")
        g.bits.copy_(sd["bits"].to(g.bits.device))
        if sd["ema"] is None:
            g.ema = None
        else:
            g.ema = sd["ema"].to(device=g.bits.device, dtype=torch.float32).clone()
        g._cursor, g._refreshes = int(sd["cursor"]), int(sd["refreshes"])
        self.steps = int(sd["steps"])


class PerViewOccupancy:
    """The grid side of --occupancy-per-view: one OccupancySchedule per training view -- the grid of a use_dino field belongs to the
    source view it is conditioned on -- sharing one all-ones grid for their warm-ups."""

    def __init__(self, n_views, res, device=None, **kw):
        self.views = []
        for _ in range(int(n_views)):
            self.views.append(OccupancySchedule(res, device=device, full=self.views[0].full if self.views else None, **kw))

    @classmethod
    def from_args(cls, args, n_views, device):
        f = flags_of(args)
        return cls(n_views, f.occupancy_res, device=device, **_grid_keywords(f))

    def view(self, v):
        return self.views[v]

    @property
    def occupied_fraction(self):
        """Mean over the views of the fraction of occupied cells in the grid their next step runs under."""
        return sum(s.current().occupied_fraction for s in self.views) / max(len(self.views), 1)

    def state_dict(self):
        return {"views": [s.state_dict() for s in self.views]}

    def load_state_dict(self, sd):
        if len(sd["views"]) != len(self.views):
            raise ValueError("occupancy state: the checkpoint holds grids for another number of training views")
        for s, d in zip(self.views, sd["views"]):
            s.load_state_dict(d)


class ExtractorTrainer:
    """The extractor side of --train-extractor: the LoRA parameters (config.lora_trainable_parameters) in a torch.optim.Adam, one
    live map per view and one step per view with the map gradient summed over the view's batches."""

    def __init__(self, extractor, images, lr, weight_decay):
        from .config import lora_trainable_parameters
        self.extractor, self.images = extractor, images                      # images: (V,H,W,3) in [0,1] on the extractor's device
        self.params = lora_trainable_parameters(extractor)
        if not self.params:
            raise ValueError("the extractor has no parameter with `lora` in its name: nothing to train")
        self.opt = torch.optim.Adam(self.params, lr=lr, weight_decay=weight_decay)
        self.map = self.d_map = self.d_feats = None
        self.steps = 0

    def set_lr(self, lr):
        for g in self.opt.param_groups:
            g["lr"] = lr

    def begin_view(self, v):
        """Run the extractor on view v under grad (train mode); returns the detached (1,Hp,Wp,C) map the batches read."""
        self.extractor.train()
        self.map = precompute_dino_features(self.extractor, self.images[v:v + 1], requires_grad=True).float()
        self.d_map = torch.zeros_like(self.map)
        return self.map.detach()

    def feats_grad_buffer(self, n, c):
        if self.d_feats is None or self.d_feats.shape[0] < n or self.d_feats.shape[1] != c:
            self.d_feats = torch.empty((n, c), dtype=torch.float32, device=self.map.device)
        return self.d_feats[:n]

    def add_batch(self, dino, pts, d_feats):
        """d_map += the fetch adjoint of this batch's dL/d features."""
        project_fetch_backward(dino, pts, d_feats, self.d_map, accumulate=True)

    def end_view(self):
        """map.backward(sum of the view's batches) and one extractor step."""
        if self.map is None:
            return
        self.opt.zero_grad(set_to_none=True)
        self.map.backward(self.d_map)
        self.opt.step()
        self.steps += 1
        self.map = self.d_map = None


# ---- one epoch ------------------------------------------------------------------------------------------------------------------
def _epoch_route(model, occupancy, extractor, fused_inputs, n_importance, patches, draws):
    """train_epoch's combination checks; returns (whether the batches run on the fused-input route, whether `occupancy` holds one
    grid per view)."""
    use_dino, per_view = model.net == L.NRF_NET_V3, isinstance(occupancy, PerViewOccupancy)
    grid, fused = occupancy is not None, fused_inputs or occupancy is not None or n_importance > 0
    problem = _refusal(
        (per_view and not use_dino, "per-view occupancy grids belong to use_dino models: the other fields do not depend on the view"),
        (grid and not per_view and (use_dino or extractor is not None),
         "training under an occupancy grid is not combined with use_dino models or a trained extractor"),
        (n_importance > 0 and (grid or extractor is not None), "the hierarchical step is not combined with an occupancy grid or a trained extractor"),
        (patches is not None and (fused or extractor is not None),
         "patches go with the staged route alone: not with fused_inputs, an occupancy grid, the hierarchical step or a trained extractor"),
        (patches is not None and draws is not None, "patches are not combined with draws: a recorded run holds no jitter for the patch rays"))
    if problem:
        raise ValueError(problem)
    return fused, per_view


def _view_batch(ep, vw, idx, t_rand, seed):
    """One batch of the fused-input route: one `step.step_view` (or `step_view_hierarchical`) on the pixel ids `idx` of the view `vw`,
    under the view's grid when there is one, then the grid's and the extractor's share.  Returns (loss, ray-samples)."""
    step, extractor, S = ep.step, ep.extractor, ep.S
    n = idx.shape[0]
    kw = dict(dino=vw.dino, seed=seed, target=vw.tgt[idx])
    if extractor is not None:
        d_feats = extractor.feats_grad_buffer(n * S, int(vw.view_map.shape[-1]))
        if ep.pts_buf is None or ep.pts_buf.shape[0] < n * S:
            ep.pts_buf = torch.empty((n * S, 3), dtype=torch.float32, device=vw.tgt.device)
        kw.update(d_dino_out=d_feats, points_out=ep.pts_buf[:n * S])
    if vw.sched is not None:
        kw["occupancy"] = vw.sched.current()
    if ep.per_view:
        kw["grid_inputs"] = "rays"
    if ep.Ni > 0:
        loss = step.step_view_hierarchical(None, vw.c2w, ep.Ht, ep.Wt, vw.f_t, idx, ep.near, ep.far, S, ep.Ni, perturb=True, t_rand=t_rand,
                                           coarse_weight=ep.coarse_weight, **kw)
    else:
        loss = step.step_view(None, vw.c2w, ep.Ht, ep.Wt, vw.f_t, idx, ep.near, ep.far, S, perturb=True, t_rand=t_rand, **kw)
    if vw.sched is not None:
        vw.sched.after_step(step.model, dino=vw.cam if ep.per_view else None)
    if extractor is not None:
        rows = step.last_count if ep.per_view else n * S          # under a grid: the kept samples, as dense rows
        if rows:
            extractor.add_batch(vw.cam, ep.pts_buf[:rows], d_feats[:rows])
    return loss, n * (S + ep.Ni)


def _staged_batch(ep, vw, idx, t_rand, seed):
    """One batch of the staged route: torch gathers, sample_points_along_rays, the expanded directions and fetch_features in front of
    one `step(...)`, the patches of unseen poses behind the supervised rays when the epoch draws them.  Returns (loss, ray-samples)."""
    step, extractor, S = ep.step, ep.extractor, ep.S
    o, d, t = vw.ro[idx], vw.rd[idx], vw.tgt[idx]
    n_p = 0
    if ep.patches is not None:
        n_p = int(ep.patches["n"])
        pp = sample_patch_poses(ep.train_poses, n_p, ep.patches["generator"]).to(o.device)
        o_p, d_p = patch_rays(ep.Ht, ep.Wt, ep.f_s, pp, step.patch_size, ep.patches["generator"], ep.patches["stride"])
        o, d = torch.cat([o, o_p]), torch.cat([d, d_p])
    pts, z = sample_points_along_rays(o, d, ep.near, ep.far, S, perturb=True, t_rand=t_rand, seed=seed)
    n = o.shape[0]
    dirs = d[:, None, :].expand(n, S, 3).reshape(-1, 3)                         # train.py:225: raw ray directions per sample
    feats = fetch_features(vw.dino, pts.reshape(-1, 3)) if ep.use_dino else None
    if extractor is not None:
        d_feats = extractor.feats_grad_buffer(n * S, feats.shape[1])
        loss = step(pts.reshape(-1, 3), z, d, t, dirs=dirs, dino=feats, d_dino_out=d_feats)
        extractor.add_batch(vw.cam, pts.reshape(-1, 3), d_feats)
    else:
        loss = step(pts.reshape(-1, 3), z, d, t, dirs=dirs, dino=feats, **({"n_patches": n_p} if n_p else {}))
    return loss, n * S


def train_epoch(step, cfg, epoch, images, poses, H, W, focal, near, far, gen, dino_maps=None, max_batches=None, rank=0, world=1,
                extractor=None, fused_inputs=False, occupancy=None, draws=None, n_importance=0, coarse_weight=1.0, patches=None):
    """One pass of train.py:261-290 over the training views; returns (mean loss, ray-samples processed).
    fused_inputs: every batch is one `step.step_view` on its pixel ids (--fused-inputs; module docstring) instead of torch gathers,
    sample_points_along_rays, the expanded directions and fetch_features in front of `step(...)`.
    occupancy: an OccupancySchedule (--occupancy-res; module docstring) -- the fused_inputs route with `occupancy=` its current grid,
    and a refresh of the grid when one is due; or a PerViewOccupancy (--occupancy-per-view): view v's batches step under view v's grid
    with grid_inputs="rays", use_dino models and a trained extractor included.
    extractor: an ExtractorTrainer (--train-extractor; module docstring) -- the view's map comes from it, live, instead of
    dino_maps[v], and it takes one step per view.
    n_importance > 0 (--n-importance; module docstring): every batch is one `step.step_view_hierarchical` with that many resampled
    depths and `coarse_weight`; the fused_inputs route, without a grid or a trained extractor.
    draws: the epoch's random draws as inputs (parity runs against a recorded run of the reference's trainer): an object whose
    `permutation(v, n)` returns view v's shuffle of its n rays (train.py:272's torch.randperm) and whose `jitter(v, i, n, S)` returns the
    (n,S) uniforms of the batch starting at position i (ray_utils.py:78's torch.rand), handed on as `t_rand=`.  None: `gen` shuffles and
    the counter RNG jitters, as before.
    patches: dict(n=, stride=, generator=) (--depth-smooth-weight; module docstring) -- every batch of the staged route gets n patches
    of step.patch_size^2 rays from freshly drawn poses behind its supervised rays, drawn from the CPU generator.  Refused with
    fused_inputs, occupancy, n_importance, extractor and draws (a recorded run holds no jitter for the patch rays).
    world > 1 (data parallel, `FusedStep(data_parallel=True)`): every rank draws the SAME shuffle (same generator seed) and
    takes rays rank, rank+world, ... of each batch -- the batches are those of one process (the stratified jitter of a ray is
    keyed by its position inside the call, so the sample depths differ from a single-process run's)."""
    Ht, Wt, S, batch = schedule_for(cfg, epoch)
    use_dino = step.model.net == L.NRF_NET_V3
    fused_inputs, per_view = _epoch_route(step.model, occupancy, extractor, fused_inputs, int(n_importance), patches, draws)
    run_batch = _view_batch if fused_inputs else _staged_batch
    # what every batch of the epoch reads; pts_buf: the fused route's sample positions for the extractor, grown when a batch needs more
    ep = SimpleNamespace(step=step, extractor=extractor, per_view=per_view, use_dino=use_dino, patches=patches, Ht=Ht, Wt=Wt, S=S,
                         Ni=int(n_importance), near=near, far=far, coarse_weight=coarse_weight, pts_buf=None,
                         train_poses=torch.stack([p.detach().cpu() for p in poses]) if patches is not None else None,      # what the unseen poses are drawn around
                         f_s=focal if (Ht, Wt) == (H, W) else focal * (Ht / H))      # the focal length of the schedule's rays (view_target)
    total, n_batches, samples = None, 0, 0
    for v in range(len(images)):
        vw = SimpleNamespace()                            # what the view's batches read
        if fused_inputs:
            vw.tgt, vw.f_t = view_target(images[v], H, W, focal, Ht, Wt)
            n_view, dev_v, vw.c2w = Ht * Wt, vw.tgt.device, _c2w12(poses[v])        # the camera of the view's batches, converted once
        else:
            vw.ro, vw.rd, vw.tgt = view_rays(images[v], poses[v], H, W, focal, Ht, Wt)
            n_view, dev_v = vw.ro.shape[0], vw.ro.device
        vw.view_map = extractor.begin_view(v) if extractor is not None else (dino_maps[v:v + 1] if use_dino else None)
        vw.dino = make_dino(vw.view_map, poses[v], focal, H, W) if use_dino else None           # train.py:204-206: full-resolution intrinsics
        vw.cam = dict(features=vw.view_map, pose=poses[v], focal=focal, H=H, W=W)
        vw.sched = occupancy.view(v) if per_view else occupancy
        if draws is None:
            order = torch.randperm(n_view, device=dev_v, generator=gen)
        else:
            order = torch.as_tensor(draws.permutation(v, n_view), dtype=torch.int64).to(dev_v)
        for i in range(0, order.shape[0], batch):
            idx = order[i:i + batch]
            if world > 1:
                idx = idx[: idx.shape[0] // world * world][rank::world]        # equal shards: the all-reduce averages per-rank means
                if idx.shape[0] == 0:
                    continue
            t_rand = None if draws is None else draws.jitter(v, i, idx.shape[0], S)
            loss, done = run_batch(ep, vw, idx, t_rand, epoch * 1_000_003 + v * 10_007 + i)
            total = loss if total is None else total + loss
            n_batches += 1
            samples += done
            if max_batches is not None and n_batches >= max_batches:
                if extractor is not None:
                    extractor.end_view()                                                # step with what has been accumulated
                return float(total) / n_batches, samples
        if extractor is not None:
            extractor.end_view()
    return (float(total) / max(n_batches, 1)) if total is not None else 0.0, samples


def step_options(cfg, recipe="train"):
    """FusedStep's keyword arguments for a config under a recipe.  'train': train.py:36-44,113-118 (rgb_weight * mse, Adam with
    weight decay in the gradient).  'multiscale': train_multiscale.py:41-45,61-65,207-211,259-264 (NeRFLoss with the
    regulariser, density noise, clip_grad_norm_ at 1.0, AdamW)."""
    o, lw, r = cfg["optimizer"], cfg.get("loss", {}) or {}, cfg.get("rendering", {}) or {}
    kw = dict(lr=float(o["lr"]), weight_decay=float(o["weight_decay"]), rgb_weight=float(lw.get("rgb_weight", 1.0)))
    if recipe == "multiscale":
        kw.update(reg_weight=float(lw.get("reg_weight", 0.01)), depth_weight=float(lw.get("depth_weight", 0.1)),
                  noise_std=float(r.get("noise_std", 0.0)), max_grad_norm=1.0, decoupled_weight_decay=True)
    elif recipe != "train":
        raise ValueError(f"unknown recipe {recipe!r}")
    return kw


def save_checkpoint(path, model, step, epoch, best_psnr, cfg, recipe="train", extractor=None, occupancy=None):
    """train.py:374-389's dictionary: `nerf_model_state_dict` is what evaluate.py:27 / load_checkpoint_into read; the multiscale
    recipe adds train_multiscale.py:368-376's `nerf_state_dict` (the same tensors); --train-extractor adds
    `dino_model_state_dict` (train.py:384) and the extractor optimizer's state; --occupancy-per-view (a PerViewOccupancy) adds
    `occupancy_per_view_state`.  The single grid of --occupancy-res is not saved.  Under a frequency mask (--freq-reg-end) the weights
    are the RAW ones, as resuming needs them, and the active mask is saved beside them as `freq_mask_pos` / `freq_mask_dirs`
    (load_checkpoint_into applies it; NeRFMLP.effective_state_dict() is the masked field for a consumer that knows no masks)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    opt = step.opt
    o = cfg["optimizer"]
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    torch.save({"epoch": epoch, "best_psnr": best_psnr,
                "nerf_model_state_dict": sd, **({"nerf_state_dict": sd} if recipe == "multiscale" else {}),
                # flat-vector Adam state (training.Adam; layout = include/nerfhip.h's flat parameter order), restored by --checkpoint
                "optimizer_state_dict": {"step": opt.step_count, "exp_avg": None if opt.exp_avg is None else opt.exp_avg.cpu(),
                                         "exp_avg_sq": None if opt.exp_avg_sq is None else opt.exp_avg_sq.cpu(), "lr": opt.lr},
                # MultiStepLR is a pure function of the epoch (lr_at): its state is the epoch counter
                "scheduler_state_dict": {"last_epoch": epoch + 1, "milestones": list(o["lr_milestones"]), "gamma": float(o["lr_gamma"])},
                **({"dino_model_state_dict": {k: v.detach().cpu().clone() for k, v in extractor.extractor.state_dict().items()},
                    "dino_optimizer_state_dict": extractor.opt.state_dict()} if extractor is not None else {}),
                **({"occupancy_per_view_state": occupancy.state_dict()} if isinstance(occupancy, PerViewOccupancy) else {}),
                **{k: v for k, v in zip(("freq_mask_pos", "freq_mask_dirs"), model.freq_mask) if v is not None},
                "config": cfg}, path)


def resume_from(ckpt, model, step):
    """Restore what save_checkpoint wrote beyond the weights: Adam moments + step count; returns (first epoch to run, best PSNR).
    A checkpoint without them (e.g. one written by the reference) resumes the weights only, from epoch 0."""
    os_ = ckpt.get("optimizer_state_dict") if isinstance(ckpt, dict) else None
    start, best = 0, 0.0
    if isinstance(os_, dict) and os_.get("exp_avg") is not None and "step" in os_:
        fp, flat = step.opt._buffers()
        if os_["exp_avg"].numel() == flat.numel():
            step.opt.exp_avg.copy_(os_["exp_avg"].to(flat.device))
            step.opt.exp_avg_sq.copy_(os_["exp_avg_sq"].to(flat.device))
            step.opt.step_count = int(os_["step"])
            start, best = int(ckpt.get("epoch", -1)) + 1, float(ckpt.get("best_psnr", 0.0))
    return start, best


# ---- the command, phase by phase ------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--data", required=True, help="dataset directory holding transforms_train.json / transforms_test.json")
    ap.add_argument("--recipe", default="train", choices=["train", "multiscale"],
                    help="the optimisation step: train.py's (rgb_weight * mse, Adam) or train_multiscale.py's (density noise, NeRFLoss with "
                         "the weights regulariser, gradient clipping at 1.0, AdamW)")
    ap.add_argument("--epochs", type=int, default=None, help="default: training.epochs of the config")
    ap.add_argument("--mode", default="bf16", choices=["bf16", "f16", "f32"],
                    help="arithmetic of the TRAINING kernels (bf16: its exponent range suits the unscaled gradients)")
    ap.add_argument("--eval-mode", default="f16", choices=["bf16", "f16", "f16x3", "f32"],
                    help="arithmetic of the validation renders: f16 keeps the reported PSNR within 0.01 dB of an fp32 render (bf16 does not)")
    ap.add_argument("--out", default=None, help="default: output.save_dir of the config")
    ap.add_argument("--checkpoint", default=None, help="resume from this file: weights, Adam moments / step, epoch and best PSNR")
    ap.add_argument("--dino-maps", default=None, help="precomputed feature maps (V,Hp,Wp,C), torch.save'd, one per training view")
    ap.add_argument("--dino-weights", default=None, help="local transformers Dinov2Model checkpoint (dir or file) for the extractor of the config")
    ap.add_argument("--dino-random-init", action="store_true", help="build the extractor with random weights (pipeline runs, features meaningless)")
    ap.add_argument("--train-extractor", action="store_true",
                    help="backpropagate into the feature maps and train the extractor's LoRA matrices (train.py:105-110's trainable set), one "
                         "extractor step per view; needs --dino-weights or --dino-random-init (module docstring)")
    ap.add_argument("--fused-inputs", action="store_true",
                    help="cast rays, sample, encode and fetch the DINO features inside the training forward kernel (FusedStep.step_view) instead "
                         "of building per-sample tensors in front of it; same shuffle, seeds and sharding")
    ap.add_argument("--n-importance", type=int, default=0, metavar="N",
                    help="train coarse-to-fine: N depths resampled from the coarse weights per ray, FusedStep.step_view_hierarchical per batch, "
                         "hierarchical validation (module docstring); 0: off")
    ap.add_argument("--coarse-weight", type=float, default=None, metavar="W",
                    help="with --n-importance: the coarse image's share of the loss, rgb_weight * (W * mse_coarse + mse_fine) (default 1.0)")
    ap.add_argument("--dist-weight", type=float, default=0.0, metavar="W",
                    help="add W * the distortion loss of mip-NeRF 360 (weights against interval midpoints scaled by 1 / (far - near)) to the "
                         "step's loss: FusedStep(dist_weight=W) (module docstring); 0: off")
    ap.add_argument("--occ-weight", type=float, default=0.0, metavar="W",
                    help="add W * the occlusion penalty of FreeNeRF (mean rectified density of every ray's first --occ-samples samples): "
                         "FusedStep(occ_weight=W, occ_samples=K) (module docstring); 0: off")
    ap.add_argument("--occ-samples", type=int, default=None, metavar="K", help="with --occ-weight: the samples at the front of every ray it covers")
    ap.add_argument("--depth-smooth-weight", type=float, default=0.0, metavar="W",
                    help="add W * RegNeRF's depth-smoothness loss on patches rendered from unseen poses to the step's loss: "
                         "FusedStep(depth_smooth_weight=W, patch_size=P) (module docstring); 0: off")
    ap.add_argument("--patch-size", type=int, default=8, metavar="P", help="with --depth-smooth-weight: a patch is P x P rays (2 ... 16)")
    ap.add_argument("--patches-per-step", type=int, default=16, metavar="N", help="with --depth-smooth-weight: patches behind every batch's supervised rays")
    ap.add_argument("--patch-stride", type=int, default=1, metavar="K", help="with --depth-smooth-weight: neighbouring patch pixels are K image pixels apart")
    ap.add_argument("--entropy-weight", type=float, default=0.0, metavar="W",
                    help="add W * InfoNeRF's ray entropy (mean over every ray of the batch of the entropy of its per-sample distribution): "
                         "FusedStep(ent_weight=W, ent_threshold=T) (module docstring); 0: off")
    ap.add_argument("--entropy-threshold", type=float, default=None, metavar="T",
                    help="with --entropy-weight / --kl-weight: rays whose summed opacity is at most T take no part (default 0.01)")
    ap.add_argument("--entropy-unseen", action="store_true",
                    help="with --entropy-weight: also draw --patches-per-step patches of unseen poses per batch, as --depth-smooth-weight does")
    ap.add_argument("--kl-weight", type=float, default=0.0, metavar="W",
                    help="add W * InfoNeRF's information-gain loss, the KL divergence between neighbouring rays of patches from unseen poses: "
                         "FusedStep(kl_weight=W, patch_size=P) (module docstring); 0: off")
    ap.add_argument("--freq-reg-end", type=int, default=0, metavar="N",
                    help="FreeNeRF's frequency regularisation: reveal the bands of the positional encodings linearly over the first N steps "
                         "(FusedStep(freq_reg_end=N); a column scale in the re-pack and the weight gradients, no launch more); 0: off")
    ap.add_argument("--no-freq-reg-dirs", action="store_true", help="with --freq-reg-end: mask the position encoding only")
    ap.add_argument("--occupancy-res", type=int, default=0,
                    help="train under an occupancy grid of N^3 cells (a multiple of 32; 0: off): the network runs on the samples in occupied "
                         "cells alone, FusedStep.step_view(occupancy=) (module docstring)")
    ap.add_argument("--occupancy-box", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="the grid's cube (default -1.5 1.5)")
    ap.add_argument("--occupancy-threshold", type=float, default=None, help="a cell is occupied when its value exceeds this (default 0.01)")
    ap.add_argument("--occupancy-decay", type=float, default=None, help="value = max(decay * value, probe) per refresh (default 0.95)")
    ap.add_argument("--occupancy-refresh-every", type=int, default=None, metavar="K", help="refresh the grid every K steps (default 16)")
    ap.add_argument("--occupancy-cells-per-refresh", type=int, default=None, help="cells probed per refresh, a multiple of 32 (default: 1/16 of the grid)")
    ap.add_argument("--occupancy-warmup", type=int, default=None, metavar="STEPS", help="steps under an all-ones grid first (default 256)")
    ap.add_argument("--occupancy-per-view", action="store_true",
                    help="use_dino configs: one grid per training view, stepped with grid_inputs=\"rays\" and saved in the checkpoint "
                         "(module docstring); needs --occupancy-res")
    ap.add_argument("--max-test-views", type=int, default=None)
    ap.add_argument("--max-batches", type=int, default=None, help="stop every epoch after this many ray batches (smoke runs)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--data-parallel", action="store_true",
                    help="launched with torch.distributed.run, one process per GPU: ray batches shard over the ranks, one all-reduce of the "
                         "flat gradient vector per step (RCCL); rank 0 validates and writes")
    ap.add_argument("--rehearse", action="store_true",
                    help="--data-parallel on a box with ONE GPU: every rank on cuda:0, the gradient all-reduce over gloo through host memory "
                         "(RCCL refuses two ranks on one card); exercises the sharding and the collective, not multi-GPU speed")
    return ap


def refuse(f):
    """SystemExit with the first refusal of FLAG_CHECKS, then of CONFIG_CHECKS; returns the config, which is read here, once."""
    problem = next(filter(None, (check(f) for check in FLAG_CHECKS)), None)
    cfg = None if problem else load_config(f.config)
    problem = problem or next(filter(None, (check(f, cfg) for check in CONFIG_CHECKS)), None)
    if problem:
        raise SystemExit(problem)
    return cfg


@contextlib.contextmanager
def distributed(f):
    """(rank, world) of this process: (0, 1), or under --data-parallel those of the process group, open for the length of the block."""
    if not f.data_parallel:
        yield 0, 1
        return
    import torch.distributed as dist
    local = 0 if f.rehearse else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if not dist.is_initialized():
        dist.init_process_group(**(dict(backend="gloo") if f.rehearse else dict(backend="nccl", device_id=torch.device("cuda", local))))
    yield dist.get_rank(), dist.get_world_size()
    dist.barrier()
    dist.destroy_process_group()


def load_scene(f, cfg):
    """The run record, with what --data holds: dev, the training views on it (images, poses, H, W, focal) and the test views (test_images,
    test_poses).  `main` adds the rest, each field where the phase that makes it returns: rank, world, out_dir, name; dino_maps, ext;
    model, step; gen, patches, occ, first_epoch, best; targets, eval_dino."""
    res = cfg["data"].get("resolution")
    images, poses, (H, W, focal) = load_blender_data(f.data, "train", img_size=res)
    nv = cfg["data"].get("num_views")
    if nv:
        images, poses = images[:nv], poses[:nv]                                          # train.py:141-143
    dev = torch.device("cuda", torch.cuda.current_device())
    images = [im.permute(1, 2, 0).float().to(dev) for im in images]
    poses = [p.float() for p in poses]
    test_images, test_poses, _ = load_blender_data(f.data, "test", img_size=res)
    if f.max_test_views:
        test_images, test_poses = test_images[: f.max_test_views], test_poses[: f.max_test_views]
    return SimpleNamespace(dev=dev, images=images, poses=poses, H=H, W=W, focal=focal, test_images=test_images, test_poses=test_poses)


def dino_source(f, cfg, run):
    """(maps (V,Hp,Wp,C), their channel count, ExtractorTrainer or None) of a use_dino config -- --dino-maps, or the config's extractor
    run once over the training views (and kept, under --train-extractor); (None, 64, None) otherwise."""
    if not bool(cfg.get("model", {}).get("use_dino", True)):
        return None, 64, None
    ext = None
    if f.dino_maps:
        dino_maps = torch.load(f.dino_maps, map_location="cpu", weights_only=True).float().to(run.dev)
    elif f.dino_weights or f.dino_random_init:
        extractor = dino_model_from_config(cfg, weights=f.dino_weights).to(run.dev)           # train.py:57-75
        dino_maps = precompute_dino_features(extractor, torch.stack(run.images)[..., :3]).float()   # train.py:158-169: once, under no_grad
        if f.train_extractor:
            ext = ExtractorTrainer(extractor, torch.stack(run.images)[..., :3], float(cfg["optimizer"]["lr"]), float(cfg["optimizer"]["weight_decay"]))
    else:
        raise SystemExit("this config conditions on DINO features: pass --dino-weights <local Dinov2Model checkpoint> (or --dino-random-init), "
                         "or --dino-maps <tensor (V,Hp,Wp,C) saved with torch.save>, one map per training view")
    if dino_maps.dim() != 4 or dino_maps.shape[0] < len(run.images):
        raise SystemExit("--dino-maps must hold one (Hp,Wp,C) map per training view")
    return dino_maps, int(dino_maps.shape[-1]), ext


def build_step(f, cfg, rs, run, dino_dim):
    """(model, FusedStep, the --checkpoint's dictionary or None): the model of the config with the checkpoint's weights (and the
    extractor's) loaded, on the device, and the step the flags ask for."""
    model = model_from_config(cfg, dino_dim=dino_dim, mma_mode=f.mode)
    ckpt = torch.load(f.checkpoint, map_location="cpu", weights_only=True) if f.checkpoint else None
    if ckpt is not None:
        load_checkpoint_into(model, ckpt)
        if run.ext is not None and "dino_model_state_dict" in ckpt:
            run.ext.extractor.load_state_dict(ckpt["dino_model_state_dict"])
            if "dino_optimizer_state_dict" in ckpt:
                run.ext.opt.load_state_dict(ckpt["dino_optimizer_state_dict"])
    model.dino_grad = run.ext is not None
    model = model.to(run.dev).train()
    step = FusedStep(model, white_bkgd=rs["white_bkgd"], data_parallel=run.world > 1, **step_options(cfg, f.recipe),
                     **({"seed": f.seed} if f.recipe == "multiscale" else {}), **ray_reg_options(f, rs["near"], rs["far"]),
                     **freq_reg_options(f), **patch_reg_options(f), **info_reg_options(f))
    return model, step, ckpt


def training_state(f, run, ckpt):
    """What the epochs carry besides the weights: (the shuffle generator, the patch draws or None, the occupancy grids or None -- the
    single grid is not part of a checkpoint: a resumed run starts again from the all-ones grid and its warm-up; the per-view grids
    are -- and from the checkpoint the first epoch to run and the best PSNR)."""
    gen = torch.Generator(device=run.dev)
    gen.manual_seed(f.seed)
    patches = None
    if f.draws_patches:                                   # the patch draws: a CPU generator of their own, another stream on every rank
        patches = dict(n=f.patches_per_step, stride=f.patch_stride,
                       generator=torch.Generator().manual_seed(f.seed * 1_000_003 + 7919 * (run.rank + 1)))
    occ = None
    if f.occupancy_res:
        occ = PerViewOccupancy.from_args(f, len(run.images), run.dev) if f.occupancy_per_view else OccupancySchedule.from_args(f, run.dev)
    if ckpt is not None and isinstance(occ, PerViewOccupancy) and "occupancy_per_view_state" in ckpt:
        occ.load_state_dict(ckpt["occupancy_per_view_state"])
    return (gen, patches, occ, *(resume_from(ckpt, run.model, run.step) if ckpt is not None else (0, 0.0)))


def run_epoch(f, cfg, rs, run, epoch, epochs):
    """One epoch's record: the epoch trained at its learning rate and, on rank 0 (every rank holds the same parameters), the
    validation and the checkpoints that are due behind it."""
    step, ext, occ, model = run.step, run.ext, run.occ, run.model
    step.opt.lr = lr_at(cfg, epoch)
    if ext is not None:
        ext.set_lr(lr_at(cfg, epoch))
    t0 = time.perf_counter()
    loss, samples = train_epoch(step, cfg, epoch, run.images, run.poses, run.H, run.W, run.focal, rs["near"], rs["far"], run.gen, run.dino_maps,
                                f.max_batches, run.rank, run.world, extractor=ext, fused_inputs=f.fused_inputs, occupancy=occ,
                                n_importance=f.n_importance, coarse_weight=1.0 if f.coarse_weight is None else f.coarse_weight, patches=run.patches)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"epoch": epoch + 1, "loss": loss, "lr": step.opt.lr, "seconds": round(dt, 3), "Msamples_per_s": round(run.world * samples / dt / 1e6, 2)}
    if occ is not None:
        rec["occupied_fraction"] = round(occ.occupied_fraction if f.occupancy_per_view else occ.current().occupied_fraction, 4)
    if run.rank != 0:
        return rec
    if (epoch + 1) % int(cfg["output"]["val_freq"]) == 0 or epoch + 1 == epochs:
        if ext is not None:                                               # the extractor moved: view 0's map as it is now, under no_grad
            run.eval_dino["features"] = precompute_dino_features(ext.extractor, ext.images[0:1]).float()
        m = evaluate_views(model, run.test_poses, run.H, run.W, run.focal, rs["near"], rs["far"], rs["n_samples"], targets=run.targets,
                           white_bkgd=rs["white_bkgd"], mma_mode=f.eval_mode, dino=run.eval_dino, out_dir=os.path.join(run.out_dir, f"val_{epoch + 1}"),
                           N_importance=f.n_importance)
        model.train()
        rec.update(psnr=m["psnr"], ssim=m["ssim"])
        if m["psnr"] > run.best:
            run.best = m["psnr"]
            save_checkpoint(os.path.join(run.out_dir, f"best_{run.name}.pth"), model, step, epoch, run.best, cfg, f.recipe, ext, occ)
    if (epoch + 1) % int(cfg["output"]["save_freq"]) == 0:
        save_checkpoint(os.path.join(run.out_dir, f"epoch_{epoch + 1}.pth"), model, step, epoch, run.best, cfg, f.recipe, ext, occ)
    print(json.dumps(rec), flush=True)
    return rec


def main(argv=None):
    f = flags_of(build_parser().parse_args(argv))
    cfg = refuse(f)
    with distributed(f) as (rank, world):
        torch.manual_seed(f.seed)                         # parameter init (when no checkpoint is given) and the ray shuffles
        rs = render_settings(cfg)
        out_dir = f.out or cfg["output"]["save_dir"]
        epochs = f.epochs if f.epochs is not None else int(cfg["training"]["epochs"])
        run = load_scene(f, cfg)
        run.rank, run.world, run.out_dir, run.name = rank, world, out_dir, cfg.get("experiment", {}).get("name", "run")
        run.dino_maps, dino_dim, run.ext = dino_source(f, cfg, run)
        run.model, run.step, ckpt = build_step(f, cfg, rs, run, dino_dim)
        run.gen, run.patches, run.occ, run.first_epoch, run.best = training_state(f, run, ckpt)
        run.targets = run.test_images.permute(0, 2, 3, 1).contiguous()
        use_dino = run.dino_maps is not None              # train.py:203-208: validation conditions on training view 0
        run.eval_dino = dict(features=run.dino_maps[0:1], pose=run.poses[0], focal=run.focal, H=run.H, W=run.W) if use_dino else None
        log = [run_epoch(f, cfg, rs, run, epoch, epochs) for epoch in range(run.first_epoch, epochs)]
        if rank == 0:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, "train_log.json"), "w") as fh:
                json.dump(log, fh, indent=1)
    return log


if __name__ == "__main__":
    main()
