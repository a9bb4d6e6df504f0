"""python -m nerf_few_shot_limitations_amd.evaluate_cli --config experiments/baseline.yaml --data data/nerf_synthetic/lego \\
        [--checkpoint results/.../best.pth] [--split test] [--out results/eval] [--mode f16x3|f32|f16|bf16] [--max-views N]

What `NeRFDINOTrainer.evaluate` does (src/training/train.py:294-342) for a use_dino=False config, on the fused renderer:
load the YAML unchanged, the Blender split, the checkpoint (either key set), render every view (8 per launch), score
PSNR/SSIM, dump PNGs and a metrics.json.  Without --checkpoint the weights are the module's random init (smoke use).
A checkpoint written under a frequency mask (train_cli --freq-reg-end: keys `freq_mask_pos` / `freq_mask_dirs` beside the raw
weights) is rendered under that mask (load_checkpoint_into applies it).
use_dino configs condition every test view on the feature map and pose of TRAINING view 0 (train.py:203-208: `feat_idx = 0` outside
training).  The map comes from the config's extractor (config.dino_model_from_config) run once on that view -- --dino-weights
names a local transformers Dinov2Model checkpoint, --dino-random-init builds it with random weights (the published weights are
not available offline) -- or from --dino-map, a saved (1,Hp,Wp,C) tensor; without any of them the CLI refuses.
"""
from __future__ import annotations

import argparse
import json
import os

import torch

from . import (dino_model_from_config, evaluate_views, load_blender_data, load_checkpoint_into, load_config, model_from_config,
               precompute_dino_features, render_settings)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", required=True)
    ap.add_argument("--data", required=True, help="dataset directory holding transforms_<split>.json")
    ap.add_argument("--checkpoint")
    ap.add_argument("--split", default="test")
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default="f16x3", choices=["f16x3", "f32", "f16", "bf16"],
                    help="f16x3 / f32: parity-grade (1e-4 of the reference); f16 / bf16: full MFMA rate")
    ap.add_argument("--tail-mode", default=None, choices=["f16x3"],
                    help="with --mode f16 / bf16: evaluate every ray's last sample (composited with dist = 1e10) in split-f16")
    ap.add_argument("--max-views", type=int, default=None)
    ap.add_argument("--ert", type=float, default=0.0)
    ap.add_argument("--n-importance", type=int, default=0, metavar="N",
                    help="hierarchical render: N importance samples resampled from the coarse pass' weights on top of the config's sample count "
                         "(0 = off; not with --tail-mode, --ert or --occupancy-res)")
    ap.add_argument("--hier-chunk-rays", type=int, default=1 << 15, metavar="M", help="with --n-importance: rays per range of the frame's march")
    ap.add_argument("--occupancy-res", type=int, default=0,
                    help="skip empty space with an occupancy grid of N^3 cells built from the checkpoint (0 = off; N a multiple of 32, <= 512)")
    ap.add_argument("--occupancy-threshold", type=float, default=0.0, help="a cell is occupied when a probed density exceeds this")
    ap.add_argument("--occupancy-samples", type=int, default=4, help="densities probed per cell")
    ap.add_argument("--occupancy-dilate", type=int, default=1, help="cells the occupied set is grown by")
    ap.add_argument("--occupancy-box", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="the grid's box on every axis (default: -far .. far)")
    ap.add_argument("--occupancy-prune-views", type=int, default=0, metavar="N",
                    help="prune the grid by the weights the first N views of the train split render (0 = off; needs --occupancy-res)")
    ap.add_argument("--occupancy-weight-threshold", type=float, default=None,
                    help="pruning: a cell stays when a sample of weight above this fell into it (default 0: the marking views render unchanged)")
    ap.add_argument("--occupancy-seen-eps", type=float, default=None,
                    help="pruning: a cell counts as seen when a ray reached it with transmittance above this (default 1e-2)")
    ap.add_argument("--occupancy-unseen", default=None, choices=["keep", "drop"],
                    help="pruning: cells no marking ray reached keep what the probed grid says (keep, the default) or are emptied (drop)")
    ap.add_argument("--dino-map", default=None)
    ap.add_argument("--dino-weights", default=None, help="local transformers Dinov2Model checkpoint (dir or file) for the extractor of the config")
    ap.add_argument("--dino-random-init", action="store_true", help="build the extractor with random weights (pipeline runs, features meaningless)")
    args = ap.parse_args(argv)
    pruning = (args.occupancy_prune_views != 0 or args.occupancy_weight_threshold is not None or args.occupancy_seen_eps is not None
               or args.occupancy_unseen is not None)
    if pruning and not args.occupancy_res:
        raise SystemExit("--occupancy-prune-views / --occupancy-weight-threshold / --occupancy-seen-eps / --occupancy-unseen prune the grid "
                         "of --occupancy-res: pass --occupancy-res N as well")
    if args.n_importance < 0 or args.hier_chunk_rays < 1:
        raise SystemExit("--n-importance must be >= 0 and --hier-chunk-rays >= 1")
    if args.n_importance and (args.tail_mode or args.ert > 0.0 or args.occupancy_res):
        raise SystemExit("--n-importance renders every sample of both passes: it takes no --tail-mode, --ert or --occupancy-res")
    if args.occupancy_prune_views < 0:
        raise SystemExit("--occupancy-prune-views must be >= 0")
    if pruning and not args.occupancy_prune_views:
        raise SystemExit("--occupancy-weight-threshold / --occupancy-seen-eps / --occupancy-unseen set how --occupancy-prune-views N prunes: "
                         "pass --occupancy-prune-views N (N >= 1) as well")
    tau, eps = args.occupancy_weight_threshold, args.occupancy_seen_eps
    if tau is not None and not (0.0 <= tau < float("inf")):
        raise SystemExit("--occupancy-weight-threshold must be finite and >= 0")
    if eps is not None and not (0.0 <= eps < 1.0):
        raise SystemExit("--occupancy-seen-eps must be in [0, 1)")

    cfg = load_config(args.config)
    rs = render_settings(cfg)
    images, poses, (H, W, focal) = load_blender_data(args.data, args.split, img_size=cfg["data"].get("resolution"))
    if args.max_views:
        images, poses = images[: args.max_views], poses[: args.max_views]
    use_dino = bool(cfg.get("model", {}).get("use_dino", True))
    prune_poses = None
    if args.occupancy_prune_views:
        prune_poses = load_blender_data(args.data, "train", img_size=cfg["data"].get("resolution"))[1][: args.occupancy_prune_views]
    dino = None
    dino_dim = 128 if cfg.get("model", {}).get("dino_model_type") == "multi_scale" else 64
    if use_dino:
        # the source view of every evaluation render is TRAINING view 0: its map and its pose (train.py:203-208)
        tr_images, tr_poses, _ = load_blender_data(args.data, "train", img_size=cfg["data"].get("resolution"))
        if args.dino_map:
            fm = torch.load(args.dino_map, map_location="cpu", weights_only=True)
        elif args.dino_weights or args.dino_random_init:
            extractor = dino_model_from_config(cfg, weights=args.dino_weights).cuda()
            fm = precompute_dino_features(extractor, tr_images[:1]).float()
            del extractor
        else:
            raise SystemExit("this config conditions on DINO features: pass --dino-weights <local Dinov2Model checkpoint> (or --dino-random-init), "
                             "or --dino-map <tensor (1,Hp,Wp,C) saved with torch.save>")
        dino = dict(features=fm[:1], pose=tr_poses[0], focal=focal, H=H, W=W)
        dino_dim = int(fm.shape[-1])
    model = model_from_config(cfg, dino_dim=dino_dim, mma_mode=args.mode)
    if args.checkpoint:
        load_checkpoint_into(model, torch.load(args.checkpoint, map_location="cpu", weights_only=True))
    model = model.cuda().eval()
    targets = images.permute(0, 2, 3, 1).contiguous()
    grid = None
    if args.occupancy_res:
        # built from the loaded weights; a use_dino model's grid belongs to its source view, and every evaluation render has the
        # same one (training view 0), so one grid is built, on first use
        from .occupancy import OccupancyGrid
        lo, hi = args.occupancy_box if args.occupancy_box else (-rs["far"], rs["far"])
        grid = OccupancyGrid.from_model(model, lo, hi, resolution=args.occupancy_res, threshold=args.occupancy_threshold,
                                        samples_per_cell=args.occupancy_samples, dilate=args.occupancy_dilate, mma_mode=args.mode, dino=dino)
        if prune_poses is not None:
            # the probed grid is the base: the train views empty the cells they show to be empty, nothing is added
            prune = {"prune_views": int(prune_poses.shape[0]),
                     "weight_threshold": 0.0 if args.occupancy_weight_threshold is None else args.occupancy_weight_threshold,
                     "seen_eps": 1e-2 if args.occupancy_seen_eps is None else args.occupancy_seen_eps,
                     "unseen": args.occupancy_unseen or "keep", "occupied_fraction_before": grid.occupied_fraction}
            grid = grid.prune(model, prune_poses, H, W, focal, rs["near"], rs["far"], rs["n_samples"], weight_threshold=prune["weight_threshold"],
                              seen_eps=prune["seen_eps"], unseen=prune["unseen"], dilate=args.occupancy_dilate, mma_mode=args.mode, dino=dino)
            prune["occupied_fraction_after"] = grid.occupied_fraction
    res = evaluate_views(model, poses, H, W, focal, rs["near"], rs["far"], rs["n_samples"], targets=targets, out_dir=args.out,
                         white_bkgd=rs["white_bkgd"], mma_mode=args.mode, ert_eps=args.ert, dino=dino, tail_mode=args.tail_mode, occupancy=grid,
                         return_stats=grid is not None, N_importance=args.n_importance, hier_chunk_rays=args.hier_chunk_rays)
    metrics = {"psnr": res["psnr"], "ssim": res["ssim"], "views": len(res["per_view"]), "per_view": res["per_view"],
               "H": H, "W": W, "n_samples": rs["n_samples"], "mode": args.mode}
    if args.n_importance:
        metrics["n_importance"] = args.n_importance
    if args.tail_mode:
        metrics["tail_mode"] = args.tail_mode
    if grid is not None:
        metrics["occupancy"] = {"res": args.occupancy_res, "threshold": args.occupancy_threshold, "samples": args.occupancy_samples,
                                "dilate": args.occupancy_dilate, "occupied_fraction": grid.occupied_fraction,
                                "evaluated_share": res["evaluated_share"]}
        if prune_poses is not None:
            metrics["occupancy"].update(prune)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "metrics.json"), "w") as f:
            json.dump(metrics, f, indent=1)
    print(json.dumps({k: metrics[k] for k in ("psnr", "ssim", "views")}))
    return metrics


if __name__ == "__main__":
    main()
