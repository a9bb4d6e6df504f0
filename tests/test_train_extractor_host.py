"""--train-extractor on the host: the trainable set of train.py:105-110 (`lora` in the name), a live feature map from
config.precompute_dino_features(requires_grad=True) whose backward reaches exactly those parameters, and train_cli's argument
checks.  The tiny random-init backbone of tests/test_dino_extractors.py; everything here runs without a GPU."""
import warnings

import pytest
import torch

TINY = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, image_size=56, patch_size=14)


def tiny_extractor(seed=0):
    from nerf_few_shot_limitations_amd import dino_feature_model as F
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # "randomly initialised"
        return F.SpatialDINOFeatures(None, use_lora=True, lora_rank=4, lora_alpha=8, image_size=56, pos_embed_dim=8, config=TINY)


def test_live_map_backpropagates_into_exactly_the_lora_parameters():
    from nerf_few_shot_limitations_amd import config
    ext = tiny_extractor()
    params = config.lora_trainable_parameters(ext)
    names = {n for n, p in ext.named_parameters() if p.requires_grad}
    assert names and all("lora" in n for n in names) and len(params) == len(names) == 2 * 3 * TINY["num_hidden_layers"]
    assert not any(p.requires_grad for n, p in ext.named_parameters() if "lora" not in n)          # feature_proj, pos table: frozen too
    images = torch.rand(2, 56, 56, 3)
    ext.eval()                                                   # LoRA dropout off: the gradients below are deterministic
    maps = config.precompute_dino_features(ext, images, requires_grad=True)
    assert maps.shape == (2, 4, 4, 64) and maps.grad_fn is not None and not ext.training
    maps.backward(torch.randn_like(maps))
    for n, p in ext.named_parameters():
        if "lora_B" in n:
            assert p.grad is not None and p.grad.abs().max() > 0, n
        elif "lora_A" in n:
            assert p.grad is not None and not p.grad.any(), n   # B = 0 at init: nothing reaches A yet
        else:
            assert p.grad is None, n
    # the default call is today's: eval mode, no graph, the mode restored
    ext.train()
    plain = config.precompute_dino_features(ext, images)
    assert plain.grad_fn is None and not plain.requires_grad and ext.training
    # requires_grad=True runs in the CURRENT mode (the trainer puts the extractor in train mode, train.py:246-247)
    assert config.precompute_dino_features(ext, images[:1], requires_grad=True).grad_fn is not None and ext.training
    ext.eval()
    assert torch.equal(config.precompute_dino_features(ext, images, requires_grad=True).detach(), plain)


def test_an_extractor_step_moves_lora_b_and_then_lora_a():
    from nerf_few_shot_limitations_amd import train_cli
    ext = tiny_extractor(1).eval()
    images = torch.rand(1, 56, 56, 3)
    tr = train_cli.ExtractorTrainer(ext, images, lr=1e-2, weight_decay=0.0)
    before = {n: p.detach().clone() for n, p in ext.named_parameters()}
    for _ in range(2):
        m = tr.begin_view(0)
        assert m.shape == (1, 4, 4, 64) and not m.requires_grad and ext.training
        tr.d_map += torch.ones_like(m)
        tr.end_view()
    assert tr.steps == 2 and tr.map is None
    for n, p in ext.named_parameters():
        moved = not torch.equal(p.detach(), before[n])
        assert moved == ("lora" in n), n                        # B in the first step, A (through the now non-zero B) in the second


_CFG = ("experiment: {{name: t}}\ndata: {{near: 2.0, far: 6.0, resolution: 16}}\nmodel: {{use_dino: {dino}{extra}}}\n"
        "nerf_model: {{pos_freq: 12, dir_freq: 4, hidden_dim: 256, num_layers: 8}}\n"
        "optimizer: {{lr: 1.0e-3, weight_decay: 0.0, lr_milestones: [2], lr_gamma: 0.5}}\n"
        "dino_model: {{name: facebook/dinov2-small, lora_rank: 4, lora_alpha: 8, use_lora: {lora}}}\n")


@pytest.mark.parametrize("dino,extra,lora,flags,word", [
    ("true", "", "true", ["--dino-maps", "maps.pt"], "--dino-maps"),
    ("true", "", "true", [], "--dino-weights"),
    ("true", "", "true", ["--dino-random-init", "--data-parallel"], "--data-parallel"),
    ("true", ", dino_model_type: multi_scale", "true", ["--dino-random-init"], "no_grad"),
    ("false", "", "true", ["--dino-random-init"], "use_dino"),
    ("true", "", "false", ["--dino-random-init"], "use_lora"),
])
def test_train_extractor_argument_checks(tmp_path, dino, extra, lora, flags, word):
    from nerf_few_shot_limitations_amd import train_cli
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text(_CFG.format(dino=dino, extra=extra, lora=lora))
    with pytest.raises(SystemExit) as e:                         # decided before the data set is read or a device is touched
        train_cli.main(["--config", str(cfg), "--data", str(tmp_path / "nowhere"), "--train-extractor", *flags])
    assert word in str(e.value), e.value
