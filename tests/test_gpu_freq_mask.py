"""The frequency mask on the positional encodings on the GPU (nerfhip.h: nrf_model_set_freq_mask; NeRFMLP.set_freq_mask;
FusedStep(freq_reg_end=)).

The yardstick throughout is a PRE-SCALED TWIN: model B with no mask whose affected weight columns hold fl32(W m), built here from
model A's weights (NeRFMLP.effective_state_dict, held to the direct product in tests/test_freq_mask_host.py).  B runs the code the
other GPU tests tie to the oracle and the reference; A under the mask must give B's bits on every forward and render route, B's
input gradients, and for the weights fl32(m g_B) on the masked columns and g_B everywhere else.

Shapes: R = 8 rays x S = 5 samples = 40 rows (two 32-row tiles, the second partial), 2 layers of 256, V1 pos_dim 63, V2 pos_freq
10, V3 pos_freq 12 with 64-d features.  Masks: (i) bands {1, 1/2, 0, ...} -- dyadic, tells sin from cos and axis from axis only
through the ids, (ii) a distinct non-dyadic value per column, 0.3 + 0.006 id."""
import ctypes as C
import gc
import json
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests.test_gpu_train_launch_order import DINO_DIM, FAR, NEAR, R, S, Recorder, scene

pytestmark = pytest.mark.gpu

NETS = ("v1", "v2", "v3")
MODES4 = ("bf16", "f16", "f32", "f16x3")
TRAIN_MODES = ("bf16", "f16", "f32")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "freq_mask_launch_order.json")
EINVAL = -1


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def L(N):
    from nerf_few_shot_limitations_amd import _lib as L
    return L


def make(N, net, mode="bf16", seed=11, **kw):
    torch.manual_seed(seed)
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2, mma_mode=mode, **kw)
    elif net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=False, mma_mode=mode, **kw)
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=DINO_DIM, mma_mode=mode, **kw)
    with torch.no_grad():           # a density of about 0.5 everywhere: the default initialisation alone renders black on these rays
        (m.sigma_out if net == "v1" else m.density_mlp.density_head).bias.add_(0.5)
    return m.cuda().train()


def mask_for(N, model, kind):
    """(pos, dirs) of mask (i), (ii) or (iii) for `model` (dirs None for V1)."""
    n_pos, n_dir = model._freq_cols()
    if kind == "i":
        pos, dirs = N.freq_mask_columns(model.pos_freq, 1.5), (N.freq_mask_columns(model.dir_freq, 1.5) if n_dir else None)
        assert pos[3:9].eq(1).all() and pos[9:15].eq(0.5).all() and pos[15:].eq(0).all()
    elif kind == "ii":
        pos = (0.3 + 0.006 * torch.arange(n_pos)).float()
        dirs = (0.3 + 0.006 * (n_pos + torch.arange(n_dir))).float() if n_dir else None
    else:
        pos, dirs = torch.ones(n_pos), (torch.ones(n_dir) if n_dir else None)
    return pos, dirs


def sync_twin(A, B):
    """B <- the masked field of A as plain weights."""
    B.load_state_dict(A.effective_state_dict())
    assert B.freq_mask == (None, None)


def flat_scale(L, model):
    """(n_params,) device vector: the mask value of every flat parameter (1 where it has no scale id)."""
    arr, n, keep = model._host_linears()
    arch = model._arch()
    total = sum(l.weight.numel() + l.bias.numel() for l in model.linears())
    ids = np.empty(total, dtype=np.int8)
    L.check(L.lib().nrf_debug_freq_mask_ids(C.byref(arch), arr, n, ids.ctypes.data_as(C.c_void_p), total, None))
    pos, dirs = model.freq_mask
    n_pos, n_dir = model._freq_cols()
    table = torch.cat([pos if pos is not None else torch.ones(n_pos), dirs if dirs is not None else torch.ones(n_dir), torch.ones(1)])
    idx = torch.from_numpy(ids.astype(np.int64))
    idx[idx < 0] = n_pos + n_dir
    return table[idx].cuda()


def expect_grad(g_b, scale):
    """fl32(m g_B) on the masked columns, g_B everywhere else."""
    return torch.where(scale == 1.0, g_b, g_b * scale)


def field_inputs(N, net, sc, live=False, rows=None):
    """What the module's forward takes, as tests/test_gpu_train_launch_order.py's forward_case builds it."""
    if rows is None:
        pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3).contiguous()
        dirs = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
        feats = (torch.rand(R * S, DINO_DIM, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()
    else:
        g = torch.Generator().manual_seed(17)
        pts = (torch.rand(rows, 3, generator=g) * 4 - 2).cuda()
        dirs = torch.nn.functional.normalize(torch.rand(rows, 3, generator=g) - 0.5, dim=-1).cuda().contiguous()
        feats = (torch.rand(rows, DINO_DIM, generator=g) * 2 - 1).cuda()
    pts, dirs, feats = (t.requires_grad_(live) for t in (pts, dirs, feats))
    if net == "v1":
        enc = N.PositionalEncoding(10)(pts.detach()).contiguous().requires_grad_(live)
        return dict(args=(enc,), kw=dict(points=pts) if live else {}, leaves=(enc, pts))
    if net == "v2":
        return dict(args=(pts, dirs), kw={}, leaves=(pts, dirs))
    return dict(args=(pts, dirs, feats), kw={}, leaves=(pts, dirs, feats))


def out_weights(outs, seed=23):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(o.shape, generator=g) - 0.5).cuda() for o in outs]


def forward_backward(model, inp, gw=None, zero=True):
    """One saving forward + backward of sum(out * gw) through the module: (outputs, flat gradient)."""
    if zero:
        for p in model.parameters():
            p.grad = None
    out = model(*inp["args"], **inp["kw"])
    outs = (out,) if isinstance(out, torch.Tensor) else tuple(out)
    gw = gw if gw is not None else out_weights(outs)
    sum((o * w).sum() for o, w in zip(outs, gw)).backward()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], model._flat_grad.clone()


def same(a, b, what=""):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{what}[{i}]")
    else:
        assert torch.isfinite(a).all(), what
        assert torch.equal(a, b), (what, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------
# 1. forward and render identity
# ---------------------------------------------------------------------------------------------
def routes(N, model, net, sc, mode):
    """Every inference route of `model` in `mode`: {name: tensors}."""
    cam = sc["cam"] if net == "v3" else None
    occ = N.OccupancyGrid.from_mask(torch.rand(8, 8, 32, generator=torch.Generator().manual_seed(2)) > 0.3, -8.0, 8.0).to(torch.device("cuda", 0))
    kw = dict(perturb=True, seed=3, dino=cam, mma_mode=mode)
    inp = field_inputs(N, net, sc)
    out = {}
    with torch.no_grad():
        model.mma_mode = mode
        out["staged"] = model(*inp["args"])
        out["tile"] = N.render_rays(model, sc["o"], sc["d"], NEAR, FAR, S, **kw)
        out["queue"] = N.render_rays(model, sc["o"], sc["d"], NEAR, FAR, S, ert_eps=1e-4, **kw)
        out["grid"] = N.render_rays(model, sc["o"], sc["d"], NEAR, FAR, S, occupancy=occ, **kw)
        if mode in ("bf16", "f16"):
            out["tail"] = N.render_rays(model, sc["o"], sc["d"], NEAR, FAR, S, tail_mode="f16x3", **kw)
        hier = N.render_hierarchical(model, sc["o"], sc["d"], NEAR, FAR, S, 3, perturb=False, reuse_coarse=True, dino=cam, mma_mode=mode)
        out["hier"] = {k: v for k, v in hier.items() if isinstance(v, torch.Tensor)}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("net", NETS)
def test_forward_and_render_identity_with_the_twin(N, net, monkeypatch):
    """A under masks (i) and (ii) against B, all four modes, on the staged forward, render_rays' tile and ray-queue kernels, a render
    under a grid, a tail-mode render and render_hierarchical(reuse_coarse=True).  Pass 1 packs on the host (parameters not in the
    flat vector: nrf_model_create + nrf_model_update under the mask), passes 2 and 3 on the device (the masked re-pack)."""
    from nerf_few_shot_limitations_amd import _lib
    sc = scene()
    A, B = make(N, net).eval(), make(N, net, seed=12).eval()
    plain = None
    for path, kind in (("host", "i"), ("device", "ii"), ("device", "i")):
        if path == "device":
            A.flat_params().ensure(), B.flat_params().ensure()
        A.set_freq_mask(*mask_for(N, A, kind))
        sync_twin(A, B)
        rec = Recorder(_lib.lib())
        for mode in MODES4:
            with monkeypatch.context() as mp:
                mp.setattr(_lib, "_lib", rec)
                a = routes(N, A, net, sc, mode)
            same(a, routes(N, B, net, sc, mode), f"{net} {path} mask ({kind}) {mode}")
        assert ("nrf_model_update_device" in rec.names) == (path == "device"), rec.names
        if plain is None:                       # the mask does something: the unmasked field renders another image
            A.set_freq_mask(None, None)
            plain = routes(N, A, net, sc, "f32")
            assert plain["tile"]["rgb"].abs().min() > 0 and plain["tile"]["weights"].abs().max() > 0
            assert not torch.equal(plain["tile"]["rgb"], a["tile"]["rgb"]) and not torch.equal(plain["staged"][0], a["staged"][0])
    # mask (iii) clears: the raw field, bit for bit
    A.set_freq_mask(*mask_for(N, A, "iii"))
    assert A.freq_mask == (None, None)
    same(routes(N, A, net, sc, "f32"), plain)


# ---------------------------------------------------------------------------------------------
# 2. weight gradients
# ---------------------------------------------------------------------------------------------
CASES2 = [(net, kind, mode) for net in ("v1", "v2") for kind in ("i", "ii") for mode in TRAIN_MODES] + [("v3", "i", mode) for mode in TRAIN_MODES]


def no_subnormal_sums(g):
    nz = g[g != 0]
    return nz.numel() > 0 and float(nz.abs().min()) >= 2.0 ** -120


@pytest.mark.parametrize("net,kind,mode", CASES2)
def test_weight_gradient_is_the_twins_scaled_by_the_mask(N, L, net, kind, mode):
    """From a zeroed gradient vector: g_A = fl32(m g_B) on the masked columns, g_B elsewhere, bit for bit; the saving forward's
    outputs are B's.  V3 under the dyadic mask (i): dino_fusion.fusion.0 receives two scaled adds, and s a + s b = s (a + b) exactly
    for s in {1, 1/2, 0} as long as nothing is subnormal, which is asserted."""
    sc = scene()
    A, B = make(N, net, mode), make(N, net, mode, seed=12)
    A.set_freq_mask(*mask_for(N, A, kind))
    sync_twin(A, B)
    inp = field_inputs(N, net, sc)
    out_a, g_a = forward_backward(A, inp)
    out_b, g_b = forward_backward(B, inp)
    same(out_a, out_b, "saving forward")
    scale = flat_scale(L, A)
    assert (scale != 1).sum() > 0 and g_b[scale != 1].abs().max() > 0
    if net == "v3":
        assert no_subnormal_sums(g_b[scale != 1])
    assert torch.equal(g_a, expect_grad(g_b, scale)), float((g_a - expect_grad(g_b, scale)).abs().max())
    assert torch.all(g_a[scale == 0] == 0)
    if kind == "ii":
        assert not torch.equal(g_a, g_b)


def test_v3_non_dyadic_mask_against_the_oracle(N, L):
    """V3 under mask (ii): two scaled adds into fusion.0 no longer commute with the scale bit for bit, so the yardstick is the
    oracle (float autograd) on B's weights with the scale applied to its gradient, under the bound
    tests/test_gpu_training.py:test_v3_gradients_fp32_mode_match_autograd asserts for this mode and family (rel_to_max < 2e-4, the
    incoming gradient zeroed within MARGIN of a ReLU kink); every parameter but fusion.0's weight still has B's bits."""
    from tests.test_gpu_training import MARGIN, make_v3, rel_to_max, v3_inputs
    n, n_layers = 500, 2
    A, p = make_v3(N, "f32", scene="solid", n_layers=n_layers)
    B, _ = make_v3(N, "f32", scene="solid", n_layers=n_layers)
    A.set_freq_mask(*mask_for(N, A, "ii"))
    sync_twin(A, B)
    p_b = {k: v.detach().cpu().clone() for k, v in A.effective_state_dict().items() if k in p}
    pos, dirs, dino, g_rgb, g_den = v3_inputs(n, 64)
    keep = (O.relu_margin(p_b, "v3", pos, dirs, dino) > MARGIN)[:, None]
    assert keep.float().mean() > 0.85
    g_rgb, g_den = g_rgb * keep, g_den * keep
    inp = dict(args=(pos.cuda(), dirs.cuda(), dino.cuda()), kw={})
    gw = [g_rgb.cuda(), g_den.cuda()]
    _, g_a = forward_backward(A, inp, gw)
    _, g_b = forward_backward(B, inp, gw)
    pp = {k: v.clone().requires_grad_(True) for k, v in p_b.items()}
    o_rgb, o_den = O.mlp_v3(pp, pos, dirs, dino)
    ((o_rgb * g_rgb).sum() + (o_den * g_den).sum()).backward()
    scale = flat_scale(L, A)
    fp = A.flat_params()
    names = {id(q): k for k, q in A.named_parameters()}
    checked = 0
    for q, off in zip(fp.params(), fp.offsets):
        name, sl = names[id(q)], slice(off, off + q.numel())
        want = pp[name].grad.reshape(-1) * scale[sl].cpu()
        e = rel_to_max(g_a[sl], want)
        print(f"{name}: {e / 2e-4:.3f} of 2e-4")
        assert e < 2e-4, (name, e)
        if name != "dino_fusion.fusion.0.weight":
            assert torch.equal(g_a[sl], expect_grad(g_b[sl], scale[sl])), name
        checked += 1
    assert checked == 2 * (n_layers + 10)


def reduce_blocks(L, model, mode, n):
    """Partial blocks per weight-gradient job at n rows: train_impl.hpp's wgrad_grid on the plan the library reports."""
    arr, nl, keep = model._host_linears()
    arch = model._arch()
    cnt = C.c_int64()
    L.check(L.lib().nrf_debug_train_plan(C.byref(arch), arr, nl, None, 0, C.byref(cnt)))
    buf = np.zeros(cnt.value, np.int32)
    L.check(L.lib().nrf_debug_train_plan(C.byref(arch), arr, nl, buf.ctypes.data_as(C.c_void_p), cnt.value, None))
    it = iter(buf.tolist())
    for _ in range(next(it)):
        next(it)
    costs = []
    for _ in range(next(it)):
        _, _, KT, MT, _ = (next(it) for _ in range(5))
        for _ in range(2 * 32 * MT + 32 * KT):
            next(it)
        costs.append(max(KT + MT, 10))
    tiles32 = (n + 255) // 256 * 8
    ST = 1 if mode == "f32" else 2
    max_splits = max(1, -(-tiles32 // (4 * ST)))
    budget = (2 if tiles32 >= 8192 else 1) * torch.cuda.get_device_properties(0).multi_processor_count
    return [max(1, min(budget * c // sum(costs), max_splits)) for c in costs]


def test_reduce_runs_its_three_load_group_forms(N, L):
    """21 x 256 rows in bf16: wgrad_grid caps every job at 21 slabs, so the masked reduce sums 16 + 4 + 1 partial blocks per
    weight -- the three copied summation loops -- and the bias rows 16 + 5 x 1."""
    net, mode, n = "v1", "bf16", 21 * 256
    A, B = make(N, net, mode), make(N, net, mode, seed=12)
    blocks = reduce_blocks(L, A, mode, n)
    print("partial blocks per job:", blocks)
    assert blocks[0] >= 16 and blocks[0] % 16 >= 4 and blocks[0] % 4 >= 1
    A.set_freq_mask(*mask_for(N, A, "ii"))
    sync_twin(A, B)
    inp = field_inputs(N, net, None, rows=n)
    out_a, g_a = forward_backward(A, inp)
    out_b, g_b = forward_backward(B, inp)
    same(out_a, out_b)
    scale = flat_scale(L, A)
    assert torch.equal(g_a, expect_grad(g_b, scale)) and not torch.equal(g_a, g_b)


def test_two_backwards_add_two_scaled_contributions(N, L):
    """The gradient vector accumulates across calls: backward twice gives fl(fl(m g1) + fl(m g2)), not m fl(g1 + g2)."""
    net, mode = "v2", "f32"
    sc = scene()
    A, B = make(N, net, mode), make(N, net, mode, seed=12)
    A.set_freq_mask(*mask_for(N, A, "ii"))
    sync_twin(A, B)
    inp = field_inputs(N, net, sc)
    gw1, gw2 = out_weights([torch.empty(R * S, 3), torch.empty(R * S, 1)], 31), out_weights([torch.empty(R * S, 3), torch.empty(R * S, 1)], 32)
    _, g1 = forward_backward(B, inp, gw1)
    _, g2 = forward_backward(B, inp, gw2)
    forward_backward(A, inp, gw1)
    _, g_a = forward_backward(A, inp, gw2, zero=False)
    scale = flat_scale(L, A)
    want = expect_grad(g1, scale) + expect_grad(g2, scale)
    assert torch.equal(g_a, want), float((g_a - want).abs().max())
    assert not torch.equal(want, expect_grad(g1 + g2, scale))          # the other order of scaling and adding is another number


# ---------------------------------------------------------------------------------------------
# 3. input gradients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,kind,mode", [(net, kind, mode) for net in NETS for kind in ("i", "ii") for mode in ("bf16", "f32")])
def test_input_gradients_are_the_twins(N, net, kind, mode):
    """d points / d dirs (V1 also d x_encoded, V3 also d features) of A equal B's bit for bit: the transposed tiles ride in the
    re-packed backward stream."""
    sc = scene()
    kw = {"point_grad": True} if net == "v3" else {"input_grad": True}
    A, B = make(N, net, mode, **kw), make(N, net, mode, seed=12, **kw)
    A.set_freq_mask(*mask_for(N, A, kind))
    sync_twin(A, B)
    grads = []
    for model in (A, B):
        inp = field_inputs(N, net, sc, live=True)
        forward_backward(model, inp)
        assert all(t.grad is not None and t.grad.abs().max() > 0 for t in inp["leaves"])
        grads.append([t.grad.clone() for t in inp["leaves"]])
    same(grads[0], grads[1], f"{net} ({kind}) {mode}")


# ---------------------------------------------------------------------------------------------
# 4. steps
# ---------------------------------------------------------------------------------------------
def step_call(N, net, sc):
    inp = field_inputs(N, net, sc)
    kw = {}
    if net != "v1":
        kw["dirs"] = inp["args"][1]
    if net == "v3":
        kw["dino"] = inp["args"][2]
    return lambda step: step(inp["args"][0], sc["z"], sc["d"], sc["target"], **kw)


def moments_of(g, b1=0.9, b2=0.999):
    """Adam's first step from zero moments, in adam_kernel's fp32 operations."""
    one = torch.tensor(1.0)
    c1, c2 = (one - torch.tensor(b1, dtype=torch.float32)).item(), (one - torch.tensor(b2, dtype=torch.float32)).item()
    return g * torch.tensor(c1, dtype=torch.float32, device=g.device), (g * torch.tensor(c2, dtype=torch.float32, device=g.device)) * g


@pytest.mark.parametrize("net", NETS)
def test_one_fused_step_under_a_fixed_mask_equals_the_twins(N, L, net):
    """Same loss bits; gradient and Adam moments by the rule of test 2."""
    sc = scene()
    A, B = make(N, net), make(N, net, seed=12)
    A.set_freq_mask(*mask_for(N, A, "i" if net == "v3" else "ii"))
    sync_twin(A, B)
    sa, sb = N.FusedStep(A, lr=1e-3), N.FusedStep(B, lr=1e-3)
    run = step_call(N, net, sc)
    la, lb = run(sa), run(sb)
    torch.cuda.synchronize()
    assert torch.isfinite(la) and torch.equal(la, lb)
    scale = flat_scale(L, A)
    assert torch.equal(sa.grad, expect_grad(sb.grad, scale))
    m1, m2 = moments_of(sa.grad)
    assert torch.equal(sa.opt.exp_avg, m1) and torch.equal(sa.opt.exp_avg_sq, m2)
    assert torch.equal(sa.opt.exp_avg[scale == 1], sb.opt.exp_avg[scale == 1]) and torch.equal(sa.opt.exp_avg_sq[scale == 1], sb.opt.exp_avg_sq[scale == 1])
    assert A.freq_mask[0] is not None                          # freq_reg_end = 0 leaves a hand-set mask alone


def test_columns_hidden_throughout_keep_their_bits(N, L):
    """3 steps of FusedStep(freq_reg_end=) with weight_decay = 0: a column hidden in all of them has its initial bits and zero
    moments; the visible ones moved."""
    sc = scene()
    A = make(N, "v2")
    step = N.FusedStep(A, lr=1e-3, freq_reg_end=1000)
    w0 = A.flat_params().ensure().clone()
    for i in range(3):
        step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=3 + i)
    torch.cuda.synchronize()
    assert step.opt.step_count == 3
    scale = flat_scale(L, A)                                    # the mask of the last step, the most open of the three
    want_pos = N.freq_mask_columns(10, N.freq_mask_visible(2, 1000, 10))
    assert torch.equal(A.freq_mask[0], want_pos) and torch.equal(A.freq_mask[1], N.freq_mask_columns(4, N.freq_mask_visible(2, 1000, 4)))
    hidden, open_ = scale == 0, scale == 1
    assert hidden.sum() == 256 * 48 + 128 * 12
    flat = A.flat_params().flat
    assert torch.equal(flat[hidden], w0[hidden])
    assert torch.all(step.opt.exp_avg[hidden] == 0) and torch.all(step.opt.exp_avg_sq[hidden] == 0)
    assert (flat[open_] != w0[open_]).float().mean() > 0.1
    partly = (scale > 0) & (scale < 1)
    assert partly.sum() == 256 * 6 + 128 * 6 and (flat[partly] != w0[partly]).any()


def route_runs(N, sc):
    """name -> (FusedStep keywords, mask kind, run(step)) of the routes of test 4, on V2 at the smallest shape each accepts."""
    ray = lambda **kw: (lambda step: step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=3, **kw))
    ones = lambda: N.OccupancyGrid.full((32, 8, 8), -8.0, 8.0, device="cuda")
    return {
        "rays": ({}, "ii", ray()),
        "grid-staged": ({}, "ii", ray(occupancy=ones(), grid_inputs="staged")),
        "grid-rays": ({}, "ii", ray(occupancy=ones(), grid_inputs="rays")),
        # two backward calls into one vector: the dyadic mask
        "hier": ({}, "i", lambda step: step.step_rays_hierarchical(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, 3, perturb=False)),
        "multi": (dict(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True, weight_decay=1e-2, seed=4), "ii", ray()),
    }


@pytest.mark.parametrize("route", ["rays", "grid-staged", "grid-rays", "hier", "multi"])
def test_every_fused_route_under_a_mask_equals_the_twins(N, L, route):
    sc = scene()
    kw, kind, run = route_runs(N, sc)[route]
    A, B = make(N, "v2"), make(N, "v2", seed=12)
    A.set_freq_mask(*mask_for(N, A, kind))
    sync_twin(A, B)
    sa, sb = N.FusedStep(A, lr=1e-3, **kw), N.FusedStep(B, lr=1e-3, **kw)
    la, lb = run(sa), run(sb)
    torch.cuda.synchronize()
    assert torch.isfinite(la) and torch.equal(la, lb)
    same({k: v for k, v in sa.last_losses.items()}, {k: v for k, v in sb.last_losses.items()}, route)
    scale = flat_scale(L, A)
    if route == "hier":
        assert no_subnormal_sums(sb.grad[scale != 1])
    assert sb.grad.abs().max() > 0 and torch.equal(sa.grad, expect_grad(sb.grad, scale))


def test_autograd_route_under_a_mask_equals_the_twins(N, L):
    """render_rays in train mode under grad + training.Adam."""
    from nerf_few_shot_limitations_amd.training import Adam
    sc = scene()
    A, B = make(N, "v2"), make(N, "v2", seed=12)
    A.set_freq_mask(*mask_for(N, A, "ii"))
    sync_twin(A, B)
    outs, opts = [], []
    for model in (A, B):
        opt = Adam(model, lr=1e-3)
        opt.zero_grad()
        out = N.render_rays(model, sc["o"], sc["d"], NEAR, FAR, S, perturb=True, seed=3)
        ((out["rgb"] - sc["target"]) ** 2).mean().backward()
        outs.append({k: v.detach().clone() for k, v in out.items()})
        grad = model._flat_grad.clone()
        opt.step()
        opts.append((grad, opt))
    torch.cuda.synchronize()
    same(outs[0], outs[1])
    scale = flat_scale(L, A)
    assert torch.equal(opts[0][0], expect_grad(opts[1][0], scale))
    m1, m2 = moments_of(opts[0][0])
    assert torch.equal(opts[0][1].exp_avg, m1) and torch.equal(opts[0][1].exp_avg_sq, m2)
    # the next forward packs the updated raw weights under the same mask
    A_next = N.render_rays(A, sc["o"], sc["d"], NEAR, FAR, S, perturb=True, seed=3)
    sync_twin(A, B)
    B_next = N.render_rays(B, sc["o"], sc["d"], NEAR, FAR, S, perturb=True, seed=3)
    same({k: v.detach() for k, v in A_next.items()}, {k: v.detach() for k, v in B_next.items()})


@pytest.mark.parametrize("end", [0, 4])
def test_without_a_mask_the_step_is_the_plain_step(N, end, monkeypatch):
    """freq_reg_end = 0, and freq_reg_end = 4 from step 4 on (all 10 bands visible from 4 x 9 / 10 = 3.6): the plain step's calls,
    loss bits and parameters."""
    from nerf_few_shot_limitations_amd import _lib
    sc = scene()
    P, A = make(N, "v2"), make(N, "v2")
    sp, sa = N.FusedStep(P, lr=1e-3), N.FusedStep(A, lr=1e-3, freq_reg_end=end)
    sp.opt.step_count = sa.opt.step_count = 4
    names = []
    for step in (sp, sa):
        rec = Recorder(_lib.lib())
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "_lib", rec)
            losses = [step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=3 + i) for i in range(2)]
        torch.cuda.synchronize()
        names.append((rec.names, losses))
    assert names[0][0] == names[1][0] and "nrf_model_set_freq_mask" not in names[1][0]
    same(names[0][1], names[1][1])
    assert torch.equal(P.flat_params().flat, A.flat_params().flat) and A.freq_mask == (None, None)


# ---------------------------------------------------------------------------------------------
# 5. mask currency
# ---------------------------------------------------------------------------------------------
def test_raw_backward_is_refused_after_a_new_mask_until_the_mode_is_repacked(N, L):
    from nerf_few_shot_limitations_amd.training import _train_handle
    lib, st, dev = L.lib(), L.stream_ptr(), torch.device("cuda", 0)
    A = make(N, "v1")
    h, mode = _train_handle(A, dev)
    n = R * S
    x = field_inputs(N, "v1", scene())["args"][0]
    nbytes = lib.nrf_train_context_bytes(h, mode, n)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cb = C.c_void_p(buf.data_ptr())
    out, g, grad = torch.empty(n, 4, device=dev), torch.ones(n, 4, device=dev), torch.zeros(A.flat_params().flat.numel(), device=dev)
    backward = lambda: lib.nrf_mlp_backward_v1(h, mode, L.ptr(out), L.ptr(g), n, cb, nbytes, L.ptr(grad), st)
    L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(x), n, L.ptr(out), cb, nbytes, st))
    assert backward() == 0
    pos = (C.c_float * 63)(*mask_for(N, A, "ii")[0].tolist())
    active = C.c_int(-1)
    L.check(lib.nrf_model_set_freq_mask(h, pos, None))
    L.check(lib.nrf_model_get_freq_mask(h, None, None, C.byref(active)))
    assert active.value == 1
    assert backward() == EINVAL and b"older" in lib.nrf_last_error()
    L.check(lib.nrf_model_set_freq_mask(h, pos, None))                  # the recorded mask again: nothing changes, still stale
    assert backward() == EINVAL
    L.check(lib.nrf_model_update_device(h, L.ptr(A.flat_params().flat), 1 << mode, st))
    L.check(lib.nrf_mlp_forward_train_v1(h, mode, L.ptr(x), n, L.ptr(out), cb, nbytes, st))
    assert backward() == 0
    back = (C.c_float * 63)()
    L.check(lib.nrf_model_get_freq_mask(h, back, None, C.byref(active)))
    assert list(back) == list(pos)
    one = (C.c_float * 63)(*([1.0] * 63))
    L.check(lib.nrf_model_set_freq_mask(h, one, None))                  # all ones clears, and is a change
    L.check(lib.nrf_model_get_freq_mask(h, None, None, C.byref(active)))
    assert active.value == 0 and backward() == EINVAL
    bad = (C.c_float * 63)(*([1.0] * 62 + [1.5]))
    assert lib.nrf_model_set_freq_mask(h, bad, None) == EINVAL
    bad[62] = float("nan")
    assert lib.nrf_model_set_freq_mask(h, bad, None) == EINVAL
    assert lib.nrf_model_set_freq_mask(h, None, one) == EINVAL          # V1 reads no direction encoding
    torch.cuda.synchronize()
    A._gen += 1                                                          # the module's bookkeeping: the handle was changed behind its back


def test_a_new_mask_between_forward_and_backward_is_refused(N):
    sc = scene()
    A = make(N, "v2")
    A.set_freq_mask(*mask_for(N, A, "i"))
    inp = field_inputs(N, "v2", sc)
    rgb, den = A(*inp["args"])
    A.set_freq_mask(*mask_for(N, A, "ii"))
    with pytest.raises(RuntimeError, match="between forward and backward"):
        (rgb.sum() + den.sum()).backward()
    torch.cuda.synchronize()


def test_a_render_in_a_second_mode_after_a_masked_step_sees_the_mask(N):
    sc = scene()
    A, B = make(N, "v2"), make(N, "v2", seed=12)
    A.set_freq_mask(*mask_for(N, A, "ii"))
    step = N.FusedStep(A, lr=1e-2)
    step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=3)
    sync_twin(A, B)
    with torch.no_grad():
        for mode in ("f16", "f16x3"):
            a = N.render_rays(A, sc["o"], sc["d"], NEAR, FAR, S, mma_mode=mode)
            b = N.render_rays(B, sc["o"], sc["d"], NEAR, FAR, S, mma_mode=mode)
            same(a, b, mode)
    # and the next step still finds its own mode's backward weights current
    step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=4)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 6. call sequence
# ---------------------------------------------------------------------------------------------
SEQ_ROUTES = ("call", "rays", "grid", "hier")


def record_step(N, route, masked, monkeypatch):
    """The nrf_* calls of one FusedStep step on V2 behind a warm-up step; masked: freq_reg_end so large that every step has a new mask."""
    from nerf_few_shot_limitations_amd import _lib
    sc = scene()
    A = make(N, "v2")
    step = N.FusedStep(A, lr=1e-3, **({"freq_reg_end": 100000} if masked else {}))
    runs = route_runs(N, sc)
    run = {"call": step_call(N, "v2", sc), "rays": runs["rays"][2], "grid": runs["grid-staged"][2], "hier": runs["hier"][2]}[route]
    run(step)
    torch.cuda.synchronize()
    gc.collect()
    rec = Recorder(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", rec)
        run(step)
    torch.cuda.synchronize()
    return rec.names


@pytest.mark.parametrize("route", SEQ_ROUTES)
def test_masked_step_is_the_plain_steps_calls_behind_the_setter(N, route, monkeypatch):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert sorted(gold) == sorted(SEQ_ROUTES)
    plain, masked = record_step(N, route, False, monkeypatch), record_step(N, route, True, monkeypatch)
    print(route, masked)
    assert masked == ["nrf_model_set_freq_mask"] + plain
    assert masked == gold[route]
