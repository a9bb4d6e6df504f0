"""The sequence of library calls every training route makes, pinned to a recording.

The numeric tests hold every route's results to the bit; none of them sees an extra, a missing or a reordered launch, and at the
reference's batch sizes the step is bound by the host path between the launches.  Here `_lib._lib` is replaced by a proxy that
records the name of every nrf_* function called and forwards the call; each route runs once after a warm-up call (first-use
packing, plans and cached workspaces are not in the list) and the recorded names are compared with
tests/golden/train_launch_order.json.

That file was recorded with this module's own `record` at commit 988f478 ("Test weight currency against a fresh twin; let every
fresh mode ride"), the parent of the commit that gave training.py one copy of each launch sequence: the test passes at that
parent and after it with the same file.  It holds only lists of names per case."""
import gc
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

R, S = 8, 5
N_LAYERS = 2                      # the smallest depth the GPU tests of each family use (hidden 256 everywhere)
DINO_DIM, MAP = 64, 9
NEAR, FAR = 2.0, 6.0
H = W = 8
FOCAL = 8.0
NETS = ("v1", "v2", "v3")
MULTI = dict(reg_weight=1e-4, noise_std=0.1, max_grad_norm=1.0, decoupled_weight_decay=True)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_launch_order.json")


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


class Recorder:
    """Stands in for the loaded library: forwards everything, keeps the names of the nrf_* calls."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nrf_"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def make(N, net, **kw):
    if net == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=N_LAYERS, mma_mode="bf16", **kw)
    elif net == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=4, hidden_dim=256, num_density_layers=N_LAYERS, use_dino=False, mma_mode="bf16", **kw)
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=N_LAYERS, use_dino=True, dino_dim=DINO_DIM, mma_mode="bf16", **kw)
    return m.cuda().train()


def scene():
    g = torch.Generator().manual_seed(5)
    u = lambda *shape: torch.rand(*shape, generator=g)
    o = (u(R, 3) * 0.4 - 0.2).cuda()
    d = torch.nn.functional.normalize(u(R, 3) - 0.5, dim=-1).cuda().contiguous()
    z = (NEAR + (FAR - NEAR) * (torch.arange(S) + 0.5) / S).expand(R, S).contiguous().cuda()
    pose = torch.eye(4)
    pose[2, 3] = 4.0
    src = pose.clone()
    src[0, 3] = 0.3
    return dict(o=o, d=d, z=z, target=u(R, 3).cuda(), noise=torch.randn(R, S, generator=g).cuda(), pose=pose,
                image=u(H, W, 3).cuda(), pixels=torch.arange(R, dtype=torch.int64, device="cuda") * 3,
                cam=dict(features=(u(1, MAP, MAP, DINO_DIM) * 2 - 1).cuda(), pose=src, focal=FOCAL, H=H, W=W))


def grid(N, kind):
    if kind == "ones":
        return N.OccupancyGrid.full((32, 8, 8), -8.0, 8.0, device="cuda")
    return N.OccupancyGrid.from_mask(torch.zeros(8, 8, 32, dtype=torch.bool), -8.0, 8.0).to(torch.device("cuda", 0))


def fused_case(net, route, multi=False, occupancy=None, d_dino_out=False):
    def build(N):
        sc = scene()
        model = make(N, net, **({"dino_grad": True} if d_dino_out else {}))
        step = N.FusedStep(model, lr=1e-3, **(MULTI if multi else {}))
        kw = {"noise": sc["noise"]} if multi else {}
        if occupancy is not None:
            kw["occupancy"] = grid(N, occupancy)
        if route == "call":
            pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3)
            if net == "v1":
                pts = N.PositionalEncoding(10)(pts)
            else:
                kw["dirs"] = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
            if net == "v3":
                kw["dino"] = torch.rand(R * S, DINO_DIM, generator=torch.Generator().manual_seed(6)).cuda()
            if d_dino_out:
                kw["d_dino_out"] = torch.empty(R * S, DINO_DIM, device="cuda")
            return lambda: step(pts, sc["z"], sc["d"], sc["target"], **kw)
        if net == "v3":
            kw["dino"] = sc["cam"]
        if route == "rays":
            return lambda: step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=3, **kw)
        return lambda: step.step_view(sc["image"], sc["pose"], H, W, FOCAL, sc["pixels"], NEAR, FAR, S, perturb=True, seed=3, **kw)
    return build


def forward_case(net, live):
    """model(x) + backward(): _MLPV1Fn / _MLPV2Fn, with or without inputs that require grad."""
    def build(N):
        sc = scene()
        model = make(N, net, **({} if not live else {"point_grad": True} if net == "v3" else {"input_grad": True}))
        pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3).contiguous().requires_grad_(live)
        dirs = sc["d"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous().requires_grad_(live)
        enc = N.PositionalEncoding(10)(pts.detach()).contiguous().requires_grad_(live)
        feats = torch.rand(R * S, DINO_DIM, generator=torch.Generator().manual_seed(6)).cuda().requires_grad_(live)

        def run():
            if net == "v1":
                model(enc, points=pts if live else None).sum().backward()
            else:
                rgb, den = model(pts, dirs, feats if net == "v3" else None)
                (rgb.sum() + den.sum()).backward()
        return run
    return build


def render_case(net, live_rays=False, live_map=False):
    """render_rays + backward(): _RenderFn (rays as data), _RenderGeomFn / _RenderPointFn (rays and depths that require grad)."""
    def build(N):
        sc = scene()
        kw = {}
        if live_rays:
            kw["point_grad" if net == "v3" else "input_grad"] = True
        if live_map:
            kw["dino_grad"] = True
        model = make(N, net, **kw)
        o, d, z = (sc[k].clone().requires_grad_(live_rays) for k in ("o", "d", "z"))
        cam = dict(sc["cam"], features=sc["cam"]["features"].clone().requires_grad_(live_map)) if net == "v3" else None

        def run():
            out = N.render_rays(model, o, d, NEAR, FAR, S, perturb=True, seed=3, dino=cam, z_in=z if live_rays else None)
            (out["rgb"].sum() + out["depth"].sum()).backward()
        return run
    return build


def normals_case(net):
    def build(N):
        sc = scene()
        model = make(N, net, **({"point_grad": True} if net == "v3" else {"input_grad": True}))
        pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3).contiguous()
        return lambda: N.density_normals(model, pts, dino=sc["cam"] if net == "v3" else None)
    return build


CASES = {}
for _net in NETS:
    for _form, _multi in (("plain", False), ("multi", True)):
        for _route in ("call", "rays", "view"):
            CASES[f"{_net}-{_route}-{_form}"] = fused_case(_net, _route, _multi)
        CASES[f"{_net}-rays-grid-ones-{_form}"] = fused_case(_net, "rays", _multi, occupancy="ones")
    CASES[f"{_net}-rays-grid-zeros"] = fused_case(_net, "rays", occupancy="zeros")
    CASES[f"{_net}-forward"] = forward_case(_net, False)
    CASES[f"{_net}-forward-live-inputs"] = forward_case(_net, True)
    CASES[f"{_net}-render"] = render_case(_net)
    CASES[f"{_net}-render-live-rays"] = render_case(_net, live_rays=True)
    CASES[f"{_net}-normals"] = normals_case(_net)
CASES["v3-call-d-dino-out"] = fused_case("v3", "call", d_dino_out=True)
CASES["v3-render-live-map"] = render_case("v3", live_map=True)
CASES["v3-render-live-rays-live-map"] = render_case("v3", live_rays=True, live_map=True)


def record(N, name, monkeypatch):
    """The names of the nrf_* calls of one run of case `name`, behind a warm-up run."""
    from nerf_few_shot_limitations_amd import _lib
    run = CASES[name](N)
    run()
    torch.cuda.synchronize()
    gc.collect()                  # an earlier case's module that dies inside the recording would add its nrf_model_destroy
    rec = Recorder(_lib.lib())
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_lib", rec)
        run()
    torch.cuda.synchronize()
    return rec.names


@pytest.fixture(scope="module")
def recorded():
    """The recording, read once; without the file every test of the module reports this one line."""
    if not os.path.exists(GOLDEN):
        pytest.fail("tests/golden/train_launch_order.json is missing: there is no recording to compare with", pytrace=False)
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_order_is_the_recorded_one(N, name, recorded, monkeypatch):
    want = recorded[name]
    assert len(want) > 0
    assert record(N, name, monkeypatch) == want
