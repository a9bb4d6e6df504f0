"""Every library call a FusedStep makes, with its arguments, pinned to a recording: tests/test_gpu_train_launch_order.py taken one
step further.

The launch-order test sees an extra, a missing or a reordered launch; it does not see a wrong argument, and it runs only the plain
and the multi-term step.  Here the proxy that stands in for `_lib._lib` also keeps what every nrf_* call was handed, classified by the
entry's argtypes in `_lib.SIGNATURES`: integers as they are, floats as float.hex() of the value rounded through c_float / c_double,
pointers as "null" or "ptr" (never the address, nor which buffer it belongs to: the caching allocator may hand a temporary another
block), a struct passed by reference (or reached through a pointer field: nrf_render_opts.dino) as the dict of its fields under the
same rules, c_float / c_int32 arrays as lists.  tests/test_fused_step_transcript_host.py rehearses the recorder without a GPU.

Each case builds its FusedStep under torch.manual_seed(0), runs once as a warm-up (first-use packing and every buffer set), and its
second run is the one recorded.  The cases cover every route (call, rays, view, the two hierarchical ones) with the ray-regulariser,
patch, information, frequency-mask, occupancy (staged and rays inputs), d_dino_out / points_out and target_depth options, and a
plain and a hierarchical step taken in turn on one object (the buffer hand-over).  step_view refuses a step object with the patch
term or kl_weight, so under a grid the view route runs the ray-regulariser kind and the information kind with ent_weight alone.

Next to the transcript a case stores SHA-256 digests of `pred`, of the values of `last_losses` (with their names) and, where the step
leaves them, of pred_coarse, last_z, last_patch_depth, last_weights and last_z_new -- taken behind the FIRST step of the fresh object, before any
update has touched the weights (the forward, the compositor and the loss launches use no atomics; the weight gradients do, so
parameters and gradients are not digested).  A digest is in the file only if two recordings made in two separate processes agreed on
it.  Dropped: none -- both recordings agreed on every digest of every case.

tests/golden/fused_step_transcript.json was recorded with this module's own

    python -m tests.test_gpu_fused_step_transcript record A.json        (twice, two processes)
    python -m tests.test_gpu_fused_step_transcript merge A.json B.json tests/golden/fused_step_transcript.json

at commit 9a40b7c ("Loss launches: one batch walk, one finish body, one argument block"), the parent of the commit that gave
FusedStep one loss plan, one ray front end and one buffer cache: the test passes at that parent and after it with the same file."""
import ctypes as C
import gc
import hashlib
import json
import os
import sys

import pytest
import torch

from tests.test_gpu_train_launch_order import DINO_DIM, FAR, FOCAL, H, MULTI, NEAR, NETS, R, S, W, grid, make, scene

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_step_transcript.json")
PATCH, N_PATCHES = 2, 2                     # the smallest legal patch: 2 * 2 * 2 = 8 patch rays behind the 8 supervised ones
N_IMPORTANCE = 3
SEED = 7                                    # FusedStep(seed=): no seed of a transcript comes from fresh_seed()
KEPT = ("pred", "pred_coarse", "last_z", "last_patch_depth", "last_weights", "last_z_new")


# ---- the recorder ------------------------------------------------------------------------------------------------------------------
def _struct(s):
    return {name: encode(ftype, getattr(s, name)) for name, ftype in s._fields_}


def encode(argtype, v):
    """One argument (or struct field) as the golden file holds it; argtype is its ctypes type from the signature."""
    if isinstance(v, C._SimpleCData) and not isinstance(v, (C.c_void_p, C.c_char_p)):
        v = v.value
    if issubclass(argtype, C._Pointer):
        if v is None or (isinstance(v, C._Pointer) and not v):
            return "null"
        target = v._obj if hasattr(v, "_obj") else v.contents if isinstance(v, C._Pointer) else v      # byref() | pointer() | the object
        return _struct(target) if isinstance(target, C.Structure) else "ptr"
    if issubclass(argtype, (C.c_void_p, C.c_char_p)):
        if isinstance(v, (C.c_void_p, C.c_char_p)):
            v = v.value
        return "ptr" if v else "null"
    if issubclass(argtype, C.Array):
        return [encode(argtype._type_, x) for x in v]
    if issubclass(argtype, C.Structure):
        return _struct(v)
    if issubclass(argtype, (C.c_float, C.c_double)):
        return argtype(v).value.hex()
    return int(argtype(v).value)            # the integer kinds, wrapped as the library receives them


class Transcript:
    """Stands in for the loaded library: forwards everything, keeps [name, argument, ...] of the nrf_* calls."""

    def __init__(self, lib, signatures):
        self._lib, self._signatures, self.calls = lib, signatures, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("nrf_"):
            return fn
        argtypes = self._signatures[name][1]

        def call(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
            self.calls.append([name] + [encode(t, a) for t, a in zip(argtypes, args)])
            return fn(*args)
        return call


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def patch_scene(sc):
    """The scene with 8 patch rays behind its 8 supervised ones (any rays will do: nothing here looks at the image)."""
    g = torch.Generator().manual_seed(11)
    o_p = (torch.rand(N_PATCHES * PATCH * PATCH, 3, generator=g) * 0.4 - 0.2).cuda()
    d_p = torch.nn.functional.normalize(torch.rand(N_PATCHES * PATCH * PATCH, 3, generator=g) - 0.5, dim=-1).cuda().contiguous()
    o, d = torch.cat([sc["o"], o_p]).contiguous(), torch.cat([sc["d"], d_p]).contiguous()
    return dict(sc, o=o, d=d, z=sc["z"][:1].expand(o.shape[0], S).contiguous())


def case(net, route, ctor=None, multi=False, occupancy=None, grid_inputs=None, patches=False, outputs=False, target_depth=False,
         then=None):
    """build(N) -> (step, [closures]): one closure per step of the case, in order.  route: call | rays | view | rays-hier | view-hier;
    then: the route of a second step on the same object."""
    def build(N):
        sc = scene()
        if patches:
            sc = patch_scene(sc)
        n_rays = sc["o"].shape[0]
        model = make(N, net, **({"dino_grad": True} if outputs else {}))
        step = N.FusedStep(model, lr=1e-3, seed=SEED, **dict(MULTI if multi else {}, **(ctor or {})))
        kw = {"noise": sc["noise"]} if multi else {}
        if patches:
            kw["n_patches"] = N_PATCHES
        if target_depth:
            kw["target_depth"] = torch.rand(R, generator=torch.Generator().manual_seed(12)).cuda() * (FAR - NEAR) + NEAR
        if outputs:
            kw["d_dino_out"] = torch.empty(n_rays * S, DINO_DIM, device="cuda")
        gkw = {}
        if occupancy is not None:
            gkw = dict(occupancy=grid(N, occupancy), grid_inputs=grid_inputs or "staged")
        cam = {"dino": sc["cam"]} if net == "v3" else {}

        def one(route):
            if route == "call":
                ckw = dict(kw)
                pts = (sc["o"][:, None, :] + sc["d"][:, None, :] * sc["z"][:, :, None]).reshape(-1, 3)
                if net == "v1":
                    pts = N.PositionalEncoding(10)(pts)
                else:
                    ckw["dirs"] = sc["d"][:, None, :].expand(n_rays, S, 3).reshape(-1, 3).contiguous()
                if net == "v3":
                    ckw["dino"] = torch.rand(n_rays * S, DINO_DIM, generator=torch.Generator().manual_seed(6)).cuda()
                return lambda: step(pts, sc["z"], sc["d"], sc["target"], **ckw)
            if route == "rays":
                rkw = dict(kw, **gkw, **cam)
                if outputs:
                    rkw["points_out"] = torch.empty(n_rays * S, 3, device="cuda")
                return lambda: step.step_rays(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, perturb=True, seed=3, **rkw)
            if route == "view":
                return lambda: step.step_view(sc["image"], sc["pose"], H, W, FOCAL, sc["pixels"], NEAR, FAR, S, perturb=True, seed=3,
                                              **dict(kw, **gkw, **cam))
            if route == "rays-hier":
                return lambda: step.step_rays_hierarchical(sc["o"], sc["d"], sc["target"], NEAR, FAR, S, N_IMPORTANCE, perturb=True, seed=3, **cam)
            assert route == "view-hier"
            return lambda: step.step_view_hierarchical(sc["image"], sc["pose"], H, W, FOCAL, sc["pixels"], NEAR, FAR, S, N_IMPORTANCE,
                                                       perturb=True, seed=3, **cam)
        return step, [one(route)] + ([one(then)] if then else [])
    return build


REG = dict(dist_weight=1e-2, occ_weight=1e-2, occ_samples=2)
SMOOTH = dict(depth_smooth_weight=0.1, patch_size=PATCH)
INFO = dict(ent_weight=1e-3, ent_threshold=0.01, kl_weight=1e-5, patch_size=PATCH)
ENT = dict(ent_weight=1e-3, ent_threshold=0.01)

CASES = {}
for _net in NETS:
    for _route in ("call", "rays", "view"):
        CASES[f"{_net}-{_route}-plain"] = case(_net, _route)
        CASES[f"{_net}-{_route}-multi"] = case(_net, _route, multi=True)
    for _route in ("rays", "view"):
        CASES[f"{_net}-{_route}-reg"] = case(_net, _route, REG)
        CASES[f"{_net}-{_route}-hier"] = case(_net, _route + "-hier")
    CASES[f"{_net}-call-dist-span"] = case(_net, "call", dict(dist_weight=1e-2, dist_span=FAR - NEAR))
    for _route in ("rays", "call"):
        CASES[f"{_net}-{_route}-smooth"] = case(_net, _route, SMOOTH, patches=True)
    CASES[f"{_net}-rays-info"] = case(_net, "rays", INFO, patches=True)
    CASES[f"{_net}-rays-ent"] = case(_net, "rays", ENT)
    CASES[f"{_net}-view-ent"] = case(_net, "view", ENT)
    for _inputs in ("staged", "rays"):
        CASES[f"{_net}-rays-reg-grid-{_inputs}"] = case(_net, "rays", REG, occupancy="ones", grid_inputs=_inputs)
        CASES[f"{_net}-rays-smooth-grid-{_inputs}"] = case(_net, "rays", SMOOTH, patches=True, occupancy="ones", grid_inputs=_inputs)
        CASES[f"{_net}-rays-info-grid-{_inputs}"] = case(_net, "rays", INFO, patches=True, occupancy="ones", grid_inputs=_inputs)
        CASES[f"{_net}-view-reg-grid-{_inputs}"] = case(_net, "view", REG, occupancy="ones", grid_inputs=_inputs)
        CASES[f"{_net}-view-ent-grid-{_inputs}"] = case(_net, "view", ENT, occupancy="ones", grid_inputs=_inputs)
    CASES[f"{_net}-rays-info-grid-zeros"] = case(_net, "rays", INFO, patches=True, occupancy="zeros")
    CASES[f"{_net}-rays-hier-clip-adamw"] = case(_net, "rays-hier", dict(max_grad_norm=1.0, decoupled_weight_decay=True))
    CASES[f"{_net}-rays-freq-masked"] = case(_net, "rays", dict(freq_reg_end=4))        # the recorded step (t = 1) runs under a mask
    CASES[f"{_net}-rays-freq-cleared"] = case(_net, "rays", dict(freq_reg_end=1))       # at t = 1 every band is visible: the mask is cleared
    CASES[f"{_net}-call-target-depth"] = case(_net, "call", dict(depth_weight=0.1), target_depth=True)
    CASES[f"{_net}-rays-hier-then-plain"] = case(_net, "rays-hier", then="rays")
    CASES[f"{_net}-rays-plain-then-hier"] = case(_net, "rays", then="rays-hier")
CASES["v3-rays-outputs"] = case("v3", "rays", outputs=True)
CASES["v3-rays-outputs-grid-rays"] = case("v3", "rays", outputs=True, occupancy="ones", grid_inputs="rays")


def sha(t):
    return hashlib.sha256(t.detach().to("cpu", copy=True).contiguous().numpy().tobytes()).hexdigest()


def digests(step):
    """What the first step of a fresh object left behind, before the second one overwrites it."""
    losses = step.last_losses
    out = {"loss_names": list(losses), "losses": sha(torch.stack([v.reshape(()) for v in losses.values()]))}
    for name in KEPT:
        t = getattr(step, name, None)
        if t is not None:
            out[name] = sha(t)
    return out


def record(N, name):
    """{'calls': the transcript of the second run of case `name`, 'digests': of its first step}."""
    from nerf_few_shot_limitations_amd import _lib
    torch.manual_seed(0)
    step, runs = CASES[name](N)
    runs[0]()
    first = digests(step)
    for run in runs[1:]:
        run()
    torch.cuda.synchronize()
    gc.collect()                  # an earlier case's module that dies inside the recording would add its nrf_model_destroy
    real = _lib.lib()
    rec = Transcript(real, _lib.SIGNATURES)
    _lib._lib = rec
    try:
        for run in runs:
            run()
    finally:
        _lib._lib = real
    torch.cuda.synchronize()
    return {"calls": rec.calls, "digests": first}


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


@pytest.fixture(scope="module")
def recorded():
    if not os.path.exists(GOLDEN):
        pytest.fail("tests/golden/fused_step_transcript.json is missing: there is no recording to compare with", pytrace=False)
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    for name, want in recorded.items():
        assert {"pred", "losses", "loss_names"} <= set(want["digests"]), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_transcript_and_first_step_are_the_recorded_ones(N, name, recorded):
    want = recorded[name]
    assert len(want["calls"]) > 0
    got = record(N, name)
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
    assert {k: got["digests"].get(k) for k in want["digests"]} == want["digests"]


# ---- recording ---------------------------------------------------------------------------------------------------------------------
def dump(cases, path):
    """One call per line: a changed argument shows as one changed line."""
    with open(path, "w") as f:
        f.write("{\n")
        for i, name in enumerate(sorted(cases)):
            c = cases[name]
            f.write(f" {json.dumps(name)}: {{\n  \"digests\": {json.dumps(c['digests'], sort_keys=True)},\n  \"calls\": [\n")
            f.write(",\n".join("   " + json.dumps(call, separators=(",", ":")) for call in c["calls"]))
            f.write("\n  ]\n }" + ("," if i + 1 < len(cases) else "") + "\n")
        f.write("}\n")


def main(argv):
    if argv[:1] == ["record"] and len(argv) == 2:
        import nerf_few_shot_limitations_amd as N
        out = {}
        for name in sorted(CASES):
            out[name] = record(N, name)
            print(name, len(out[name]["calls"]), "calls", flush=True)
        dump(out, argv[1])
        return 0
    if argv[:1] == ["merge"] and len(argv) == 4:
        with open(argv[1]) as f:
            a = json.load(f)
        with open(argv[2]) as f:
            b = json.load(f)
        assert sorted(a) == sorted(b) == sorted(CASES)
        for name in sorted(a):
            assert a[name]["calls"] == b[name]["calls"], f"{name}: the two recordings differ in their transcripts"
            da, db = a[name]["digests"], b[name]["digests"]
            for k in sorted(da):
                if da[k] != db.get(k):
                    print(f"dropped: {name}: {k} (the two recordings differ)")
                    del a[name]["digests"][k]
        dump(a, argv[3])
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
