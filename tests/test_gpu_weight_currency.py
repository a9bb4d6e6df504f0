"""Weight currency across modes, routes and optimisers: which of a NeRFMLP's seven packed copies (four forward streams, three
backward streams, one bias table) a kernel reads after any history of steps, loads, moves, copies and reads in other modes.

The oracle is a fresh twin: after every operation of a plan (tests/currency_ops.py) each observable of the subject -- eval forwards
and fused renders in all four modes, tail renders, an occupancy refresh, render_rays under grad with its parameter gradients -- must
equal the same observable of a model built from nothing but the subject's state_dict(), whose streams come from nrf_model_create's
host packer.  Device re-pack equals host pack bit for bit (test_device_repack_of_every_mode_equals_host_pack), so outputs are held
to torch.equal; gradients to 1e-5 of their tensor's largest element (test_device_repack_equals_host_pack: "atomics: order only").
A twin shares the subject's kernels; every plan ends with the subject's f32 forward against the CPU oracle at 1e-4, so the two
cannot be wrong together.  A fused step is also held to the autograd route on a twin of the state before it (step.pred, step.grad),
and the parameters' accumulated .grad to a ledger of the twins' gradients.

RECORD (MI355X, 114 tests in 21 s): largest parameter-gradient error against the twin 1.2e-7 of its tensor's largest element, largest
.grad-against-ledger error 9.4e-8, step.grad against the twin's autograd route bit-equal (0.0), anchor 3.9e-6.  On the parent commit the
eight two/three-training-mode scenarios of every family fail with "backward weights of this mode are older than the parameters".
"""
import pytest
import torch

from tests import currency_ops as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def N():
    import nerf_few_shot_limitations_amd as N
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return N


SCRIPTED = [(f, name) for f in X.FAMILIES for name in X.scripted(f)]


@pytest.mark.parametrize("family,name", SCRIPTED, ids=[f"{f}-{n}" for f, n in SCRIPTED])
def test_scripted_scenarios(N, family, name):
    mode, plan = X.scripted(family)[name]
    X.run_plan(N, family, mode, "solid", plan)
    print("RECORD   largest relative errors so far:", X.RECORD)


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("family", X.FAMILIES)
def test_seeded_walks(N, family, seed):
    mode, scene = X.walk_subject(family, seed)
    sub = X.run_plan(N, family, mode, scene, X.walk_plan(family, seed))
    assert sub.twins <= X.WALK_UNITS
    print("RECORD   largest relative errors so far:", X.RECORD)


class _Counted:
    """nrf_model_update_device behind a proxy that keeps the mode masks it was called with."""

    def __init__(self, fn):
        self.fn, self.masks = fn, []

    def __call__(self, model, flat, mask, stream):
        self.masks.append(int(mask))
        return self.fn(model, flat, mask, stream)


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("render_between", [False, True])
def test_a_training_step_repacks_one_mode_once(N, family, render_between, monkeypatch):
    """The steady state does not pay for the ride-along rule: five fused steps (with or without an eval render in the training mode
    between them) cost exactly one nrf_model_update_device call each, with exactly one mode bit set."""
    from nerf_few_shot_limitations_amd import _lib as L
    sub = X.Subject(N, family, X.make_subject_model(N, family, "bf16", "solid"))
    d = sub.d
    step = lambda k: sub.step(d["pts"], d["z"], d["rd"], d["tgt"][k % 4], dirs=d["dirs"] if family != "v1" else None, dino=d["dino"])
    step(0)                                                     # first use: the backward plan and both directions packed
    proxy = _Counted(L.lib().nrf_model_update_device)
    monkeypatch.setattr(L.lib(), "nrf_model_update_device", proxy)
    for k in range(1, 6):
        before = len(proxy.masks)
        if render_between:                                      # packs the stepped parameters; the step behind it finds them current
            sub._render(sub.model, "bf16")
        step(k)
        assert proxy.masks[before:] == [1 << L.MMA_MODES["bf16"]], (k, proxy.masks)
    assert len(proxy.masks) == 5
    monkeypatch.undo()
    sub.op_fwd("f32")
    sub.anchor()
