"""Operations, plans and the fresh-twin oracle of tests/test_gpu_weight_currency.py (a plain helper module, no fixtures).

A plan is a literal list of tuples, one per operation:

    changing    ("fused_call", k)  ("fused_rays", k)  ("fused_rays_occ", k)  ("adam_step", k)  ("torch_step", m, k)
                ("load_inplace", k)  ("load_assign", k)  ("inplace_edit", k)  ("move",)  ("snapshot",)
                ("guard", m, change)            the forward of grad[m], the change, then a backward that must be refused
    observing   ("fwd", m)  ("render", m)  ("render_tail", b)  ("refresh",)  ("grad", m)
                ("split_grad", m, [observing ...])     the forward of grad[m], the listed operations, then its backward
                ("grad_fwd", m)                        inside split_grad only: a training forward whose backward never runs
    neither     ("zero_grad", "none" | "inplace" | "foreign")
                ("snapshot_keep", [operations ...])    a deepcopy that takes the listed operations and is dropped

m: "bf16" | "f16" | "f32" | "f16x3"; k: a small integer that picks the batch, the weights or the factor.  Everything below the
plan generator needs the GPU; the generator, SCRIPTED and the event model are pure Python (tests/test_weight_currency_plans_host.py).
"""
import copy

import numpy as np

MODES = ("bf16", "f16", "f32", "f16x3")
TRAIN_MODES = ("bf16", "f16", "f32")
TRAIN_MODE = {"bf16": "bf16", "f16": "f16", "f32": "f32", "f16x3": "f32"}
FAMILIES = ("v1", "v2", "v3")
CHANGES = {"v1": ("fused_call", "adam_step", "torch_step", "load_inplace", "load_assign", "inplace_edit", "move", "snapshot"),
           "v2": ("fused_call", "fused_rays", "fused_rays_occ", "adam_step", "torch_step", "load_inplace", "load_assign", "inplace_edit",
                  "move", "snapshot")}
CHANGES["v3"] = CHANGES["v2"]
OBSERVATIONS = tuple([("fwd", m) for m in MODES] + [("render", m) for m in MODES] + [("render_tail", b) for b in ("bf16", "f16")]
                     + [("refresh",)] + [("grad", m) for m in TRAIN_MODES])
WALK_UNITS = 14                    # operations of a walk that build a twin


def key(op):
    """'fwd[f16]', 'refresh', 'fused_call': an operation without its draw."""
    if op[0] in ("fwd", "render", "render_tail", "grad", "grad_fwd", "split_grad", "guard"):
        return f"{op[0]}[{op[1]}]"
    return op[0]


# ---------------------------------------------------------------------------------------------
# plans (pure Python)
# ---------------------------------------------------------------------------------------------
def change_op(name, k, mode="bf16"):
    if name in ("move", "snapshot"):
        return (name,)
    if name == "torch_step":
        return (name, mode, k)
    return (name, k)


def cross_plan(family, change):
    """`change` followed by every observation, one after the other, on a model that has trained before."""
    plan = [("fused_call", 0)]
    for i, ob in enumerate(OBSERVATIONS):
        plan += [change_op(change, i % 4, TRAIN_MODES[i % 3]), ob]
    return plan


def _third(a, b):
    return [m for m in TRAIN_MODES if m not in (a, b)][0]


def scripted(family):
    """{name: (the subject's own mma_mode, plan)} for one family."""
    rays = family != "v1"
    step = "fused_rays" if rays else "fused_call"
    out = {}
    # the backward streams of two training modes are current, a third mode is read: neither may be left stale
    for a in TRAIN_MODES:
        for b in TRAIN_MODES:
            if a != b:
                out[f"two_training_modes_and_a_third_reader[{a}>{b}]"] = (a, [("split_grad", a, [("grad_fwd", b), ("render", _third(a, b))]),
                                                                             ("grad", b), ("grad", a)])
    out["three_training_modes_in_turn"] = ("bf16", [("grad", "bf16"), ("grad", "f32"), ("grad", "f16"), ("grad", "bf16")])
    out["two_training_modes_and_a_tail_reader"] = ("bf16", [("split_grad", "bf16", [("grad_fwd", "f32"), ("render_tail", "f16")]), ("grad", "f32")])
    out["validation_after_a_refresh_between_steps"] = ("bf16", [(step, 0), ("refresh",), ("render", "f32"), (step, 1), ("fwd", "bf16")])
    if rays:
        out["validation_after_a_refresh_between_steps_under_a_grid"] = ("bf16", [("fused_rays_occ", 0), ("refresh",), ("render", "f16x3"),
                                                                                 ("fused_rays_occ", 1), ("fwd", "bf16")])
    for c in CHANGES[family]:
        out[f"every_observation_after[{c}]"] = ("bf16", cross_plan(family, c))
    out["the_training_stream_is_the_only_stale_stream"] = ("bf16", [("fused_call", 0), ("fwd", "f16"), ("fwd", "f32"), ("fused_call", 1), ("fwd", "f16")])
    out["first_fused_step_after_move_and_load"] = ("bf16", [("fused_call", 0), ("move",), ("load_inplace", 1), ("fused_call", 1), ("fwd", "f32")])
    out["first_fused_step_after_load_assign"] = ("f16", [("fused_call", 0), ("load_assign", 1), ("fused_call", 1), ("render", "bf16")])
    out["first_use_render_then_train"] = ("bf16", [("render", "f32"), ("fused_call", 0), ("render", "f32"), ("grad", "bf16")])
    out["first_use_train_then_render_in_another_mode"] = ("bf16", [("fused_call", 0), ("render", "f16"), ("fused_call", 1), ("fwd", "bf16")])
    out["first_use_fused_step_before_any_forward"] = ("f16x3", [("fused_call", 0), ("grad", "f32"), ("fwd", "f16x3")])
    out["first_use_after_a_host_repack"] = ("f16", [("fwd", "f16"), ("inplace_edit", 0), ("grad", "f16"), ("adam_step", 0), ("fwd", "f16")])
    out["snapshot_kept_in_the_middle_of_training"] = ("bf16", [("fused_call", 0), ("snapshot_keep", [("fused_call", 1), ("fwd", "f32"), ("grad", "bf16")]),
                                                               ("fused_call", 0), ("fwd", "f32"), ("grad", "bf16")])
    # snapshot is left out: a deepcopy does not modify the module the pending graph belongs to, its backward is legal
    out["a_backward_across_every_change_is_refused"] = ("bf16", [("fused_call", 0)] + [("guard", "bf16", change_op(c, 1, "f16"))
                                                                                       for c in CHANGES[family] if c != "snapshot"]
                                                        + [("grad", "bf16")])
    return out


def walk_subject(family, seed):
    """(mma_mode, scene) of a walk's subject."""
    return MODES[seed % 4], ("solid", "fog")[(seed // 4) % 2]


def walk_plan(family, seed):
    """14 twin-building operations drawn by numpy.random.RandomState: never more than two changing or two observing ones in a row."""
    rng = np.random.RandomState(1000 * FAMILIES.index(family) + seed)
    pick = lambda seq: seq[rng.randint(len(seq))]
    simple = lambda: pick([("fwd", pick(MODES)), ("render", pick(MODES)), ("render_tail", pick(("bf16", "f16"))), ("refresh",)])
    plan, kinds, units = [], [], 0
    while units < WALK_UNITS:
        kind = pick("co")
        if len(kinds) >= 2 and kinds[-1] == kinds[-2]:
            kind = "o" if kinds[-1] == "c" else "c"
        room = WALK_UNITS - units
        if kind == "c":
            name = pick(CHANGES[family] + ("guard", "snapshot_keep"))
            if name == "guard":
                op = ("guard", pick(TRAIN_MODES), change_op(pick([c for c in CHANGES[family] if c != "snapshot"]), int(rng.randint(4)), pick(TRAIN_MODES)))
                cost = 1
            elif name == "snapshot_keep":
                op, cost = ("snapshot_keep", [simple()]), 1
            else:
                op, cost = change_op(name, int(rng.randint(4)), pick(TRAIN_MODES)), 1
        else:
            what = pick(["fwd", "render", "render_tail", "refresh", "grad", "grad", "split_grad", "zero_grad"])
            if what == "split_grad" and room >= 2:
                inner = [pick([simple(), ("grad_fwd", pick(TRAIN_MODES))]) for _ in range(1 + int(rng.randint(min(2, room - 1))))]
                op, cost = ("split_grad", pick(TRAIN_MODES), inner), 1 + len(inner)
            elif what == "zero_grad":
                op, cost = ("zero_grad", pick(("none", "inplace", "foreign"))), 0
            elif what in ("grad", "split_grad"):
                op, cost = ("grad", pick(TRAIN_MODES)), 1
            else:
                op, cost = {"fwd": ("fwd", pick(MODES)), "render": ("render", pick(MODES)), "render_tail": ("render_tail", pick(("bf16", "f16"))),
                            "refresh": ("refresh",)}[what], 1
        plan.append(op)
        kinds.append(kind)
        units += cost
    return plan


def all_plans():
    """[(family, name, subject mode, plan)]: the scripted scenarios and the 8 walks of every family."""
    out = []
    for f in FAMILIES:
        out += [(f, name, mode, plan) for name, (mode, plan) in scripted(f).items()]
        out += [(f, f"walk{seed}", walk_subject(f, seed)[0], walk_plan(f, seed)) for seed in range(8)]
    return out


def events(plan, own_mode):
    """The plan as the state machines see it: ("C", name) a change of the parameters, ("T", m) a training forward in mode m,
    ("R", {modes}) a read of the forward streams of those modes.  `own_mode`: the subject's mma_mode."""
    tm = TRAIN_MODE[own_mode]
    ev = []
    for op in plan:
        name = op[0]
        if name in ("fwd", "render"):
            ev.append(("R", {op[1]}))
        elif name == "render_tail":
            ev.append(("R", {op[1], "f16x3"}))
        elif name == "refresh":
            ev.append(("R", {own_mode}))
        elif name in ("grad", "grad_fwd"):
            ev.append(("T", op[1]))
        elif name == "split_grad":
            ev += [("T", op[1])] + events(op[2], own_mode)
        elif name == "guard":
            ev += [("T", op[1])] + events([op[2]], own_mode)
        elif name == "torch_step":
            ev += [("T", op[1]), ("C", name)]
        elif name in ("fused_call", "fused_rays", "fused_rays_occ", "adam_step"):
            ev += [("T", tm), ("C", name)]
        elif name in ("load_inplace", "load_assign", "inplace_edit", "move", "snapshot"):
            ev.append(("C", name))
        elif name not in ("zero_grad", "snapshot_keep"):
            raise ValueError(f"unknown operation {op!r}")
    return ev


# ---------------------------------------------------------------------------------------------
# inputs (built once per process, on the GPU)
# ---------------------------------------------------------------------------------------------
R, S, HW = 64, 16, 16
NEAR, FAR = 2.0, 6.0
LR = 1e-3
_cache = {}
RECORD = {"grad": 0.0, "ledger": 0.0, "fused_grad": 0.0, "anchor": 0.0}


def _u01(seed, *shape):
    import torch
    from oracle import nerf_oracle as O
    return torch.from_numpy(O.uniform01(seed, int(np.prod(shape))).reshape(shape)).float()


def inputs(family):
    """Everything the operations feed a `family` model, deterministic; at most 64 rays x 16 samples."""
    if family in _cache:
        return _cache[family]
    import torch
    import nerf_few_shot_limitations_amd as N
    from oracle import nerf_oracle as O
    from tests.test_gpu_point_grad import random_map, views
    from tests.test_gpu_train_occupancy import grid_of
    d = {}
    n = R * S
    pose = torch.from_numpy(O.LEGO_LIKE_C2W.copy())
    focal = O.focal_for(HW)
    d["pose"], d["focal"] = pose, focal
    d["cam"] = dict(features=random_map(14, 22, 64).cuda(), **views()["orbit"]) if family == "v3" else None
    ro, rd = N.get_rays(HW, HW, focal, pose)
    ro, rd = ro.reshape(-1, 3).cuda(), rd.reshape(-1, 3).cuda()
    d["pix"] = [torch.randperm(HW * HW, generator=torch.Generator().manual_seed(40 + i))[:R].cuda() for i in range(4)]
    d["rays"] = [(ro[p].contiguous(), rd[p].contiguous()) for p in d["pix"]]
    d["image"] = _u01(601, HW, HW, 3).cuda()
    d["tgt"] = [_u01(602 + i, R, 3).cuda() for i in range(4)]
    d["g"] = (_u01(606, R, 3) - 0.5).cuda()
    # the per-sample batch of FusedStep.__call__ and of model(x)
    pos = _u01(607, n, 3) * 4 - 2
    d["z"] = torch.sort(_u01(608, R, S) * 4 + 2, dim=-1).values.cuda()
    d["rd"] = (_u01(609, R, 3) - 0.5).cuda()
    d["dirs"] = d["rd"][:, None, :].expand(R, S, 3).reshape(-1, 3).contiguous()
    d["pts"] = (O.positional_encoding(pos, 10) if family == "v1" else pos).cuda()
    d["dino"] = (_u01(610, n, 64) * 2 - 1).cuda() if family == "v3" else None
    d["g_out"] = (_u01(611, n, 4) - 0.5).cuda()
    d["grid"] = grid_of("half") if family != "v1" else None
    _cache[family] = d
    return d


def net_args(family, d, n):
    """The first n samples as NeRFMLP.forward takes them."""
    if family == "v1":
        return (d["pts"][:n],)
    return (d["pts"][:n], d["dirs"][:n], d["dino"][:n] if family == "v3" else None)


def weights(family, k):
    from oracle import nerf_oracle as O
    kw = dict(n_layers=2)
    if family == "v3":
        kw["dino_dim"] = 64
    return O.make_weights(family, 10 + k, ("solid", "fog")[k % 2], **kw)


def make_subject_model(N, family, mode, scene):
    from tests.test_gpu_training import make_model, make_v2, make_v3
    if family == "v1":
        return make_model(N, mode, scene=scene, n_layers=2)[0]
    if family == "v2":
        return make_v2(N, mode, scene=scene, n_layers=2)[0]
    return make_v3(N, mode, scene=scene, n_layers=2, dino_dim=64)[0]


def outputs(x):
    return list(x) if isinstance(x, (tuple, list)) else [x]


def flat_grad(model):
    """The parameters' .grad in the flat layout (weight, bias per Linear); a missing .grad counts as zeros."""
    import torch
    ps = [p for m in model.linears() for p in (m.weight, m.bias)]
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).float() for p in ps]).clone()


def within(got, want, what, record=None):
    """max |got - want| relative to max |want| <= 1e-5 ("atomics: order only", test_device_repack_equals_host_pack)."""
    err = float((got.double() - want.double()).abs().max())
    top = float(want.double().abs().max())
    rel = err / top if top > 0 else (0.0 if err == 0 else float("inf"))
    if record:
        RECORD[record] = max(RECORD[record], rel)
    assert rel <= 1e-5, f"{what}: {err:.3e} off, {rel:.3e} of the largest element {top:.3e}"


# ---------------------------------------------------------------------------------------------
# the subject and its operations
# ---------------------------------------------------------------------------------------------
class Subject:
    def __init__(self, N, family, model):
        self.N, self.family, self.model = N, family, model
        self.d = inputs(family)
        self.twins = 0
        self._helpers()
        self.ledger = flat_grad(model)

    def _helpers(self):
        from nerf_few_shot_limitations_amd.training import Adam, FusedStep
        self.step = FusedStep(self.model, lr=LR)
        self.adam = Adam(self.model, lr=LR)

    # ---- the oracle ----------------------------------------------------------------------------
    def twin(self):
        """A model built from nothing but the subject's state_dict(): never trained, never reused."""
        m, N = self.model, self.N
        if self.family == "v1":
            t = N.NeRFMLP(pos_dim=3 * (2 * m.pos_freq + 1), hidden_dim=m.hidden_dim, n_layers=m.n_layers, mma_mode=m.mma_mode)
        else:
            t = N.NeRFMLP(pos_freq=m.pos_freq, dir_freq=m.dir_freq, hidden_dim=m.hidden_dim, num_density_layers=m.n_layers,
                          use_dino=self.family == "v3", dino_dim=m.dino_dim, mma_mode=m.mma_mode)
        t.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        self.twins += 1
        return t.cuda().train()

    def anchor(self):
        """The subject's f32 eval forward on 64 samples against the CPU oracle on the same state_dict, within 1e-4 (the parity bar):
        subject and twin cannot be wrong together."""
        from oracle import nerf_oracle as O
        p = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        got = [t.cpu() for t in outputs(self._fwd(self.model, "f32", 64))]
        cpu = [None if a is None else a.cpu() for a in net_args(self.family, self.d, 64)]
        if self.family == "v1":
            want = O.mlp_v1(p, cpu[0])
            got, want = [got[0][:, :3], got[0][:, 3:]], [want[:, :3], want[:, 3:]]
        elif self.family == "v2":
            want = list(O.mlp_v2(p, cpu[0], cpu[1]))
        else:
            want = list(O.mlp_v3(p, cpu[0], cpu[1], cpu[2]))
        e_rgb = float((got[0] - want[0]).abs().max())                              # test_v3_gradients_fp32_mode_match_autograd's pair of bars
        e_den = float((got[1] - want[1]).abs().max() / want[1].abs().max().clamp_min(1e-30))
        RECORD["anchor"] = max(RECORD["anchor"], e_rgb, e_den)
        assert e_rgb < 1e-4 and e_den < 1e-4, f"anchor: rgb {e_rgb:.3e}, density {e_den:.3e} (of its largest) from the CPU oracle"

    # ---- observations --------------------------------------------------------------------------
    def _fwd(self, model, mode, n=200):
        import torch
        own, was = model.mma_mode, model.training
        model.eval()
        model.mma_mode = mode
        try:
            with torch.no_grad():
                return model(*net_args(self.family, self.d, n))
        finally:
            model.mma_mode = own
            model.train(was)

    def _render(self, model, mode, tail=None):
        import torch
        was = model.training
        try:
            with torch.no_grad():
                return self.N.render_camera(model.eval(), HW, HW, self.d["focal"], self.d["pose"], NEAR, FAR, S, mma_mode=mode, dino=self.d["cam"],
                                            tail_mode=tail)
        finally:
            model.train(was)

    def _refresh(self, model):
        import torch
        from nerf_few_shot_limitations_amd.occupancy import OccupancyGrid
        grid = OccupancyGrid.full((32, 4, 4), -1.5, 1.5, device=torch.device("cuda", 0))      # 512 = 8^3 cells (rx is a multiple of 32)
        grid.refresh(model, decay=0.9, threshold=0.0, samples_per_cell=2, dino=self.d["cam"])
        return grid.ema

    def _same(self, observe, what):
        import torch
        got, want = outputs(observe(self.model)), outputs(observe(self.twin()))
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.isfinite(b).all() and torch.equal(a, b), f"{what}: output {i} differs from the fresh twin's in {int((a != b).sum())} of {a.numel()} elements"

    def op_fwd(self, mode):
        self._same(lambda m: self._fwd(m, mode), f"fwd[{mode}]")

    def op_render(self, mode):
        self._same(lambda m: self._render(m, mode), f"render[{mode}]")

    def op_render_tail(self, base):
        self._same(lambda m: self._render(m, base, "f16x3"), f"render_tail[{base}]")

    def op_refresh(self):
        self._same(self._refresh, "refresh")

    def _train_forward(self, model, mode, k=0):
        o, dd = self.d["rays"][k]
        return self.N.render_rays(model.train(), o, dd, NEAR, FAR, S, perturb=True, seed=20 + k, mma_mode=mode, dino=self.d["cam"])

    def op_grad_fwd(self, mode):
        self._train_forward(self.model, mode)

    def op_grad(self, mode, between=(), loss=None, k=0):
        """grad[m] / split_grad[m; between]: outputs equal to the twin's; every parameter's .grad within 1e-5 of its tensor's largest
        element of what it held before plus the twin's gradient (a backward ADDS into .grad in fp32: on top of an earlier, larger
        gradient its own share is not recoverable below that sum's rounding, so the sum is what is compared; after a zero_grad it
        is the backward's gradient alone); the whole .grad vector within 1e-5 of the ledger's largest element."""
        import torch
        loss = loss or (lambda out: (out["rgb"] * self.d["g"]).sum())
        twin = self.twin()
        before = flat_grad(self.model)
        out = self._train_forward(self.model, mode, k)
        for op in between:
            self.run(op)
        loss(out).backward()
        ref = self._train_forward(twin, mode, k)
        loss(ref).backward()
        for name in ("rgb", "depth", "weights"):
            assert torch.equal(out[name], ref[name]), f"grad[{mode}]: {name} differs from the fresh twin's"
        want, after = flat_grad(twin), flat_grad(self.model)
        expect = before + want
        off = 0
        for lin in twin.linears():
            for p in (lin.weight, lin.bias):
                within(after[off:off + p.numel()], expect[off:off + p.numel()], f"grad[{mode}] parameter at {off} {tuple(p.shape)}", "grad")
                off += p.numel()
        self.ledger = self.ledger + want
        within(after, self.ledger, f"accumulated .grad after grad[{mode}] against the ledger", "ledger")

    def op_split_grad(self, mode, between):
        self.op_grad(mode, between)

    def op_guard(self, mode, change):
        import pytest
        out = self._train_forward(self.model, mode)
        self.run(change)
        with pytest.raises(RuntimeError, match="parameters were modified between"):
            (out["rgb"] * self.d["g"]).sum().backward()

    def op_zero_grad(self, how):
        import torch
        if how == "foreign":                    # some other code produced a .grad: the backward falls back to autograd's accumulation
            ps = list(self.model.parameters())
            for p in ps:
                p.grad = None
            ps[0].grad = torch.zeros_like(ps[0])
        else:
            torch.optim.SGD(self.model.parameters(), lr=0.0).zero_grad(set_to_none=how == "none")
        self.ledger = torch.zeros_like(self.ledger)

    # ---- changes -------------------------------------------------------------------------------
    def _mse(self, pred, tgt):
        import torch
        return torch.nn.functional.mse_loss(pred, tgt)

    def _check_step(self, pred, grad, what):
        import torch
        assert torch.equal(self.step.pred, pred), f"{what}: step.pred differs from the autograd route on a fresh twin of the state before the step"
        within(self.step.grad, grad, f"{what}: step.grad against the twin's flat gradient", "fused_grad")

    def op_fused_call(self, k):
        d, N = self.d, self.N
        tgt = d["tgt"][k]
        twin = self.twin()
        if self.family == "v1":
            pred = N.volume_render_radiance(twin(d["pts"]).view(R, 1, S, 4), d["z"].view(R, 1, S), d["rd"].view(R, 1, 3)).view(R, 3)
        else:
            c, sg = twin(d["pts"], d["dirs"], d["dino"])
            pred = N.VolumeRenderer()(c.view(R, S, 3), sg.view(R, S, 1), d["z"], d["rd"])[0]
        self._mse(pred, tgt).backward()
        self.step(d["pts"], d["z"], d["rd"], tgt, dirs=d["dirs"] if self.family != "v1" else None, dino=d["dino"])
        self._check_step(pred.detach(), flat_grad(twin), "fused_call")

    def _ray_step(self, step, k, **kw):
        d = self.d
        if k % 2:
            return step.step_view(d["image"], d["pose"], HW, HW, d["focal"], d["pix"][k], NEAR, FAR, S, seed=30 + k, dino=d["cam"], **kw)
        o, dd = d["rays"][k]
        return step.step_rays(o, dd, d["tgt"][k], NEAR, FAR, S, perturb=True, seed=30 + k, dino=d["cam"], **kw)

    def op_fused_rays(self, k):
        d = self.d
        twin = self.twin()
        o, dd = d["rays"][k]
        tgt = d["image"].reshape(-1, 3)[d["pix"][k]] if k % 2 else d["tgt"][k]
        pred = self.N.render_rays(twin, o, dd, NEAR, FAR, S, perturb=True, seed=30 + k, dino=d["cam"])["rgb"]
        self._mse(pred, tgt).backward()
        self._ray_step(self.step, k)
        self._check_step(pred.detach(), flat_grad(twin), "fused_rays")

    def op_fused_rays_occ(self, k):
        """The autograd route refuses a grid; the stand-in is the same step taken once by a fresh twin, which is then dropped."""
        from nerf_few_shot_limitations_amd.training import FusedStep
        other = FusedStep(self.twin(), lr=LR)
        self._ray_step(other, k, occupancy=self.d["grid"])
        self._ray_step(self.step, k, occupancy=self.d["grid"])
        assert 0 < self.step.last_count < R * S and self.step.last_count == other.last_count
        self._check_step(other.pred, other.grad, "fused_rays_occ")

    def op_adam_step(self, k):
        self.adam.zero_grad(set_to_none=bool(k % 2))
        n = R * S
        out = outputs(self.model.train()(*net_args(self.family, self.d, n)))
        g = self.d["g_out"]
        (out[0] * g[:, :out[0].shape[1]]).sum().add((out[1] * g[:, 3:]).sum() if len(out) > 1 else 0.0).backward()
        self.adam.step()
        self.ledger = flat_grad(self.model)

    def op_torch_step(self, mode, k):
        import torch
        self.op_zero_grad(("none", "inplace")[k % 2])
        self.op_grad(mode, loss=lambda out: self._mse(out["rgb"], self.d["tgt"][k]), k=k)          # the gradient SGD consumes is checked first
        torch.optim.SGD(self.model.parameters(), lr=LR).step()

    def op_load_inplace(self, k):
        self.model.load_state_dict(weights(self.family, k), strict=self.family == "v1")

    def op_load_assign(self, k):
        self.model.load_state_dict({n: v.cuda() for n, v in weights(self.family, k).items()}, strict=self.family == "v1", assign=True)
        self.ledger = flat_grad(self.model)

    def op_inplace_edit(self, k):
        import torch
        ps = list(self.model.parameters())
        with torch.no_grad():
            for p in (ps[k % len(ps)], ps[(k + 3) % len(ps)]):
                p.mul_((0.97, 1.03)[k % 2])

    def op_move(self):
        self.model = self.model.cpu().cuda()
        self.ledger = flat_grad(self.model)

    def op_snapshot(self):
        self.model = copy.deepcopy(self.model)          # the original is dropped with its helpers
        self._helpers()
        self.ledger = flat_grad(self.model)

    def op_snapshot_keep(self, ops):
        other = Subject(self.N, self.family, copy.deepcopy(self.model))
        for op in ops:
            other.run(op)
        other.anchor()
        self.twins += other.twins

    def run(self, op):
        getattr(self, "op_" + op[0])(*op[1:])


def run_plan(N, family, mode, scene, plan):
    """Run `plan` on a fresh subject, then the anchor.  A failure carries the plan up to the failing operation as a literal that can
    be pasted into scripted() as a regression."""
    sub = Subject(N, family, make_subject_model(N, family, mode, scene))
    for i, op in enumerate(plan):
        try:
            sub.run(op)
        except Exception as e:
            raise AssertionError(f"{family} subject in {mode} ({scene}) failed at operation {i} {op!r}: {type(e).__name__}: {e}\n"
                                 f"plan = {plan[:i + 1]!r}") from e
    try:
        sub.anchor()
    except AssertionError as e:
        raise AssertionError(f"{family} subject in {mode} ({scene}): {e}\nplan = {plan!r}") from e
    return sub
