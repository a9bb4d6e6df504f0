"""Coverage of the weight-currency plans (tests/currency_ops.py), asserted on the plans themselves: nothing here runs an operation.
A condition that fails is a fault of the seeds or of the draw, never of the condition."""
import pytest

from tests import currency_ops as X

PLANS = X.all_plans()
ALL_CHANGES = X.CHANGES["v2"]
OBS_KEYS = [X.key(ob) for ob in X.OBSERVATIONS]


def test_the_plans_are_what_the_gpu_tests_run():
    walks = [p for p in PLANS if p[1].startswith("walk")]
    assert len(walks) == 24 and len(OBS_KEYS) == 14 and len(ALL_CHANGES) == 10
    for family, name, mode, plan in walks:
        assert plan == X.walk_plan(family, int(name[4:]))                    # the draw is a function of (family, seed) alone
        kinds = ["c" if op[0] in ALL_CHANGES + ("guard", "snapshot_keep") else "o" for op in plan]
        assert all(len(set(kinds[i:i + 3])) == 2 for i in range(len(kinds) - 2)), (family, name, kinds)
        cost = sum(0 if op[0] == "zero_grad" else 1 + (len(op[2]) if op[0] == "split_grad" else 0) for op in plan)
        assert cost == X.WALK_UNITS, (family, name, cost)


def test_every_change_is_followed_by_every_observation():
    seen = set()
    for _, _, _, plan in PLANS:
        for a, b in zip(plan, plan[1:]):
            if a[0] in ALL_CHANGES:
                seen.add((a[0], X.key(b)))
    missing = [(c, o) for c in ALL_CHANGES for o in OBS_KEYS if (c, o) not in seen]
    assert not missing, missing


def test_every_mode_follows_every_change():
    seen = set()
    for _, _, mode, plan in PLANS:
        ev = X.events(plan, mode)
        for a, b in zip(ev, ev[1:]):
            if a[0] == "C":
                seen |= {(a[1], m) for m in (b[1] if b[0] == "R" else {b[1]} if b[0] == "T" else ())}
    missing = [(c, m) for c in ALL_CHANGES for m in X.MODES if (c, m) not in seen]
    assert not missing, missing


def test_every_ordered_pair_of_training_modes_meets_a_third_reader():
    """T a, T b, then a read that touches neither, with no change of the parameters in between: the run in which a re-pack for the
    reader can leave a's or b's backward stream stale."""
    seen = set()
    for _, _, mode, plan in PLANS:
        ev = X.events(plan, mode)
        for a, b, c in zip(ev, ev[1:], ev[2:]):
            if a[0] == "T" and b[0] == "T" and a[1] != b[1]:
                third = c[1] if c[0] == "R" else {c[1]} if c[0] == "T" else {a[1]}
                if not third & {a[1], b[1]}:
                    seen.add((a[1], b[1]))
    missing = [(a, b) for a in X.TRAIN_MODES for b in X.TRAIN_MODES if a != b and (a, b) not in seen]
    assert not missing, missing


def test_no_plan_asks_a_family_for_what_it_does_not_have():
    def names(plan):
        for op in plan:
            yield op[0]
            for arg in op[1:]:
                if isinstance(arg, list):
                    yield from names(arg)
                elif isinstance(arg, tuple):
                    yield from names([arg])

    for family, name, _, plan in PLANS:
        used = set(names(plan))
        assert not used & (set(ALL_CHANGES) - set(X.CHANGES[family])), (family, name)
        assert repr(plan) == repr(eval(repr(plan)))                          # a literal: a failing plan can be pasted into scripted()
    assert "fused_rays" not in X.CHANGES["v1"] and "fused_rays_occ" not in X.CHANGES["v1"]


@pytest.mark.parametrize("family", X.FAMILIES)
def test_the_issue_scenarios_are_scripted(family):
    s = X.scripted(family)
    assert s["two_training_modes_and_a_third_reader[bf16>f32]"][1][0] == ("split_grad", "bf16", [("grad_fwd", "f32"), ("render", "f16")])
    assert s["three_training_modes_in_turn"][1] == [("grad", "bf16"), ("grad", "f32"), ("grad", "f16"), ("grad", "bf16")]
    guards = [op[2][0] for op in s["a_backward_across_every_change_is_refused"][1] if op[0] == "guard"]
    assert guards == [c for c in X.CHANGES[family] if c != "snapshot"]
