"""What train_cli.train_epoch calls, in which order and with what, and what train_cli.main leaves behind, pinned to a recording:
tests/golden/train_cli_transcript.json, made by tools/record_train_cli.py (which documents the fixture and holds the cases) on an
MI355X at commit 27dbe07 ("api.cpp: one copy of each argument check, one block of entries"), the parent of the commit that gave
train_epoch one batch tail and main its phases.  The test passes at that parent and after it with the same file: every case is
recorded again with the tool's own functions and compared.

train_epoch: a recording FusedStep, ExtractorTrainer and occupancy schedules log every call with its keyword names, tensors by
shape, dtype and digest (output buffers by which storage they are a view of), scalars and ctypes arrays by value, a grid by which
object it is and the digest of its bits, every returned loss bit for bit; then the returned (mean, samples) and the digest of the
final state_dict.  The raising combinations are pinned by their message.  main: the log without its timings, the files written, every
checkpoint's key set and the digests of its tensors.  The fixture was recorded twice, in two processes: both agreed on every field
(its "dropped" list is empty), so all of it is compared.
"""
import json
import os

import pytest
import torch

from tests.test_train_cli_flags_host import ROOT, load_recorder

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "train_cli_transcript.json")
R = load_recorder()


@pytest.fixture(scope="module")
def recorded():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with open(GOLDEN) as f:
        return json.load(f)


def fields(recorded, section, name):
    return {k[len(name) + 1:]: v for k, v in recorded[section].items() if k.startswith(name + "/")}


def test_the_fixture_holds_exactly_these_cases(recorded):
    assert sorted({k.rsplit("/", 1)[0] for k in recorded["epoch"]}) == sorted(R.EPOCH_CASES)
    assert sorted({k.rsplit("/", 1)[0] for k in recorded["main"]}) == sorted(R.MAIN_CASES)
    assert recorded["dropped"] == []
    for name in R.EPOCH_CASES:
        want = fields(recorded, "epoch", name)
        assert ("raised" in want) == (name.startswith("raises-") or name == "staged-v1"), name     # (a V1 step takes encoded points: the staged route has none)
        assert name.startswith("raises-") or len(want["calls"]) > 0


@pytest.mark.parametrize("name", sorted(R.EPOCH_CASES))
def test_train_epoch_makes_the_recorded_calls(recorded, name):
    want, got = fields(recorded, "epoch", name), R.epoch_case(name)
    assert sorted(got) == sorted(want)
    assert [c["call"] for c in got["calls"]] == [c["call"] for c in want["calls"]]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert R.matches(g, w, f"{name}/calls[{i}]") is None
    for field in want:
        assert R.matches(got[field], want[field], f"{name}/{field}") is None


@pytest.mark.parametrize("name", sorted(R.MAIN_CASES))
def test_main_leaves_what_was_recorded(recorded, name, tmp_path):
    want, got = fields(recorded, "main", name), R.main_case(name, str(tmp_path))
    assert sorted(got) == sorted(want)
    for field in want:
        assert R.matches(got[field], want[field], f"{name}/{field}") is None
