"""train_cli's flags pinned to a recording: tests/golden/train_cli_flags.json, made by tools/record_train_cli.py (which documents the
fixture) at commit 27dbe07 ("api.cpp: one copy of each argument check, one block of entries"), the parent of the commit that made
train_cli read each flag once.  The test passes at that parent and after it with the same file: it makes the recording again, with
the tool's own functions, and compares.

Pinned: what `main` ends in for every fragment and pair of fragments of FRAGMENTS against four configs (the refusal's text, or the
class of what the missing data set raises); what every *_args_error, *_options and draws_patches returns or raises on the empty
namespace, on every namespace holding one attribute and on every fragment's parsed namespace; the digest of --help; what
OccupancySchedule / PerViewOccupancy.from_args hand to the grids; the key set save_checkpoint writes.  Both recordings of the fixture
agreed on every field (its "dropped" list is empty).
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_cli_flags.json")


def load_recorder():
    spec = importlib.util.spec_from_file_location("record_train_cli", os.path.join(ROOT, "tools", "record_train_cli.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorder():
    return load_recorder()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fresh(recorder):
    return recorder.flags()


def test_the_fixture_holds_these_fragments_and_dropped_nothing(recorder, recorded):
    assert recorded["tables"]["fragments"] == recorder.NAMES
    assert recorded["dropped"] == []
    n = len(recorder.NAMES)
    assert len(recorded["main"]) == len(recorder.CONFIGS) * (n + 1)                               # every fragment, and no flag at all
    assert sum(len(row) for row in recorded["main"].values()) == len(recorder.CONFIGS) * (n * (n + 1) // 2 + 1)      # singles and pairs
    assert all(len(row) == len(recorder.FUNCTIONS) for row in recorded["functions"].values())
    assert recorded["tables"]["texts"][0] == "FileNotFoundError"                                  # an accepted argv dies on the missing data set
    assert recorded["help"]["columns"] == recorder.COLUMNS


@pytest.mark.parametrize("section", ["tables", "main", "functions", "help", "grids", "checkpoints"])
def test_flags_are_the_recorded_ones(recorder, recorded, fresh, section):
    assert sorted(fresh[section]) == sorted(recorded[section])
    for field, want in recorded[section].items():
        assert recorder.matches(fresh[section][field], want, f"{section}/{field}") is None


def test_build_parser_parses_what_main_parses(recorder):
    """The parser can be had without running main, and it is the one main uses.  (The recorded parent, which has no `flags_of`
    either, built its parser inside main: there is nothing to compare there.)"""
    from nerf_few_shot_limitations_amd import train_cli
    if not hasattr(train_cli, "flags_of"):
        return
    base = ["--config", "c.yaml", "--data", "d"]
    for frag in recorder.FRAGMENTS:
        assert repr(vars(train_cli.build_parser().parse_args(base + frag))) == repr(vars(recorder.parsed(base + frag)))
