"""How a render launch's rays are dealt to the workgroups (csrc/ray_deal.hpp), replayed on the host through nrf_debug_ray_deal:
the export walks the deal with the functions render_march itself calls.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

CU = 256            # compute units of an MI355X
WAVES = 4


@pytest.fixture(scope="module")
def L():
    from nerf_few_shot_limitations_amd import _lib
    _lib.lib()
    return _lib


def deal(L, n_rays, S, cols, cu=CU):
    head = (C.c_int64 * 4)()
    n = C.c_int64(0)
    L.check(L.lib().nrf_debug_ray_deal(n_rays, S, cols, cu, head, None, 0, C.byref(n)))
    items = (C.c_int64 * (4 * max(n.value, 1)))()
    L.check(L.lib().nrf_debug_ray_deal(n_rays, S, cols, cu, head, items, n.value, C.byref(n)))
    it = np.ctypeslib.as_array(items).reshape(-1, 4)[: n.value].copy()
    return dict(even=bool(head[0]), spw_log2=int(head[1]), grid=int(head[2]), passes=int(head[3])), it


def passes_of(items, S, grid):
    per = np.zeros(grid, np.int64)
    for b, _, _, l in items:
        per[b] += -(-S // (1 << l))
    return per


def check_cover(items, n_rays, cols):
    """Every ray belongs to exactly one work item; an item of split l is WAVES * (cols >> l) rays; only the launch's last item
    may reach past the last ray, and by less than one unit in the even deal."""
    order = np.argsort(items[:, 1], kind="stable")
    first, rays, l = items[order, 1], items[order, 2], items[order, 3]
    assert first[0] == 0 and np.array_equal(first[1:], (first + rays)[:-1])
    assert np.array_equal(rays, WAVES * (cols >> l)) and l.min() >= 0 and (cols >> l).min() >= 1
    assert first[-1] < n_rays <= first[-1] + rays[-1]


def test_headline_frame_is_dealt_in_the_ideal_number_of_passes(L, monkeypatch):
    monkeypatch.delenv("NRF_SPW", raising=False)
    n_rays, S = 800 * 800, 64
    h, it = deal(L, n_rays, S, 64)
    assert h["even"] and h["grid"] == CU and h["passes"] == 625                 # 160 000 column-filling passes over 256 workgroups
    check_cover(it, n_rays, 64)
    per = passes_of(it, S, CU)
    assert per.max() == 625 and per.min() == 625
    wg0 = it[it[:, 0] == 0]
    assert list(wg0[:, 2]) == [256] * 9 + [128, 64, 4] and list(wg0[:, 3]) == [0] * 9 + [1, 2, 6]
    assert np.array_equal(wg0[:, 1], np.concatenate([[0], np.cumsum(wg0[:-1, 2])]))      # one contiguous range, marched in order
    monkeypatch.setenv("NRF_SPW", "3")                                            # pinned: the uniform deal, 79 rounds x 8 passes
    h, it = deal(L, n_rays, S, 64)
    assert not h["even"] and h["spw_log2"] == 3 and h["passes"] == 79 * 8
    check_cover(it, n_rays, 64)
    assert passes_of(it, S, CU).max() == 632
    monkeypatch.setenv("NRF_SPW", "0")
    h, it = deal(L, n_rays, S, 64)
    assert not h["even"] and h["spw_log2"] == 0 and h["passes"] == 10 * 64


@pytest.mark.parametrize("n_rays,S,cols,split", [(100 * 100, 32, 64, 5), (64 * 64, 48, 64, 4), (32 * 32, 32, 64, 5),
                                                 (100 * 100, 32, 32, 4), (64 * 64, 48, 32, 3), (32 * 32, 32, 32, 5)])
def test_small_frames_keep_the_uniform_deal(L, monkeypatch, n_rays, S, cols, split):
    """One short tile per workgroup either way: the even deal's pass count is not lower, the launch stays what it was."""
    monkeypatch.delenv("NRF_SPW", raising=False)
    h, it = deal(L, n_rays, S, cols)
    assert not h["even"] and h["spw_log2"] == split
    check_cover(it, n_rays, cols)
    assert passes_of(it, S, h["grid"]).max() == h["passes"]


def test_every_launch_is_covered_once_and_never_takes_more_passes(L, monkeypatch):
    """Seeded sweep over ray counts (ragged ones included), sample counts, both geometries and a few device sizes: the items tile
    the rays exactly, the ranges of the even deal differ by at most one unit of 4 rays, the reported pass count is the longest
    workgroup's, and the even deal is only ever taken where that count is lower than the uniform deal's own."""
    rng = np.random.default_rng(11)
    cases = [(159997, 32, 64, 256), (160000, 32, 32, 256), (160000, 33 - 1, 64, 256), (80000, 13, 64, 256), (5, 7, 64, 256), (1, 1, 32, 3)]
    for _ in range(150):
        cases.append((int(rng.integers(1, 900000)), int(rng.integers(1, 200)), int(rng.choice([32, 64])), int(rng.choice([8, 104, 256, 304]))))
    n_even = 0
    for n_rays, S, cols, cu in cases:
        monkeypatch.delenv("NRF_SPW", raising=False)
        h, it = deal(L, n_rays, S, cols, cu)
        check_cover(it, n_rays, cols)
        assert h["grid"] <= cu and set(it[:, 0]) == set(range(h["grid"]))
        assert passes_of(it, S, h["grid"]).max() == h["passes"], (n_rays, S, cols, cu)
        if h["even"]:
            n_even += 1
            per_wg = np.bincount(it[:, 0], weights=it[:, 2]).astype(np.int64)
            assert per_wg.max() - per_wg.min() <= WAVES and (per_wg % WAVES == 0).all()
            for b in range(h["grid"]):                                             # a range: contiguous, largest tiles first
                mine = it[it[:, 0] == b]
                assert np.array_equal(mine[1:, 1], (mine[:, 1] + mine[:, 2])[:-1]) and (np.diff(mine[:, 2]) <= 0).all()
            monkeypatch.setenv("NRF_SPW", str(h["spw_log2"]))
            hu, _ = deal(L, n_rays, S, cols, cu)
            assert not hu["even"] and h["passes"] < hu["passes"], (n_rays, S, cols, cu)
    assert n_even > 30
