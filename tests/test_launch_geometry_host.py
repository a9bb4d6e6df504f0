"""The census of launch geometry (tests/launch_geometry.py) held to the sources, without a GPU: every hipLaunchKernelGGL of the
staged, hierarchical, regulariser and shared training units has a row or a reason, every row's cap still stands in its launch
function as the row quotes it, and every size tests/test_gpu_launch_geometry.py uses lies above cap x items."""
import os
import re

import pytest

from tests import launch_geometry as G


def source(name):
    with open(os.path.join(G.CSRC, name)) as f:
        return f.read()


def functions(text):
    """The top-level pieces of a source file: a piece ends with a line that starts with `}` (a function's, a struct's or a
    namespace's close), so a launch's piece is its launch function (with the comment in front of it)."""
    out, cur = [], []
    for line in text.splitlines():
        cur.append(line)
        if line.startswith("}"):
            out.append("\n".join(cur))
            cur = []
    if cur:
        out.append("\n".join(cur))
    return out


def launches(name):
    """[(kernel as written, the launch's function)] of one file, in source order."""
    out = []
    for fn in functions(source(name)):
        for m in re.finditer(r"hipLaunchKernelGGL\(\s*([^,]+?)\s*,", fn):
            out.append((m.group(1), fn))
    return out


def scope_text(row, own):
    if row.scope is None:
        return own
    file, marker = row.scope
    got = [fn for fn in functions(source(file)) if marker in fn]
    assert len(got) == 1, (row.scope, len(got))
    return got[0]


def test_every_launch_has_a_row_or_a_reason_and_every_cap_stands_in_its_function():
    seen_rows, seen_uncapped, n = set(), set(), 0
    for name in G.FILES:
        for kernel, fn in launches(name):
            n += 1
            if (name, kernel) in G.UNCAPPED:
                seen_uncapped.add((name, kernel))
                assert not any(r.file == name and r.kernel == kernel for r in G.ROWS), (name, kernel)
                continue
            rows = [r for r in G.ROWS if r.file == name and r.kernel == kernel]
            assert rows, f"{name}: the launch of {kernel} is in neither list of tests/launch_geometry.py"
            here = [r for r in rows if r.cap_text in scope_text(r, fn)]
            assert here, f"{name}: {kernel}: none of {[r.cap_text for r in rows]} occurs in its launch function any more"
            seen_rows.update(here)
    assert n >= len(set((r.file, r.kernel) for r in G.ROWS)) + len(G.UNCAPPED)   # the pattern still finds the launches
    assert seen_rows == set(G.ROWS), set(G.ROWS) - seen_rows                  # no row without a launch
    assert seen_uncapped == set(G.UNCAPPED), set(G.UNCAPPED) - seen_uncapped
    for reason in G.UNCAPPED.values():
        assert len(reason) > 40


def test_the_grid_function_of_the_resampling_kernels_is_in_the_census():
    text = scope_text(G.row("sample_pdf_kernel"), "")
    assert "g.waves = 4" in text and "60 * 1024" in text                      # what test_gpu_launch_geometry.pdf_waves restates
    assert G.reach(G.row("sample_pdf_kernel")) == G.reach(G.row("sample_pdf_sorted_kernel")) == 16384


@pytest.mark.parametrize("r", G.ROWS, ids=lambda r: f"{r.file}:{r.kernel}:{G.ROWS.index(r)}")
def test_the_gpu_files_size_exceeds_cap_times_items(r):
    assert G.cap(r) >= 1 and r.items >= 1
    if r.kernel in G.RUNTIME_SHAPED:
        assert r.tail is None and r.kernel not in G.SHAPED
        return
    used = G.SHAPED[r.kernel] if r.tail is None else G.reach(r) + r.tail
    assert used > G.reach(r), (r.kernel, used, G.reach(r))
    assert used < 2 * G.reach(r) + 4096, (r.kernel, used)                      # the smallest size that enters the regime, not more
    if r.tail is not None:
        assert r.kernel not in G.SHAPED and 0 < r.tail < 512


def test_items_per_workgroup_follow_the_kernels_loops():
    """items is what the kernel's outer loop counts per workgroup and trip, read from the kernel, not from the launch expression."""
    staged = source("staged_kernels.hip")
    assert "constexpr int kBlock = 256;" in staged and "constexpr int kFetchPtLanes = 16;" in staged
    assert "constexpr int kGroups = kBlock / kFetchPtLanes;" in staged         # 16 samples per workgroup
    assert G.row("fetch_points_backward_kernel<true>").items == 256 // 16
    wave_per_ray = [r for r in G.ROWS if r.cap_text in (G.WAVE_RAYS, G.WORK_RAYS)]
    assert len(wave_per_ray) >= 13 and all(r.items == 256 // 64 for r in wave_per_ray)
    # the merging compositor strides by threads, not by waves
    hier = source("hier_kernels.hip")
    assert "for (int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x; r < A.n_rays; r += (int64_t)gridDim.x * kBlock)" in hier
    assert G.row("composite_merge_kernel<false>").items == 256
    # the single-workgroup kernels step by the 1024 their launch names
    for name, kernel, step in (("staged_kernels.hip", "occupancy_compact_scan_kernel", "base += 1024"),
                               ("staged_kernels.hip", "mse_grad_kernel", "i += 1024"), ("ray_reg.hip", "ray_terms_finish_kernel", "i += 1024")):
        assert step in source(name) and G.reach(G.row(kernel)) == 1024
    shared = source("train_shared.hip")
    assert "for (; r + 7 * 256 < n; r += 8 * 256)" in shared                    # block_sum_fixed's unrolled loop: every thread runs it from 2048 values on
