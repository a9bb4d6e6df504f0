"""The census of launch geometry of the staged, hierarchical, regulariser and shared training kernels: for every
`hipLaunchKernelGGL(` of FILES either a row of ROWS -- the cap of the grid (or the round of a single-workgroup kernel) as its text
stands in the source, the items one workgroup takes per trip, and the ragged tail the GPU tests add -- or an entry of UNCAPPED with
the reason why there is no second regime to enter.

tests/test_launch_geometry_host.py holds the table to the sources (no GPU); tests/test_gpu_launch_geometry.py takes every size from
size() / reach(), so a cap that changes in the source fails the host test until `cap_text` follows, and the GPU shapes then move
with it.  An item is what the kernel's outer loop counts: a ray for the wave-per-ray kernels (a 256-thread workgroup holds 4
waves), a sample for the 16-lanes-per-sample fetch adjoint (16 per workgroup), an element otherwise -- read from each kernel's
loop, not from its launch expression (n_rays * 64 and n * kFetchPtLanes count threads)."""
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nerf_few_shot_limitations_amd", "csrc")
FILES = ("staged_kernels.hip", "hier_kernels.hip", "hier_train.hip", "ray_reg.hip", "train_shared.hip")

# file: where the launch is; kernel: the first argument of hipLaunchKernelGGL as written; cap_text: a piece of source that ends in
# the cap -- workgroups, or for `round` rows the items of one round of a single workgroup; scope: None = the launch's own function,
# otherwise (file, text) naming the function that holds cap_text; items: items per workgroup and trip; tail: what the GPU tests add
# to cap x items; unit: what an item is
Row = namedtuple("Row", "file kernel cap_text scope items tail unit")

WAVE_RAYS = "grid_for(n_rays * 64, kBlock, 16384)"
WORK_RAYS = "grid_for(work, kBlock, 16384)"
PDF_SCOPE = ("sample_pdf_impl.hpp", "inline bool sample_pdf_grid(")
ADAM_SCOPE = ("train_shared.hip", "static unsigned adam_blocks(")
ROUND = "dim3(1), dim3(1024)"

ROWS = [
    # staged_kernels.hip
    Row("staged_kernels.hip", "fetch_backward_reduce_kernel", "grid_for(elems, kBlock, 4096)", None, 256, None, "map element"),
    Row("staged_kernels.hip", "fetch_points_backward_kernel<true>", "grid_for(n * kFetchPtLanes, kBlock, 8192)", None, 16, 37, "sample"),
    Row("staged_kernels.hip", "fetch_points_backward_kernel<false>", "grid_for(n * kFetchPtLanes, kBlock, 8192)", None, 16, 37, "sample"),
    Row("staged_kernels.hip", "occupancy_compact_count_kernel", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "occupancy_compact_scan_kernel", ROUND, None, 1, 1, "ray of a round"),
    Row("staged_kernels.hip", "occupancy_compact_write_kernel", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "occupancy_mark_kernel<true>", WAVE_RAYS, None, 4, None, "ray"),
    Row("staged_kernels.hip", "occupancy_mark_kernel<false>", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "occupancy_pack_kernel", "grid_for(n_cells, kBlock, 8192)", None, 256, 96, "cell"),
    Row("staged_kernels.hip", "occupancy_dilate_kernel", "grid_for((int64_t)wx * res[1] * res[2], kBlock, 8192)", None, 256, None, "word"),
    Row("staged_kernels.hip", "get_rays_kernel", "grid_for(n, kBlock, 4096)", None, 256, None, "ray"),
    Row("staged_kernels.hip", "sample_kernel", "grid_for(n_rays * S, kBlock, 8192)", None, 256, None, "sample"),
    Row("staged_kernels.hip", "encode_kernel", "grid_for(total, kBlock, 8192)", None, 256, None, "output element"),
    Row("staged_kernels.hip", "composite_kernel", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "composite_backward_geom_kernel", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "ray_grad_kernel", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "composite_backward_kernel", WAVE_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "composite_loss_backward_kernel<false>", WORK_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "indexed_loss_backward_kernel", WORK_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "composite_loss_backward_kernel<true>", WORK_RAYS, None, 4, 37, "ray"),
    Row("staged_kernels.hip", "mse_grad_kernel", ROUND, None, 1, 1, "value of a round"),
    Row("staged_kernels.hip", "sample_pdf_kernel", "g.blocks = 256 * 16", PDF_SCOPE, 4, 5, "ray"),
    Row("staged_kernels.hip", "project_fetch_kernel", "grid_for(n * d.C, kBlock, 8192)", None, 256, None, "feature"),
    Row("staged_kernels.hip", "project_fetch_kernel", "grid_for(n * C, kBlock, 8192)", None, 256, None, "feature"),
    # hier_kernels.hip: the merging compositor is one THREAD per ray
    Row("hier_kernels.hip", "composite_merge_kernel<true>", "blocks < 16384 ? blocks : 16384", None, 256, 37, "ray"),
    Row("hier_kernels.hip", "composite_merge_kernel<false>", "blocks < 16384 ? blocks : 16384", None, 256, 37, "ray"),
    Row("hier_kernels.hip", "sample_pdf_sorted_kernel", "g.blocks = 256 * 16", PDF_SCOPE, 4, 5, "ray"),
    # hier_train.hip
    Row("hier_train.hip", "merge_gather_kernel", "grid_for(N, kBlock, 16384)", None, 256, None, "sample of the union"),
    Row("hier_train.hip", "scatter_add_kernel", "grid_for(N, kBlock, 16384)", None, 256, None, "sample of the union"),
    # ray_reg.hip
    Row("ray_reg.hip", "reg_loss_backward_kernel<true>", WORK_RAYS, None, 4, 37, "ray"),
    Row("ray_reg.hip", "reg_loss_backward_kernel<false>", WORK_RAYS, None, 4, 37, "ray"),
    Row("ray_reg.hip", "ray_terms_finish_kernel", ROUND, None, 1, 1, "ray of a round"),
    # train_shared.hip
    Row("train_shared.hip", "repack3_kernel", "blocks < 4096 ? blocks : 4096", None, 256, None, "work item"),
    Row("train_shared.hip", "adam_kernel<false>", "(n + 255) / 256 : 4096", ADAM_SCOPE, 256, 300, "parameter"),
    Row("train_shared.hip", "adam_kernel<true>", "(n + 255) / 256 : 4096", ADAM_SCOPE, 256, 300, "parameter"),
    # the weight gradient: not a grid cap but the batch size (in 32-sample tiles) from which wgrad_grid deals two rounds of workgroups
    Row("train_shared.hip", "kernel", "n_tiles32 >= 8192", ("train_impl.hpp", "inline int wgrad_grid("), 32, None, "sample"),
    Row("train_shared.hip", "weight_grad_reduce_kernel", "n_tiles32 >= 8192", ("train_impl.hpp", "inline int wgrad_grid("), 32, None, "sample"),
]

# launches with no cap and no trip loop over the grid: (file, kernel) -> reason
UNCAPPED = {
    ("staged_kernels.hip", "project_fetch_backward_kernel"):
        "grid = (texel chunks x channel chunks, slabs) from fetch_bwd_geo, a function of the sizes alone; a workgroup owns one slab of "
        "samples and walks it 64 at a time at every n -- no stride over the grid, and the slab walk runs in every existing test",
    ("train_shared.hip", "grad_sqnorm_partials_kernel"):
        "sqnorm_partials(n) workgroups, at most kMaxSqnormPartials: every thread strides from the first element on (the cap only "
        "lengthens a double-precision chain); test_grad_norm_matches_float64_and_is_reproducible already runs n well past 256 x the grid",
}


def reach(row):
    """Items one trip of the whole grid (or one round of the single workgroup) covers: a kernel enters its second regime above it."""
    return cap(row) * row.items


def cap(row):
    """The number `cap_text` ends in (digits, `*` and `<<` only)."""
    m = re.search(r"([0-9][0-9 *<]*)\)*$", row.cap_text)
    assert m, row.cap_text
    return int(eval(m.group(1), {"__builtins__": {}}))          # noqa: S307 -- digits and two operators, see the pattern


def row(kernel, file=None, cap_text=None):
    got = [r for r in ROWS if r.kernel == kernel and (file is None or r.file == file) and (cap_text is None or r.cap_text == cap_text)]
    assert got and all(reach(r) == reach(got[0]) for r in got), kernel
    return got[0]


def size(kernel, **kw):
    """The smallest count the GPU tests use to enter `kernel`'s second regime: reach + the row's ragged tail."""
    r = row(kernel, **kw)
    assert r.tail is not None, f"{kernel}: the GPU file shapes this case itself (see SHAPED)"
    return reach(r) + r.tail


# ---- the shapes the GPU file builds from more than one number, as functions of the rows ---------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


R_RAYS = size("composite_kernel")                                   # 65 536 + 37 rays for every wave-per-ray kernel
SHAPED = {
    # kernel: the count of items the GPU file's shape amounts to
    "fetch_backward_reduce_kernel": 130 * 128 * 64,
    "occupancy_mark_kernel<true>": 257 * 256,
    "occupancy_dilate_kernel": (512 // 32) * 512 * 257,
    "get_rays_kernel": 1025 * 1024,
    "sample_kernel": (reach(row("sample_kernel")) // 64 + 1) * 64,
    "encode_kernel": (_ceil_div(reach(row("encode_kernel")), 63) + 7) * 63,
    "project_fetch_kernel": (reach(row("project_fetch_kernel", cap_text="grid_for(n * d.C, kBlock, 8192)")) // 64 + 5) * 64,
    "merge_gather_kernel": R_RAYS * 65,
    "scatter_add_kernel": R_RAYS * 65,
    # reached through a model's parameter count alone: the fp32 mode re-packs one work item per stream element, and a V3 model
    # (64-d features, 8 layers of 256) has 946 176 + 901 120 of them and 3936 biases (V2: 1 178 112 in all; V1: 952 352, below)
    "repack3_kernel": 946176 + 901120 + 3936,
}
# not shaped here: the training chain -- its batch comes from nrf_train_context_bytes at run time (the smallest multiple of 1000 with
# tiles32(n) >= the row's cap whose context passes 2^32 bytes), and the GPU file asserts both conditions itself
RUNTIME_SHAPED = {"kernel", "weight_grad_reduce_kernel"}          # (`kernel`: run_weight_grad launches weight_grad_kernel<Mode, ST> by that name)
