"""The build's source table (no GPU, no compiler): build.SOURCES is derived from one tuple of families and one table of kinds, and
names the objects the library has always had."""
import os
import re

from nerf_few_shot_limitations_amd import build as B

# the object list of the build before the instantiation units became one source, spelled out
OBJECTS = [
    "fused_v1_16", "fused_v1_32", "fused_v2_16", "fused_v2_32", "fused_v3_16", "fused_v3_32", "fused_v3w_16", "fused_v3w_32",
    "fused_occ_v1_16", "fused_occ_v1_32", "fused_occ_v2_16", "fused_occ_v2_32", "fused_occ_v3_16", "fused_occ_v3_32", "fused_occ_v3w_16",
    "fused_occ_v3w_32",
    "fused_emit_v1_16", "fused_emit_v1_32", "fused_emit_v2_16", "fused_emit_v2_32", "fused_emit_v3_16", "fused_emit_v3_32",
    "fused_emit_v3w_16", "fused_emit_v3w_32",
    "hier_kernels", "train_rays_indexed_v1", "train_rays_indexed_v2", "train_rays_indexed_v3", "fused_tail",
    "fused_kernels", "train_shared", "train_v1", "train_v2", "train_v3", "train_dino_grad", "train_input_grad", "train_input_grad_v3",
    "staged_kernels", "api", "packing",
]


def _define(flags, name):
    got = [f.split("=", 1)[1] for f in flags if f.startswith(f"-D{name}=")]
    assert len(got) <= 1, flags
    return got[0] if got else None


def test_every_kind_family_and_half_is_built_exactly_once():
    cells = [(_define(fl, "NRF_KIND"), _define(fl, "NRF_FAMILY"), _define(fl, "NRF_TU_HALF")) for src, _, fl in B.SOURCES if src == "fused_inst.hip"]
    want = [(k, f, h) for k in ("plain", "occ", "emit") for f in ("v1", "v2", "v3", "v3w") for h in ("16", "32")] + [("tail", "all", "32")]
    assert sorted(cells, key=str) == sorted(want, key=str)
    # no other unit is compiled per kind, family or half
    assert all(fl == [] for src, _, fl in B.SOURCES if src != "fused_inst.hip")
    assert all(os.path.isfile(os.path.join(B.CSRC, src)) for src, _, _ in B.SOURCES)


def test_object_names_are_those_of_the_parent_build():
    names = [name for _, name, _ in B.SOURCES]
    assert len(names) == len(set(names)) == len(OBJECTS) == 40
    assert set(names) == set(OBJECTS)
    assert all(os.sep not in n and "/" not in n for n in names)                    # one object directory
    by_name = {name: fl for _, name, fl in B.SOURCES}
    for fam in ("v1", "v2", "v3", "v3w"):
        for half in ("16", "32"):
            for stem, kind in (("fused", "plain"), ("fused_occ", "occ"), ("fused_emit", "emit")):
                fl = by_name[f"{stem}_{fam}_{half}"]
                assert (_define(fl, "NRF_KIND"), _define(fl, "NRF_FAMILY"), _define(fl, "NRF_TU_HALF")) == (kind, fam, half)
    assert (_define(by_name["fused_tail"], "NRF_KIND"), _define(by_name["fused_tail"], "NRF_FAMILY")) == ("tail", "all")     # one object, every family


def test_occ_and_emit_objects_carry_their_siblings_flags():
    by_name = {name: [f for f in fl if not f.startswith("-DNRF_KIND=")] for _, name, fl in B.SOURCES}
    for fam in ("v1", "v2", "v3", "v3w"):
        assert "-amdgpu-mfma-vgpr-form=1" in by_name[f"fused_{fam}_16"] and "-DNRF_ACT_AGPR=1" in by_name[f"fused_{fam}_16"]
        assert "-amdgpu-mfma-vgpr-form=1" not in by_name[f"fused_{fam}_32"] and "-DNRF_ACT_AGPR=1" not in by_name[f"fused_{fam}_32"]
        for half in ("16", "32"):
            for stem in ("fused_occ", "fused_emit"):
                assert by_name[f"{stem}_{fam}_{half}"] == by_name[f"fused_{fam}_{half}"], (stem, fam, half)


def test_the_build_names_the_rows_of_the_family_table():
    text = open(os.path.join(B.CSRC, "fused_impl.hpp")).read()
    rows = re.findall(r"^#define NRF_FAMILY_(\w+)\(X\) X\((\w+),", text, re.M)
    assert [r[0] for r in rows] == [r[1] for r in rows] == list(B.FAMILIES)
    listed = re.search(r"^#define NRF_FAMILIES\(X\) (.*)$", text, re.M).group(1)
    assert re.findall(r"NRF_FAMILY_(\w+)\(X\)", listed) == list(B.FAMILIES)
