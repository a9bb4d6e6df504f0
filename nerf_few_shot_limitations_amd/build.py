"""Build libnerfhip.so (gfx950) in-tree with hipcc.

    python -m nerf_few_shot_limitations_amd.build [--force]

hipcc cross-compiles for gfx950 without a GPU, so this runs in the build
container; the resulting .so (git-ignored) travels to the GPU box with the
repository snapshot.  There is exactly one target architecture and no fallback.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
OBJ = os.path.join(PKG, "build")
LIB = os.path.join(PKG, "libnerfhip.so")
INCLUDE = os.path.join(os.path.dirname(PKG), "include")

# Every kind of the fused renderer / forward of every network family is compiled twice (fused_impl.hpp, NRF_TU_HALF): once for the 16-bit
# MFMA modes -- with VGPR-form MFMAs, so that the pinned walk can park finished operand images in the AGPR half of the register
# file (mlp_core.hpp NRF_PARK_ACT) -- and once for the fp32-class modes (split-f16, fp32 MFMA) with hipcc's own choice.
HALF16 = ["-DNRF_TU_HALF=16", "-DNRF_ACT_AGPR=1", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]
HALF32 = ["-DNRF_TU_HALF=32"]
# The instantiations of the fused renderer are one source, fused_inst.hip, compiled once per (kind, family, half): -DNRF_KIND picks the
# body, -DNRF_FAMILY the row of the family table (fused_impl.hpp: NRF_FAMILIES -- FAMILIES names its rows), the half's flags the modes.
# An occ or emit object carries the half flags of its fused_<family> sibling.  Tail mode's last-sample kernels (split-f16 only) are one
# object for all four families (-DNRF_FAMILY=all).  A new family is a row there and a name here; a new kind a body there and a row of KINDS.
FAMILIES = ("v1", "v2", "v3", "v3w")
HALVES = (("16", HALF16), ("32", HALF32))
# kind: (object name stem, per family and half?)
KINDS = {"plain": ("fused", True), "occ": ("fused_occ", True), "emit": ("fused_emit", True), "tail": ("fused_tail", False)}
FUSED = [("fused_inst.hip", f"{stem}_{fam}_{half}", [*flags, f"-DNRF_KIND={kind}", f"-DNRF_FAMILY={fam}"])
         for kind, (stem, split) in KINDS.items() if split for fam in FAMILIES for half, flags in HALVES]
FUSED += [("fused_inst.hip", stem, [*HALF32, f"-DNRF_KIND={kind}", "-DNRF_FAMILY=all"]) for kind, (stem, split) in KINDS.items() if not split]
SOURCES = FUSED + [(f, os.path.splitext(f)[0], []) for f in
                   ("fused_kernels.hip", "hier_kernels.hip", "train_rays_indexed_v1.hip", "train_rays_indexed_v2.hip", "train_rays_indexed_v3.hip",
                    "train_shared.hip", "train_v1.hip", "train_v2.hip", "train_v3.hip", "train_dino_grad.hip", "train_input_grad.hip",
                    "train_input_grad_v3.hip", "staged_kernels.hip", "api.cpp", "packing.cpp")]
# Units built into a sub-directory of the object directory: (source, object name, flags, sub-directory) -- the object, its .d, .cmd and
# .remarks live there, the object is linked into the same library.  kernel_resources() reads one directory and does not recurse, so
# such a unit keeps a census of its own (tests/golden/kernel_resources_hier_train.json) beside the closed one of the main directory
# (tests/golden/kernel_resources.json), and SOURCES stays the table of the main directory's objects.
HIER_TRAIN_DIR = "hier_train"
SUBDIR_SOURCES = [("hier_train.hip", "hier_train", [], HIER_TRAIN_DIR)]
# The regularised loss launch (ray_reg.hip): a further sub-directory unit of the same shape, with its own census
# (tests/golden/kernel_resources_ray_reg.json).
RAY_REG_DIR = "ray_reg"
RAY_REG_SOURCES = [("ray_reg.hip", "ray_reg", [], RAY_REG_DIR)]
# The frequency mask's re-pack and weight-gradient reduce (freq_mask.hip): likewise (tests/golden/kernel_resources_freq_mask.json).
FREQ_MASK_DIR = "freq_mask"
FREQ_MASK_SOURCES = [("freq_mask.hip", "freq_mask", [], FREQ_MASK_DIR)]
# The loss launch with the patch-based depth-smoothness term (patch_reg.hip): likewise (tests/golden/kernel_resources_patch_reg.json).
PATCH_REG_DIR = "patch_reg"
PATCH_REG_SOURCES = [("patch_reg.hip", "patch_reg", [], PATCH_REG_DIR)]
# The loss launch with InfoNeRF's ray entropy and patch KL terms (info_reg.hip): likewise (tests/golden/kernel_resources_info_reg.json).
INFO_REG_DIR = "info_reg"
INFO_REG_SOURCES = [("info_reg.hip", "info_reg", [], INFO_REG_DIR)]
# -Rpass-analysis=kernel-resource-usage: the backend reports every kernel's registers / spills / scratch; kept beside the object
# (<name>.o.remarks, see kernel_resources()) so that a toolchain or flag change that breaks the AGPR parking or introduces
# spills in a headline kernel is caught by tests/test_kernel_resources.py
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
         "-fno-gpu-rdc", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", f"-I{INCLUDE}"]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libnerfhip.so cannot be built (ROCm toolchain required)")
    return exe


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths)


def _deps():
    # (build.py's flag lists -- VGPR-form MFMAs, AGPR parking, per-half defines -- decide the code too: every object records the
    # command that built it and is rebuilt when that changes, see _obj_fresh)
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))] + [os.path.join(INCLUDE, "nerfhip.h"), os.path.abspath(__file__)]


def _obj_fresh(obj: str, cmd_key: str) -> bool:
    """An object is reused when the command that built it is unchanged (recorded beside it: flag lists are part of the code) and it
    is newer than every file hipcc read for it (its -MD dependency list: the source and the headers it includes)."""
    dep, key = obj + ".d", obj + ".cmd"
    if not (os.path.exists(obj) and os.path.exists(dep) and os.path.exists(key)):
        return False
    with open(key) as f:
        if f.read() != cmd_key:
            return False
    with open(dep) as f:
        words = f.read().replace("\\\n", " ").split()
    files = [w for w in words[1:] if not w.endswith(":")]
    t = os.path.getmtime(obj)
    return all(os.path.exists(p) and os.path.getmtime(p) <= t for p in files)


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile (what is stale) and return the path of libnerfhip.so."""
    deps = _deps()
    # fast path (and the only one on the GPU box, where the object directory does not travel): the library is newer than every
    # source, header and this file
    if not force and os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest(deps):
        return LIB
    os.makedirs(OBJ, exist_ok=True)

    def one(item):
        src, name, flags, *sub = item
        obj = os.path.join(OBJ, *sub, name + ".o")
        os.makedirs(os.path.dirname(obj), exist_ok=True)
        cmd = [hipcc(), *FLAGS, *flags, "-MD", "-MF", obj + ".d", "-c", os.path.join(CSRC, src), "-o", obj]
        cmd_key = " ".join(cmd)
        if not force and _obj_fresh(obj, cmd_key):
            return obj, False
        if verbose:
            print(cmd_key, flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        with open(obj + ".remarks", "w") as f:
            f.write(r.stderr)
        with open(obj + ".cmd", "w") as f:
            f.write(cmd_key)
        return obj, True

    with cf.ThreadPoolExecutor(max_workers=os.cpu_count() or 8) as ex:
        res = list(ex.map(one, [*SOURCES, *SUBDIR_SOURCES, *RAY_REG_SOURCES, *FREQ_MASK_SOURCES, *PATCH_REG_SOURCES, *INFO_REG_SOURCES]))
    objs = [o for o, _ in res]
    if not any(built for _, built in res) and os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest(objs):
        os.utime(LIB)          # nothing to do (e.g. only a comment of this file changed): restore the fast path
        return LIB
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB + ".tmp", *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    os.replace(LIB + ".tmp", LIB)
    return LIB


def kernel_resources(obj_dir: str = OBJ):
    """{demangled kernel name: {'vgprs', 'agprs', 'sgprs', 'scratch', 'vgpr_spill', 'sgpr_spill', 'occupancy', 'tu'}} of the last build,
    parsed from the backend's kernel-resource-usage remarks (hipcc's stderr, saved per object)."""
    import re
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch", "VGPRs Spill": "vgpr_spill",
            "SGPRs Spill": "sgpr_spill", "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}
    out, mangled = {}, []
    for fn in sorted(os.listdir(obj_dir)):
        if not fn.endswith(".o.remarks"):
            continue
        cur = None
        with open(os.path.join(obj_dir, fn)) as f:
            for line in f:
                m = re.search(r"remark:\s+Function Name: (\S+)", line)
                if m:
                    cur = {"tu": fn[: -len(".o.remarks")]}
                    out[(fn, m.group(1))] = cur
                    mangled.append((fn, m.group(1)))
                    continue
                m = re.search(r"remark:\s+([A-Za-z ]+(?:\[[^\]]+\])?): (\d+)", line)
                if m and cur is not None and m.group(1).strip() in keys:
                    cur[keys[m.group(1).strip()]] = int(m.group(2))
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/usr/bin/c++filt"
    names = [n for _, n in mangled]
    if names and os.path.exists(filt):
        names = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {f"{out[k]['tu']}: {n}": out[k] for k, n in zip(mangled, names)}


if __name__ == "__main__":
    print(build(force="--force" in sys.argv[1:], verbose=True))
