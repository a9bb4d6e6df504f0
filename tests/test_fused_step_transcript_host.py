"""The recorder of tests/test_gpu_fused_step_transcript.py rehearsed without a GPU: a fake library whose functions carry the real
argtypes of `_lib.SIGNATURES` stands where libnerfhip.so would, and every kind of argument the training host path hands over is
classified -- integers, floats rounded through their C type, null and non-null pointers in each form the callers use (None, 0, an
address, a c_void_p), structs by reference with pointer, array and nested-struct fields, and c_float arrays."""
import ctypes as C
import types

import pytest

from nerf_few_shot_limitations_amd import _lib as L
from tests.test_gpu_fused_step_transcript import CASES, Transcript, encode


def fake_library(names):
    """An object with one function per name: it carries the entry's argtypes, keeps what it was called with and returns 0."""
    lib = types.SimpleNamespace(received=[], helper=lambda: "not recorded")
    for name in names:
        def fn(*args, _name=name):
            lib.received.append((_name, args))
            return 0
        fn.restype, fn.argtypes = L.SIGNATURES[name]
        setattr(lib, name, fn)
    return lib


def f32(x):
    return C.c_float(x).value.hex()


def test_integers_floats_and_pointers():
    lib = fake_library(["nrf_adam_step_loss"])
    rec = Transcript(lib, L.SIGNATURES)
    args = (0x7f0000001000, C.c_void_p(0x7f0000002000), 0, None, 12345, 1e-3, 0.9, 0.999, 1e-8, 0.0, 2, C.c_void_p(None), 2 ** 33, 1.0, 4096, None)
    assert rec.nrf_adam_step_loss(*args) == 0
    assert lib.received == [("nrf_adam_step_loss", args)]                  # forwarded untouched
    assert rec.calls == [["nrf_adam_step_loss", "ptr", "ptr", "null", "null", 12345, f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.0), 2,
                          "null", 2 ** 33, f32(1.0), "ptr", "null"]]
    assert f32(1e-3) != (1e-3).hex() and float.fromhex(f32(1e-3)) == C.c_float(1e-3).value      # rounded to the C type, exactly
    assert rec.helper() == "not recorded" and len(rec.calls) == 1          # only nrf_* calls are kept


def test_float_kinds_round_through_their_own_type():
    assert encode(C.c_double, 0.1) == (0.1).hex() and encode(C.c_float, 0.1) == f32(0.1) != (0.1).hex()
    assert encode(C.c_float, C.c_float(0.25)) == (0.25).hex()
    assert encode(C.c_int, C.c_int(7)) == 7 and encode(C.c_int64, 2 ** 40) == 2 ** 40 and encode(C.c_int32, True) == 1
    assert encode(C.c_uint64, 2 ** 64 - 1) == 2 ** 64 - 1
    assert encode(C.c_float * 3, (C.c_float * 3)(1.0, 0.1, -2.0)) == [f32(1.0), f32(0.1), f32(-2.0)]
    assert encode(C.c_int32 * 3, (C.c_int32 * 3)(32, 8, 8)) == [32, 8, 8]


def test_structs_by_reference_are_walked():
    lib = fake_library(["nrf_info_terms_finish", "nrf_composite_hier_loss_backward"])
    rec = Transcript(lib, L.SIGNATURES)
    lo = L.loss_opts(1.0, 1e-4, 0.0, None, 0.1, 0xdead000, 10)
    reg, patch, info = L.ray_reg(1e-2, 0.25, 0.0, 0), L.patch_reg(0.1, 2, 2), L.info_reg(1e-3, 0.01, 1e-5)
    rec.nrf_info_terms_finish(0x1000, 16, 5, C.byref(lo), C.byref(reg), C.byref(patch), 0x2000, C.byref(info), 0x3000, 0x4000, 0x5000, None)
    name, *a = rec.calls[0]
    assert name == "nrf_info_terms_finish" and a[:3] == ["ptr", 16, 5] and a[6:7] + a[8:] == ["ptr", "ptr", "ptr", "ptr", "null"]
    assert a[3] == {"struct_bytes": C.sizeof(L.nrf_loss_opts), "rgb_weight": f32(1.0), "reg_weight": f32(1e-4), "depth_weight": f32(0.0),
                    "target_depth": "null", "noise_std": f32(0.1), "noise": "ptr", "rng_seed": 10}
    assert a[4] == {"struct_bytes": C.sizeof(L.nrf_ray_reg), "dist_weight": f32(1e-2), "dist_inv_span": f32(0.25), "occ_weight": f32(0.0),
                    "occ_samples": 0}
    assert a[5] == {"struct_bytes": C.sizeof(L.nrf_patch_reg), "depth_smooth_weight": f32(0.1), "patch_size": 2, "n_patches": 2}
    assert a[7] == {"struct_bytes": C.sizeof(L.nrf_info_reg), "ent_weight": f32(1e-3), "ent_threshold": f32(0.01), "kl_weight": f32(1e-5)}
    h = L.hier_loss(white_bkgd=1, rgb_stride=4, rgb_coarse=0x1000, w_coarse=0.3, zero_n=2 ** 35)
    rec.nrf_composite_hier_loss_backward(C.byref(h), 8, 5, 3, 0)
    name, hs, *rest = rec.calls[1]
    assert rest == [8, 5, 3, "null"] and set(hs) == {f for f, _ in L.nrf_hier_loss._fields_}
    assert (hs["rgb_coarse"], hs["sigma_coarse"], hs["w_coarse"], hs["w_fine"], hs["zero_n"], hs["white_bkgd"]) == ("ptr", "null", f32(0.3), f32(0.0), 2 ** 35, 1)


def test_arrays_pointer_fields_and_null_structs():
    lib = fake_library(["nrf_mlp_forward_train_rays", "nrf_occupancy_compact_rays", "nrf_project_fetch"])
    rec = Transcript(lib, L.SIGNATURES)
    c2w = [0.1 * i for i in range(12)]
    rays = L.train_rays(pixels=0x1000, H=8, W=8, focal=8.0, c2w=c2w, z_vals=0x2000)
    dino = L.nrf_dino(features=0x3000, Hp=9, Wp=9, C=64, focal=8.0, H=8, W=8)
    dino.inv_pose = (C.c_float * 16)(*[float(i) for i in range(16)])
    opts = L.nrf_render_opts(near=2.0, far=6.0, n_samples=5, perturb=1, z_ladder=0x4000, rng_seed=3)
    rec.nrf_mlp_forward_train_rays(C.c_void_p(0x10), C.byref(rays), 8, C.byref(opts), 0x5000, None, C.c_void_p(0x6000), 4096, 0)
    a = rec.calls[0][1:]
    assert a[0] == "ptr" and a[2] == 8 and a[4:] == ["ptr", "null", "ptr", 4096, "null"]
    assert a[1]["c2w"] == [f32(x) for x in c2w] and a[1]["pixels"] == "ptr" and a[1]["rays_o"] == "null" and a[1]["focal"] == f32(8.0)
    assert a[3]["dino"] == "null" and a[3]["t_rand"] == "null" and a[3]["z_ladder"] == "ptr" and a[3]["rng_seed"] == 3 and a[3]["near"] == f32(2.0)
    opts.dino = C.pointer(dino)                                            # a pointer field that is set: the struct behind it
    occ = L.occupancy(bits=0x7000, res=(32, 8, 8), lo=(-8.0, -8.0, -8.0), scale=(2.0, 0.5, 0.5))
    cp = L.compact(40, 0x1, 0x2, 0x3, None, 0x4, 0x5, 256)
    rec.nrf_occupancy_compact_rays(C.byref(rays), 8, C.byref(opts), C.byref(occ), C.byref(cp), None)
    a = rec.calls[1][1:]
    assert a[2]["dino"]["inv_pose"] == [float(i).hex() for i in range(16)] and a[2]["dino"]["features"] == "ptr" and a[2]["dino"]["C"] == 64
    assert a[3]["res"] == [32, 8, 8] and a[3]["lo"] == [f32(-8.0)] * 3 and a[3]["scale"] == [f32(2.0), f32(0.5), f32(0.5)] and a[3]["stats"] == "null"
    assert a[4]["capacity"] == 40 and a[4]["directions"] == "null" and a[4]["positions"] == "ptr" and a[4]["workspace_bytes"] == 256
    rec.nrf_project_fetch(None, 0x1000, 4, 0x2000, None, None)             # a struct pointer may be null, too
    assert rec.calls[2] == ["nrf_project_fetch", "null", "ptr", 4, "ptr", "null", "null"]
    rec.nrf_project_fetch(C.pointer(dino), 0x1000, 4, 0x2000, None, None)  # and pointer() reads like byref()
    assert rec.calls[3][1] == a[2]["dino"]


def test_a_call_with_the_wrong_number_of_arguments_is_caught():
    rec = Transcript(fake_library(["nrf_ray_terms_finish"]), L.SIGNATURES)
    with pytest.raises(AssertionError, match="nrf_ray_terms_finish"):
        rec.nrf_ray_terms_finish(0x1000, 8)


def test_case_names_are_well_formed():
    assert len(CASES) == len(set(CASES)) and all(n.split("-")[0] in ("v1", "v2", "v3") for n in CASES)
