"""The kernels that run behind a finished dZ chain -- dino_grad_kernel (nrf_mlp_backward_dino), input_grad_kernel
(nrf_mlp_backward_inputs) and input_grad_v3_kernel (nrf_mlp_backward_inputs_v3) -- held bit for bit to a record of their outputs.

tests/golden/post_grad_digests.json holds the SHA-256 of every output buffer of every case below, taken on an MI355X before the
resident-fragment prologue, the K walk, the adjoint of the encoding, the direction block and the launcher of these kernels were
each written once (csrc/train_post_grad_core.hpp, csrc/train_post_grad_launch.hpp).  The kernels use no atomics and fix every
order of summation, and the dZ slots the chain leaves are reproducible (test_bit_properties of the GPU files of these kernels
relies on the same), so the same inputs give the same bytes: a digest that moves is a change of the arithmetic or of what is
written where.  `python -m tests.test_gpu_post_grad_digests` prints the JSON of the library it runs on.

Weights: oracle.nerf_oracle.make_weights with n_layers = 2, so that the chain in front is cheap.  Inputs: uniform float64 draws of a
seeded torch.Generator on the CPU and exact arithmetic on them only, rounded to fp32 once.  Sizes, the smallest at which each
shared part can still go wrong: n = 1 (one live row, the others read the last sample), 31 / 32 / 33 (a ragged tile, a whole tile,
one tile plus one row), 129 (a second workgroup that holds one wave's tile) and 32 * 4 * 2 * CUs + 33 (one row past a full trip of
the persistent grid at two workgroups per CU: the grid-stride step is taken; the CU count is read from the device and recorded).
Every output has 32 spare rows, starts as NaN and is digested whole, so a write past n moves the digest.

Cases, each in bf16, f16 and f32: V1 d_x_enc / d_positions / both; V2 d_positions / d_directions / both with dir_freq 4 and 1; V3
positions / directions / both and nrf_mlp_backward_dino with dino_dim 64 and 128.  The chain is built for dir_freq 4 only, the
input gradient takes the frequency count at run time: the dir_freq 1 cases run a dir_freq 1 model's input gradient on the context
the dir_freq 4 model's chain left (the slots are laid out alike; to the kernel dZ(color_layers.0) is data)."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_grad_digests.json")
MODES = ("bf16", "f16", "f32")
CONFIGS = ("v1", "v2", "v3-64", "v3-128")
SMALL = (1, 31, 32, 33, 129)
SPARE = 32
WANTS = {"v1": ("x", "p", "xp"), "v2": ("p", "d", "pd"), "v3": ("p", "d", "pd")}
WIDTH = {"x": 63, "p": 3, "d": 3}


def cu_count():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def sizes():
    """(label, n): the label names the case in the record, whatever the device's CU count"""
    return [(str(n), n) for n in SMALL] + [("trip", 32 * 4 * 2 * cu_count() + 33)]


def case_ids(config):
    """(family, the tags its case ids start with): V2 runs its input gradient with dir_freq 4 and 1 on one context"""
    fam = config.split("-")[0]
    tags = {"v1": ["v1"], "v2": ["v2-df4", "v2-df1"], "v3": [config]}[fam]
    return fam, tags


def inputs(n, dino_dim, number):
    g = torch.Generator().manual_seed(31000 + number)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    f = lambda t: t.float().contiguous()
    return dict(pos=f(u(n, 3) * 4.0 - 2.0), dirs=f(u(n, 3) - 0.5), dino=f(u(n, max(dino_dim, 1)) * 2.0 - 1.0), g_rgb=f(u(n, 3) - 0.5),
                g_den=f(u(n, 1) - 0.5))


def make(N, fam, mode, dino_dim=0, dir_freq=4):
    if fam == "v1":
        m = N.NeRFMLP(pos_dim=63, hidden_dim=256, n_layers=2, mma_mode=mode)
        m.load_state_dict(O.make_weights("v1", 2, "solid", n_layers=2))
    elif fam == "v2":
        m = N.NeRFMLP(pos_freq=10, dir_freq=dir_freq, hidden_dim=256, num_density_layers=2, use_dino=False, mma_mode=mode)
        m.load_state_dict(O.make_weights("v2", 2, "solid", n_layers=2, dir_freq=dir_freq), strict=False)
    else:
        m = N.NeRFMLP(pos_freq=12, dir_freq=4, hidden_dim=256, num_density_layers=2, use_dino=True, dino_dim=dino_dim, mma_mode=mode)
        m.load_state_dict(O.make_weights("v3", 2, "solid", n_layers=2, dino_dim=dino_dim), strict=False)
    return m.cuda().train()


def digest(t):
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def run(N, L, config, mode):
    """Every size and every output choice of one configuration in one mode, one chain run per size ->
    {case id: {buffer: (digest, rows < n finite and rows >= n still NaN)}}"""
    from nerf_few_shot_limitations_amd import training as TR
    fam, tags = case_ids(config)
    dino_dim = int(config.split("-")[1]) if fam == "v3" else 0
    dev = torch.device("cuda", torch.cuda.current_device())
    lib, st = L.lib(), L.stream_ptr()
    model = make(N, fam, mode, dino_dim)
    h, md = TR._train_handle(model, dev)
    handles = {tags[0]: h}
    if fam == "v2":
        low = make(N, fam, mode, dir_freq=1)            # kept alive with its handle
        handles[tags[1]] = TR._train_handle(low, dev)[0]
    out = {}
    for number, (label, n) in enumerate(sizes()):
        x = inputs(n, dino_dim, number)
        nbytes = int(lib.nrf_train_context_bytes(h, md, n))
        assert nbytes > 0 and all(int(lib.nrf_train_context_bytes(q, md, n)) == nbytes for q in handles.values())
        buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        grad = torch.zeros_like(model.flat_params().flat)
        cb = C.c_void_p(buf.data_ptr())
        pc, dc, fc, gr, gd = (x[k].cuda() for k in ("pos", "dirs", "dino", "g_rgb", "g_den"))
        if fam == "v1":
            enc = N.PositionalEncoding(10)(pc).contiguous()
            o4 = torch.empty((n, 4), device=dev)
            g4 = torch.cat([gr, gd], -1).contiguous()
            L.check(lib.nrf_mlp_forward_train_v1(h, md, L.ptr(enc), n, L.ptr(o4), cb, nbytes, st))
            L.check(lib.nrf_mlp_backward_v1(h, md, L.ptr(o4), L.ptr(g4), n, cb, nbytes, L.ptr(grad), st))
        else:
            rgb, den = torch.empty((n, 3), device=dev), torch.empty((n, 1), device=dev)
            L.check(lib.nrf_mlp_forward_train(h, md, L.ptr(pc), L.ptr(dc), L.ptr(fc) if fam == "v3" else None, n, L.ptr(rgb), L.ptr(den), cb, nbytes, st))
            L.check(lib.nrf_mlp_backward(h, md, L.ptr(rgb), L.ptr(den), L.ptr(gr), L.ptr(gd), n, cb, nbytes, L.ptr(grad), st))
        nan = lambda w: torch.full((n + SPARE, w), float("nan"), device=dev)
        for tag, q in handles.items():
            for want in WANTS[fam]:
                bufs = {k: nan(WIDTH[k]) for k in want}
                p = lambda k: L.ptr(bufs[k]) if k in bufs else None
                if fam == "v3":
                    L.check(lib.nrf_mlp_backward_inputs_v3(q, md, n, cb, nbytes, L.ptr(pc), L.ptr(dc), p("p"), p("d"), st))
                else:
                    L.check(lib.nrf_mlp_backward_inputs(q, md, n, cb, nbytes, L.ptr(pc), L.ptr(dc) if fam == "v2" else None, p("x"), p("p"), p("d"), st))
                out[f"{tag}-{mode}-n{label}-{want}"] = bufs
            if fam == "v3":
                bufs = {"f": nan(dino_dim)}
                L.check(lib.nrf_mlp_backward_dino(q, md, n, cb, nbytes, L.ptr(bufs["f"]), st))
                out[f"{tag}-{mode}-n{label}-dino"] = bufs
        torch.cuda.synchronize()
        for key in [k for k in out if f"-n{label}-" in k]:
            res = {}
            for name, t in out[key].items():
                t = t.cpu()
                # the d_x_enc rows are written whole: pe_ref_index covers all 63 columns
                res[name] = (digest(t), bool(torch.isfinite(t[:n]).all()) and bool(torch.isnan(t[n:]).all()))
            out[key] = res
    return out


@pytest.fixture(scope="module")
def NL():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import nerf_few_shot_limitations_amd as N
    from nerf_few_shot_limitations_amd import _lib as L
    L.lib()
    return N, L


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def expected_ids(config, mode):
    fam, tags = case_ids(config)
    ids = [f"{tag}-{mode}-n{label}-{want}" for tag in tags for label in [str(n) for n in SMALL] + ["trip"] for want in WANTS[fam]]
    if fam == "v3":
        ids += [f"{config}-{mode}-n{label}-dino" for label in [str(n) for n in SMALL] + ["trip"]]
    return ids


def test_the_record_covers_the_cases(golden):
    want = {i for c in CONFIGS for m in MODES for i in expected_ids(c, m)}
    assert len(want) == (3 + 6 + 2 * 4) * 3 * 6 and set(golden["digests"]) == want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("config", CONFIGS)
def test_outputs_are_the_recorded_bits(NL, golden, config, mode):
    assert cu_count() == golden["cu_count"], "the record's largest case is one row past a trip of the grid on the recorded device"
    got = run(*NL, config, mode)
    assert sorted(got) == sorted(expected_ids(config, mode))
    ragged = sorted(f"{k}:{name}" for k, bufs in got.items() for name, (_, ok) in bufs.items() if not ok)
    assert not ragged, f"rows < n not finite or rows >= n written: {ragged}"
    moved = sorted(f"{k}:{name}" for k, bufs in got.items() for name, (d, _) in bufs.items() if golden["digests"][k].get(name) != d)
    assert not moved, f"{moved} differ from the record"
    assert all(set(golden["digests"][k]) == set(bufs) for k, bufs in got.items())


if __name__ == "__main__":
    import nerf_few_shot_limitations_amd as _N
    from nerf_few_shot_limitations_amd import _lib

    _lib.lib()
    rec = {}
    for _c in CONFIGS:
        for _m in MODES:
            for _k, _bufs in run(_N, _lib, _c, _m).items():
                assert all(ok for _, ok in _bufs.values()), _k
                rec[_k] = {name: d for name, (d, _) in _bufs.items()}
    print(json.dumps({"cu_count": cu_count(), "digests": rec}, indent=1, sort_keys=True))
