"""The refusals of the C API that need a model (section `gpu` of tests/golden/api_refusals.json): the tables of
tests/test_api_refusals_host.py behind their model checks, on one real model of each family at the smallest sizes the plans
accept and 64 samples -- the render entries' checks of the options, the emitting output and the tail, the family checks of the
training entries, the side channel of the V3 network through a render and a ray-training entry, the context size at one byte
below nrf_train_context_bytes -- and, by hand, the backward entries after a changed frequency mask.  Recorded on an MI355X from
the library before the checks of api.cpp were each written once; `python -m tests.test_gpu_api_refusals` prints the JSON of the
library it runs on.

Every case is a refusal or an early NRF_OK: no kernel of the project runs apart from what nrf_model_create and the training
set-up launch themselves, and no pointer is passed that the device would read (they are aligned integers).  The cases keep the
last gate in front of each launch shut -- the missing side channel of the V3 model for the renders, a context one byte short for
the training entries -- unless they are about that gate."""
import ctypes as C
import json
import sys

import pytest

from tests import test_api_refusals_host as T
from tests.test_api_refusals_host import L, N_GPU, P

pytestmark = pytest.mark.gpu
MODE = 1
# the backward entries of each family with arguments that are in order
BACKWARDS = {
    "v1": [("nrf_mlp_backward_v1", lambda m, nb: (m, MODE, P, P, N_GPU, P, nb, P, None)),
           ("nrf_mlp_backward_inputs", lambda m, nb: (m, MODE, N_GPU, P, nb, P, None, None, P, None, None))],
    "v2": [("nrf_mlp_backward", lambda m, nb: (m, MODE, P, P, P, P, N_GPU, P, nb, P, None)),
           ("nrf_mlp_backward_inputs", lambda m, nb: (m, MODE, N_GPU, P, nb, P, P, None, P, P, None))],
    "v3": [("nrf_mlp_backward", lambda m, nb: (m, MODE, P, P, P, P, N_GPU, P, nb, P, None)),
           ("nrf_mlp_backward_dino", lambda m, nb: (m, MODE, N_GPU, P, nb, P, None)),
           ("nrf_mlp_backward_inputs_v3", lambda m, nb: (m, MODE, N_GPU, P, nb, P, P, P, P, None))],
}


def create(h, fam):
    arch, arr, n, _ = T.NETS[fam]
    m = C.c_void_p()
    L.check(h.nrf_model_create(C.byref(m), 0, C.byref(arch), arr, n))
    return m


def record_gpu(h):
    models = {fam: create(h, fam) for fam in ("v1", "v2", "v3")}
    out = {}
    try:
        for spec in T.all_specs():
            for name, faults in T.cases(spec, True):
                assert name not in out, name
                out[name] = T.call(h, spec, faults, models[spec.fam].value)       # (the address itself: call() passes ctypes objects by reference)
        # a changed mask makes every mode's transposed weights older than the parameters: the dZ chains refuse to run on them
        for fam, m in models.items():
            nbytes = h.nrf_train_context_bytes(m, MODE, N_GPU)
            assert nbytes > 0
            out[f"nrf_model_set_freq_mask[{fam}]/changed"] = {"rc": h.nrf_model_set_freq_mask(m, T.fa(*([1.0] * 8 + [0.5])), None)}
            for entry, argv in BACKWARDS[fam]:
                rc = getattr(h, entry)(*argv(m, nbytes))
                out[f"{entry}[{fam}]/stale"] = {"rc": rc, "error": h.nrf_last_error().decode()} if rc < 0 else {"rc": rc}
    finally:
        for m in models.values():
            h.nrf_model_destroy(m)
    return out


@pytest.fixture(scope="module")
def golden():
    return T.load_golden()


def test_every_case_with_a_model_is_the_recorded_answer(golden):
    got = record_gpu(T.api())
    assert sorted(got) == sorted(golden["gpu"])
    wrong = {k: (v, golden["gpu"][k]) for k, v in got.items() if v != golden["gpu"][k]}
    assert not wrong, wrong


def test_no_case_reached_a_launch(golden):
    for name, rec in golden["gpu"].items():
        assert rec["rc"] in (0, -1), name
        assert rec["rc"] == 0 or (rec["error"] and "launch failed" not in rec["error"]), name


if __name__ == "__main__":
    got = record_gpu(T.api())
    table = T.messages_of(got)
    T.dump({"messages": table, "gpu": T.pack(got, table)}, sys.stdout)
