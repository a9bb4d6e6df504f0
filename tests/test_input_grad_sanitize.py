"""The packer's part of the input gradient under AddressSanitizer + UndefinedBehaviorSanitizer (host code only):
tests/host/input_grad_sanitize.cpp builds the W0^T / color_layers.0^T plan, its streams and gather tables for the V1 and V2
networks -- alone and behind the backward chain's layers, as the device stream holds it.  A stand-alone program: nothing is
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_input_grad_packer_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "input_grad_san")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-D__host__=", "-D__device__=", f"-I{os.path.join(ROOT, 'include')}", "-o", exe,
           os.path.join(ROOT, "tests", "host", "input_grad_sanitize.cpp"), os.path.join(ROOT, "nerf_few_shot_limitations_amd", "csrc", "packing.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "asan" in (b.stderr + b.stdout).lower() and "cannot find" in (b.stderr + b.stdout).lower():
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "sanitize ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" ok:") == 6
