"""The shared arithmetic of poppunk_amd/csrc/ppk_device.h that the host can run (the condensed and lower-triangle
index maps, the float order keys, ceil_log2, chol2): device_helpers_host.hip, built for the host alone with the
undefined-behaviour and address sanitizers, and run.  No GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_device_helpers_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "device_helpers_host")
    # The sanitizers are for the host code alone: -Xarch_host keeps them off any device pass.
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O2", "-std=c++17",
                          "-Xarch_host", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                          os.path.join(HERE, "device_helpers_host.hip"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-2000:]
    assert " 0 wrong" in run.stdout
