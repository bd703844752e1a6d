"""CPU: the failure contract of the resource owners (csrc/owned.hpp), checked by a stand-alone
host program under ASan/UBSan on a machine without a HIP device, where every HIP allocation fails
cleanly."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_keep_their_failure_contract_without_a_device(tmp_path):
    """tests/owned_host_check.cpp: a failed grow returns GS_ERR_NOMEM, leaves pointer and capacity
    empty and sets the last error; a second grow tries again; moving empties the source; empty
    owners destroy as a no-op; a group whose creation fails leaves its destination untouched."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the allocations under test would succeed")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / "owned_host")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "gelly-streaming_amd", "csrc"), os.path.join(ROOT, "tests", "owned_host_check.cpp"),
                    "-o", exe, "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "owned_host_check OK (no device)" in out.stdout
