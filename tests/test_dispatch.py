"""The render dispatcher's policy without a GPU: which kernel chain a frame
takes, with which parameters, and the workspace it needs
(csrc/rt_dispatch.cpp, include/rt_dispatch.h).  The GPU suite probes single
points of it through `rt.last_kernel()`; here every threshold is walked from
both sides on the CPU."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_dispatch_policy(tmp_path):
    """tests/dispatch_check.cpp, a stand-alone program built with the host
    sources under AddressSanitizer + UndefinedBehaviorSanitizer, as
    tests/test_hit_format.py builds hit_args_check."""
    csrc = REPO / "opencl-ray-tracer_amd" / "csrc"
    exe = tmp_path / "dispatch_check"
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", "-o", str(exe),
                    str(REPO / "tests" / "dispatch_check.cpp"), str(csrc / "rt_dispatch.cpp"),
                    str(csrc / "rt_args.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "dispatch check ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
