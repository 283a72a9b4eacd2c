"""The frame stores' cache policy without a GPU: the per-device record of the
frame targets a process recently rendered to (rt_dispatch::track_target in
csrc/rt_dispatch.cpp) and the policy choose() takes from the working set.
The GPU side is tests/test_gpu_store_policy.py."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / "opencl-ray-tracer_amd" / "csrc"


def build_and_run(tmp_path, name, sanitize):
    """tests/store_policy_check.cpp, a stand-alone program built with the
    host sources under `sanitize`, as tests/test_dispatch.py builds
    dispatch_check."""
    exe = tmp_path / name
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-pthread",
                    f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'include'}", "-o", str(exe),
                    str(REPO / "tests" / "store_policy_check.cpp"), str(CSRC / "rt_dispatch.cpp"),
                    str(CSRC / "rt_args.cpp")], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "store policy check ok" in r.stdout
    return r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_store_policy_tracker_and_choice(tmp_path):
    """The same buffer counts once, two buffers sum, entries age out after 8
    renders, overlapping ranges count once, devices are separate, two threads
    record renders at once, and the working set picks the policy: under
    AddressSanitizer + UndefinedBehaviorSanitizer.  (The same program builds
    with -fsanitize=thread for a ThreadSanitizer run of the two-thread case
    by hand; that runtime does not start on every machine, so no test
    depends on it.)"""
    err = build_and_run(tmp_path, "store_policy_check", "address,undefined")
    assert "runtime error" not in err and "AddressSanitizer" not in err
