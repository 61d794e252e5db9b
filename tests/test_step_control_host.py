"""The straight-line BDF order helpers are bitwise the branch forms they replaced (host, no GPU).

Builds tests/step_control_host.cpp -- a stand-alone program with its own main that instantiates
bdf_rescale, bdf_adjust_order (+1 / -1), dky0_lane, bdf_correct_history and bdf_tau_shift of
pychemkin_amd/csrc/ckmi_reactor.hpp on a plain-array history and BdfS -- with the host sanitizers and
runs it directly.  The program compares every output word with a restatement of the branch forms for
every q in 1..5, nst in {0, 1, 2, 20}, seeded random histories and +-0, denormals, +-inf and NaN.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "step_control_host.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_control") / "step_control_host")
    # host code only, and no HIP runtime in the link: the program never touches a GPU
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-O1", "-g", "-std=c++17",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_helpers_bitwise_equal_branch_forms(program):
    r = subprocess.run([program], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("step_control_host:") and last.endswith(" 0 mismatches"), last
    assert int(last.split()[1]) > 100_000, last  # every case ran
