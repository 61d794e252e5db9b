"""The per-slot arrays of the mechanism image lie back to back at strides of IIp (host, no GPU).

The reactor kernel's strips address lnA, beta, Ea, rsp, psp and info of a slot from two offsets of the view and
the stride IIp (strip_head, ckmi_reactor.hpp), and read a padding slot's records like any other.  build_host_mech
refuses an image without that layout; tests/strip_layout_host.cpp -- a stand-alone program with its own main,
linked with the image builder and the native parser, built with the host sanitizers as tests/test_mech_image_host.py
builds its program -- asserts it, offsets and bytes, on that test's ten inputs, annealed and in file order.
"""
import functools
import os
import subprocess
import tempfile

import pytest

from test_mech_image_host import CSRC, HIPCC, ROOT, image_inputs

SOURCES = [os.path.join(ROOT, "tests", "strip_layout_host.cpp"), os.path.join(CSRC, "ckmi_mech_host.cpp"),
           os.path.join(CSRC, "ckmi_parse.cpp")]
_TMP = []


@functools.lru_cache(maxsize=None)
def program():
    """The sanitizer build of tests/strip_layout_host.cpp, compiled once per session."""
    _TMP.append(tempfile.TemporaryDirectory(prefix="ckmi_strip_layout_"))
    exe = os.path.join(_TMP[0].name, "strip_layout_host")
    # host code only, and no HIP runtime in the link: the program never touches a GPU
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-O2", "-g", "-std=c++17",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + SOURCES
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_layout(pairs):
    """[dict(where, order, KK, II, IIp, used, pads_inside)] of the program's layout lines, and its summary line."""
    r = subprocess.run([program()] + [p for pair in pairs for p in pair], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    out = []
    for l in lines:
        if l.startswith("layout "):
            w = l.split()
            out.append(dict(where=" ".join(w[1:-11]), order=w[-11], **{w[i]: int(w[i + 1]) for i in range(-10, 0, 2)}))
    return out, lines[-1]


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    pairs = image_inputs(tmp_path_factory.mktemp("strip_layout"))
    return len(pairs), run_layout(pairs)


def test_slot_arrays_are_contiguous_on_every_input(output):
    n, (layouts, last) = output
    assert n == 10
    assert last.startswith(f"strip_layout_host: {n} inputs,") and last.endswith(" 0 violations"), last
    assert int(last.split()[3]) > 10_000, last  # the byte comparisons ran
    assert len(layouts) == 2 * n, layouts  # each input annealed and in file order
    assert all(l["IIp"] % 64 == 0 and l["used"] <= l["IIp"] for l in layouts), layouts


def test_inputs_cover_the_padding_forms(output):
    _, (layouts, _) = output
    assert any(l["pads_inside"] > 0 for l in layouts), layouts            # padding slots between two blocks
    assert any(l["used"] < l["IIp"] for l in layouts), layouts            # padding slots at the end
    assert any(l["II"] == 0 and l["IIp"] == 64 for l in layouts), layouts  # nothing but padding
    assert any(l["IIp"] > 64 for l in layouts) and any(l["IIp"] == 64 and l["II"] > 0 for l in layouts), layouts
