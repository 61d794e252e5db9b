"""The mechanism image is what the descriptor says, byte for byte (host, no GPU).

Builds tests/mech_image_host.cpp -- a stand-alone program with its own main, linked with the image builder
(pychemkin_amd/csrc/ckmi_mech_host.cpp) and the native parser (ckmi_parse.cpp) -- with the host sanitizers
and runs it directly on the six committed mechanisms, the 10-species H2 subset of GRI-Mech 3.0 (one strip),
GRI-Mech 3.0 + 10 tracers (KK = 63: the dummy species slot is the last of the first 64), a mechanism without
reactions, and a few-line mechanism with what the others lack (SRI falloff, single-collider third bodies).
The program decodes each image with the image's own helpers and compares it with the parsed descriptor, and
reaches every refusal of the builder that a descriptor can reach; this file asserts its summary line, that
every feature of the image occurred in some input, and that every refusal was reached.
"""
import os
import subprocess

import pytest

import mechanism_variants as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pychemkin_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "mech_image_host.cpp"), os.path.join(CSRC, "ckmi_mech_host.cpp"),
           os.path.join(CSRC, "ckmi_parse.cpp")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

COMMITTED = ["grimech30_chem.inp", "gri30_plog_chem.inp", "gri30_cheb_chem.inp", "gri30_ford_chem.inp",
             "gri30_tracer161_chem.inp", "gri30_tracer161_ext_chem.inp"]

# SRI falloff (3 and 5 parameters) and single-collider third bodies: no committed mechanism has either
SRI_COLLIDER = """ELEMENTS
O H N AR
END
SPECIES
H2 H O O2 OH H2O HO2 H2O2 N2 AR
END
REACTIONS
H+O2(+N2)<=>HO2(+N2)     4.650E+12  0.440     0.00
     LOW / 6.370E+20 -1.720 525.00 /
     SRI / 0.45 797.0 979.0 1.1 0.05 /
2OH(+H2O)<=>H2O2(+H2O)   7.400E+13 -0.370     0.00
     LOW / 2.300E+18 -0.900 -1700.00 /
     SRI / 0.7346 94.0 1756.0 /
H+OH(+AR)<=>H2O(+AR)     2.500E+13  0.200     0.00
     LOW / 4.500E+22 -2.000 0.00 /
     TROE / 0.73 100.0 1.0E+05 1.0E+04 /
O+H2<=>H+OH              3.870E+04  2.700  6260.00
END
"""

NO_REACTIONS = """ELEMENTS
O H
END
SPECIES
H2 O2 H2O
END
REACTIONS
END
"""

FEATURES = ["pad_taken", "pad_not_taken", "geffd_dense", "geffd_stub", "npe", "group_third_body",
            "collider_third_body", "troe", "sri", "chemically_activated", "explicit_rev", "plog", "chebyshev",
            "landau_teller", "general", "coefficient_2", "no_reactions"]
# every refusal a descriptor can reach (the program's header names the three that none does)
REFUSALS = ["bad_sizes_KK", "bad_sizes_II", "too_many_species", "null_tables", "slot_count", "reactant_index",
            "product_index", "reaction_type", "chebyshev_record", "plog_table", "general_chebyshev", "general_plog",
            "general_landau_teller", "general_reactant_nu", "general_product_nu", "general_forward_order",
            "general_reverse_order"]


def image_inputs(dirpath):
    """[(chem, thermo)] of every mechanism the program is run on; the generated ones are written to dirpath."""
    pairs = []
    for name in COMMITTED:
        big = "tracer161" in name
        pairs.append((os.path.join(mv.DATA, name), os.path.join(mv.DATA, "gri30_tracer161_thermo.dat") if big else mv.THERM))
    for name, text in (("h2_subset", mv.gri_subset_text(mv.H2_SPECIES, ("O", "H", "N", "AR"))),
                       ("sri_collider", SRI_COLLIDER), ("no_reactions", NO_REACTIONS)):
        path = os.path.join(str(dirpath), name + "_chem.inp")
        with open(path, "w") as f:
            f.write(text)
        pairs.append((path, mv.THERM))
    pairs.append(mv.write_tracer_mechanism(os.path.join(str(dirpath), "kk63"), 10))
    return pairs


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    d = tmp_path_factory.mktemp("mech_image")
    exe = str(d / "mech_image_host")
    # host code only, and no HIP runtime in the link: the program never touches a GPU
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-O2", "-g", "-std=c++17",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe] + SOURCES
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pairs = image_inputs(d)
    r = subprocess.run([exe] + [p for pair in pairs for p in pair], capture_output=True, text=True)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    return len(pairs), r.stdout.strip().splitlines()


def _counts(lines, kind):
    return {l.split()[1]: int(l.split()[2]) for l in lines if l.startswith(kind + " ")}


def test_images_match_their_descriptors(output):
    n, lines = output
    last = lines[-1]
    assert last.startswith("mech_image_host:") and last.endswith(" 0 mismatches"), last
    assert int(last.split()[1]) > 100_000, last  # every check ran
    images = [l for l in lines if l.startswith("image ")]
    assert len(images) == 2 * n, images  # each input annealed and in file order
    sizes = {(int(l.split(" KK ")[1].split()[0]), int(l.split(" II ")[1].split()[0])) for l in images}
    assert {(10, 29), (63, 340), (3, 0)} <= sizes, sizes  # the H2 subset, the dummy-slot boundary, no reactions
    assert any(" IIp 64 " in l and " II 29 " in l for l in images), images  # the subset is one strip


def test_every_feature_occurs(output):
    got = _counts(output[1], "feature")
    assert [f for f in FEATURES if got.get(f, 0) < 1] == [], got


def test_every_reachable_refusal_is_reached(output):
    got = _counts(output[1], "refusal")
    assert [r for r in REFUSALS if got.get(r, 0) < 1] == [], got
    assert sorted(got) == sorted(REFUSALS), got
