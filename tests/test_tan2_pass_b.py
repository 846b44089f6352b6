"""The pass-B twiddles of blind_rotate_kernel_v3 in tan form, applied by the receiving lane of the second transposition
(csrc/br_core.hpp: fill_tan2, tan2_apply, dft8_scaled), on the host: br_core.hpp is host / device code, so a wrong ratio or tangent in
the per-lane constant record shows up here without a GPU.  tests/host/tan2_pass_b.cpp does the work and prints the figures."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tan2") / "tan2_pass_b")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "tfhe.jl_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "tan2_pass_b.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    print(out)
    return out


def test_tan_form_stage_is_as_accurate_as_the_plain_form(output):
    """tan2_apply + dft8_scaled against x * tw2 + dft8, both measured against a long-double evaluation in the same run: every lane
    group, both directions.  The tan form's worst error may exceed the plain form's by at most 1.5x (measured in numpy for the
    isolated stage: 1.3x; the rest covers another random draw) — asserted per group and direction, which is the stricter reading."""
    rows = re.findall(r"stage dir (fwd|inv) group (\d) tan (\S+) plain (\S+)", output)
    assert sorted((d, int(g)) for d, g, _, _ in rows) == [(d, g) for d in ("fwd", "inv") for g in range(8)], output
    for d, g, tan, plain in rows:
        tan, plain = float(tan), float(plain)
        assert 0 < plain < 1e-15, (d, g, plain)          # the yardstick itself is sane: a few ulps of the largest output
        assert tan <= 1.5 * plain, (d, g, tan, plain)


def test_chain_with_tan_form_pass_b_gives_the_integer_product(output):
    """Forward transform as the kernel runs it (digits |d| <= 512), times a prepared Int32 key spectrum, inverse transform, untwist,
    rounding: every coefficient equals the integer negacyclic schoolbook product mod 2^32 (8 random pairs of polynomials)."""
    m = re.search(r"chain wrong_words (\d+) of (\d+) max_dist_from_integer (\S+)", output)
    assert m, output
    assert int(m.group(2)) == 8 * 1024
    assert int(m.group(1)) == 0, output
    assert float(m.group(3)) < 0.25, output              # pre-rounding values stay well away from the half-integers
