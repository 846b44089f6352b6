"""The rounding-only untwist blind_rotate_kernel_v3 feeds its LDS atomic adds from (csrc/br_core.hpp: untwist_round2), on the host:
the same words as untwist_add2 on a zero accumulator, fused and unfused form, and the same rounding margin.  A second copy of the
program is built with the address and undefined-behaviour sanitizers and run directly (it is a stand-alone program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_rounding_only_untwist_equals_untwist_add2_on_zero(tmp_path, sanitize):
    exe = str(tmp_path / "untwist_round")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "tfhe.jl_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "host", "untwist_round.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    m = re.search(r"untwist_words (\d+) untwist_diff (\d+) margin_diff (\d+)", r.stdout)
    assert m, r.stdout
    words, diff, margin_diff = map(int, m.groups())
    assert words == 20000 * 32, r.stdout
    assert diff == 0 and margin_diff == 0, r.stdout
