"""tfhe_mk_rot_net_batch over the parameter space (tests/fuzz_mk_rot_net.py on the generators of tests/fuzz_leveled.py).

CPU: the generator is a function of the rng alone and leaves fuzz_leveled's multi-key draw as it was; every drawn netlist is a valid
RotNet on the sources and variables of the case's CmuxNet; over 1000 draws every planted rotation, a rotated copy and a node with
src0 = src1 and rot0 != rot1 occur; the host budget holds with the rotated network counted; and the known answer holds on the integer
schoolbook at small pinned sets.

GPU: pinned sets through the fuzzer's per-case body (forms 0, 1, 2, both accumulator placements, the known answer), chosen to run in
seconds, and one short run of the script in a fresh child process.  The 120-case run is recorded in profiles/mk_rot_net_fuzz.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz_leveled as F
import fuzz_mk_rot_net as M
import leveled_ref as R

PINNED = [(2, 2, 1, 4), (3, 16, 3, 6), (6, 64, 2, 6), (2, 256, 4, 7), (2, 2048, 3, 7)]        # P, N, l, beta (of test_leveled_fuzz.PINNED_MK)
CPU_PINNED = [s for s in PINNED if s[1] <= 64]


def test_draw_case_is_a_function_of_the_rng_alone():
    a = [M.draw_case(np.random.default_rng(77)) for _ in range(3)]
    assert a[0] == a[1] == a[2] and M.draw_case(np.random.default_rng(79)) != a[0]
    rng1, rng2, rng3 = (np.random.default_rng(78) for _ in range(3))
    for _ in range(40):
        c, again, plain = M.draw_case(rng1), M.draw_case(rng2), F.draw_case(rng3, True)
        assert c == again
        # the rotations take no draw from the fuzzer's rng: fuzz_leveled's own case comes out beside it, shed no less
        assert {k: c[k] for k in ("P", "N", "l", "beta", "n", "S", "T", "E", "V", "owners", "seed", "index")} == {k: plain[k] for k in ("P", "N", "l", "beta", "n", "S", "T", "E", "V", "owners", "seed", "index")}
        assert c["B"] <= plain["B"] and c["depth"] <= plain["depth"] and c["nodes"] == plain["nodes"][:len(c["nodes"])]
    for s in PINNED:
        assert M.pinned_case(*s) == M.pinned_case(*s)


def test_drawn_netlists_are_valid_and_cover_the_rotations(tfhe):
    from tfhe_jl_amd import leveled
    rng = np.random.default_rng(2100)
    kinds, planted, classes = set(), set(), [0, 0, 0]
    for _ in range(1000):
        c = M.draw_case(rng)
        assert c["mk"] and len(c["rnodes"]) == len(c["nodes"]) == sum(c["widths"])
        net = leveled.CmuxNet(c["widths"], c["nodes"], entries=c["E"], variables=c["V"])
        rnet = M.rot_net_of(c)                                                  # valid as the library sees it
        assert rnet.degree == c["N"] and np.array_equal(rnet.nodes[:, 2], net.nodes[:, 2]) and np.array_equal(rnet.nodes[:, 0], net.nodes[:, 0])
        assert c["rot_kinds"] == F.rot_kinds(c["rnodes"], c["N"])
        kinds |= set(c["rot_kinds"])
        nd = rnet.nodes
        if np.any((nd[:, 0] == nd[:, 1]) & (nd[:, 3] == nd[:, 4]) & (nd[:, 3] != 0)):
            planted.add("rotated copy")
        if np.any((nd[:, 0] == nd[:, 1]) & (nd[:, 3] != nd[:, 4])):
            planted.add("src0=src1,rot0!=rot1")
        if np.any(nd[:, 0] > nd[:, 1]):
            planted.add("src0>src1")
        classes[F.params_of(tfhe, c).exactness()[0]] += 1
        assert F.host_cost(c) <= F.HOST_BUDGET or (c["B"] == 1 and c["depth"] == 1 and c["widths"] == [1])
    assert kinds == set(F.ROT_KINDS) and planted == {"rotated copy", "src0=src1,rot0!=rot1", "src0>src1"}
    assert sum(classes) == 1000 and classes[0] < 500 and classes[1] > 0 and classes[2] > 0, classes


def test_every_pinned_set_is_inside_the_exactness_domain(tfhe):
    for s in PINNED:
        c = M.pinned_case(*s)
        assert F.params_of(tfhe, c).exactness()[0] >= 1, s
        assert F.host_cost(c) <= F.HOST_BUDGET
        if c["N"] >= 2048:
            assert c["B"] == 1 and M._rot_products(c) <= 3, c


@pytest.mark.parametrize("P,N,l,beta", CPU_PINNED)
def test_known_answer_holds_on_the_schoolbook(tfhe, orc, P, N, l, beta):
    """On multiples of h and trivial selectors the schoolbook's rotated network returns exactly what RotNet.evaluate_clear selects, as
    samples and extracted."""
    c = M.pinned_case(P, N, l, beta)
    inp = F.Inputs(tfhe, orc, c)
    try:
        rnet = M.rot_net_of(c)
        tgsw, net_data, want = M.known(inp, rnet)
        assert tgsw.any() and not (net_data.astype(np.int64) % R.gadget_h(l, beta)).any()
        got = M.expected(inp, rnet, ref=inp.reference_over(orc, tgsw), data=net_data)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        inp.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", PINNED)
def test_gpu_mk_rot_pinned_set_equals_schoolbook_and_known_answer(tfhe, orc, P, N, l, beta):
    c = M.pinned_case(P, N, l, beta)
    print(M.describe(c), M.run_case(tfhe, orc, c))


@pytest.mark.gpu
def test_mk_rot_net_parameter_space_fuzz():
    """A short run of tests/fuzz_mk_rot_net.py in a fresh child process (the script's own entry point is what is under test)."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "fuzz_mk_rot_net.py"), "6", "41"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "mk rot net fuzz ok: 6 parameter sets" in r.stdout and "none skipped" in r.stdout, r.stdout[-500:]
