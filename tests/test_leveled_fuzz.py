"""Leveled mode over the parameter space (tests/fuzz_leveled.py, tests/leveled_ref.py): what backs "one general kernel on the any-N
transforms, every parameter set" for tfhe_extern_mul_batch / tfhe_cmux_tree_batch / tfhe_cmux_net_batch / tfhe_rot_net_batch and their
multi-key forms.

CPU: the case generator is deterministic, reaches every log2 N, k, P, l = 1, l >= 8, beta = 1, beta = 12 and every planted rotation
over 2000 draws, skips nothing (every draw lands in exactness class 0, 1 or 2, class 0 — known answer only — well below one half); the
known-answer identity C (.) d = b (d - (d mod h)) holds on the integer schoolbook at every pinned set the CPU can afford (single key
N <= 256: (4096, 1, 3, 7) is outside; multi-key N <= 512: (2, 2048, 3, 7) is outside; both run it on the GPU below), for extern_mul, tree,
net and rot net; the same products stay within 2^-10 of an integer in a complex128 transform at the largest sets; and five deliberate
mutations of the REFERENCE each change the expected words of a pinned case, so these inputs tell such kernels apart.

GPU: every pinned set runs the fuzzer's whole per-case body (fuzz_leveled.run_case), and one short run of each fuzzer goes through a
fresh child process (as test_any_params.py::test_parameter_space_fuzz does for the rotation fuzzers; the counts and the measured
durations of both are in profiles/leveled_fuzz.txt).

Measured, the known answer in Float64 (test_known_answer_stays_inside_float64): worst distance from an integer 1.9e-6 = 2^-19, at
(N, k, l, beta) = (8192, 1, 16, 2)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz_leveled as F
import leveled_ref as R

PINNED = [(2, 1, 1, 1), (4, 2, 3, 4), (8, 3, 2, 8), (16, 1, 8, 4), (32, 6, 1, 9), (128, 1, 16, 2), (256, 2, 3, 6), (4096, 1, 3, 7)]       # N, k, l, beta
PINNED_MK = [(2, 2, 1, 4), (2, 8, 2, 8), (3, 16, 3, 6), (5, 32, 2, 7), (6, 64, 2, 6), (2, 256, 4, 7), (3, 512, 2, 8), (2, 2048, 3, 7)]    # P, N, l, beta
CPU_N, CPU_N_MK = 256, 512                # the largest N whose schoolbook the CPU tests run


def _all_pinned():
    return [(False, s) for s in PINNED] + [(True, s) for s in PINNED_MK]


# ---- 1. the case generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mk", [False, True])
def test_draw_case_is_deterministic(mk):
    a = [F.draw_case(np.random.default_rng(77), mk) for _ in range(3)]
    assert a[0] == a[1] == a[2]
    rng1, rng2 = np.random.default_rng(78), np.random.default_rng(78)
    assert [F.draw_case(rng1, mk) for _ in range(50)] == [F.draw_case(rng2, mk) for _ in range(50)]
    assert F.draw_case(np.random.default_rng(79), mk) != a[0]
    for s in (PINNED_MK if mk else PINNED):
        assert F.pinned_case(mk, *s) == F.pinned_case(mk, *s)


@pytest.mark.parametrize("mk", [False, True])
def test_draw_case_covers_the_space_and_skips_nothing(tfhe, mk):
    from tfhe_jl_amd import leveled
    rng = np.random.default_rng(2000 + mk)
    classes = [0, 0, 0]
    seen = {key: set() for key in ("logN", "k", "P", "l", "beta", "rot", "B", "S", "T", "depth", "index", "ks", "levels", "planted")}
    for _ in range(2000):
        c = F.draw_case(rng, mk)
        N, l, beta = c["N"], c["l"], c["beta"]
        assert 1 <= beta <= 12 and 1 <= l <= min(32 // beta, 16) and c["k"] * N <= 16384 and c["t"] * c["gamma"] <= 31
        assert 1 <= c["n"] <= (6 if mk else 40) and 1 <= c["S"] <= 6 and 1 <= c["T"] <= 3 and c["B"] in F.B_CHOICES and 1 <= c["depth"] <= 3
        assert 1 <= len(c["widths"]) <= 4 and all(1 <= w <= 6 for w in c["widths"]) and 1 <= c["E"] <= 6 and 1 <= c["V"] <= 4
        net = leveled.CmuxNet(c["widths"], c["nodes"], entries=c["E"], variables=c["V"])      # the wiring is valid as the library sees it
        if mk:
            assert len(c["owners"]) == c["S"] and all(0 <= o < c["P"] for o in c["owners"]) and "rnodes" not in c
        else:
            rnet = leveled.RotNet(c["widths"], c["rnodes"], N, entries=c["E"], variables=c["V"])
            assert np.array_equal(rnet.nodes[:, 2], net.nodes[:, 2])
            seen["rot"] |= set(c["rot_kinds"])
            nd = rnet.nodes
            if np.any((nd[:, 0] == nd[:, 1]) & (nd[:, 3] == nd[:, 4]) & (nd[:, 3] != 0)):
                seen["planted"].add("rotated copy")
            if np.any((nd[:, 0] == nd[:, 1]) & (nd[:, 3] != nd[:, 4])):
                seen["planted"].add("src0=src1,rot0!=rot1")
        if np.any(net.nodes[:, 0] == net.nodes[:, 1]):
            seen["planted"].add("copy")
        if np.any(net.nodes[:, 0] > net.nodes[:, 1]):
            seen["planted"].add("src0>src1")
        # no case is skipped: the class is one of the three branches of run_case, and what the host budget could not shed is one product per call
        cls = F.params_of(tfhe, c).exactness()[0]
        assert cls in (0, 1, 2)
        classes[cls] += 1
        assert F.host_cost(c) <= F.HOST_BUDGET or (c["B"] == 1 and c["depth"] == 1 and c["widths"] == [1])
        for key, v in (("logN", N.bit_length() - 1), ("k", c["k"]), ("P", c.get("P", 1)), ("l", l), ("beta", beta), ("B", c["B"]), ("S", c["S"]), ("T", c["T"]),
                       ("depth", c["depth"]), ("index", c["index"]), ("ks", (c["t"], c["gamma"]) == (8, 2)), ("levels", len(c["widths"]))):
            seen[key].add(v)
    assert seen["logN"] == set(range(1, 12 if mk else 14))
    assert (seen["P"] == set(range(2, 7)) and seen["k"] == {1}) if mk else (seen["k"] == set(range(1, 7)) and seen["P"] == {1})
    assert 1 in seen["l"] and any(v >= 8 for v in seen["l"]) and 16 in seen["l"] and seen["beta"] == set(range(1, 13))
    assert seen["B"] == set(F.B_CHOICES) and seen["S"] == set(range(1, 7)) and seen["T"] == {1, 2, 3} and seen["depth"] == {1, 2, 3}
    assert seen["index"] == {False, True} and seen["levels"] == {1, 2, 3, 4}
    assert {"copy", "src0>src1"} <= seen["planted"]
    if not mk:
        assert seen["rot"] == set(F.ROT_KINDS) and {"rotated copy", "src0=src1,rot0!=rot1"} <= seen["planted"] and seen["ks"] == {False, True}
    assert sum(classes) == 2000 and classes[0] < 1000 and classes[1] > 0 and classes[2] > 0, classes


def test_every_pinned_set_is_inside_the_exactness_domain(tfhe):
    """Class >= 1 by SchemeParameters.exactness(): every pinned set is compared with the schoolbook word for word, none only with the
    known answer."""
    for mk, s in _all_pinned():
        c = F.pinned_case(mk, *s)
        assert F.params_of(tfhe, c).exactness()[0] >= 1, (mk, s)
        if c["N"] >= 2048:
            # one row and one product per call: three under a multi-key key; four under a single key, whose body has four calls
            # (extern_mul, tree, net, rot net) — one more than the "at most three" that fits a three-call body
            assert c["B"] == 1 and F._products(c) <= (3 if mk else 4), c
        assert F.host_cost(c) <= F.HOST_BUDGET


# ---- 2. the known answer on the schoolbook -------------------------------------------------------------------------------------------
def _cpu_pinned():
    return [(mk, s) for mk, s in _all_pinned() if (s[1] if mk else s[0]) <= (CPU_N_MK if mk else CPU_N)]


@pytest.mark.parametrize("mk,s", _cpu_pinned())
def test_known_answer_holds_on_the_schoolbook(tfhe, orc, mk, s):
    """C (.) d = b (d - (d mod h)) for a trivial selector: on multiples of h the schoolbook's extern_mul, tree, net and rot net return
    exactly what evaluate_clear selects, as samples and extracted; on arbitrary words the remainder d - C (.) d lies in [0, h)."""
    c = F.pinned_case(mk, *s)
    inp = F.Inputs(tfhe, orc, c)
    try:
        tgsw, rows, tree_data, net_data, want = inp.known()
        h = R.gadget_h(c["l"], c["beta"])
        for data in (rows, tree_data, net_data):
            assert not (data.astype(np.int64) % h).any()
        ref = inp.reference_over(orc, tgsw)
        got = inp.expected(ref=ref, data=(rows, tree_data, net_data))
        assert np.array_equal(got["extern_mul"], want["extern_mul"])
        for name in ("tree", "net") + (() if mk else ("rot",)):
            assert np.array_equal(got[name][0], want[name][0]) and np.array_equal(got[name][1], want[name][1]), name
        assert tgsw.any()                                                        # a selector of bit 1 is among them
        # arbitrary words: the remainder is d mod h
        d = F._words(np.random.default_rng(5), inp.polys, c["N"])
        one = next(i for i in range(c["S"]) if tgsw[i].any())
        rem = R.wrap32(d.astype(np.int64) - ref.extern_mul(d, one)) & 0xFFFFFFFF
        assert np.array_equal(rem, d.astype(np.int64) & (h - 1))
    finally:
        inp.close()


def _fft_trivial_product(d, l, beta):
    """C (.) d for the trivial selector of bit 1 as a Float64 transform computes it: the l digit polynomials times the constants g_p,
    summed as spectra of a complex128 negacyclic transform (twist, numpy.fft, untwist), BEFORE rounding: float64 [N]."""
    from tfhe_jl_amd.numeric import decompose
    N = d.shape[-1]
    tw = np.exp(-1j * np.pi * np.arange(N) / N)
    digits = decompose(d, l, beta).astype(np.float64)                            # [l][N]
    acc = np.zeros(N, np.complex128)
    for p in range(l):
        g = np.zeros(N)
        g[0] = float(1 << (32 - (p + 1) * beta))
        acc += np.fft.fft(digits[p] * tw) * np.fft.fft(g * tw)
    return (np.fft.ifft(acc) * np.conj(tw)).real


FLOAT64_SETS = [(4096, 1, 3, 7), (2048, 2, 3, 7), (8192, 2, 2, 12), (8192, 1, 16, 2), (2048, 6, 2, 12), (1024, 6, 16, 2), (8192, 2, 1, 12), (256, 2, 3, 6)]


def test_known_answer_stays_inside_float64():
    """The bound of leveled_ref's docstring, confirmed: with one non-zero key coefficient per row every pre-rounding value is at most
    2^32 in magnitude, whatever N, k, l, beta — the largest pinned sets ((4096, 1, 3, 7); (2, 2048, 3, 7) as k = P) and sets of class 0 that
    the fuzzer draws.  A Float64 transform of 2^14 points loses at most a few bits of 2^32 2^-53: asserted below 2^-10 of an integer,
    measured 2^-19 (module docstring)."""
    rng = np.random.default_rng(64)
    worst = (0.0, None)
    for N, k, l, beta in FLOAT64_SETS:
        d = R.multiples_of_h(F._words(rng, N), l, beta)
        d[:3] = R.multiples_of_h(np.array([2**31 - 1, -2**31, 0]), l, beta)
        y = _fft_trivial_product(d, l, beta)
        assert np.abs(y).max() <= 2.0**32
        dist = float(np.abs(y - np.rint(y)).max())
        worst = max(worst, (dist, (N, k, l, beta)))
        assert dist < 2.0**-10, (N, k, l, beta, dist)
        assert np.array_equal(R.wrap32(np.rint(y).astype(np.int64)), d.astype(np.int64)), (N, k, l, beta)       # a multiple of h comes back
    print(f"worst distance from an integer: {worst[0]:.3g} at (N, k, l, beta) = {worst[1]}")


# ---- 3. discrimination: five mutations of the reference ----------------------------------------------------------------------------
class _VarIsNode:
    """A network whose records name node i of their level (mod V) where the variable should be: sel[g][node] for sel[g][var]."""

    def __init__(self, net):
        self.net, self.levels, self.degree, self.V = net, net.levels, getattr(net, "degree", None), net.variables

    def level(self, v):
        lv = np.array(self.net.level(v))
        lv[:, 2] = np.arange(len(lv)) % self.V
        return lv


def _extract_without_negation(sample):
    s = np.asarray(sample, np.int64)
    return R.wrap32(np.concatenate([np.concatenate([p[:1], p[:0:-1]]) for p in s[:-1]] + [s[-1][:1]]))


def _flat(want):
    return [want["extern_mul"]] + [a for name in ("tree", "net", "rot") if name in want for a in want[name]]


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(_flat(a), _flat(b)))


MUTATION_CASES = [(False, (4, 2, 3, 4)), (False, (8, 3, 2, 8)), (False, (16, 1, 8, 4)), (True, (2, 8, 2, 8)), (True, (3, 16, 3, 6))]


def test_five_reference_mutations_change_the_expected_words(tfhe, orc, monkeypatch):
    """A kernel that (1) rotates by r + 1 when r = N, (2) forgets the sign change past N, (3) takes the selector from sel[g][node], (4) swaps
    d0 and d1, or (5) extracts without the negation would have to equal the correspondingly mutated reference.  Each mutation changes
    the expected words of at least one pinned case (1 and 2 need rotations: single key; 3 - 5 also change a multi-key case), so the
    inputs of these cases tell such kernels from the right one.  Nothing in the product changes."""
    import test_rot_net
    true_monomial = R.monomial
    caught = {m: set() for m in (1, 2, 3, 4, 5)}
    for mk, s in MUTATION_CASES:
        inp = F.Inputs(tfhe, orc, F.pinned_case(mk, *s))
        try:
            base = inp.expected()
            assert not _differs(base, inp.expected())                            # the reference itself is deterministic
            if not mk:
                monkeypatch.setattr(test_rot_net, "monomial", lambda p, r, n: true_monomial(p, r + 1 if r % (2 * n) == n else r, n))
                if _differs(base, inp.expected()):
                    caught[1].add((mk, s))
                monkeypatch.setattr(test_rot_net, "monomial", lambda p, r, n: np.roll(np.asarray(p, np.int64), r % n))     # coefficient j to (j + r) mod N, no sign
                if _differs(base, inp.expected()):
                    caught[2].add((mk, s))
                monkeypatch.setattr(test_rot_net, "monomial", true_monomial)
                assert not _differs(base, inp.expected())
            if _differs(base, inp.expected(net=_VarIsNode(inp.net), rnet=None if mk else _VarIsNode(inp.rnet))):
                caught[3].add((mk, s))
            swapped = copy.copy(inp.ref)
            swapped.cmux = lambda sel, d0, d1, ref=inp.ref: ref.cmux(sel, d1, d0)
            if _differs(base, inp.expected(ref=swapped)):
                caught[4].add((mk, s))
            plain = copy.copy(inp.ref)
            plain.extract = _extract_without_negation
            mutated = inp.expected(ref=plain)
            assert np.array_equal(mutated["net"][0], base["net"][0])             # the samples are untouched, only their extraction moves
            if _differs(base, mutated):
                caught[5].add((mk, s))
        finally:
            inp.close()
    for m in (1, 2, 3, 4, 5):
        assert any(not mk for mk, _ in caught[m]), (m, caught)
    for m in (3, 4, 5):
        assert any(mk for mk, _ in caught[m]), (m, caught)


# ---- 4. GPU: every pinned set through the fuzzer's per-case body ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", PINNED)
def test_gpu_pinned_set_equals_schoolbook_and_known_answer(tfhe, orc, N, k, l, beta):
    c = F.pinned_case(False, N, k, l, beta)
    print(F.describe(c), F.run_case(tfhe, orc, c))


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", PINNED_MK)
def test_gpu_mk_pinned_set_equals_schoolbook_and_known_answer(tfhe, orc, P, N, l, beta):
    c = F.pinned_case(True, P, N, l, beta)
    print(F.describe(c), F.run_case(tfhe, orc, c))


# ---- 5. GPU: one short run of each fuzzer ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cases,seed,mk", [(9, 33, False), (11, 35, True)])     # (all three exactness classes occur in both)
def test_leveled_parameter_space_fuzz(cases, seed, mk):
    """A short run of tests/fuzz_leveled.py in a fresh child process; the long runs (400 cases, and 120 with --mk) are in
    profiles/leveled_fuzz.txt, with the durations of these two beside test_parameter_space_fuzz[fuzz_params.py]'s."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, os.path.join(here, "fuzz_leveled.py"), str(cases), str(seed)] + (["--mk"] if mk else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fuzz ok" in r.stdout and "none skipped" in r.stdout, r.stdout[-500:]
