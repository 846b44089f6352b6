"""Programmable bootstrapping and the wire-table levels over the parameter space (tests/fuzz_pbs.py): what backs "any parameter set
tfhe_ctx_create accepts" for tfhe_bootstrap_tv_batch / tfhe_bootstrap_tv_multi_batch, tfhe_lut_level / tfhe_linear_level / tfhe_gates_level,
their tfhe_mk_* forms and tfhe_mk_gates_batch.

CPU: the case generator is deterministic; over 2000 draws (single and multi-key) it reaches every log2 N, every k / P, l = 1, l = 8,
beta = 1, beta = 12, keyswitches (8, 2) and others, n_out = 1, 2, N / 4 and 32, tv_index None and mixed, stays inside the host budget
except where one row per call is left, and lands in exactness class 0 (closed form and linear level only) in fewer than 15 % of the
draws; every pinned set is of class >= 1 and inside the budget; the schoolbook equals the checkers of tests/pbs_ref/ at the pinned
sets the CPU can afford (N <= 256), so two independent references agree at the new shapes before anything runs on a GPU; and seven
deliberate mutations of the REFERENCE each change the expected words of a pinned case, so these inputs tell such kernels apart.

GPU: every pinned set runs the fuzzer's whole per-case body (fuzz_pbs.run_case), and one short run of each fuzzer goes through a fresh
child process (as test_leveled_fuzz.py::test_leveled_parameter_space_fuzz; the counts, seeds and measured durations are in
profiles/pbs_fuzz.txt)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz_pbs as F
import test_independent as TI
import test_independent_pbs as TP
from test_mk_pbs import mkref  # noqa: F401  (the compile recipe of tests/pbs_ref/mk_pbs_ref.c)
from test_pbs_multi import checkers  # noqa: F401  (the compile recipe of pbs_ref.c and pbs_multi_ref.c)

# N, k, l, beta, lwe_size, t, gamma
PINNED = [(2, 1, 1, 1, 5, 8, 2), (8, 1, 2, 8, 7, 5, 3), (16, 3, 3, 6, 9, 8, 2), (32, 6, 1, 9, 4, 3, 4), (64, 2, 8, 4, 6, 8, 2), (256, 1, 2, 12, 5, 8, 2),
          (512, 2, 2, 10, 3, 16, 1), (4096, 1, 3, 7, 2, 8, 2)]
# P, N, l, beta, lwe_size, t, gamma
PINNED_MK = [(2, 2, 1, 1, 3, 8, 2), (3, 8, 2, 8, 2, 5, 3), (5, 16, 3, 6, 2, 8, 2), (6, 64, 2, 6, 1, 8, 2), (2, 128, 8, 4, 3, 8, 2), (3, 32, 2, 12, 2, 4, 4),
             (3, 512, 2, 8, 2, 3, 4), (2, 2048, 3, 7, 1, 8, 2)]
EXPANDED_ON_DEVICE = (6, 64, 2, 6, 1, 8, 2)
CPU_N = 256                                # the largest N whose schoolbook the CPU tests run


def _pinned(mk, s):
    return F.pinned_case(mk, *s, expand=(mk and s == EXPANDED_ON_DEVICE))


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
        assert _pinned(mk, s) == _pinned(mk, s)


@pytest.mark.parametrize("mk", [False, True])
def test_draw_case_covers_the_space_and_skips_nothing(tfhe, mk):
    rng = np.random.default_rng(2000 + mk)
    classes = [0, 0, 0]
    seen = {key: set() for key in ("logN", "k", "P", "l", "beta", "ks", "n_out", "n_out=N/4", "index", "n_tv", "expand", "shed")}
    for _ in range(2000):
        c = F.draw_case(rng, mk)
        N, l, beta = c["N"], c["l"], c["beta"]
        assert 1 <= beta <= 12 and 1 <= l <= min(32 // beta, 8) and c["k"] * N <= 16384 and c["t"] * c["gamma"] <= 31
        assert 1 <= c["n"] <= (6 if mk else 40) and 1 <= c["n_tv"] <= 8
        # the n_out values always hold 1 and the largest allowed power of two, all are allowed, and the refused one is not
        top = F.n_out_max(N)
        assert top == max(1, min(32, N // 4)) and c["n_outs"][0] == 1 and c["n_outs"][-1] == top and len(c["n_outs"]) <= 3
        assert all(K & (K - 1) == 0 and (K == 1 or K <= N // 4) for K in c["n_outs"])
        bad = F.n_out_refused(N)
        assert bad == (2 if N <= 4 else 2 * top) and (bad > 32 or bad > N // 4)
        # no case is skipped: the class is one of the three branches of run_case, and what the host budget could not shed is one row per call
        cls = F.params_of(tfhe, c).exactness()[0]
        assert cls in (0, 1, 2)
        classes[cls] += 1
        assert F.host_cost(c) <= F.HOST_BUDGET or F.single_row(c), c
        assert F.rows_of(c) >= 1 and c["level_rows"] >= 1 and c["gates"] >= 1       # MUX is in every gate level
        seen["shed"].add(F.single_row(c))
        for K in c["n_outs"]:
            seen["n_out"].add(K)
            if K > 1 and K == N // 4:
                seen["n_out=N/4"].add(N)
        for key, v in (("logN", N.bit_length() - 1), ("k", c["k"]), ("P", c.get("P", 1)), ("l", l), ("beta", beta), ("ks", (c["t"], c["gamma"]) == (8, 2)),
                       ("index", c["index"]), ("n_tv", c["n_tv"]), ("expand", c.get("expand", False))):
            seen[key].add(v)
    assert seen["logN"] == set(range(1, 12 if mk else 14))
    assert (seen["P"] == set(range(2, 7)) and seen["k"] == {1}) if mk else (seen["k"] == set(range(1, 7)) and seen["P"] == {1})
    assert {1, 8} <= seen["l"] and seen["beta"] == set(range(1, 13))
    assert seen["ks"] == {False, True}
    assert {1, 2, 32} <= seen["n_out"] and seen["n_out=N/4"] == {8, 16, 32, 64, 128}
    assert seen["index"] == {False, True} and seen["n_tv"] == set(range(1, 9))
    assert seen["expand"] == ({False, True} if mk else {False})
    # the class-0 cap: a condition on the generator (closed form and linear level only in fewer than 15 % of the draws)
    assert sum(classes) == 2000 and classes[0] < 0.15 * 2000 and classes[1] > 0 and classes[2] > 0, classes
    print(f"{'multi-key' if mk else 'single key'}: class 0 / 1 / 2 = {classes}")


def test_pinned_sets_are_compared_with_the_schoolbook_and_hold_what_they_must(tfhe):
    """Class >= 1 by SchemeParameters.exactness() (none falls back to the closed form alone), inside HOST_BUDGET, and the shapes the fixed
    tests do not reach are among them."""
    assert len(PINNED) == 8 and len(PINNED_MK) == 8
    cases = {(mk, s): _pinned(mk, s) for mk, s in _all_pinned()}
    for (mk, s), c in cases.items():
        assert F.params_of(tfhe, c).exactness()[0] >= 1, (mk, s)
        assert F.host_cost(c) <= F.HOST_BUDGET, (mk, s)
        assert c["index"] and c["n_tv"] == 8
    for mk in (False, True):
        cs = [c for (m, _), c in cases.items() if m == mk]

        def has(pred):
            return any(pred(c) for c in cs)

        assert has(lambda c: c["N"] == 2)
        assert has(lambda c: c["N"] == 8 and 2 in c["n_outs"])
        assert has(lambda c: c["N"] == 16 and 4 in c["n_outs"] and (mk or c["k"] == 3))
        assert has(lambda c: c["l"] == 8 and c["beta"] == 4)
        assert has(lambda c: c["beta"] == 1) and has(lambda c: c["beta"] == 12)
        assert has(lambda c: c["N"] in (128, 256) and (c["t"], c["gamma"]) == (8, 2) and 32 in c["n_outs"])
        assert has(lambda c: (c["t"], c["gamma"]) != (8, 2))
        if mk:
            assert {c["P"] for c in cs} >= {2, 3, 5, 6} and {c["N"] for c in cs} >= {2, 8, 64, 512, 2048}
            assert sum(c["expand"] for c in cs) == 1
        else:
            assert has(lambda c: c["k"] == 6) and has(lambda c: (c["N"], c["k"], c["l"], c["beta"]) == (4096, 1, 3, 7))


# ---- 2. two independent references agree at the new shapes ---------------------------------------------------------------------------
@pytest.mark.parametrize("s", [s for s in PINNED if s[0] <= CPU_N])
def test_checkers_equal_schoolbook_at_pinned_sets(orc, tfhe, checkers, s):  # noqa: F811
    """tests/pbs_ref/pbs_ref.c and pbs_multi_ref.c (both product back-ends, with and without keyswitch, every n_out of the case) on the
    case's own rows, tables and index, and on its level's rows: the schoolbook's words (the recipe of
    test_independent_pbs.py::test_checkers_equal_schoolbook)."""
    c = _pinned(False, s)
    inp = F.Inputs(tfhe, c)
    try:
        want = inp.expected()
        o = TP._Orc(orc, inp.p, inp.ck).oracle
        for mode in (orc.MODE_FFT, orc.MODE_EXACT):
            for ks in (False, True):
                assert np.array_equal(TP._pbs_ref(checkers["pbs_ref"], o, mode, inp.tables, inp.index, inp.x, ks), want["tv"][1, ks][:, 0]), (mode, ks)
                for K in c["n_outs"]:
                    got = TP._pbs_multi_ref(checkers["pbs_multi_ref"], o, mode, inp.tables, inp.index, inp.x, K, ks)
                    assert np.array_equal(got, want["tv"][K, ks]), (mode, ks, K)
            for K in inp.level_n_outs:
                got = TP._pbs_multi_ref(checkers["pbs_multi_ref"], o, mode, inp.tables, inp.lindex, want["linear"], K, True)
                assert np.array_equal(got, want["lut"][K, True]), (mode, K)
    finally:
        inp.close()


@pytest.mark.parametrize("s", [s for s in PINNED_MK if s[1] <= CPU_N])
def test_mk_checker_equals_schoolbook_at_pinned_sets(orc, tfhe, mkref, s):  # noqa: F811
    """tests/pbs_ref/mk_pbs_ref.c at the multi-key pinned sets the CPU can afford, in the same way."""
    c = _pinned(True, s)
    inp = F.Inputs(tfhe, c)
    try:
        want = inp.expected()
        o = TP._Orc(orc, inp.p, inp.ck, c["P"]).oracle
        for mode in (orc.MODE_FFT, orc.MODE_EXACT):
            for ks in (False, True):
                for K in c["n_outs"]:
                    got = TP._mk_pbs_ref(mkref.lib, o, mode, inp.tables, inp.index, inp.x, K, ks)
                    assert np.array_equal(got, want["tv"][K, ks]), (mode, ks, K)
    finally:
        inp.close()


# ---- 3. discrimination: seven mutations of the reference ----------------------------------------------------------------------------
def _flat(want):
    return [want["tv"][key] for key in sorted(want["tv"])] + [want["linear"]] + [want["lut"][key] for key in sorted(want["lut"])] + [want["gates"]]


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(_flat(a), _flat(b)))


_TRUE_EXTRACT_MASK = TI.Schoolbook.extract_mask


def _extract_mask_without_negation(p, c):
    """extract_shift_kernel's step written wrongly: word u of the sample at c is word u - c of the sample at 0 for u >= c and MINUS word
    u - c + N for u < c; this one forgets the minus."""
    true = _TRUE_EXTRACT_MASK(p, c)
    return np.where(np.arange(len(p)) < c, -true, true)


def _decode_truncating(self, phase, space):
    log2 = space.bit_length() - 1
    return int(TI.wrap32(int(phase))) >> (32 - log2)


MUTATION_CASES = [(False, PINNED[1]), (False, PINNED[2]), (False, PINNED[4]), (True, PINNED_MK[1]), (True, PINNED_MK[2])]


def test_seven_reference_mutations_change_the_expected_words(tfhe, monkeypatch):
    """A kernel that (1) extracts at c_j without the negation for u < c_j, (2) takes c_j = j for j N / n_out, (3) takes row g's table as
    tv[g mod n_tv] for tv[tv_index[g]], (4) truncates in the modulus switch where it should round, (5) drops cst from a level row, (6) swaps
    the MUX operands y and z, or (7, multi-key) reads party p + 1's mask column in party p's keyswitch would have to equal the
    correspondingly mutated reference.  Each mutation changes the expected words of a single-key and of a multi-key pinned case
    (7: of a multi-key one), so the inputs of these cases tell such kernels from the right one."""
    true_combine, true_gate, true_mk_gate, true_mk_ks = TP.combine, TI.schoolbook_gate, TI.MKSchoolbook.mk_gate, TI.MKSchoolbook.mk_keyswitch

    def mk_keyswitch_next_party(self, ext):
        N, P = self.N, self.P
        moved = np.concatenate([np.asarray(ext[((p + 1) % P) * N:((p + 1) % P + 1) * N]) for p in range(P)] + [np.asarray(ext[P * N:])])
        return true_mk_ks(self, moved)

    mutations = {
        1: [(TI.Schoolbook, "extract_mask", staticmethod(_extract_mask_without_negation))],
        2: [(TP, "coefficient_of", lambda j, N, n_out: j)],
        3: [(TP, "table_of", lambda tables, index, g: tables[g % len(tables)])],
        4: [(TI.Schoolbook, "decode", _decode_truncating)],
        5: [(TP, "combine", lambda rows, start, wire, coef, cst: true_combine(rows, start, wire, coef, None))],
        6: [(TI, "schoolbook_gate", lambda sb, name, x, y, z: true_gate(sb, name, x, z, y) if name == "MUX" else true_gate(sb, name, x, y, z)),
            (TI.MKSchoolbook, "mk_gate", lambda self, name, x, y=None, z=None: true_mk_gate(self, name, x, z, y) if name == "MUX" else true_mk_gate(self, name, x, y, z))],
        7: [(TI.MKSchoolbook, "mk_keyswitch", mk_keyswitch_next_party)],
    }
    caught = {m: set() for m in mutations}
    for mk, s in MUTATION_CASES:
        inp = F.Inputs(tfhe, _pinned(mk, s))
        try:
            base = inp.expected()
            assert not _differs(base, inp.expected())                            # the reference itself is deterministic
            for m, patches in mutations.items():
                with monkeypatch.context() as mp:
                    for target, name, value in patches:
                        mp.setattr(target, name, value)
                    if _differs(base, inp.expected()):
                        caught[m].add((mk, s))
            assert not _differs(base, inp.expected())                            # and every mutation is undone
        finally:
            inp.close()
    for m in mutations:
        assert any(mk for mk, _ in caught[m]), (m, caught)
        assert m == 7 or any(not mk for mk, _ in caught[m]), (m, caught)
    assert not any(not mk for mk, _ in caught[7])                                # (a single-key case has no party columns)


# ---- 4. GPU: every pinned set through the fuzzer's per-case body ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("s", PINNED, ids=["-".join(str(v) for v in s) for s in PINNED])
def test_gpu_pinned_set_equals_schoolbook_and_closed_form(tfhe, s):
    c = _pinned(False, s)
    print(F.describe(c), F.run_case(tfhe, None, c))


@pytest.mark.gpu
@pytest.mark.parametrize("s", PINNED_MK, ids=["-".join(str(v) for v in s) for s in PINNED_MK])
def test_gpu_mk_pinned_set_equals_schoolbook_and_closed_form(tfhe, s):
    c = _pinned(True, s)
    print(F.describe(c), F.run_case(tfhe, None, c))


# ---- 5. GPU: one short run of each fuzzer ----------------------------------------------------------------------------------------------
SHORT_RUNS = [(5, 1137, False), (9, 2025, True)]       # cases, seed, --mk: all three exactness classes occur in both


def test_short_runs_hold_all_three_classes(tfhe):
    for cases, seed, mk in SHORT_RUNS:
        rng = np.random.default_rng(seed)
        assert {F.params_of(tfhe, F.draw_case(rng, mk)).exactness()[0] for _ in range(cases)} == {0, 1, 2}, (cases, seed, mk)


@pytest.mark.gpu
@pytest.mark.parametrize("cases,seed,mk", SHORT_RUNS)
def test_pbs_parameter_space_fuzz(cases, seed, mk):
    """A short run of tests/fuzz_pbs.py in a fresh child process; the long runs (300 cases, and 100 with --mk) are in
    profiles/pbs_fuzz.txt, with the durations of these two beside test_parameter_space_fuzz[fuzz_params.py-80-21]'s."""
    here = os.path.dirname(os.path.abspath(__file__))
    cmd = [sys.executable, os.path.join(here, "fuzz_pbs.py"), str(cases), str(seed)] + (["--mk"] if mk else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "fuzz ok" in r.stdout and "none skipped" in r.stdout, r.stdout[-500:]
