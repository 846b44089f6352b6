"""Multi-key private-table rotation on the 2-party gates' own kernel and key (tfhe_mk_bootstrap_acc_batch, tfhe_mk_bootstrap_acc_level;
Engine.mk_bootstrap_acc, Engine.mk_bootstrap_acc_level; tuned=True in tfhe_jl_amd.leveled's multi-key helpers) against three references:
the C checker tests/pbs_ref/mk_rotate_ref.c (`rotref` of tests/test_mk_blind_rotate.py: the oracle's source plus mk_blind_rotate from a full
accumulator, extraction at a coefficient and mk_keyswitch), Engine.mk_blind_rotate / Engine.mk_blind_rotate_level on the same inputs after
mk_tgsw_load(*mk_bootstrap_key_selectors(ck)), and, for a trivial accumulator, Engine.mk_bootstrap_tv_multi.  Every comparison is word for
word: there are no tolerances.

The kernel exists for 2 parties, N = 1024, l = 4 only.  `mk_small` (tests/test_mk_pbs.py) is that shape at n = 24: P n = 48 steps, so each
party's loop passes the workgroup barrier of step 0 and, for party 1, that of step 32.  B = 5 rows run as five workgroups (mk_rw 1), as
three workgroups of two rotations with one padding rotation (mk_rw 2), and by size (mk_rw 0: one rotation per workgroup up to one row per
compute unit); B = 1 and B = 3 are the issue's two other geometries.  Keys made on the spot with n = 1 and n = 2 give 2 and 4 steps, and
cu_count + 1 rows at n = 2 cross the switch of mk_rw 0 to pairs.  The checker's words of a case are computed once and shared."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_bootstrap_acc import _cu_count
from test_mk_blind_rotate import full, rotref          # noqa: F401  (fixtures: the C checker; mktfhe_parameters_2party with its expected words)
from test_mk_leveled import Setup, _words
from test_mk_pbs import mk_small, mkref          # noqa: F401  (fixtures: the 2-party N = 1024, n = 24 keys; rotref's sibling)
from test_tlwe_levels import ACC_SLOT, IN_WIRES, OUT_SLOT, SLOTS, TERM_COEF, TERM_START, TERM_WIRE, WIRES, _mem_free, form_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_KEY, STATE, NOMEM = 0, 1, 3, 5, 6
N, P, L, BETA = 1024, 2, 4, 7
ACC_INDEX = np.array([2, 0, 2, 1, 0], np.int32)
B_ROWS = 5
UNIT = 2**21                                                        # 2^32 / 2N: one step of the exponent
NEW = {"tfhe_mk_bootstrap_acc_batch": 9, "tfhe_mk_bootstrap_acc_level": 11}


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _name(rw2):
    return "mk_blind_rotate_kernel_w2_acc<4,rw2>" if rw2 else "mk_blind_rotate_kernel_w2_acc<4>"


# ---- 1. CPU -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(tfhe):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read(), flags=re.S)
    lib = tfhe._lib.load()
    for name, argc in NEW.items():
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m and len(m.group(1).split(",")) == argc, name
        assert m.group(1).lstrip().startswith("tfhe_ctx *ctx"), name
        assert name in tfhe._lib.ABI_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == argc, name
    assert lib.tfhe_abi_version() == 7
    assert lib.tfhe_mk_bootstrap_acc_batch(None, None, 1, None, None, 1, 0, None, 1) == INVALID          # NULL context
    assert lib.tfhe_mk_bootstrap_acc_level(None, None, None, None, None, None, 1, 0, None, None, 1) == INVALID
    assert callable(getattr(tfhe.Engine, "mk_bootstrap_acc")) and callable(getattr(tfhe.Engine, "mk_bootstrap_acc_level"))
    from tfhe_jl_amd import leveled
    for f in (leveled.mk_blind_rotate_lookup, leveled.mk_two_stage_lookup, leveled.mk_two_stage_lookup_device, leveled.mk_pbs_to_tlwe):
        assert inspect.signature(f).parameters["tuned"].default is False, f.__name__


def _word(e, off=0):
    """The int32 word that the modulus switch takes to exponent e (mod 2N) when off lies in [-2^20, 2^20)."""
    return int(np.array([(e * UNIT + off) % 2**32], np.uint32).view(np.int32)[0])


def _rows(rng, steps):
    """Multi-key LWE words [5][steps + 1] whose switched exponents include 0, 1, N and 2N - 1 in the steps and in barb, the words 2^31 - 1
    and -2^31, both sides of a rounding boundary, and an all-zero row."""
    plant = [0, 1, N, 2 * N - 1]
    x = _words(rng, B_ROWS, steps + 1)
    x[0, :steps] = [_word(plant[i % 4]) for i in range(steps)]
    x[0, steps] = _word(0)
    x[1, 0] = 2**31 - 1
    x[1, steps - 1] = -2**31
    x[1, steps] = _word(N)
    x[2, :steps] = [_word(plant[(i + 1) % 4], -5) for i in range(steps)]
    x[2, steps] = _word(2 * N - 1)
    x[3, :] = 0
    x[4, 0] = _word(3, 2**20 - 1)                                    # just below a rounding boundary: 3
    x[4, steps] = _word(0, 2**20)                                    # on it: 0 -> 1
    return x


def _accs(rng):
    """T = 3 MK TLWE samples of arbitrary words, none trivial, with the extreme words planted."""
    acc = _words(rng, 3, P + 1, N)
    acc[0, 0, 0], acc[0, P, 1], acc[1, 1, N - 1], acc[2, P, 0] = 2**31 - 1, -2**31, -2**31, 2**31 - 1
    return acc


def _wants(rotref, oracle, acc, idx, x):
    """The checker's final accumulators and their extractions, plain and keyswitched, of every row."""
    want = {(0, 1): rotref(oracle, acc, idx, x, 1, 0)}
    for n_out in (1, 4, 32):
        want[(1, n_out)] = rotref(oracle, acc, idx, x, n_out, 1)
        want[(2, n_out)] = rotref(oracle, acc, idx, x, n_out, 2)
    return want


@pytest.fixture(scope="module")
def case(tfhe, mk_small, rotref):
    """mk_small's engine with the key's P n entries loaded as selectors (for the any-N calls alone: the new call reads none), T = 3
    accumulators, B = 5 rows and the checker's words of those rows under ACC_INDEX."""
    from tfhe_jl_amd import leveled
    K = mk_small
    n = K.params.lwe_size
    rng = np.random.default_rng(4242)
    eng = K.ck.engine(0)
    eng.mk_tgsw_load(*leveled.mk_bootstrap_key_selectors(K.ck))
    acc, x = _accs(rng), _rows(rng, P * n)
    shift = 32 - 11
    exps = (((x.astype(np.int64) & 0xFFFFFFFF) + (1 << (shift - 1))) >> shift) & (2 * N - 1)
    assert list(exps[0, :4]) == [0, 1, N, 2 * N - 1] and exps[0, -1] == 0 and exps[1, 0] == N and exps[1, -2] == N and exps[1, -1] == N
    assert list(exps[2, :4]) == [1, N, 2 * N - 1, 0] and exps[2, -1] == 2 * N - 1 and not exps[3].any() and exps[4, 0] == 3 and exps[4, -1] == 1
    return dict(K=K, n=n, rng=rng, eng=eng, acc=acc, x=x, want=_wants(rotref, K.oracle, acc, ACC_INDEX, x))


def _check_rows(eng, acc, x, idx, want, rows, rw2, tag):
    """Every out_form and n_out of the batch call on the rows `rows` of a case against the checker's words of those rows."""
    rows = list(rows)
    B, n = len(rows), (x.shape[1] - 1) // P
    got0 = eng.mk_bootstrap_acc(acc, x[rows], acc_index=idx[rows], out_form=0)
    assert eng.last_kernel_name() == _name(rw2), (tag, eng.last_kernel_name())
    assert eng.last_rotation_count() == B and eng.last_timing_ms(0) > 0
    assert got0.shape == (B, P + 1, N) and np.array_equal(got0, want[(0, 1)][rows]), (tag, "out_form 0")
    for n_out in (1, 4, 32):
        got1 = eng.mk_bootstrap_acc(acc, x[rows], acc_index=idx[rows], n_out=n_out, out_form=1)
        assert got1.shape == (B, n_out, P * N + 1) and np.array_equal(got1, want[(1, n_out)][rows]), (tag, "out_form 1", n_out)
        got2 = eng.mk_bootstrap_acc(acc, x[rows], acc_index=idx[rows], n_out=n_out, out_form=2)
        assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
        assert got2.shape == (B, n_out, P * n + 1) and np.array_equal(got2, want[(2, n_out)][rows]), (tag, "out_form 2", n_out)


# ---- 2. GPU: word for word ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_option_and_kernel_name(tfhe, case):
    eng = case["eng"]
    assert eng.get_option("mk_bootstrap_acc") == 1 and eng.get_option("bootstrap_acc") == 0
    eng.mk_bootstrap_acc(case["acc"], case["x"][:1], out_form=0)
    assert eng.last_kernel_name() == "mk_blind_rotate_kernel_w2_acc<4>" and eng.last_rotation_count() == 1
    try:
        eng.set_option("mk_rw", 2)
        eng.mk_bootstrap_acc(case["acc"], case["x"][:1], out_form=0)
        assert eng.last_kernel_name() == "mk_blind_rotate_kernel_w2_acc<4,rw2>"
        eng.set_option("mk_general", 1)                             # ignored: there is one ACC family and the key layout is shared
        assert eng.get_option("mk_bootstrap_acc") == 1
        got = eng.mk_bootstrap_acc(case["acc"], case["x"], acc_index=ACC_INDEX, out_form=0)
        assert eng.last_kernel_name() == "mk_blind_rotate_kernel_w2_acc<4,rw2>" and np.array_equal(got, case["want"][(0, 1)])
    finally:
        eng.set_option("mk_general", 0)
        eng.set_option("mk_rw", 0)


@pytest.mark.gpu
def test_gpu_references_agree(tfhe, case):
    """Engine.mk_blind_rotate(in_form 0, sel None) on the key's selectors gives the checker's words: the two references are one."""
    eng, acc, x, want = case["eng"], case["acc"], case["x"], case["want"]
    assert np.array_equal(eng.mk_blind_rotate(acc, x, acc_index=ACC_INDEX, in_form=0, out_form=0), want[(0, 1)])
    assert eng.last_kernel_name().startswith("mk_tlwe_rotate_kernel(")
    assert np.array_equal(eng.mk_blind_rotate(acc, x, acc_index=ACC_INDEX, in_form=0, n_out=32, out_form=1), want[(1, 32)])
    assert np.array_equal(eng.mk_blind_rotate(acc, x, acc_index=ACC_INDEX, in_form=0, n_out=4, out_form=2), want[(2, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize("rw,B", [(1, 1), (2, 3), (0, 5), (1, 5), (2, 5)], ids=["rw1-B1", "rw2-B3", "rw0-B5", "rw1-B5", "rw2-B5"])
def test_gpu_mk_bootstrap_acc_equals_checker(tfhe, case, rw, B):
    """mk_rw 1 with one row, mk_rw 2 with three (a padding rotation beside row 2), mk_rw 0 (by size: one rotation per workgroup), and all
    five rows under both forced geometries; out_form 0, 1, 2 and n_out 1, 4, 32 each."""
    eng, acc, x = case["eng"], case["acc"], case["x"]
    rows = [2] if B == 1 else range(B)                              # (B = 1: the row with barb = 2N - 1 on accumulator 2)
    try:
        eng.set_option("mk_rw", rw)
        _check_rows(eng, acc, x, ACC_INDEX, case["want"], rows, rw == 2, (rw, B))
        if B == 5:
            # NULL acc_index = accumulator 0 for every row: rows 1 and 4 of the calls above
            assert np.array_equal(eng.mk_bootstrap_acc(acc, x[[1, 4]], out_form=0), case["want"][(0, 1)][[1, 4]]), "NULL acc_index"
    finally:
        eng.set_option("mk_rw", 0)


@pytest.mark.gpu
def test_gpu_trivial_accumulator_equals_mk_bootstrap_tv_multi(tfhe, case):
    """(0, 0, tv): tfhe_mk_bootstrap_tv_multi_batch word for word, n_out 1 and 4, with and without keyswitch."""
    from tfhe_jl_amd import leveled
    eng, x, rng = case["eng"], case["x"], case["rng"]
    tv = _words(rng, 2, N)
    idx = np.array([0, 1, 1, 0, 1], np.int32)
    for n_out in (1, 4):
        for ks in (False, True):
            want = eng.mk_bootstrap_tv_multi(tv, x, n_out, index=idx, with_keyswitch=ks)
            assert eng.last_kernel_name() == "mk_blind_rotate_kernel_w2<4>+tv"
            got = eng.mk_bootstrap_acc(leveled.mk_tlwe_trivial(tv, P), x, acc_index=idx, n_out=n_out, out_form=2 if ks else 1)
            assert eng.last_kernel_name() == _name(False)
            assert got.shape == want.shape and np.array_equal(got, want), (n_out, ks)


# ---- 3. GPU: the level form ---------------------------------------------------------------------------------------------------------
def _tables(case, eng=None, wires=WIRES):
    """The case's engine (or `eng`) with an MK TLWE table (the three accumulators, then arbitrary samples) and a multi-key wire table
    (arbitrary rows, the case's rows in wires 1 ... 5); wires 0: no wire table."""
    eng, rng, n = eng or case["eng"], case["rng"], case["n"]
    full_t = np.ascontiguousarray(np.concatenate([case["acc"], _words(rng, SLOTS - 3, P + 1, N)]))
    allw = _words(rng, max(wires, 1 + B_ROWS), P * n + 1)
    allw[1:1 + B_ROWS] = case["x"]
    eng.mk_tlwe_alloc(SLOTS)
    eng.mk_tlwe_upload(0, full_t)
    if wires:
        eng.mk_wires_alloc(wires)
        eng.wires_upload(0, allw)
    return full_t, allw


@pytest.mark.gpu
def test_gpu_mk_bootstrap_acc_level_equals_mk_blind_rotate_level(tfhe, case):
    """Rows of 0, 1 and 3 terms with coefficients that wrap, cst NULL and set, a repeated acc_slot, out_form 0 into a permuted out_slot and
    out_form 2 into permuted wires with n_out 1 and 4: the tables after the call are those after Engine.mk_blind_rotate_level, every slot
    and every wire; under mk_rw 1 and 2."""
    eng, rng = case["eng"], case["rng"]
    full_t, allw = _tables(case)
    B = len(ACC_SLOT)
    assert len(set(ACC_SLOT.tolist())) < B and (np.diff(OUT_SLOT) < 0).any() and {0, 1, 3} <= set(np.diff(TERM_START).tolist())
    cst_set = _words(rng, B)
    cst_set[5] = 0
    try:
        for cst, rw in ((cst_set, 1), (None, 2)):
            eng.set_option("mk_rw", rw)
            eng.mk_blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, out_form=0, out_slot=OUT_SLOT)
            want = eng.mk_tlwe_download(0, SLOTS)
            assert not np.array_equal(want, full_t)
            eng.mk_tlwe_upload(0, full_t)
            eng.mk_bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, out_form=0, out_slot=OUT_SLOT)
            assert eng.last_kernel_name() == _name(rw == 2) and eng.last_rotation_count() == B and eng.last_timing_ms(0) > 0
            assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), want), ("out_form 0", cst is None)
            assert np.array_equal(eng.wires_download(0, WIRES), allw)
            eng.mk_tlwe_upload(0, full_t)
            # ... and the batch call on the rows the terms form
            rows = form_rows(allw, TERM_START, TERM_WIRE, TERM_COEF, cst)
            assert np.array_equal(want[OUT_SLOT], eng.mk_bootstrap_acc(full_t, rows, acc_index=ACC_SLOT, out_form=0))
            for n_out in (1, 4):
                out_wires = (IN_WIRES + rng.permutation(WIRES - IN_WIRES)[:B * n_out]).astype(np.int32)
                eng.mk_blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
                want_w = eng.wires_download(0, WIRES)
                assert not np.array_equal(want_w, allw)
                eng.wires_upload(0, allw)
                eng.mk_bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
                assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
                assert np.array_equal(eng.wires_download(0, WIRES), want_w), ("out_form 2", n_out, cst is None)
                assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), full_t)
                eng.wires_upload(0, allw)
    finally:
        eng.set_option("mk_rw", 0)
        eng.mk_tlwe_alloc(0)
        eng.mk_wires_alloc(0)


@pytest.mark.gpu
def test_gpu_level_without_a_wire_table_runs(tfhe, case, rotref):
    """A context with the multi-key bootstrapping key and an MK TLWE table, no wire table, no keyswitch key and no selector set: a call
    without terms and with out_form 0 reads and writes no wire and succeeds; its rows are (0, ..., 0, cst[g]), all zero with cst NULL."""
    K, rng, n = case["K"], case["rng"], case["n"]
    raw = tfhe.Engine(K.params)
    try:
        raw.mk_load_bootstrap_key(K.ck.bootstrap_key, P)
        full_t, _ = _tables(case, eng=raw, wires=0)
        acc_slot, out_slot, start = np.array([1, 0, 1, 2], np.int32), np.array([9, 4, 12, 5], np.int32), np.zeros(5, np.int32)
        cst_set = _words(rng, 4)
        cst_set[0] = _word(N + 3, -7)
        for cst in (cst_set, None):
            raw.mk_bootstrap_acc_level(acc_slot, start, [], [], cst=cst, out_form=0, out_slot=out_slot)
            assert raw.last_kernel_name() == _name(False) and raw.last_rotation_count() == 4
            rows = np.zeros((4, P * n + 1), np.int32)
            if cst is not None:
                rows[:, P * n] = cst
            want = full_t.copy()
            want[out_slot] = rotref(K.oracle, full_t, acc_slot, rows, 1, 0)
            assert (cst is None) == np.array_equal(want[out_slot], full_t[acc_slot])                 # (all exponents 0: a copy)
            assert np.array_equal(raw.mk_tlwe_download(0, SLOTS), want), ("cst NULL" if cst is None else "cst set")
            raw.mk_tlwe_upload(0, full_t)
    finally:
        raw.close()


# ---- 4. GPU: step counts 2 and 4, and the switch to pairs by size --------------------------------------------------------------------
def _tiny(tfhe, orc, n, seed, owners=(0, 1, 1, 0)):
    s = Setup(tfhe, P, N, L, BETA, seed, owners=list(owners), n=n)
    o = orc.Oracle(n, N, 1, L, BETA, s.p.ks_decomp_length, s.p.ks_log2_base, parties=P)
    o.load_bootstrap_key(s.ck.bootstrap_key)
    o.load_keyswitch_key(s.ck.keyswitch_key)
    return s, o


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
def test_gpu_step_counts_two_and_four(tfhe, orc, rotref, n):
    """n = 1: one step per party, each loop's look-ahead read lands on the other party's word and on barb; n = 2: two."""
    s, o = _tiny(tfhe, orc, n, 5100 + n)
    eng = s.ck.engine(0)
    acc, x = _accs(s.rng), _rows(s.rng, P * n)
    want = _wants(rotref, o, acc, ACC_INDEX, x)
    assert eng.get_option("mk_bootstrap_acc") == 1
    try:
        for rw in (1, 2):
            eng.set_option("mk_rw", rw)
            _check_rows(eng, acc, x, ACC_INDEX, want, range(B_ROWS), rw == 2, (n, rw))
    finally:
        s.ck.close()


@pytest.mark.gpu
def test_gpu_batch_size_switch_to_pairs(tfhe, orc):
    """mk_rw 0 chooses by the batch: one rotation per workgroup up to one row per compute unit, pairs beyond; cu_count + 1 rows are pairs
    with a padding rotation in the last workgroup.  n = 2; eight sampled rows and the last against Engine.mk_blind_rotate."""
    from tfhe_jl_amd import leveled
    n = 2
    s, _ = _tiny(tfhe, orc, n, 5200)
    eng = s.ck.engine(0)
    try:
        eng.mk_tgsw_load(*leveled.mk_bootstrap_key_selectors(s.ck))
        cu = _cu_count()
        acc = _accs(s.rng)
        for R in (cu, cu + 1):
            x = _words(s.rng, R, P * n + 1)
            idx = (np.arange(R) % 3).astype(np.int32)
            got = eng.mk_bootstrap_acc(acc, x, acc_index=idx, out_form=0)
            assert eng.last_kernel_name() == _name(R > cu), (R, cu, eng.last_kernel_name())
            assert eng.last_rotation_count() == R and got.shape == (R, P + 1, N)
            pick = np.unique(np.concatenate([s.rng.integers(0, R - 1, 8), [R - 1]]))
            want = eng.mk_blind_rotate(acc, x[pick], acc_index=idx[pick], in_form=0, out_form=0)
            assert np.array_equal(got[pick], want), (R, pick.tolist())
            got2 = eng.mk_bootstrap_acc(acc, x, acc_index=idx, n_out=2, out_form=2)
            want2 = eng.mk_blind_rotate(acc, x[pick], acc_index=idx[pick], in_form=0, n_out=2, out_form=2)
            assert np.array_equal(got2[pick], want2), (R, "out_form 2")
    finally:
        s.ck.close()


# ---- 5. GPU: mktfhe_parameters_2party at full size ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_private_table_full_size_equals_checker(tfhe, full):          # noqa: F811
    """B = 4 rows of a private table Z_4 -> Z_2 at n = 500, the key expanded on the device and never loaded as selectors: out_form 1 and 2
    equal the C checker word for word and decrypt F[m], through mk_blind_rotate_lookup(tuned=True)."""
    from tfhe_jl_amd import leveled, lut
    ck = tfhe.MKCloudKey(full.parts, expand="device")
    try:
        eng = ck.engine(0)
        got1 = leveled.mk_blind_rotate_lookup(ck, full.acc, full.x, out_form=1, tuned=True)
        assert eng.last_kernel_name() == _name(False) and eng.last_rotation_count() == 4
        assert got1.shape == (4, 1, 2 * N + 1) and np.array_equal(got1, full.want[1])
        got2 = leveled.mk_blind_rotate_lookup(ck, full.acc, full.x, tuned=True)
        assert got2.shape == (4, 2 * full.p.lwe_size + 1) and np.array_equal(got2, full.want[2][:, 0])
        assert list(lut.mk_lut_decrypt(full.sks, got2, 2)) == [full.F[v] for v in full.m]
    finally:
        ck.close()


# ---- 6. GPU: the helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_tuned_helpers_equal_the_untuned_ones(tfhe, orc):
    """mk_two_stage_lookup, mk_pbs_to_tlwe and mk_two_stage_lookup_device with tuned=True at (2, 1024, 4, 7), n = 2: the words of
    tuned=False; the device form twice, the second request swapping its address bits into the set of the first."""
    from tfhe_jl_amd import leveled, lut
    B, d, p = 3, 2, 4
    highs = [1, 2, 3]
    s = Setup(tfhe, P, N, L, BETA, 5300, owners=[0, 1] * B, bits=[(h >> v) & 1 for h in highs for v in range(d)], n=2)
    try:
        table = [int(v) for v in np.random.default_rng(5).integers(0, p, p << d)]
        tables = np.concatenate([leveled.mk_tlwe_trivial(lut.make_test_vector(lambda m, h=h: table[p * h + m], p, N), P) for h in range(1 << d)])
        x = lut.mk_lut_encrypt(s.rng, s.sks, np.arange(B) & (p - 1), p)
        uni = [a.reshape(B, d, L, N) for a in s.uni]
        for form in (0, 2):
            want = leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, p, out_form=form)
            got = leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, p, out_form=form, tuned=True)
            assert s.ck.engine(0).last_kernel_name() == _name(False)
            assert np.array_equal(got, want), form
        assert np.array_equal(leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, p, expand="host", tuned=True), want)
        want = leveled.mk_pbs_to_tlwe(s.ck, x, lambda m: table[m], p)
        assert np.array_equal(leveled.mk_pbs_to_tlwe(s.ck, x, lambda m: table[m], p, tuned=True), want)
        # between the tables
        eng = s.ck.engine(0)
        eng.mk_tlwe_alloc(8)
        eng.mk_tlwe_upload(0, tables)
        eng.mk_wires_alloc(8)
        eng.wires_upload(0, x)
        outs = {}
        for tuned in (False, True, True):
            leveled.mk_two_stage_lookup_device(s.ck, 0, uni, [0, 1], [0, 1, 2], [4, 5, 6], 4, tuned=tuned)
            outs[tuned] = eng.wires_download(4, 3)
            eng.wires_upload(4, np.zeros((3, P * 2 + 1), np.int32))
        assert eng.last_kernel_name() == _name(False)
        assert np.array_equal(outs[True], outs[False])
        assert np.array_equal(outs[True], leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, p))
    finally:
        s.ck.close()


# ---- 7. GPU: the contract -----------------------------------------------------------------------------------------------------------
class _Call:
    """A valid raw call of tfhe_mk_bootstrap_acc_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, acc, rows):
        self.eng = eng
        self.args = dict(acc=acc, T=acc.shape[0], acc_index=np.zeros(rows.shape[0], np.int32), rows=rows, n_out=1, out_form=0, B=rows.shape[0])

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        out = np.zeros((self.args["B"], 4, 3 * N), np.int32)
        rc = e._lib.tfhe_mk_bootstrap_acc_batch(e._h, _p(a["acc"]), a["T"], _p(a["acc_index"]), _p(a["rows"]), a["n_out"], a["out_form"], _p(a.get("out", out)),
                                                a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode(), out


@pytest.mark.gpu
def test_gpu_contract_refusals_leave_the_context_usable(tfhe, orc, case):
    K, eng, acc, x, n = case["K"], case["eng"], case["acc"], case["x"], case["n"]
    rows = x[:2]
    call = _Call(eng, acc, rows)
    rc, msg, out = call()
    assert rc == OK, msg
    want = out.copy()
    full_t, allw = _tables(case)
    xs, ys = tfhe.mk_encrypt(K.rng, K.sks, [True, False, True]), tfhe.mk_encrypt(K.rng, K.sks, [True, True, False])

    def still_right():
        rc, msg, out = call()
        assert rc == OK and np.array_equal(out, want), msg
        assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), full_t) and np.array_equal(eng.wires_download(0, WIRES), allw)
        assert np.array_equal(tfhe.mk_decrypt(K.sks, eng.mk_gate_nand(xs, ys)), [False, True, True])

    def refused(code, word, **over):
        rc, msg, _ = call(**over)
        assert rc == code and word in msg and msg.startswith("mk_bootstrap_acc_batch:"), (list(over), rc, msg)
        still_right()

    def level(e=None, **over):
        a = dict(acc_slot=ACC_SLOT, term_start=TERM_START, term_wire=TERM_WIRE, term_coef=TERM_COEF, cst=None, n_out=1, out_form=0, out_slot=OUT_SLOT,
                 out_wires=None, B=len(ACC_SLOT))
        a.update(over)
        e = e or eng
        arr = {k: None if a[k] is None else np.ascontiguousarray(a[k], np.int32) for k in ("acc_slot", "term_start", "term_wire", "term_coef", "cst", "out_slot", "out_wires")}
        rc = e._lib.tfhe_mk_bootstrap_acc_level(e._h, _p(arr["acc_slot"]), _p(arr["term_start"]), _p(arr["term_wire"]), _p(arr["term_coef"]), _p(arr["cst"]),
                                                a["n_out"], a["out_form"], _p(arr["out_slot"]), _p(arr["out_wires"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode()

    def level_refused(code, word, **over):
        rc, msg = level(**over)
        assert rc == code and word in msg and msg.startswith("mk_bootstrap_acc_level:"), (list(over), rc, msg)
        still_right()

    try:
        still_right()
        assert call(B=0)[0] == OK and call(B=0, acc=None, rows=None, out=None)[0] == OK and level(B=0)[0] == OK          # B = 0 is TFHE_OK
        refused(INVALID, "negative", B=-1)
        for name in ("acc", "rows", "out"):
            refused(INVALID, "NULL", **{name: None})
        for form in (3, -1):
            refused(INVALID, f"out_form = {form}", out_form=form)
        refused(INVALID, "T = 0", T=0)
        refused(INVALID, "n_out = 0", n_out=0)
        refused(INVALID, "n_out = 3", n_out=3, out_form=1)
        refused(INVALID, "n_out = 64", n_out=64, out_form=1)
        refused(INVALID, "n_out = 4 with out_form 0", n_out=4)
        refused(INVALID, "acc_index[1] = 3", acc_index=np.array([0, 3], np.int32))
        refused(INVALID, "acc_index[0] = -1", acc_index=np.array([-1, 0], np.int32))
        level_refused(INVALID, "negative", B=-1)
        level_refused(INVALID, "NULL", acc_slot=None)
        level_refused(INVALID, "NULL out_slot", out_slot=None)
        level_refused(INVALID, "out_form = 1", out_form=1)
        level_refused(INVALID, "written twice", out_slot=[7, 8, 9, 15, 10, 12, 14, 14])
        level_refused(INVALID, "output slot of the same call", out_slot=[7, 8, 9, 15, 10, 12, 14, 3])
        level_refused(INVALID, "outside the table", acc_slot=[3, 2, 3, 5, 4, 6, 0, SLOTS])
        level_refused(INVALID, "reads wire", term_wire=[1, 2, 3, 2, 4, 5, 6, WIRES])
        level_refused(INVALID, "which the same call writes", out_form=2, out_wires=[20, 21, 22, 23, 24, 25, 26, 1])
        # measure_margin: no DIAG instantiation
        eng.set_option("measure_margin", 1)
        rc, msg, _ = call()
        assert rc == STATE and "measure_margin" in msg
        rc, msg = level()
        assert rc == STATE and "measure_margin" in msg
        eng.set_option("measure_margin", 0)
        still_right()
        # an oversized batch: refused before anything is allocated (the device's free memory reads unchanged)
        lib = eng._lib
        before = _mem_free()
        rc = lib.tfhe_mk_bootstrap_acc_batch(eng._h, _p(acc), 3, None, _p(rows), 1, 0, _p(np.zeros(1, np.int32)), 2**31 - 1)
        assert rc == NOMEM and "MB" in lib.tfhe_last_error(eng._h).decode()
        assert _mem_free() == before
        still_right()
        # a multi-device context
        multi = K.ck.engine([0, 0])
        rc, msg, _ = call(multi)
        assert rc == STATE and "multi-device" in msg
        still_right()
    finally:
        eng.set_option("measure_margin", 0)
        eng.mk_tlwe_alloc(0)
        eng.mk_wires_alloc(0)

    # no multi-key bootstrapping key, then out_form 2 without the multi-key keyswitch key (forms 0 and 1 do not need it); no selector set
    # is ever asked for
    raw = tfhe.Engine(K.params)
    try:
        assert raw.get_option("mk_bootstrap_acc") == 1
        rc, msg, _ = call(raw)
        assert rc == NO_KEY and "bootstrapping key" in msg, (rc, msg)
        raw.mk_load_bootstrap_key(K.ck.bootstrap_key, P)
        rc, msg, _ = call(raw, out_form=2)
        assert rc == NO_KEY and "keyswitch" in msg, (rc, msg)
        rc, msg, _ = call(raw, out_form=2, n_out=0)
        assert rc == INVALID and "n_out" in msg                       # a bad scalar is named before the missing keyswitch key
        rc, msg, out = call(raw)
        assert rc == OK and np.array_equal(out, want), msg
        raw.mk_load_keyswitch_key(K.ck.keyswitch_key, P)
        assert np.array_equal(raw.mk_bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=4), case["want"][(2, 4)])
        # an injected allocation failure through the new entry point: NOMEM, and the context goes on working (on this context, which is
        # closed next: the message of a caught exception stays this thread's answer for the context)
        lib = raw._lib
        assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
        rc, msg, _ = call(raw)
        lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
        assert rc == NOMEM and "memory" in msg, (rc, msg)
        rc, _, out = call(raw)
        assert rc == OK and np.array_equal(out, want)
        assert np.array_equal(raw.mk_bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=4), case["want"][(2, 4)])
    finally:
        raw.close()
    # the any-N key layout at the served shape (option br_anyn, before the key is loaded)
    raw = tfhe.Engine(K.params)
    try:
        raw.set_option("br_anyn", 1)
        assert raw.get_option("mk_bootstrap_acc") == 0
        raw.mk_load_bootstrap_key(K.ck.bootstrap_key, P)
        rc, msg, _ = call(raw)
        assert rc == STATE and "any-N" in msg and "tfhe_mk_blind_rotate_batch" in msg, (rc, msg)
    finally:
        raw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P_,N_,l_,beta_", [(2, 1024, 2, 10), (3, 1024, 4, 7), (2, 64, 3, 7)], ids=["l2", "3party", "N64"])
def test_gpu_shapes_not_served_are_refused(tfhe, orc, P_, N_, l_, beta_):
    """l != 4, parties != 2 and N != 1024 (whose key is in the any-N layout): TFHE_ERR_STATE naming the shape and pointing to
    tfhe_mk_blind_rotate_batch, option mk_bootstrap_acc 0, tuned=True a ValueError; the any-N call and the gates go on."""
    from tfhe_jl_amd import leveled
    s = Setup(tfhe, P_, N_, l_, beta_, 5400 + P_ + l_, owners=[0], n=2)
    try:
        eng = s.ck.engine(0)
        assert eng.get_option("mk_bootstrap_acc") == 0
        acc = s.encrypt(_words(s.rng, 1, N_))
        x = _words(s.rng, 2, P_ * 2 + 1)
        out = np.zeros((2, P_ + 1, N_), np.int32)
        rc = eng._lib.tfhe_mk_bootstrap_acc_batch(eng._h, _p(acc), 1, None, _p(x), 1, 0, _p(out), 2)
        msg = eng._lib.tfhe_last_error(eng._h).decode()
        assert rc == STATE and f"{P_} parties, N = {N_}, l = {l_}" in msg and "tfhe_mk_blind_rotate_batch" in msg, (rc, msg)
        assert not out.any()
        with pytest.raises(ValueError, match="mk_bootstrap_acc is 0"):
            leveled.mk_blind_rotate_lookup(s.ck, acc, x, out_form=0, tuned=True)
        got = leveled.mk_blind_rotate_lookup(s.ck, acc, x, out_form=0, expand="host")
        assert got.shape == (2, P_ + 1, N_)
        xs, ys = tfhe.mk_encrypt(s.rng, s.sks, [True, False]), tfhe.mk_encrypt(s.rng, s.sks, [True, True])
        assert np.array_equal(tfhe.mk_decrypt(s.sks, eng.mk_gate_nand(xs, ys)), [False, True])
    finally:
        s.ck.close()


@pytest.mark.gpu
def test_gpu_single_key_context_is_refused_both_ways(tfhe, case):
    """A single-key context refuses the new calls and its gates go on; the single-key tfhe_bootstrap_acc_batch keeps refusing a multi-key
    context."""
    rng = np.random.default_rng(77)
    p1 = tfhe.SchemeParameters(16, 1 / 2**15, N, 1, 2, 10, 1e-7, 8, 2, 1 / 2**15, 1)
    sk1, ck1 = tfhe.make_key_pair(rng, p1)
    try:
        e1 = ck1.engine(0)
        assert e1.get_option("mk_bootstrap_acc") == 0
        rc, msg, _ = _Call(e1, case["acc"], case["x"][:2])()
        assert rc == STATE and "single-key" in msg and msg.startswith("mk_bootstrap_acc_batch:"), (rc, msg)
        rc = e1._lib.tfhe_mk_bootstrap_acc_level(e1._h, _p(np.zeros(1, np.int32)), _p(np.zeros(2, np.int32)), None, None, None, 1, 0, _p(np.ones(1, np.int32)), None, 1)
        assert rc == STATE and "single-key" in e1._lib.tfhe_last_error(e1._h).decode()
        bx = tfhe.encrypt(rng, sk1, [True, False]).data
        assert np.array_equal(tfhe.decrypt(sk1, e1.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    finally:
        ck1.close()
    eng = case["eng"]
    with pytest.raises(tfhe.EngineError) as err:
        eng.bootstrap_acc(np.zeros((1, 2, N), np.int32), np.zeros((1, case["n"] + 1), np.int32), out_form=0)
    assert err.value.code == STATE and "multi-key" in str(err.value)
    assert np.array_equal(eng.mk_bootstrap_acc(case["acc"], case["x"], acc_index=ACC_INDEX, out_form=0), case["want"][(0, 1)])
