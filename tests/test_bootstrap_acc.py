"""Private-table rotation on the gates' own kernel and key (tfhe_bootstrap_acc_batch, tfhe_bootstrap_acc_level; Engine.bootstrap_acc,
Engine.bootstrap_acc_level; tuned=True in tfhe_jl_amd.leveled) against three references: tests/test_blind_rotate.py's integer schoolbook
`Rotation.rotate_lwe` over the bootstrapping key as selectors (with `extract_at` and leveled_ref.ks_ref behind it), Engine.blind_rotate /
Engine.blind_rotate_level on the same inputs after tgsw_load(bootstrap_key_selectors(ck)), and, for a trivial accumulator,
Engine.bootstrap_tv_multi.  Every comparison is word for word.

The kernel exists at N = 1024, k = 1 only.  (l, beta) = (2, 10), (3, 8), (4, 6) take the L = 2 and L = 3 instantiations and the run-time-l
one; n = 5 is an odd step count inside one lockstep period of four steps, n = 9 crosses the barriers at steps 0, 4 and 8.  B = 5 runs as
five workgroups (v3_rw 1) and as two workgroups of four waves with three padding waves (v3_rw 4).  The schoolbook words of a case are
computed once and shared by the tests of that case.

Section 3b holds the edges that the random programs of tests/test_bootstrap_acc_programs.py cannot reach: the switch of v3_rw 0 to four
rotations per workgroup at 6 rotations per compute unit (the count read from the HIP runtime), n = 1, 4 and 8 steps, n_out 2, 8, 16 and 32,
the level form under v3_rw 4 with padding waves and a permuted out_slot, a successful level call on a context without a wire table, and
workspaces that grow behind a gate level that is still queued; each against the schoolbook alone."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from test_blind_rotate import Rotation
from test_independent import Schoolbook
from test_leveled import _params, _words
from test_tlwe_levels import ACC_SLOT, IN_WIRES, OUT_SLOT, SLOTS, TERM_COEF, TERM_START, TERM_WIRE, WIRES, form_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_KEY, STATE, NOMEM = 0, 1, 3, 5, 6
N, K = 1024, 1
SHAPES = [(2, 10), (3, 8), (4, 6)]
STEPS = [5, 9]
ACC_INDEX = np.array([2, 0, 2, 1, 0], np.int32)
B_ROWS = 5
UNIT = 2**21                                                        # 2^32 / 2N: one step of the exponent


# ---- 1. CPU -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(tfhe):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read(), flags=re.S)
    lib = tfhe._lib.load()
    for name, argc in (("tfhe_bootstrap_acc_batch", 9), ("tfhe_bootstrap_acc_level", 11)):
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m and len(m.group(1).split(",")) == argc, name
        assert name in tfhe._lib.ABI_SYMBOLS and hasattr(lib, name), name
    assert callable(getattr(tfhe.Engine, "bootstrap_acc")) and callable(getattr(tfhe.Engine, "bootstrap_acc_level"))
    from tfhe_jl_amd import leveled
    for f in (leveled.blind_rotate_lookup, leveled.two_stage_lookup, leveled.pbs_to_tlwe):
        assert inspect.signature(f).parameters["tuned"].default is False, f.__name__


def _word(e, off=0):
    """The int32 word that the modulus switch takes to exponent e (mod 2N) when off lies in [-2^20, 2^20)."""
    return int(np.array([(e * UNIT + off) % 2**32], np.uint32).view(np.int32)[0])


def _rows(rng, n):
    """LWE words whose switched exponents include 0, 1, N and 2N - 1, barb in {0, N, 2N - 1}, both sides of a rounding boundary, and an
    all-zero row."""
    plant = [0, 1, N, 2 * N - 1]
    x = _words(rng, B_ROWS, n + 1)
    if n < 4:                                                        # the planted exponents down the rows, at step 0: 1, N, 2N - 1, 0
        x[0, :n], x[0, n] = _word(1, 2**20 - 1), _word(0)            # (just below a rounding boundary)
        x[1, :n], x[1, n] = _word(N), _word(N)
        x[2, :n], x[2, n] = _word(2 * N - 2, 2**20), _word(2 * N - 1)      # (on the boundary: 2N - 2 -> 2N - 1)
        x[3, :] = 0
        return x
    x[0, :n] = [_word(plant[i % 4]) for i in range(n)]
    x[0, n] = _word(0)
    x[1, 0], x[1, 1] = _word(3, 2**20 - 1), _word(3, 2**20)          # e 2^21 + 2^20 - 1 -> e, e 2^21 + 2^20 -> e + 1
    x[1, n] = _word(N)
    x[2, :n] = [_word(plant[(i + 1) % 4], -5) for i in range(n)]
    x[2, n] = _word(2 * N - 1)
    x[3, :] = 0
    return x


@functools.lru_cache(maxsize=None)
def _case(tfhe, l, beta, n):
    """A real key pair at (N, k, l, beta, n), its engine with the key's n entries loaded as selectors, T = 3 accumulators, B = 5 rows, and
    the schoolbook's final accumulators of the rows under ACC_INDEX."""
    from tfhe_jl_amd import leveled
    p = _params(tfhe, N, K, l, beta, n=n)
    rng = np.random.default_rng(8800 + 10 * l + n)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    sels = leveled.bootstrap_key_selectors(ck)
    eng.tgsw_load(sels)
    msg = _words(rng, 1, N)
    msg[0, 0], msg[0, 1] = 2**31 - 1, -2**31
    tv = _words(rng, 1, N)
    acc = np.ascontiguousarray(np.concatenate([leveled.tlwe_encrypt(rng, sk, msg), leveled.tlwe_trivial(tv, K), np.zeros((1, K + 1, N), np.int32)]))
    x = _rows(rng, n)
    sb = Schoolbook(n, N, K, l, beta, 8, 2, sels)
    exps = np.array([sb.modswitch(r) for r in x], np.int64) % (2 * N)
    if n < 4:
        assert list(exps[:4, 0]) == [1, N, 2 * N - 1, 0] and list(exps[:4, n]) == [0, N, 2 * N - 1, 0] and not exps[3].any()
    else:
        assert list(exps[0, :4]) == [0, 1, N, 2 * N - 1] and exps[0, n] == 0 and list(exps[1, :2]) == [3, 4] and exps[1, n] == N
        assert exps[2, n] == 2 * N - 1 and list(exps[2, :4]) == [1, N, 2 * N - 1, 0] and not exps[3].any()
    ref = Rotation(N, K, l, beta, sels)
    want = np.stack([ref.rotate_lwe(acc[ACC_INDEX[g]], x[g]) for g in range(B_ROWS)])
    return dict(rng=rng, sk=sk, ck=ck, eng=eng, sels=sels, acc=acc, tv=tv, x=x, ref=ref, want=want)


def _name(l, rw4):
    rest = ",8,tw2reg,rw4" if rw4 else ",8,tw2reg"
    return f"blind_rotate_kernel_v3_acc<{l}{rest}>" if l in (2, 3) else f"blind_rotate_kernel_v3_acc<0{rest}>(l={l})"


# ---- 2. GPU: word for word ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("l,beta", SHAPES)
def test_gpu_bootstrap_acc_equals_schoolbook_and_blind_rotate(tfhe, l, beta, n):
    from leveled_ref import ks_ref, ks_schoolbook
    c = _case(tfhe, l, beta, n)
    eng, acc, x, ref, want = c["eng"], c["acc"], c["x"], c["ref"], c["want"]
    assert eng.get_option("bootstrap_acc") == 1
    sbk = ks_schoolbook(c["ck"].params, c["ck"].keyswitch_key)
    want_ext = {n_out: np.stack([[ref.extract_at(w, j * (N // n_out)) for j in range(n_out)] for w in want]).astype(np.int32) for n_out in (1, 4, 32)}
    want_ks = {n_out: ks_ref(sbk, want_ext[n_out]) for n_out in (1, 4)}
    other0 = eng.blind_rotate(acc, x, acc_index=ACC_INDEX, in_form=0, out_form=0)
    assert eng.last_kernel_name().startswith("tlwe_rotate_kernel(")
    assert np.array_equal(other0, want.astype(np.int32)), "the references agree"
    try:
        for rw in (1, 4):
            eng.set_option("v3_rw", rw)
            got0 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, out_form=0)
            assert eng.last_kernel_name() == _name(l, rw == 4), eng.last_kernel_name()
            assert eng.last_rotation_count() == B_ROWS and eng.last_timing_ms(0) > 0
            assert got0.shape == (B_ROWS, K + 1, N) and np.array_equal(got0, want.astype(np.int32)), ("out_form 0", rw)
            for n_out in (1, 4, 32):
                got1 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=n_out, out_form=1)
                assert got1.shape == (B_ROWS, n_out, K * N + 1) and np.array_equal(got1, want_ext[n_out]), ("out_form 1", n_out, rw)
            assert np.array_equal(got1, eng.blind_rotate(acc, x, acc_index=ACC_INDEX, in_form=0, n_out=32, out_form=1))
            for n_out in (1, 4):
                got2 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=n_out, out_form=2)
                assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
                assert got2.shape == (B_ROWS, n_out, n + 1) and np.array_equal(got2, want_ks[n_out]), ("out_form 2", n_out, rw)
            assert np.array_equal(got2, eng.blind_rotate(acc, x, acc_index=ACC_INDEX, in_form=0, n_out=4, out_form=2))
            # NULL acc_index = accumulator 0 for every row: rows 1 and 4 of the calls above; B = 1: row 2 alone
            assert np.array_equal(eng.bootstrap_acc(acc, x[[1, 4]], out_form=0), want[[1, 4]].astype(np.int32)), ("NULL acc_index", rw)
            one = eng.bootstrap_acc(acc[2:], x[2:3], n_out=4, out_form=1)
            assert eng.last_rotation_count() == 1 and np.array_equal(one, want_ext[4][2:3]), ("B = 1", rw)
    finally:
        eng.set_option("v3_rw", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("l,beta", SHAPES)
def test_gpu_trivial_accumulator_equals_bootstrap_tv_multi(tfhe, l, beta):
    from tfhe_jl_amd import leveled
    c = _case(tfhe, l, beta, 9)
    eng, tv, x = c["eng"], c["tv"], c["x"]
    for n_out in (1, 4):
        for ks in (False, True):
            want = eng.bootstrap_tv_multi(tv, x, n_out, with_keyswitch=ks)
            assert eng.last_kernel_name().endswith("+tv")
            got = eng.bootstrap_acc(leveled.tlwe_trivial(tv, K), x, n_out=n_out, out_form=2 if ks else 1)
            assert eng.last_kernel_name() == _name(l, False)
            assert got.shape == want.shape and np.array_equal(got, want), (n_out, ks)


# ---- 3. GPU: the level form ---------------------------------------------------------------------------------------------------------
def _tables(c, n, wires=WIRES, eng=None):
    """The case's engine (or `eng`) with a TLWE table (the three accumulators, then encryptions) and a wire table (arbitrary rows, the
    case's rows in wires 1 ... 5); wires 0: no wire table."""
    from tfhe_jl_amd import leveled
    eng, rng = eng or c["eng"], c["rng"]
    full = np.ascontiguousarray(np.concatenate([c["acc"], leveled.tlwe_encrypt(rng, c["sk"], _words(rng, SLOTS - 3, N))]))
    allw = _words(rng, max(wires, 1 + B_ROWS), n + 1)
    allw[1:1 + B_ROWS] = c["x"]
    eng.tlwe_alloc(SLOTS)
    eng.tlwe_upload(0, full)
    eng.wires_alloc(wires)
    if wires:
        eng.wires_upload(0, allw)
    return full, allw


@pytest.mark.gpu
def test_gpu_bootstrap_acc_level_equals_blind_rotate_level(tfhe):
    """Rows of 0, 1 and 3 terms with coefficients that wrap, cst NULL and set, a repeated acc_slot (test_tlwe_levels' rows), out_form 0 into
    slots and out_form 2 into permuted wires with n_out 1 and 4: the tables after the call are those after Engine.blind_rotate_level; and a
    call queued behind an asynchronous gates_level reads what that level wrote."""
    l, beta, n = 2, 10, 9
    c = _case(tfhe, l, beta, n)
    eng, rng = c["eng"], c["rng"]
    full, allw = _tables(c, n)
    B = len(ACC_SLOT)
    cst_set = _words(rng, B)
    cst_set[5] = 0
    try:
        for cst in (cst_set, None):
            eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, out_form=0, out_slot=OUT_SLOT)
            want = eng.tlwe_download(0, SLOTS)
            assert not np.array_equal(want, full)
            eng.tlwe_upload(0, full)
            eng.bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, out_form=0, out_slot=OUT_SLOT)
            assert eng.last_kernel_name() == _name(l, False) and eng.last_rotation_count() == B and eng.last_timing_ms(0) > 0
            assert np.array_equal(eng.tlwe_download(0, SLOTS), want), ("out_form 0", cst is None)
            assert np.array_equal(eng.wires_download(0, WIRES), allw)
            eng.tlwe_upload(0, full)
            # ... and the batch call on the rows the terms form
            rows = form_rows(allw, TERM_START, TERM_WIRE, TERM_COEF, cst)
            assert np.array_equal(want[OUT_SLOT], eng.bootstrap_acc(full, rows, acc_index=ACC_SLOT, out_form=0))
            for n_out in (1, 4):
                out_wires = (IN_WIRES + rng.permutation(WIRES - IN_WIRES)[:B * n_out]).astype(np.int32)
                eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
                want_w = eng.wires_download(0, WIRES)
                assert not np.array_equal(want_w, allw)
                eng.wires_upload(0, allw)
                eng.bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
                assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
                assert np.array_equal(eng.wires_download(0, WIRES), want_w), ("out_form 2", n_out, cst is None)
                assert np.array_equal(eng.tlwe_download(0, SLOTS), full)
                eng.wires_upload(0, allw)
        # four waves per workgroup: two workgroups of the eight rows
        eng.set_option("v3_rw", 4)
        eng.bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, out_form=0, out_slot=OUT_SLOT)
        assert eng.last_kernel_name() == _name(l, True) and np.array_equal(eng.tlwe_download(0, SLOTS), want)
        eng.set_option("v3_rw", 0)
        eng.tlwe_upload(0, full)
        # queued behind an asynchronous level: the NAND's output wire is the rotating row
        eng.gates_level(np.zeros(1, np.uint8), [20], [21], None, [40])
        eng.bootstrap_acc_level([0], [0, 1], [40], [1], out_form=2, out_wires=[41])
        row = eng.wires_gather([40])
        assert not np.array_equal(row[0], allw[40])
        assert np.array_equal(eng.wires_gather([41])[0], eng.bootstrap_acc(full, row, acc_index=[0], out_form=2)[0, 0])
    finally:
        eng.set_option("v3_rw", 0)
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


# ---- 3b. GPU: the edges random programs do not reach (tests/test_bootstrap_acc_programs.py) -------------------------------------------
def _cu_count():
    hip = C.CDLL("libamdhip64.so")
    count = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(count), 63, 0) == 0 and count.value > 0      # hipDeviceAttributeMultiprocessorCount
    return count.value


def _extractions(ref, accs, n_out):
    """extract_at of every final accumulator at the coefficients j N / n_out: int32 [B][n_out][N+1]."""
    return np.stack([[ref.extract_at(w, j * (N // n_out)) for j in range(n_out)] for w in accs]).astype(np.int32)


def _level_want(c, full, allw, acc_slot, start, wire, coef, cst):
    """The schoolbook's final accumulators of a level call's rows: int32 [B][2][N]."""
    rows = form_rows(allw, start, wire, coef, cst)
    return np.stack([c["ref"].rotate_lwe(full[a], rows[g]) for g, a in enumerate(acc_slot)]).astype(np.int32)


@pytest.mark.gpu
def test_gpu_batch_size_switch_to_four_rotations_per_workgroup(tfhe):
    """v3_rw 0 chooses by the batch: one wave per workgroup below R0 = 6 compute units' worth of rows, four from R0 up; R0 + 1 is a full set
    of groups plus one wave and three padding waves.  The case's five rows tiled, against the tiled schoolbook words."""
    from leveled_ref import ks_ref, ks_schoolbook
    l, beta, n = 2, 10, 5
    c = _case(tfhe, l, beta, n)
    eng, acc, x, ref = c["eng"], c["acc"], c["x"], c["ref"]
    R0 = 6 * _cu_count()
    want5 = c["want"].astype(np.int32)
    assert set(ACC_INDEX.tolist()) == {0, 1, 2}
    eng.set_option("v3_rw", 0)
    for R in (R0 - 1, R0, R0 + 1):
        tile = np.arange(R) % B_ROWS
        got = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], out_form=0)
        assert eng.last_kernel_name() == _name(l, R >= R0), (R, R0, eng.last_kernel_name())
        assert eng.last_rotation_count() == R and got.shape == (R, K + 1, N)
        bad = np.nonzero((got != want5[tile]).reshape(R, -1).any(axis=1))[0]
        assert bad.size == 0, (R, R0, f"{bad.size} rows differ, the first is row {bad[:1]}")
    ext4 = _extractions(ref, want5, 4)
    got1 = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], n_out=4, out_form=1)
    assert eng.last_kernel_name() == _name(l, True) and np.array_equal(got1, ext4[tile]), "R0 + 1, out_form 1, n_out 4"
    ks1 = ks_ref(ks_schoolbook(c["ck"].params, c["ck"].keyswitch_key), _extractions(ref, want5, 1))
    got2 = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], n_out=1, out_form=2)
    assert eng.last_kernel_name() == _name(l, True) and np.array_equal(got2, ks1[tile]), "R0 + 1, out_form 2, n_out 1"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4, 8])
def test_gpu_step_counts_one_four_eight(tfhe, n):
    """n = 1: the key prefetch of a one-step loop; 4 and 8: the loop ends exactly at the end of a lockstep period."""
    l, beta = 2, 10
    c = _case(tfhe, l, beta, n)
    eng, acc, x, ref = c["eng"], c["acc"], c["x"], c["ref"]
    want = c["want"].astype(np.int32)
    ext4 = _extractions(ref, want, 4)
    try:
        for rw in (1, 4):
            eng.set_option("v3_rw", rw)
            got0 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, out_form=0)
            assert eng.last_kernel_name() == _name(l, rw == 4), eng.last_kernel_name()
            assert np.array_equal(got0, want), ("out_form 0", n, rw)
            got1 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=4, out_form=1)
            assert np.array_equal(got1, ext4), ("out_form 1", n, rw)
    finally:
        eng.set_option("v3_rw", 0)


@pytest.mark.gpu
def test_gpu_extractions_of_the_batch_call(tfhe):
    """n_out 2, 8, 16, 32 (out_form 1) and 2, 8 (out_form 2) against extract_at and ks_ref."""
    from leveled_ref import ks_ref, ks_schoolbook
    l, beta, n = 3, 8, 5
    c = _case(tfhe, l, beta, n)
    eng, acc, x, ref = c["eng"], c["acc"], c["x"], c["ref"]
    sbk = ks_schoolbook(c["ck"].params, c["ck"].keyswitch_key)
    try:
        for rw in (1, 4):
            eng.set_option("v3_rw", rw)
            for n_out in (2, 8, 16, 32):
                ext = _extractions(ref, c["want"], n_out)
                got1 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=n_out, out_form=1)
                assert got1.shape == (B_ROWS, n_out, N + 1) and np.array_equal(got1, ext), ("out_form 1", n_out, rw)
                if n_out <= 8:
                    got2 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=n_out, out_form=2)
                    assert got2.shape == (B_ROWS, n_out, n + 1) and np.array_equal(got2, ks_ref(sbk, ext)), ("out_form 2", n_out, rw)
    finally:
        eng.set_option("v3_rw", 0)


@pytest.mark.gpu
def test_gpu_extractions_of_the_level_call(tfhe):
    """n_out 2, 8, 32 with out_form 2 into permuted wires: the wire table after the call, every wire."""
    from leveled_ref import ks_ref, ks_schoolbook
    l, beta, n = 3, 8, 5
    c = _case(tfhe, l, beta, n)
    eng, rng, ref = c["eng"], c["rng"], c["ref"]
    W = IN_WIRES + 3 * 32 + 5
    full, allw = _tables(c, n, W)
    sbk = ks_schoolbook(c["ck"].params, c["ck"].keyswitch_key)
    acc_slot, start, wire, coef = np.array([2, 0, 2], np.int32), [0, 1, 1, 3], [1, 2, 3], [1, -3, 2**31 - 1]
    cst = _words(rng, 3)
    want = _level_want(c, full, allw, acc_slot, start, wire, coef, cst)
    try:
        for n_out in (2, 8, 32):
            out_wires = (IN_WIRES + rng.permutation(W - IN_WIRES)[:3 * n_out]).astype(np.int32)
            assert (np.diff(out_wires) < 0).any()
            eng.bootstrap_acc_level(acc_slot, start, wire, coef, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
            want_w = allw.copy()
            want_w[out_wires] = ks_ref(sbk, _extractions(ref, want, n_out)).reshape(3 * n_out, n + 1)
            assert np.array_equal(eng.wires_download(0, W), want_w), n_out
            assert np.array_equal(eng.tlwe_download(0, SLOTS), full)
            eng.wires_upload(0, allw)
    finally:
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 9])
def test_gpu_level_with_padding_waves_and_permuted_out_slot(tfhe, B):
    """v3_rw 4 with B = 5 and 9: two and three workgroups, three padding waves each time, which recompute row B - 1 and store nothing;
    out_form 0 into a permuted out_slot; the slots nobody writes stay as they were (the whole table is compared)."""
    l, beta, n = 4, 6, 5
    c = _case(tfhe, l, beta, n)
    eng, rng = c["eng"], c["rng"]
    full, allw = _tables(c, n)
    out_slot = np.random.default_rng(B).permutation(np.arange(3, 3 + B + 2))[:B].astype(np.int32)      # slots 0 ... 2: the accumulators; two of the range stay
    assert (np.diff(out_slot) < 0).any()
    acc_slot = np.array([2, 0, 1, 2, 0, 0, 1, 2, 1][:B], np.int32)
    start = np.arange(B + 1, dtype=np.int32)
    wire = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9][:B], np.int32)                      # one term per row: the case's rows, then arbitrary ones
    coef = np.array([1, 1, 1, 1, 1, -3, 2**31 - 1, -2**31, 7][:B], np.int32)
    cst = _words(rng, B)
    want = full.copy()
    want[out_slot] = _level_want(c, full, allw, acc_slot, start, wire, coef, cst)
    try:
        eng.set_option("v3_rw", 4)
        eng.bootstrap_acc_level(acc_slot, start, wire, coef, cst=cst, out_form=0, out_slot=out_slot)
        assert eng.last_kernel_name() == _name(l, True) and eng.last_rotation_count() == B
        got = eng.tlwe_download(0, SLOTS)
        bad = np.nonzero((got != want).reshape(SLOTS, -1).any(axis=1))[0]
        assert bad.size == 0, (f"slots {bad.tolist()} differ", out_slot.tolist())
        assert np.array_equal(eng.wires_download(0, WIRES), allw)
    finally:
        eng.set_option("v3_rw", 0)
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


@pytest.mark.gpu
def test_gpu_level_without_a_wire_table_runs(tfhe):
    """A context with the bootstrapping key and a TLWE table, no wire table and no keyswitch key: a call without terms and with out_form 0
    reads and writes no wire and succeeds; its rows are (0, ..., 0, cst[g]), all zero with cst NULL."""
    l, beta, n = 2, 10, 5
    c = _case(tfhe, l, beta, n)
    ck, rng = c["ck"], c["rng"]
    raw = tfhe.Engine(ck.params)
    try:
        raw.load_bootstrap_key(ck.bootstrap_key)
        full, _ = _tables(c, n, 0, eng=raw)
        acc_slot, out_slot, start = np.array([1, 0, 1, 2], np.int32), np.array([9, 4, 12, 5], np.int32), np.zeros(5, np.int32)
        cst_set = _words(rng, 4)
        cst_set[0] = _word(N + 3, -7)
        for cst in (cst_set, None):
            raw.bootstrap_acc_level(acc_slot, start, [], [], cst=cst, out_form=0, out_slot=out_slot)
            assert raw.last_kernel_name() == _name(l, False) and raw.last_rotation_count() == 4
            rows = np.zeros((4, n + 1), np.int32)
            if cst is not None:
                rows[:, n] = cst
            want = full.copy()
            want[out_slot] = np.stack([c["ref"].rotate_lwe(full[a], rows[g]) for g, a in enumerate(acc_slot)]).astype(np.int32)
            assert (cst is None) == np.array_equal(want[out_slot], full[acc_slot])                 # (all exponents 0: a copy)
            assert np.array_equal(raw.tlwe_download(0, SLOTS), want), ("cst NULL" if cst is None else "cst set")
            raw.tlwe_upload(0, full)
    finally:
        raw.close()


@pytest.mark.gpu
def test_gpu_workspaces_grow_behind_a_queued_gate_level(tfhe, orc):
    """A fresh context: an asynchronous gates_level of 8 gates sizes bara, ext and map for 8 rotations; the bootstrap_acc_level right behind
    it needs 20 rows and 40 extractions, so all three are replaced while the gate level may still be running.  The gates' wires are
    wire_table_model's arithmetic, the rotation's the schoolbook's; its rows read the gates' outputs."""
    import wire_table_model as M
    from leveled_ref import ks_ref, ks_schoolbook
    l, beta, n = 2, 10, 9
    c = _case(tfhe, l, beta, n)
    ck, rng, ref = c["ck"], c["rng"], c["ref"]
    p = ck.params
    oracle = orc.Oracle(p.lwe_size, N, K, l, beta, p.ks_decomp_length, p.ks_log2_base)
    oracle.load_bootstrap_key(ck.bootstrap_key)
    oracle.load_keyswitch_key(ck.keyswitch_key)
    arith = M.single_key_arith(oracle, None)
    B, n_out, W = 20, 2, 72
    raw = tfhe.Engine(p)
    try:
        raw.load_bootstrap_key(ck.bootstrap_key)
        raw.load_keyswitch_key(ck.keyswitch_key)
        full, allw = _tables(c, n, W, eng=raw)
        ops = np.array([M.OPS[nm] for nm in ("NAND", "XOR", "MUX", "OR", "ANDNY", "NOT", "XNOR", "AND")], np.uint8)      # 8 rotations (a MUX is two)
        a, b, z = np.arange(1, 9, dtype=np.int32), np.arange(2, 10, dtype=np.int32), np.arange(3, 11, dtype=np.int32)
        gate_out = np.arange(12, 20, dtype=np.int32)
        assert M.rotations(ops) == 8
        acc_slot = (np.arange(B) % 3).astype(np.int32)
        start = np.arange(B + 1, dtype=np.int32)
        wire = np.concatenate([gate_out, gate_out, np.arange(1, 5)]).astype(np.int32)                # every row reads a wire, 16 of them a gate's output
        coef = np.where(np.arange(B) % 3 == 0, 1, _words(rng, B)).astype(np.int32)
        cst = _words(rng, B)
        out_wires = (20 + rng.permutation(W - 20)[:B * n_out]).astype(np.int32)
        raw.gates_level(ops, a, b, z, gate_out)
        raw.bootstrap_acc_level(acc_slot, start, wire, coef, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
        assert raw.last_kernel_name() == _name(l, False) and raw.last_rotation_count() == B
        got = raw.wires_download(0, W)
        want = allw.copy()
        want[gate_out] = arith.gates(ops, allw[a], allw[b], allw[z])
        assert np.array_equal(got[gate_out], want[gate_out]), "the gate level's outputs"
        accs = _level_want(c, full, want, acc_slot, start, wire, coef, cst)
        want[out_wires] = ks_ref(ks_schoolbook(p, ck.keyswitch_key), _extractions(ref, accs, n_out)).reshape(B * n_out, n + 1)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"wires {bad.tolist()} differ"
        assert np.array_equal(raw.tlwe_download(0, SLOTS), full)
    finally:
        raw.close()


# ---- 4. GPU: refusals ---------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mem_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    return free.value


class _Batch:
    """A valid raw call of tfhe_bootstrap_acc_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, acc, rows):
        self.eng = eng
        self.args = dict(acc=acc, T=acc.shape[0], acc_index=np.zeros(rows.shape[0], np.int32), rows=rows, n_out=1, out_form=0,
                         out=np.empty((rows.shape[0], 32, N + 1), np.int32), B=rows.shape[0])

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        rc = e._lib.tfhe_bootstrap_acc_batch(e._h, _ptr(a["acc"]), a["T"], _ptr(a["acc_index"]), _ptr(a["rows"]), a["n_out"], a["out_form"], _ptr(a["out"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode()


class _Level:
    """The same for tfhe_bootstrap_acc_level."""

    def __init__(self, eng):
        self.eng = eng
        self.args = dict(acc_slot=[1, 1, 2], term_start=[0, 0, 1, 3], term_wire=[4, 5, 4], term_coef=[1, -2, 3], cst=[5, 6, 7], n_out=1, out_form=0,
                         out_slot=[8, 9, 10], out_wires=None, B=3)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        arr = {key: None if a[key] is None else np.asarray(a[key], np.int32) for key in ("acc_slot", "term_start", "term_wire", "term_coef", "cst", "out_slot", "out_wires")}
        rc = e._lib.tfhe_bootstrap_acc_level(e._h, _ptr(arr["acc_slot"]), _ptr(arr["term_start"]), _ptr(arr["term_wire"]), _ptr(arr["term_coef"]), _ptr(arr["cst"]),
                                             a["n_out"], a["out_form"], _ptr(arr["out_slot"]), _ptr(arr["out_wires"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode()


@pytest.mark.gpu
def test_gpu_refusals_change_nothing_and_the_next_call_is_right(tfhe):
    from tfhe_jl_amd import leveled
    l, beta, n = 2, 10, 5
    c = _case(tfhe, l, beta, n)
    eng, ck, acc, x, sels = c["eng"], c["ck"], c["acc"], c["x"], c["sels"]
    full, allw = _tables(c, n)
    bat, lvl = _Batch(eng, acc, x), _Level(eng)
    a = lvl.args
    want_bat = eng.blind_rotate(acc, x, in_form=0, out_form=0)
    want_lvl = eng.blind_rotate(full, form_rows(allw, a["term_start"], a["term_wire"], a["term_coef"], a["cst"]), acc_index=a["acc_slot"], in_form=0, out_form=0)
    probe = np.ascontiguousarray(np.repeat(acc[:1], n, axis=0))
    every = np.arange(n, dtype=np.int32)
    selectors_before = eng.extern_mul(probe, every)

    def unchanged_and_still_right():
        assert np.array_equal(eng.tlwe_download(0, SLOTS), full) and np.array_equal(eng.wires_download(0, WIRES), allw)
        assert np.array_equal(eng.bootstrap_acc(acc, x, out_form=0), want_bat)
        assert lvl()[0] == OK and np.array_equal(eng.tlwe_download(8, 3), want_lvl)
        eng.tlwe_upload(8, full[8:11])

    try:
        unchanged_and_still_right()
        assert bat(B=0)[0] == OK and lvl(B=0)[0] == OK
        # TFHE_ERR_INVALID_ARG, as the existing calls
        for over in (dict(B=-1), dict(acc=None), dict(rows=None), dict(out=None), dict(T=0), dict(out_form=3), dict(out_form=-1), dict(n_out=0), dict(n_out=3, out_form=1),
                     dict(n_out=64, out_form=1), dict(n_out=4), dict(acc_index=np.array([0, 3, 0, 0, 0], np.int32)), dict(acc_index=np.array([0, 0, -1, 0, 0], np.int32))):
            rc, msg = bat(**over)
            assert rc == INVALID and msg.startswith("bootstrap_acc_batch:"), (over, rc, msg)
        assert "acc_index[1] = 3" in bat(acc_index=np.array([0, 3, 0, 0, 0], np.int32))[1]
        for over, offender in ((dict(B=-1), "B = -1"), (dict(acc_slot=None), "NULL"), (dict(out_slot=[8, 9, 9]), "slot 9 written twice"),
                               (dict(out_slot=[8, 9, 2]), "acc_slot[2] = 2 is an output slot"), (dict(out_slot=[8, 9, SLOTS]), f"out_slot[2] = {SLOTS}"),
                               (dict(acc_slot=[1, SLOTS, 2]), f"acc_slot[1] = {SLOTS}"), (dict(term_wire=[4, WIRES, 4]), f"reads wire {WIRES}"),
                               (dict(term_start=[0, 2, 1, 3]), "term_start decreases"), (dict(n_out=2), "n_out = 2"), (dict(out_form=1), "out_form = 1"),
                               (dict(out_form=2), "NULL out_wires"), (dict(out_form=2, out_wires=[20, 21, 21]), "wire 21 written twice"),
                               (dict(out_form=2, out_wires=[20, 21, 5]), "reads wire 5, which the same call writes"), (dict(out_slot=None), "NULL out_slot")):
            rc, msg = lvl(**over)
            assert rc == INVALID and msg.startswith("bootstrap_acc_level:") and offender in msg, (over, rc, msg)
            unchanged_and_still_right()
        # TFHE_ERR_STATE: measure_margin, before the arguments are looked at
        eng.set_option("measure_margin", 1)
        for rc, msg in (bat(T=0), lvl(out_slot=[8, 9, 9])):
            assert rc == STATE and "measure_margin" in msg, (rc, msg)
        eng.set_option("measure_margin", 0)
        unchanged_and_still_right()
        # a multi-device context
        multi = ck.engine([0, 0])
        for rc, msg in (bat(eng=multi), lvl(eng=multi)):
            assert rc == STATE and "multi-device" in msg, (rc, msg)
        assert multi.get_option("bootstrap_acc") == 0
        # TFHE_ERR_NO_KEY: no bootstrapping key; out_form 2 without the keyswitch key; forms 0 and 1 do not need it
        raw = tfhe.Engine(ck.params)
        assert raw.get_option("bootstrap_acc") == 1
        rc, msg = bat(eng=raw)
        assert rc == NO_KEY and "bootstrapping key" in msg, (rc, msg)
        rc, msg = lvl(eng=raw)
        assert rc == STATE and "no TLWE table" in msg, (rc, msg)
        raw.tlwe_alloc(SLOTS)
        raw.tlwe_upload(0, full)
        rc, msg = lvl(eng=raw)
        assert rc == STATE and "no wire table" in msg, (rc, msg)               # the call has terms
        rc, msg = lvl(eng=raw, term_start=[0, 0, 0, 0])
        assert rc == NO_KEY and "bootstrapping key" in msg, (rc, msg)
        raw.load_bootstrap_key(ck.bootstrap_key)
        raw.wires_alloc(WIRES)
        raw.wires_upload(0, allw)
        for rc, msg in (bat(eng=raw, out_form=2), lvl(eng=raw, out_form=2, out_wires=[20, 21, 22])):
            assert rc == NO_KEY and "keyswitch" in msg, (rc, msg)
        assert np.array_equal(raw.tlwe_download(0, SLOTS), full) and np.array_equal(raw.wires_download(0, WIRES), allw)
        assert np.array_equal(raw.bootstrap_acc(acc, x, out_form=0), want_bat)                       # ... without any selector set
        assert lvl(eng=raw)[0] == OK and np.array_equal(raw.tlwe_download(8, 3), want_lvl)
        raw.close()
        # TFHE_ERR_NOMEM: a batch whose workspaces cannot fit, refused before anything is allocated, and an injected allocation failure
        before = _mem_free()
        rc, msg = bat(acc_index=None, B=2**31 - 1)
        assert rc == NOMEM and "MB" in msg, (rc, msg)
        assert _mem_free() == before
        unchanged_and_still_right()
        lib = eng._lib
        for call in (bat, lvl):
            assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
            rc, msg = call()
            lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
            assert rc == NOMEM and "memory" in msg, (rc, msg)
            unchanged_and_still_right()
        # the loaded selector set is what it was: one external product per selector
        assert np.array_equal(eng.extern_mul(probe, every), selectors_before)
    finally:
        eng.set_option("measure_margin", 0)
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


@pytest.mark.gpu
def test_gpu_shapes_the_kernel_does_not_serve_are_refused(tfhe):
    """N != 1024, k != 1, and a key in the any-N kernels' layout (br_anyn): TFHE_ERR_STATE naming the shape and tfhe_blind_rotate_batch,
    option bootstrap_acc 0, and tuned=True raises ValueError."""
    from tfhe_jl_amd import leveled, lut
    acc = np.zeros((1, 2, N), np.int32)
    for Ns, ks in ((64, 1), (1024, 2), (2048, 1), (512, 1)):
        raw = tfhe.Engine(_params(tfhe, Ns, ks, 3, 8))
        assert raw.get_option("bootstrap_acc") == 0
        a = np.zeros((1, ks + 1, Ns), np.int32)
        x = np.zeros((1, raw.n + 1), np.int32)
        rc = raw._lib.tfhe_bootstrap_acc_batch(raw._h, _ptr(a), 1, None, _ptr(x), 1, 0, _ptr(np.empty_like(a)), 1)
        msg = raw._lib.tfhe_last_error(raw._h).decode()
        assert rc == STATE and f"N = {Ns}, k = {ks}" in msg and "tfhe_blind_rotate_batch" in msg, (rc, msg)
        rc = raw._lib.tfhe_bootstrap_acc_level(raw._h, _ptr(np.zeros(1, np.int32)), _ptr(np.zeros(2, np.int32)), None, None, None, 1, 0, _ptr(np.ones(1, np.int32)), None, 1)
        assert rc == STATE, raw._lib.tfhe_last_error(raw._h).decode()          # (no TLWE table comes first)
        raw.tlwe_alloc(2)
        rc = raw._lib.tfhe_bootstrap_acc_level(raw._h, _ptr(np.zeros(1, np.int32)), _ptr(np.zeros(2, np.int32)), None, None, None, 1, 0, _ptr(np.ones(1, np.int32)), None, 1)
        msg = raw._lib.tfhe_last_error(raw._h).decode()
        assert rc == STATE and f"N = {Ns}, k = {ks}" in msg and "tfhe_blind_rotate_batch" in msg, (rc, msg)
        raw.close()
    p = _params(tfhe, N, K, 2, 10, n=5)
    raw = tfhe.Engine(p)
    assert raw.get_option("bootstrap_acc") == 1
    raw.set_option("br_anyn", 1)
    assert raw.get_option("bootstrap_acc") == 0
    x = np.zeros((1, 6), np.int32)
    rc = raw._lib.tfhe_bootstrap_acc_batch(raw._h, _ptr(acc), 1, None, _ptr(x), 1, 0, _ptr(np.empty_like(acc)), 1)
    msg = raw._lib.tfhe_last_error(raw._h).decode()
    assert rc == STATE and "br_anyn" in msg and "tfhe_blind_rotate_batch" in msg, (rc, msg)
    raw.close()
    # tuned=True on a shape with option 0
    ps = _params(tfhe, 64, 1, 3, 8, bs_noise=1e-7)
    rng = np.random.default_rng(3)
    sk, ck = tfhe.make_key_pair(rng, ps)
    t = leveled.private_lut_encrypt(rng, sk, lambda m: m, 4)
    xs = lut.lut_encrypt(rng, sk, [1, 2], 4)
    with pytest.raises(ValueError, match="bootstrap_acc"):
        leveled.blind_rotate_lookup(ck, t, xs, tuned=True)
    with pytest.raises(ValueError, match="bootstrap_acc"):
        leveled.pbs_to_tlwe(ck, xs, lambda m: m, 4, tuned=True)
    assert list(lut.lut_decrypt(sk, leveled.blind_rotate_lookup(ck, t, xs), 4)) == [1, 2]            # the default keeps today's calls
    ck.close()


@pytest.mark.gpu
def test_gpu_multikey_context_refuses_bootstrap_acc(tfhe):
    from test_independent import _mk_setup
    p, sks, ck, xs, ys, want = _mk_setup(tfhe, 2, 4, 7, 3, 405)
    eng = ck.engine(0)
    assert eng.get_option("bootstrap_acc") == 0
    with pytest.raises(tfhe.EngineError) as e:
        eng.bootstrap_acc(np.zeros((1, 2, 1024), np.int32), np.zeros((1, eng.n + 1), np.int32), out_form=0)
    assert e.value.code == STATE and "multi-key" in str(e.value)
    with pytest.raises(tfhe.EngineError) as e:
        eng.bootstrap_acc_level([0], [0, 0], [], [], out_form=0, out_slot=[1])
    assert e.value.code == STATE and "multi-key" in str(e.value)
    assert np.array_equal(eng.mk_gate_nand(xs, ys), want)            # the context still runs its own gates
    ck.close()


# ---- 5. GPU: the 80-bit set at full size --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_private_table_full_size_tuned_equals_default(tfhe, keys80):
    """8 rows of a private p = q = 8 table at tfhe_parameters_80: tuned=True returns Engine.blind_rotate's words, and they all decrypt
    (the condition tests/test_blind_rotate.py's full-size test meets with the same words); the two-stage lookup and pbs_to_tlwe likewise."""
    from tfhe_jl_amd import leveled, lut
    Kp = keys80
    prm = Kp.params
    k, l = prm.tlwe_mask_size, prm.bs_decomp_length
    assert prm.tlwe_polynomial_degree == N and k == 1
    rng = np.random.default_rng(8081)
    f = [int(v) for v in rng.integers(0, 8, 8)]
    m = np.arange(8)
    acc = leveled.private_lut_encrypt(rng, Kp.sk, lambda v: f[v], 8)
    x = lut.lut_encrypt(rng, Kp.sk, m, 8)
    want = leveled.blind_rotate_lookup(Kp.ck, acc, x)
    got = leveled.blind_rotate_lookup(Kp.ck, acc, x, tuned=True)
    assert Kp.ck.engine(0).last_kernel_name() == "blind_rotate_kernel_v3_acc<2,8,tw2reg>"
    assert np.array_equal(got.data, want.data)
    assert list(lut.lut_decrypt(Kp.sk, got, 8)) == [f[v] for v in m]
    table = [int(v) for v in rng.integers(0, 8, 32)]
    tables = np.concatenate([leveled.tlwe_trivial(lut.make_test_vector(lambda v, h=h: table[8 * h + v], 8, N), k) for h in range(4)])
    addr = rng.integers(0, 32, 4)
    hbits = ((addr >> 3)[:, None] >> np.arange(2)[None, :]) & 1
    tg = leveled.tgsw_encrypt_bits(rng, Kp.sk, hbits.reshape(-1)).reshape(4, 2, l, k + 1, k + 1, N)
    low = lut.lut_encrypt(rng, Kp.sk, addr & 7, 8)
    got = leveled.two_stage_lookup(Kp.ck, tables, tg, low, 8, tuned=True)
    assert np.array_equal(got.data, leveled.two_stage_lookup(Kp.ck, tables, tg, low, 8).data)
    assert list(lut.lut_decrypt(Kp.sk, got, 8)) == [table[a] for a in addr]
    t = leveled.pbs_to_tlwe(Kp.ck, x, lambda v: f[v], 8, tuned=True)
    assert np.array_equal(t, leveled.pbs_to_tlwe(Kp.ck, x, lambda v: f[v], 8))
