"""Private-table rotation on the multi-wave gate kernels (option acc_dispatch = 1 of tfhe_bootstrap_acc_batch / tfhe_bootstrap_acc_level:
blind_rotate_kernel_h2_acc, blind_rotate_kernel_w2_acc, blind_rotate_kernel_v3_acc and the split of a large call, chosen by batch size as
a gate batch's kernel is) and Circuit.blind_rotate(..., tuned=True), against tests/test_bootstrap_acc.py's references: the integer
schoolbook's final accumulators of `_case` (T = 3 accumulators, one a real encryption so that the mask polynomial is live from step 0,
B = 5 rows with the planted exponents), `extract_at` and leveled_ref.ks_ref behind them, and Engine.blind_rotate_level for the tables.
Every comparison is word for word.

The kernels exist at N = 1024, k = 1.  (l, beta) = (2, 10), (3, 8), (4, 6): the L = 2 and L = 3 instantiations of both families and the
run-time-l one of the two-wave kernel (the 4 l-wave kernel has none: l = 4 falls through to it).  n = 5 and 9 are odd step counts, n = 8
an even one: the 4 l-wave kernel keeps its rotated differences in two buffers by step parity, and the last step leaves them in either.
B = 5 with two rows per workgroup is three workgroups, the last with a padding rotation; B = 1 one real and one padding.  The thresholds
between the families and the seam of a split call are computed from the device's compute-unit count."""
import contextlib
import functools
import importlib.util
import os

import numpy as np
import pytest

from test_bootstrap_acc import (ACC_INDEX, B_ROWS, INVALID, K, N, OK, SHAPES, STATE, STEPS, _Batch, _case, _cu_count, _extractions, _Level, _name, _ptr,
                                _tables)
from test_leveled import _params, _words
from test_tlwe_levels import ACC_SLOT, IN_WIRES, OUT_SLOT, SLOTS, TERM_COEF, TERM_START, TERM_WIRE, WIRES, form_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the options that force each family on a small batch under acc_dispatch 1
FAMILIES = {"default": {}, "w2_rw1": {"br_tiny": -1, "w2_rw": 1}, "w2_rw2": {"br_tiny": -1, "w2_rw": 2}, "v3": {"br_tiny": -1, "br_small": -1}}


@contextlib.contextmanager
def _options(eng, **opts):
    before = {name: eng.get_option(name) for name in opts}
    try:
        for name, value in opts.items():
            eng.set_option(name, value)
        yield
    finally:
        for name, value in before.items():
            eng.set_option(name, value)


def _family_name(l, family, pairs_by_default=False):
    """tfhe_last_kernel_name of a batch that the family's options send to one launch (name_kernel's style)."""
    if family == "v3":
        return _name(l, False)
    if family == "default" and l in (2, 3):
        return f"blind_rotate_kernel_h2_acc<{l}>"
    rw2 = family == "w2_rw2" or (family == "default" and pairs_by_default)
    rest = ",rw2" if rw2 else ""
    return f"blind_rotate_kernel_w2_acc<{l}{rest}>" if l in (2, 3) else f"blind_rotate_kernel_w2_acc<0{rest}>(l={l})"


def _w2_pairs(R, cus):
    """Option w2_rw 0: two rows per workgroup from more than one row up to one pair per compute unit, and at (nearly) two pairs."""
    cus2 = 2 * cus
    return (cus2 // 2 < R <= cus2) or R > 2 * cus2 - cus2 // 8


@functools.lru_cache(maxsize=None)
def _refs(tfhe, l, beta, n):
    """The schoolbook's extractions and their keyswitched words for a case, computed once."""
    from leveled_ref import ks_ref, ks_schoolbook
    c = _case(tfhe, l, beta, n)
    sbk = ks_schoolbook(c["ck"].params, c["ck"].keyswitch_key)
    ext = {n_out: _extractions(c["ref"], c["want"], n_out) for n_out in (1, 4, 32)}
    return ext, {n_out: ks_ref(sbk, ext[n_out]) for n_out in (1, 4)}


def _first_bad_row(got, want):
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
    return f"{bad.size} rows differ, the first is row {bad[:1]}" if bad.size else ""


# ---- CPU: the planner -----------------------------------------------------------------------------------------------------------------
def _two_rotations(tfhe, tuned_first, tuned_second):
    c = tfhe.Circuit()
    a, b = c.inputs(2)
    tl = c.tlwe_inputs(2)
    r0 = c.blind_rotate(tl[0], [a], tuned=tuned_first)
    r1 = c.blind_rotate(tl[1], [(b, 3)], const=7, tuned=tuned_second)
    c.set_outputs([r0, r1])
    return c


def test_planner_groups_tuned_rotations_apart(tfhe):
    c = _two_rotations(tfhe, True, False)
    assert c._rotation_tuned == [True, False] and [len(r) for r in c._rotations] == [9, 9]
    plan = c.level_plan(N)
    assert len(plan) == 1 and len(plan[0]["blind_rotate"]) == 1 and len(plan[0]["bootstrap_acc"]) == 1
    acc, start, wire, coef, cst, sel, n_out, form, out_slot, out_wires = plan[0]["bootstrap_acc"][0]
    assert acc.tolist() == [0] and start.tolist() == [0, 1] and wire.tolist() == [0] and coef.tolist() == [1] and cst.tolist() == [0]
    assert sel is None and n_out == 1 and form == 2 and out_slot is None and out_wires.tolist() == [2]
    acc, start, wire, coef, cst, sel, n_out, form, out_slot, out_wires = plan[0]["blind_rotate"][0]
    assert acc.tolist() == [1] and wire.tolist() == [1] and coef.tolist() == [3] and cst.tolist() == [7] and sel is None and out_wires.tolist() == [3]
    # two tuned rotations of one (n_out, out) share a call
    both = _two_rotations(tfhe, True, True).level_plan(N)[0]
    assert both["blind_rotate"] == [] and len(both["bootstrap_acc"]) == 1 and both["bootstrap_acc"][0][0].tolist() == [0, 1]


def test_tuned_with_a_selector_list_raises(tfhe):
    c = tfhe.Circuit()
    a = c.input()
    tl = c.tlwe_inputs(1)
    with pytest.raises(ValueError, match="gates' key"):
        c.blind_rotate(tl[0], [a], sel=[0, 1, 2], tuned=True)
    assert c._rotations == [] and c._rotation_tuned == [] and c.num_wires == 1 and c.num_tlwe == 1      # nothing was recorded


def test_default_circuits_plan_what_they_planned_before(tfhe):
    plan = _two_rotations(tfhe, False, False).level_plan(N)
    assert sorted(plan[0]) == ["blind_rotate", "gates", "linear", "lut", "rot_net"]
    assert len(plan[0]["blind_rotate"]) == 1 and plan[0]["blind_rotate"][0][0].tolist() == [0, 1] and len(plan[0]["blind_rotate"][0]) == 10
    plain = tfhe.Circuit()
    x, y = plain.inputs(2)
    plain.set_outputs([plain.nand(x, y)])
    assert sorted(plain.level_plan(N)[0]) == ["gates", "linear", "lut"]


# ---- 1. GPU: words, per family --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("l,beta", SHAPES)
def test_gpu_words_per_family(tfhe, l, beta, n, family):
    c = _case(tfhe, l, beta, n)
    eng, acc, x = c["eng"], c["acc"], c["x"]
    want = c["want"].astype(np.int32)
    want_ext, want_ks = _refs(tfhe, l, beta, n)
    name = _family_name(l, family)
    assert eng.get_option("bootstrap_acc") == 1 and eng.get_option("acc_dispatch") == 0
    with _options(eng, acc_dispatch=1, **FAMILIES[family]):
        got0 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, out_form=0)
        assert eng.last_kernel_name() == name, eng.last_kernel_name()
        assert eng.last_rotation_count() == B_ROWS and eng.last_timing_ms(0) > 0
        assert got0.shape == (B_ROWS, K + 1, N) and np.array_equal(got0, want), ("out_form 0", _first_bad_row(got0, want))
        got1, got2 = {}, {}
        for n_out in (1, 4, 32):
            got1[n_out] = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=n_out, out_form=1)
            assert got1[n_out].shape == (B_ROWS, n_out, N + 1) and np.array_equal(got1[n_out], want_ext[n_out]), ("out_form 1", n_out)
        for n_out in (1, 4):
            got2[n_out] = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=n_out, out_form=2)
            assert eng.last_kernel_name() == name and eng.last_timing_ms(1) > 0
            assert got2[n_out].shape == (B_ROWS, n_out, n + 1) and np.array_equal(got2[n_out], want_ks[n_out]), ("out_form 2", n_out)
        # NULL acc_index = accumulator 0 for every row: rows 1 and 4 of the calls above; B = 1: row 2 alone
        two = eng.bootstrap_acc(acc, x[[1, 4]], out_form=0)
        assert eng.last_kernel_name() == name and np.array_equal(two, want[[1, 4]]), "NULL acc_index"
        one = eng.bootstrap_acc(acc[2:], x[2:3], n_out=4, out_form=1)
        assert eng.last_kernel_name() == name and eng.last_rotation_count() == 1 and np.array_equal(one, want_ext[4][2:3]), "B = 1"
        # the same words under acc_dispatch 0, on the one-wave kernel
        eng.set_option("acc_dispatch", 0)
        assert np.array_equal(eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, out_form=0), got0)
        assert eng.last_kernel_name() == _name(l, False)
        assert np.array_equal(eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=32, out_form=1), got1[32])
        assert np.array_equal(eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=4, out_form=2), got2[4])
    assert eng.get_option("acc_dispatch") == 0


@pytest.mark.gpu
def test_gpu_h2_even_step_count(tfhe):
    """n = 8: the last step leaves the rotated differences in the other buffer than an odd count does."""
    l, beta, n = 2, 10, 8
    c = _case(tfhe, l, beta, n)
    eng, acc, x = c["eng"], c["acc"], c["x"]
    want = c["want"].astype(np.int32)
    with _options(eng, acc_dispatch=1):
        got0 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, out_form=0)
        assert eng.last_kernel_name() == "blind_rotate_kernel_h2_acc<2>", eng.last_kernel_name()
        assert np.array_equal(got0, want), _first_bad_row(got0, want)
        got1 = eng.bootstrap_acc(acc, x, acc_index=ACC_INDEX, n_out=4, out_form=1)
        assert np.array_equal(got1, _extractions(c["ref"], want, 4))


# ---- 2. GPU: the level form -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family", ["default", "w2_rw2"])
def test_gpu_level_form_equals_blind_rotate_level(tfhe, family):
    """tests/test_bootstrap_acc.py's level rows (0, 1 and 3 terms, coefficients that wrap, cst set and NULL, a repeated acc_slot), out_form 0
    into a permuted out_slot and out_form 2 into permuted wires with n_out 1 and 4: the tables after the call are those after
    Engine.blind_rotate_level, the other table is unchanged; and a call queued behind an asynchronous gates_level reads what it wrote."""
    l, beta, n = 2, 10, 9
    c = _case(tfhe, l, beta, n)
    eng, rng = c["eng"], c["rng"]
    full, allw = _tables(c, n)
    B = len(ACC_SLOT)
    name = _family_name(l, family)
    assert (np.diff(OUT_SLOT) < 0).any()
    cst_set = _words(rng, B)
    cst_set[5] = 0
    try:
        with _options(eng, acc_dispatch=1, **FAMILIES[family]):
            for cst in (cst_set, None):
                eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, out_form=0, out_slot=OUT_SLOT)
                want = eng.tlwe_download(0, SLOTS)
                assert not np.array_equal(want, full)
                eng.tlwe_upload(0, full)
                eng.bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, out_form=0, out_slot=OUT_SLOT)
                assert eng.last_kernel_name() == name and eng.last_rotation_count() == B and eng.last_timing_ms(0) > 0
                assert np.array_equal(eng.tlwe_download(0, SLOTS), want), ("out_form 0", cst is None)
                assert np.array_equal(eng.wires_download(0, WIRES), allw)
                eng.tlwe_upload(0, full)
                for n_out in (1, 4):
                    out_wires = (IN_WIRES + rng.permutation(WIRES - IN_WIRES)[:B * n_out]).astype(np.int32)
                    eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
                    want_w = eng.wires_download(0, WIRES)
                    assert not np.array_equal(want_w, allw)
                    eng.wires_upload(0, allw)
                    eng.bootstrap_acc_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, n_out=n_out, out_form=2, out_wires=out_wires)
                    assert eng.last_kernel_name() == name and eng.last_timing_ms(1) > 0
                    assert np.array_equal(eng.wires_download(0, WIRES), want_w), ("out_form 2", n_out, cst is None)
                    assert np.array_equal(eng.tlwe_download(0, SLOTS), full)
                    eng.wires_upload(0, allw)
            # queued behind an asynchronous level: the NAND's output wire is the rotating row
            eng.gates_level(np.zeros(1, np.uint8), [20], [21], None, [40])
            eng.bootstrap_acc_level([0], [0, 1], [40], [1], out_form=2, out_wires=[41])
            assert eng.last_kernel_name() == name
            row = eng.wires_gather([40])
            assert not np.array_equal(row[0], allw[40])
            eng.set_option("acc_dispatch", 0)
            assert np.array_equal(eng.wires_gather([41])[0], eng.bootstrap_acc(full, row, acc_index=[0], out_form=2)[0, 0])
    finally:
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


# ---- 3. GPU: the thresholds between the families --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_thresholds_between_the_families(tfhe):
    """One row per compute unit is the last batch of the 4 l-wave kernel, four per compute unit (br_small as the context sets it) the last
    of the two-wave kernel.  The case's five rows tiled, against the tiled schoolbook words."""
    l, beta, n = 2, 10, 5
    c = _case(tfhe, l, beta, n)
    eng, acc, x = c["eng"], c["acc"], c["x"]
    cus = _cu_count()
    want5 = c["want"].astype(np.int32)
    assert eng.get_option("br_tiny") == -2 and eng.get_option("br_small") == 4 * cus and eng.get_option("w2_rw") == 0 and eng.get_option("v3_rw") == 0
    w2 = lambda R: f"blind_rotate_kernel_w2_acc<{l}{',rw2' if _w2_pairs(R, cus) else ''}>"
    with _options(eng, acc_dispatch=1):
        for R, name in ((cus, f"blind_rotate_kernel_h2_acc<{l}>"), (cus + 1, w2(cus + 1)), (4 * cus, w2(4 * cus)), (4 * cus + 1, _name(l, False))):
            tile = np.arange(R) % B_ROWS
            got = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], out_form=0)
            assert eng.last_kernel_name() == name, (R, cus, eng.last_kernel_name())
            assert eng.last_rotation_count() == R and got.shape == (R, K + 1, N)
            assert not _first_bad_row(got, want5[tile]), (R, cus, _first_bad_row(got, want5[tile]))


# ---- 4. GPU: the seam of a split call -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["h2", "w2"])
def test_gpu_split_seam(tfhe, tail):
    """R = 8 compute units' worth of rows + 5: the whole rounds on the one-wave kernel, four rows per workgroup, the last five on the 4 l-wave
    kernel or (br_tiny -1) the two-wave kernel, whose arguments start at row 8 CUs.  The batch call with out_form 0 and out_form 1, n_out 4,
    and the level form into a permuted out_slot over all R rows; with br_split 0 the same words from one launch."""
    l, beta, n = 2, 10, 5
    c = _case(tfhe, l, beta, n)
    eng, acc, x = c["eng"], c["acc"], c["x"]
    R = 8 * _cu_count() + 5
    tile = np.arange(R) % B_ROWS
    want5 = c["want"].astype(np.int32)
    ext4 = _extractions(c["ref"], want5, 4)
    name = _name(l, True) + " + " + (f"blind_rotate_kernel_h2_acc<{l}>" if tail == "h2" else f"blind_rotate_kernel_w2_acc<{l}>")
    assert name.startswith("blind_rotate_kernel_v3_acc<") and eng.get_option("br_split") == 1
    _, allw = _tables(c, n)
    try:
        with _options(eng, acc_dispatch=1, **({} if tail == "h2" else {"br_tiny": -1})):
            got0 = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], out_form=0)
            assert eng.last_kernel_name() == name, eng.last_kernel_name()
            assert eng.last_rotation_count() == R and eng.last_timing_ms(0) > 0
            assert not _first_bad_row(got0, want5[tile]), ("out_form 0", _first_bad_row(got0, want5[tile]))
            got1 = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], n_out=4, out_form=1)
            assert eng.last_kernel_name() == name and not _first_bad_row(got1, ext4[tile]), ("out_form 1", _first_bad_row(got1, ext4[tile]))
            # the level form: row g rotates slot ACC_INDEX[g mod 5] by wire 1 + g mod 5 (the case's rows) into slot out_slot[g]
            eng.tlwe_alloc(3 + R)
            eng.tlwe_upload(0, acc)
            out_slot = (3 + np.random.default_rng(R).permutation(R)).astype(np.int32)
            assert np.array_equal(form_rows(allw, np.arange(B_ROWS + 1), np.arange(1, 1 + B_ROWS), np.ones(B_ROWS, np.int32), None), x)
            eng.bootstrap_acc_level(ACC_INDEX[tile], np.arange(R + 1, dtype=np.int32), (1 + tile).astype(np.int32), np.ones(R, np.int32), out_form=0, out_slot=out_slot)
            assert eng.last_kernel_name() == name and eng.last_rotation_count() == R
            table = eng.tlwe_download(0, 3 + R)
            assert np.array_equal(table[:3], acc), "the accumulators' slots"
            assert not _first_bad_row(table[out_slot], want5[tile]), ("level", _first_bad_row(table[out_slot], want5[tile]))
            assert np.array_equal(eng.wires_download(0, WIRES), allw)
            # one launch
            eng.set_option("br_split", 0)
            one = eng.bootstrap_acc(acc, x[tile], acc_index=ACC_INDEX[tile], out_form=0)
            assert eng.last_kernel_name() == _name(l, True), eng.last_kernel_name()
            assert np.array_equal(one, got0)
            eng.set_option("br_split", 1)
    finally:
        eng.set_option("br_split", 1)
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


# ---- 5. GPU: the option ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_option_values_refusals_and_the_selector_set(tfhe):
    l, beta, n = 2, 10, 5
    c = _case(tfhe, l, beta, n)
    eng, ck, acc, x = c["eng"], c["ck"], c["acc"], c["x"]
    fresh = tfhe.Engine(ck.params)
    assert fresh.get_option("acc_dispatch") == 0
    for bad in (2, -1):                                                  # (a context no call has failed on: the message is this refusal's)
        assert fresh._lib.tfhe_set_option(fresh._h, b"acc_dispatch", bad) == INVALID
        assert "acc_dispatch" in fresh._lib.tfhe_last_error(fresh._h).decode()
        assert fresh.get_option("acc_dispatch") == 0
    fresh.close()
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
        for value in (0, 1):
            eng.set_option("acc_dispatch", value)
            for bad in (2, -1):
                assert eng._lib.tfhe_set_option(eng._h, b"acc_dispatch", bad) == INVALID
                assert eng.get_option("acc_dispatch") == value
        # one refusal of each entry point on each family under option 1
        for family in FAMILIES:
            with _options(eng, acc_dispatch=1, **FAMILIES[family]):
                unchanged_and_still_right()
                assert eng.last_kernel_name() == _family_name(l, family), (family, eng.last_kernel_name())
                # (the codes alone: on this shared context tfhe_last_error may still hold the message of the allocation failure that
                #  tests/test_bootstrap_acc.py injects; that file asserts the refusals' wording)
                rc, msg = bat(acc_index=np.array([0, 3, 0, 0, 0], np.int32))
                assert rc == INVALID, (rc, msg)
                unchanged_and_still_right()
                rc, msg = lvl(out_slot=[8, 9, 9])
                assert rc == INVALID, (rc, msg)
                unchanged_and_still_right()
        # the loaded selector set is what it was: one external product per selector
        assert np.array_equal(eng.extern_mul(probe, every), selectors_before)
    finally:
        eng.set_option("acc_dispatch", 0)
        eng.tlwe_alloc(0)
        eng.wires_alloc(0)


@pytest.mark.gpu
def test_gpu_contexts_without_bootstrap_acc_refuse_with_either_value(tfhe):
    """N = 512, and N = 1024 with the key in the any-N kernels' layout: TFHE_ERR_STATE as without the option."""
    acc = np.zeros((1, 2, N), np.int32)
    raw = tfhe.Engine(_params(tfhe, 512, 1, 3, 8))
    a = np.zeros((1, 2, 512), np.int32)
    x = np.zeros((1, raw.n + 1), np.int32)
    raw.tlwe_alloc(2)
    for value in (0, 1):
        raw.set_option("acc_dispatch", value)
        assert raw.get_option("bootstrap_acc") == 0 and raw.get_option("acc_dispatch") == value
        rc = raw._lib.tfhe_bootstrap_acc_batch(raw._h, _ptr(a), 1, None, _ptr(x), 1, 0, _ptr(np.empty_like(a)), 1)
        msg = raw._lib.tfhe_last_error(raw._h).decode()
        assert rc == STATE and "N = 512, k = 1" in msg and "tfhe_blind_rotate_batch" in msg, (rc, msg)
        rc = raw._lib.tfhe_bootstrap_acc_level(raw._h, _ptr(np.zeros(1, np.int32)), _ptr(np.zeros(2, np.int32)), None, None, None, 1, 0, _ptr(np.ones(1, np.int32)), None, 1)
        msg = raw._lib.tfhe_last_error(raw._h).decode()
        assert rc == STATE and "N = 512, k = 1" in msg and "tfhe_blind_rotate_batch" in msg, (rc, msg)
    raw.close()
    raw = tfhe.Engine(_params(tfhe, N, K, 2, 10, n=5))
    raw.set_option("br_anyn", 1)
    x = np.zeros((1, 6), np.int32)
    for value in (0, 1):
        raw.set_option("acc_dispatch", value)
        assert raw.get_option("bootstrap_acc") == 0
        rc = raw._lib.tfhe_bootstrap_acc_batch(raw._h, _ptr(acc), 1, None, _ptr(x), 1, 0, _ptr(np.empty_like(acc)), 1)
        msg = raw._lib.tfhe_last_error(raw._h).decode()
        assert rc == STATE and "br_anyn" in msg and "tfhe_blind_rotate_batch" in msg, (rc, msg)
    raw.close()


# ---- 6. GPU: the circuit at full size -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_private_lookup_circuit_tuned_equals_default_at_full_size(tfhe, keys80, monkeypatch):
    """examples/private_lut_circuit.py's circuit over two requests at tfhe_parameters_80: with its rotation node tuned and acc_dispatch 1
    it returns the words of the same circuit with tuned=False, they decrypt to the table's entries, and the node's one row ran on the
    4 l-wave kernel."""
    spec = importlib.util.spec_from_file_location("private_lut_circuit", os.path.join(ROOT, "examples", "private_lut_circuit.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    Kp = keys80
    P, DEPTH = example.P, example.DEPTH
    rng = np.random.default_rng(8282)
    table = [int(v) for v in rng.integers(0, P, P << DEPTH)]
    high, da, db = np.array([5, 2]), np.array([3, 0]), np.array([2, 1])
    want = np.array([table[P * h + example.digit_of(a + b)] for h, a, b in zip(high, da, db)])
    enc_table, tgsw, digits = example.request_inputs(rng, Kp.sk, table, high, da, db)
    eng = Kp.ck.engine(0)
    assert eng.get_option("bootstrap_acc") == 1
    plain = example.circuit_path(Kp.ck, enc_table, tgsw, digits)
    names, level = [], eng.bootstrap_acc_level

    def recording(*args, **kwargs):
        level(*args, **kwargs)
        names.append((eng.last_kernel_name(), eng.get_option("acc_dispatch")))

    monkeypatch.setattr(eng, "bootstrap_acc_level", recording, raising=False)
    tuned = example.circuit_path(Kp.ck, enc_table, tgsw, digits, tuned=True)
    assert names == [("blind_rotate_kernel_h2_acc<2>", 1)] * 2, names
    assert eng.get_option("acc_dispatch") == 0
    assert tuned.shape == plain.shape and np.array_equal(tuned, plain)
    got = tfhe.lut_decrypt(Kp.sk, tfhe.LweSampleArray(np.ascontiguousarray(tuned[:, 0])), P)
    assert np.array_equal(got, want), (got, want)
    parity = tfhe.decrypt(Kp.sk, tfhe.LweSampleArray(np.ascontiguousarray(tuned[:, 1])))
    assert np.array_equal(parity, [bin(int(v)).count("1") & 1 == 1 for v in want])
    # a context that does not serve it: the node raises at run time, with the helpers' wording
    ps = _params(tfhe, 64, 1, 3, 8, bs_noise=1e-7)
    sk64, ck64 = tfhe.make_key_pair(np.random.default_rng(3), ps)
    c = tfhe.Circuit()
    a = c.input()
    t = c.tlwe_inputs(1)
    c.set_outputs([c.blind_rotate(t[0], [a], tuned=True)])
    with pytest.raises(ValueError, match="bootstrap_acc"):
        c.run(ck64, np.zeros((1, ps.lwe_size + 1), np.int32), tlwe_inputs=np.zeros((1, 2, 64), np.int32))
    ck64.close()
