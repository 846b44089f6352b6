"""The multi-key leveled half's device-resident table and its level calls (tfhe_mk_tlwe_alloc / _upload / _download,
tfhe_mk_tgsw_update, tfhe_mk_tgsw_expand_update, tfhe_mk_rot_net_level, tfhe_mk_blind_rotate_level; Engine.mk_tlwe_*, mk_tgsw_update,
mk_tgsw_expand_update, mk_rot_net_level, mk_blind_rotate_level; leveled.mk_two_stage_lookup_device).

Every GPU comparison is exact word equality against the host-buffer batch call the level call restates (tfhe_mk_blind_rotate_batch,
tfhe_mk_rot_net_batch, tfhe_mk_cmux_tree_batch, tfhe_mk_extern_mul_batch) on the same samples — those are pinned to the integer
schoolbook by tests/test_mk_blind_rotate.py and tests/test_mk_rot_net.py — so there are no tolerances.  The rotating samples x_g are
formed on the host (tests/test_tlwe_levels.py's `form_rows`: uint32 wrap-around sums of wire rows, tfhe_mk_lut_level's rule).  Two sets
of tests/test_mk_blind_rotate.py, (P, N, l, beta) = (2, 64, 3, 7) and (3, 32, 2, 8), both with n = 3: P n = 6 and 9 steps, one even and
one odd, so both ping-pong samples end up final; one planted row of each set has a zero exponent, which flips that parity.

The host-side slot / wire range and overlap rules are the single-key level calls' (`model_blind_rotate_level`, `model_rot_net_level` of
tests/test_tlwe_levels.py): run over the refusal cases on the CPU and against the library's return codes on the GPU."""
import os
import re

import numpy as np
import pytest

from test_mk_leveled import Setup, _words
from test_tlwe_levels import _mem_free, _ptr, _two_level_net, form_rows, model_blind_rotate_level, model_rot_net_level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_KEY, STATE, NOMEM = 0, 1, 3, 5, 6
SETS = [(2, 64, 3, 7), (3, 32, 2, 8)]
N_LWE = 3
NEW = {"tfhe_mk_tlwe_alloc": 2, "tfhe_mk_tlwe_upload": 4, "tfhe_mk_tlwe_download": 4, "tfhe_mk_tgsw_update": 6, "tfhe_mk_tgsw_expand_update": 13,
       "tfhe_mk_rot_net_level": 12, "tfhe_mk_blind_rotate_level": 12}
METHODS = ("mk_tlwe_alloc", "mk_tlwe_upload", "mk_tlwe_download", "mk_tgsw_update", "mk_tgsw_expand_update", "mk_rot_net_level", "mk_blind_rotate_level")
SLOTS, WIRES, IN_WIRES = 16, 48, 12

# the refusal cases of the GPU test below, as overrides of the valid calls `_Rotate` and `_Net` make (N = 64)
ROT_OK = dict(acc_slot=[1, 1, 2], term_start=[0, 0, 1, 3], term_wire=[4, 5, 4], term_coef=[1, -2, 3], cst=[5, 6, 7], sel=None, n_out=1, out_form=0,
              out_slot=[8, 9, 10], out_wires=None, B=3)
ROT_CASES = [dict(out_slot=[8, 9, 9]), dict(out_slot=[8, 9, 2]), dict(out_slot=[8, 9, SLOTS]), dict(out_slot=[-1, 9, 10]), dict(acc_slot=[1, SLOTS, 2]),
             dict(acc_slot=[1, -1, 2]), dict(term_wire=[4, WIRES, 4]), dict(term_wire=[4, -1, 4]), dict(term_start=[1, 1, 1, 3]), dict(term_start=[0, 2, 1, 3]),
             dict(n_out=2), dict(n_out=0), dict(out_form=1), dict(out_form=3), dict(out_form=-1),
             dict(out_form=2, out_wires=[20, 21, 21]), dict(out_form=2, out_wires=[20, 21, 5]), dict(out_form=2, out_wires=[20, 21, WIRES]),
             dict(out_form=2, n_out=32, out_wires=list(range(12, 12 + 96))), dict(out_form=2, n_out=3, out_wires=list(range(12, 21)))]
NET_OK = dict(table_first=[0, 2, 1], E=4, V=3, out_form=0, out_first=8, out_wires=None, B=3)
NET_CASES = [dict(out_first=5), dict(out_first=11), dict(out_first=-1), dict(table_first=[0, 13, 1]), dict(table_first=[0, -1, 1]), dict(out_form=1), dict(out_form=3),
             dict(table_first=None, out_first=3), dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 20]), dict(out_form=2, out_wires=[20, 21, 22, 23, 24, WIRES]),
             dict(out_form=2, out_wires=[20, 21, 22, 23, 24, -1])]


def _rot_model(a, N=64):
    return model_blind_rotate_level(SLOTS, WIRES, N, a["acc_slot"], a["term_start"], a["term_wire"], a["n_out"], a["out_form"], a["out_slot"], a["out_wires"])


def _net_model(a):
    return model_rot_net_level(SLOTS, WIRES, a["E"], 2, a["B"], a["table_first"], a["out_form"], a["out_first"], a["out_wires"])


# ---- 1. CPU -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(tfhe):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read(), flags=re.S)
    lib = tfhe._lib.load()
    for name, nargs in NEW.items():
        m = re.search(rf"int32_t\s+{name}\s*\(([^)]*)\)", txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert m.group(1).lstrip().startswith("tfhe_ctx *ctx"), name
        assert name in tfhe._lib.ABI_SYMBOLS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    for method in METHODS:
        assert callable(getattr(tfhe.Engine, method)), method
    assert callable(tfhe.mk_two_stage_lookup_device) and "mk_two_stage_lookup_device" in tfhe.__all__
    assert lib.tfhe_abi_version() == 7
    assert lib.tfhe_mk_tlwe_alloc(None, 1) == INVALID and lib.tfhe_mk_tgsw_update(None, None, None, 0, 1, 2) == INVALID          # NULL context


def test_model_of_the_range_and_overlap_rules_over_the_refusal_cases():
    """The cases the GPU test hands the library: each valid call passes the model, each override is refused by it."""
    assert _rot_model(ROT_OK) == OK and _net_model(NET_OK) == OK
    for over in ROT_CASES:
        assert _rot_model(dict(ROT_OK, **over)) == INVALID, over
    for over in NET_CASES:
        assert _net_model(dict(NET_OK, **over)) == INVALID, over
    assert _rot_model(dict(ROT_OK, out_form=2, n_out=4, out_wires=list(range(12, 24)))) == OK
    assert _rot_model(dict(ROT_OK, out_form=2, n_out=16, out_wires=list(range(0, 48))), N=32) == INVALID      # n_out above N / 4 = 8
    assert _net_model(dict(NET_OK, out_form=2, out_wires=[9, 0, 3, 2, 1, 4])) == OK


# ---- 2. GPU: the setup --------------------------------------------------------------------------------------------------------------
OWNERS = lambda P: [0, P - 1, 1 % P, P - 1]      # noqa: E731  (the four selectors behind the key's P n)


def _setup(tfhe, P, N, l, beta, seed, tables=True):
    """P parties' engine with S = P n + 4 selectors loaded (the bootstrapping key party-major, then four uni-encrypted bits), an MK TLWE
    table of SLOTS slots with encryptions in slots 0 ... 7 and a multi-key wire table of WIRES wires with rows in wires 0 ... IN_WIRES - 1."""
    from tfhe_jl_amd import leveled
    s = Setup(tfhe, P, N, l, beta, seed, owners=OWNERS(P), n=N_LWE)
    eng = s.ck.engine(0)
    tg, who = leveled.mk_bootstrap_key_selectors(s.ck)
    s.all_tgsw, s.all_who = np.concatenate([tg, s.tgsw]), np.concatenate([who, s.owners]).astype(np.int32)
    eng.mk_tgsw_load(s.all_tgsw, s.all_who)
    Pn = P * N_LWE
    tlwe = s.encrypt(_words(s.rng, 8, N))
    wires = _words(s.rng, IN_WIRES, Pn + 1)
    half = 2**32 // (2 * N) // 2                     # the words just below and at a rounding boundary of decode_message(., 2N)
    wires[1, :6] = [2**31 - 1, -2**31, half - 1, half, -half - 1, -half]
    wires[4, Pn - 1] = 0                             # a skipped last step: the other ping-pong sample is the final one
    wires[4, Pn - 2] = 2**30                         # (the step before it is not)
    wires[4, Pn] = 3 * half - 1
    s.full = np.concatenate([tlwe, _words(s.rng, SLOTS - 8, P + 1, N)])
    s.allw = np.concatenate([wires, _words(s.rng, WIRES - IN_WIRES, Pn + 1)])
    if tables:
        eng.mk_tlwe_alloc(SLOTS)
        eng.mk_tlwe_upload(0, s.full)
        eng.mk_wires_alloc(WIRES)
        eng.wires_upload(0, s.allw)
    return s, eng


# ---- 3. GPU: the table and the selector updates -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", SETS)
def test_gpu_mk_tlwe_table_partial_round_trip(tfhe, P, N, l, beta):
    s, eng = _setup(tfhe, P, N, l, beta, 9100 + N)
    full = s.full
    assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), full)
    part = _words(s.rng, 3, P + 1, N)
    eng.mk_tlwe_upload(5, part)
    want = full.copy()
    want[5:8] = part
    assert np.array_equal(eng.mk_tlwe_download(4, 5), want[4:9])         # a partial range across the edited one
    assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), want)          # every untouched slot intact
    assert eng.mk_tlwe_download(SLOTS, 0).shape == (0, P + 1, N)         # an empty range at the end of the table
    for first, count in ((-1, 1), (SLOTS, 1), (SLOTS - 1, 2), (0, -1)):
        with pytest.raises(tfhe.EngineError) as e:
            eng.mk_tlwe_download(first, count)
        assert e.value.code == INVALID
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_tlwe_upload(SLOTS - 2, part)
    assert e.value.code == INVALID and np.array_equal(eng.mk_tlwe_download(0, SLOTS), want)
    # an oversized table: refused with hipMemGetInfo unchanged, the present table kept
    before = _mem_free()
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_tlwe_alloc(2**31 - 1)
    assert e.value.code == NOMEM and "free memory" in str(e.value)
    assert _mem_free() == before
    assert eng._lib.tfhe_mk_tlwe_alloc(eng._h, -1) == INVALID and eng._lib.tfhe_mk_tlwe_alloc(eng._h, 2**31) == INVALID
    assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), want)
    eng.mk_tlwe_alloc(4)                                                 # reallocating discards; the new table works
    eng.mk_tlwe_upload(1, part)
    assert np.array_equal(eng.mk_tlwe_download(1, 3), part)
    eng.mk_tlwe_alloc(0)                                                 # freed
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_tlwe_download(0, 1)
    assert e.value.code == STATE
    raw = tfhe.Engine(s.p)                                               # no multi-key bootstrapping key: nothing fixes P
    assert raw._lib.tfhe_mk_tlwe_alloc(raw._h, 4) == NO_KEY and "bootstrapping key" in raw._lib.tfhe_last_error(raw._h).decode()
    raw.close()
    s.ck.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", SETS)
def test_gpu_mk_tgsw_update_equals_a_fresh_load_of_the_edited_set(tfhe, P, N, l, beta):
    s, eng = _setup(tfhe, P, N, l, beta, 9200 + N, tables=False)
    S, Pn = s.all_tgsw.shape[0], P * N_LWE
    x = np.ascontiguousarray(np.repeat(s.full[3:4], S, axis=0))
    every = np.arange(S, dtype=np.int32)
    before = eng.mk_extern_mul(x, every)
    pick = [1, 0, 3]                                                     # three of the bits behind the key, into selectors 2, 3, 4 of the key
    new, new_who = s.tgsw[pick].copy(), s.owners[pick].copy()
    assert s.all_who[2] == 0 and new_who[0] == P - 1                     # selector 2 changes its party
    eng.mk_tgsw_update(2, new, new_who)
    after = eng.mk_extern_mul(x, every)
    edited, edited_who = s.all_tgsw.copy(), s.all_who.copy()
    edited[2:5], edited_who[2:5] = new, new_who
    eng.mk_tgsw_load(edited, edited_who)
    fresh = eng.mk_extern_mul(x, every)
    assert np.array_equal(after, fresh)
    untouched = [i for i in range(S) if not 2 <= i < 5]
    assert np.array_equal(after[untouched], before[untouched]) and not np.array_equal(after[2:5], before[2:5])
    lib, h = eng._lib, eng._h
    for first, count in ((-1, 1), (S, 1), (S - 1, 2)):
        assert lib.tfhe_mk_tgsw_update(h, _ptr(new), _ptr(new_who), first, count, P) == INVALID and "mk_tgsw_update" in lib.tfhe_last_error(h).decode()
    assert lib.tfhe_mk_tgsw_update(h, None, _ptr(new_who), 0, 1, P) == INVALID and lib.tfhe_mk_tgsw_update(h, _ptr(new), _ptr(new_who), 0, 0, P) == INVALID
    assert lib.tfhe_mk_tgsw_update(h, _ptr(new), _ptr(np.array([P], np.int32)), 0, 1, P) == INVALID
    assert lib.tfhe_mk_tgsw_update(h, _ptr(new), _ptr(new_who), 0, 1, P + 1) == STATE
    assert np.array_equal(eng.mk_extern_mul(x, every), fresh)
    # the same through RGSW.Expand on the device, against tfhe_mk_tgsw_expand_load of the edited set
    uni_all = [np.concatenate([a.reshape((Pn,) + a.shape[2:]), b]) for a, b in zip(s.ck._part_arrays()[1:], s.uni)]
    eng.mk_tgsw_expand_load(s.pub, s.all_who, *uni_all)
    before = eng.mk_extern_mul(x, every)
    expanded = eng.mk_tgsw_expand_update(2, s.pub, new_who, *[a[pick] for a in s.uni], want_expanded=True)
    assert np.array_equal(expanded, new)                                 # the host expansion (leveled.mk_tgsw_expand) of the same samples
    after = eng.mk_extern_mul(x, every)
    uni_edit = [a.copy() for a in uni_all]
    for a, b in zip(uni_edit, s.uni):
        a[2:5] = b[pick]
    eng.mk_tgsw_expand_load(s.pub, edited_who, *uni_edit)
    assert np.array_equal(after, eng.mk_extern_mul(x, every)) and np.array_equal(after, fresh)
    assert np.array_equal(after[untouched], before[untouched])
    raw = tfhe.Engine(s.p)
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)
    assert raw._lib.tfhe_mk_tgsw_update(raw._h, _ptr(new), _ptr(new_who), 0, 1, P) == NO_KEY
    raw.close()
    s.ck.close()


# ---- 4. GPU: mk_blind_rotate_level against tfhe_mk_blind_rotate_batch ------------------------------------------------------------------
ACC_SLOT = np.array([3, 2, 3, 5, 4, 6, 0, 1], np.int32)                  # slot 3 twice
OUT_SLOT = np.array([7, 8, 9, 15, 10, 12, 14, 11], np.int32)             # slot 13 is written by nobody
TERM_START = np.array([0, 0, 1, 4, 5, 6, 6, 7, 8], np.int32)
TERM_WIRE = np.array([1, 2, 3, 2, 4, 5, 6, 1], np.int32)                 # row 1: the planted wire; row 2: three terms, wire 2 twice
TERM_COEF = np.array([1, -3, -2**31, 2**31 - 1, 1, -1, 7, -2**31], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", SETS)
def test_gpu_mk_blind_rotate_level_equals_the_batch_call(tfhe, P, N, l, beta):
    s, eng = _setup(tfhe, P, N, l, beta, 9300 + N)
    full, allw = s.full, s.allw
    S, B, Pn = s.all_tgsw.shape[0], len(ACC_SLOT), P * N_LWE
    cst = _words(s.rng, B)
    cst[5] = 0                                                           # row 5: no terms, no constant: the all-zero row, a plain copy
    x = form_rows(allw, TERM_START, TERM_WIRE, TERM_COEF, cst)
    two_n = 2 * N
    exps = ((x.astype(np.int64) + 2**32 // two_n // 2) >> (32 - two_n.bit_length() + 1)) % two_n
    assert not exps[0, :Pn].any() and not exps[5].any() and list(exps[1, :6]) == [N, N, 0, 1, 2 * N - 1, 0] and exps[3, Pn - 1] == 0 and exps[3, Pn - 2] != 0
    perm = np.random.default_rng(5).permutation(S)[:Pn].astype(np.int32)
    assert len(set(perm.tolist())) == Pn
    for sel in (None, perm):
        # out_form 0: the final accumulators into their slots, every other slot as it was
        want = eng.mk_blind_rotate(full, x, sel=sel, acc_index=ACC_SLOT, in_form=0, out_form=0)
        eng.mk_blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, sel=sel, out_form=0, out_slot=OUT_SLOT)
        assert eng.last_kernel_name() == f"mk_tlwe_rotate_level_kernel(N={N},P={P},l={l},steps={Pn})"
        assert eng.last_rotation_count() == B and eng.last_timing_ms(0) > 0
        table = full.copy()
        table[OUT_SLOT] = want
        got = eng.mk_tlwe_download(0, SLOTS)
        assert np.array_equal(got[OUT_SLOT], want), ("out_form 0", sel)
        assert np.array_equal(got, table) and np.array_equal(eng.wires_download(0, WIRES), allw)
        eng.mk_tlwe_upload(0, full)
        # out_form 2: the keyswitched extractions into permuted wires, every other wire as it was
        for n_out in (1, 4):
            out_wires = (IN_WIRES + s.rng.permutation(WIRES - IN_WIRES)[:B * n_out]).astype(np.int32)
            want2 = eng.mk_blind_rotate(full, x, sel=sel, acc_index=ACC_SLOT, in_form=0, n_out=n_out, out_form=2)
            eng.mk_blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, sel=sel, n_out=n_out, out_form=2, out_wires=out_wires)
            assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
            wtab = allw.copy()
            wtab[out_wires] = want2.reshape(B * n_out, Pn + 1)
            assert np.array_equal(eng.wires_gather(out_wires), want2.reshape(B * n_out, Pn + 1)), ("out_form 2", n_out, sel)
            assert np.array_equal(eng.wires_download(0, WIRES), wtab) and np.array_equal(eng.mk_tlwe_download(0, SLOTS), full)
            eng.wires_upload(0, allw)
    # cst NULL: the rows without their constants
    x0 = form_rows(allw, TERM_START, TERM_WIRE, TERM_COEF, None)
    eng.mk_blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, sel=perm, out_form=0, out_slot=OUT_SLOT)
    assert np.array_equal(eng.mk_tlwe_download(0, SLOTS)[OUT_SLOT], eng.mk_blind_rotate(full, x0, sel=perm, acc_index=ACC_SLOT, in_form=0, out_form=0))
    # a call without terms reads no wire: rows (0, ..., 0, cst[g]), staged by the host
    eng.mk_tlwe_upload(0, full)
    xc = np.zeros((3, Pn + 1), np.int32)
    xc[:, Pn] = cst[:3]
    eng.mk_blind_rotate_level([2, 0, 2], [0, 0, 0, 0], [], [], cst=cst[:3], out_form=0, out_slot=[9, 10, 13])
    assert np.array_equal(eng.mk_tlwe_download(0, SLOTS)[[9, 10, 13]], eng.mk_blind_rotate(full, xc, acc_index=[2, 0, 2], in_form=0, out_form=0))
    # the spectrum accumulators in global memory change no word
    eng.mk_tlwe_upload(0, full)
    eng.set_option("anyn_spec", 1)
    eng.mk_blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, sel=perm, out_form=0, out_slot=OUT_SLOT)
    assert eng.last_kernel_name() == f"mk_tlwe_rotate_level_kernel(N={N},P={P},l={l},steps={Pn},spec=global)"
    glob = eng.mk_tlwe_download(0, SLOTS)
    eng.set_option("anyn_spec", -1)
    assert np.array_equal(glob[OUT_SLOT], want)                          # (want: the last out_form 0 of the loop, sel = perm)
    s.ck.close()


# ---- 5. GPU: mk_rot_net_level against tfhe_mk_rot_net_batch ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", SETS)
def test_gpu_mk_rot_net_level_equals_the_batch_call(tfhe, P, N, l, beta):
    from tfhe_jl_amd import leveled
    s, eng = _setup(tfhe, P, N, l, beta, 9400 + N)
    full, allw = s.full, s.allw
    S, Pn = s.all_tgsw.shape[0], P * N_LWE
    net = _two_level_net(leveled, N)                                     # copies and rotations 0, 1, N, 2N - 1
    first = np.array([0, 2, 1], np.int32)                                # different and overlapping read ranges
    B, E, F = 3, 4, 2
    sel = s.rng.integers(0, S, (B, 3)).astype(np.int32)
    sel[0] = [0, Pn - 1, Pn + 1]                                         # selectors of different parties within one level
    assert s.all_who[sel[0, 0]] != s.all_who[sel[0, 1]]
    data = np.stack([full[f:f + E] for f in first])
    want = eng.mk_rot_net(data, net, sel, table_index=np.arange(B, dtype=np.int32), out_form=0)
    eng.mk_rot_net_level(net, sel, table_first=first, out_form=0, out_first=8)
    assert eng.last_kernel_name().startswith("mk_rot_net_level_kernel(")
    table = full.copy()
    table[8:8 + B * F] = want.reshape(B * F, P + 1, N)
    assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), table), "out_form 0"
    eng.mk_tlwe_upload(0, full)
    out_wires = (IN_WIRES + s.rng.permutation(WIRES - IN_WIRES)[:B * F]).astype(np.int32)
    want2 = eng.mk_rot_net(data, net, sel, table_index=np.arange(B, dtype=np.int32), out_form=2)
    eng.mk_rot_net_level(net, sel, table_first=first, out_form=2, out_wires=out_wires)
    wtab = allw.copy()
    wtab[out_wires] = want2.reshape(B * F, Pn + 1)
    assert np.array_equal(eng.wires_download(0, WIRES), wtab) and np.array_equal(eng.mk_tlwe_download(0, SLOTS), full), "out_form 2"
    eng.wires_upload(0, allw)
    # a packed lookup (a tree level, then rotations by -2^b) at absolute slots: table_first NULL
    depth = N.bit_length()                                               # log2 N + 1: two samples
    packed = leveled.packed_lookup_net(depth, N)
    assert packed.entries == 2 and packed.variables == depth <= S
    selp = np.stack([s.rng.permutation(S)[:depth] for _ in range(2)]).astype(np.int32)
    wantp = eng.mk_rot_net(full[:2], packed, selp, out_form=0)
    eng.mk_rot_net_level(packed, selp, out_form=0, out_first=SLOTS - 2)
    assert np.array_equal(eng.mk_tlwe_download(SLOTS - 2, 2), wantp[:, 0]) and np.array_equal(eng.mk_tlwe_download(0, SLOTS - 2), full[:SLOTS - 2])
    # a CMUX tree as the rotation-0 case: tfhe_mk_cmux_tree_batch's words
    tree = leveled.tree_net(2)
    selt = s.rng.integers(0, S, (2, 2)).astype(np.int32)
    wantt = eng.mk_cmux_tree(np.stack([full[2:6], full[3:7]]), selt, table_index=[0, 1], out_form=2)
    eng.mk_rot_net_level(tree, selt, table_first=[2, 3], out_form=2, out_wires=[40, 13])
    assert np.array_equal(eng.wires_gather([40, 13]), wantt)
    s.ck.close()


# ---- 6. GPU: the chain on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", SETS)
def test_gpu_chain_stays_on_the_device(tfhe, P, N, l, beta):
    """wires -> mk_blind_rotate_level (into slots) -> mk_rot_net_level (a depth-1 tree over two of those slots, into wires) -> a NAND
    level on those wires: the words of the same chain through the host-buffer calls."""
    from tfhe_jl_amd import leveled
    s, eng = _setup(tfhe, P, N, l, beta, 9500 + N)
    full, allw = s.full, s.allw
    S = s.all_tgsw.shape[0]
    start, wire, coef = np.array([0, 1, 3, 4, 4], np.int32), np.array([7, 8, 9, 10], np.int32), np.array([1, 2, -1, 5], np.int32)
    cst = _words(s.rng, 4)
    acc = np.array([2, 3, 4, 5], np.int32)
    tree = leveled.tree_net(1)
    selt = np.array([[S - 1], [S - 2]], np.int32)
    # the host chain
    x = form_rows(allw, start, wire, coef, cst)
    stage1 = eng.mk_blind_rotate(full, x, acc_index=acc, in_form=0, out_form=0)
    stage2 = eng.mk_rot_net(stage1.reshape(2, 2, P + 1, N), leveled.RotNet(tree.widths, [(0, 1, 0, 0, 0)], N), selt, table_index=[0, 1], out_form=2)[:, 0]
    want = eng.mk_gates_batch(np.zeros(2, np.uint8), stage2, allw[[0, 1]])
    # the device chain: slots 8 ... 11, wires 20 and 21, wires 30 and 31
    eng.mk_blind_rotate_level(acc, start, wire, coef, cst=cst, out_form=0, out_slot=[8, 9, 10, 11])
    eng.mk_rot_net_level(tree, selt, table_first=[8, 10], out_form=2, out_wires=[20, 21])
    eng.mk_gates_level(np.zeros(2, np.uint8), [20, 21], [0, 1], None, [30, 31])
    assert np.array_equal(eng.wires_gather([20, 21]), stage2)
    assert np.array_equal(eng.wires_gather([30, 31]), want)
    # ... and a level call queued behind an asynchronous mk_lut_level reads what that level wrote
    tv = _words(s.rng, 1, N)
    lut_out = eng.mk_bootstrap_tv(tv, want[:1])
    eng.mk_lut_level(tv, [0, 1], [30], [1], None, [32])
    eng.mk_blind_rotate_level([2], [0, 1], [32], [1], out_form=2, out_wires=[34])
    assert np.array_equal(eng.wires_gather([32]), lut_out)
    assert np.array_equal(eng.wires_gather([34])[0], eng.mk_blind_rotate(full, lut_out, acc_index=[2], in_form=0, out_form=2)[0, 0])
    s.ck.close()


@pytest.mark.gpu
def test_gpu_two_stage_lookup_device_equals_the_host_helper(tfhe):
    """leveled.mk_two_stage_lookup_device on two requests (the second swaps only its address bits in) against mk_two_stage_lookup."""
    from tfhe_jl_amd import leveled, lut
    P, N, l, beta = SETS[0]
    highs = [(a >> 2) for a in range(8)]
    s = Setup(tfhe, P, N, l, beta, 9550, owners=[0, 1] * 8, bits=[(h >> v) & 1 for h in highs for v in range(2)], n=N_LWE)
    table = [int(v) for v in np.random.default_rng(5).integers(0, 4, 16)]
    tables = np.concatenate([leveled.mk_tlwe_trivial(lut.make_test_vector(lambda m, h=h: table[4 * h + m], 4, N), P) for h in range(4)])
    x = lut.mk_lut_encrypt(s.rng, s.sks, np.arange(8) & 3, 4)
    uni = [a.reshape(8, 2, l, N) for a in s.uni]
    want = leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, 4)
    eng = s.ck.engine(0)
    eng.mk_tlwe_alloc(8)
    eng.mk_tlwe_upload(0, tables)
    eng.mk_wires_alloc(16)
    eng.wires_upload(0, x)
    for req in (slice(0, 4), slice(4, 8)):
        leveled.mk_two_stage_lookup_device(s.ck, 0, [a[req] for a in uni], [0, 1], np.arange(8)[req], [8, 9, 10, 11], work_slot=4)
        assert np.array_equal(eng.wires_gather([8, 9, 10, 11]), want[req]), req
    assert eng._mk_key_extra == 8                                        # the key was loaded once, with 4 x 2 address bits behind it
    s.ck.close()


# ---- 7. GPU: refusals ---------------------------------------------------------------------------------------------------------------
class _Rotate:
    """A valid raw tfhe_mk_blind_rotate_level call whose arguments can be replaced one at a time."""

    def __init__(self, eng):
        self.eng, self.args = eng, dict(ROT_OK)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        arr = {key: None if a[key] is None else np.asarray(a[key], np.int32) for key in ("acc_slot", "term_start", "term_wire", "term_coef", "cst", "sel", "out_slot", "out_wires")}
        rc = e._lib.tfhe_mk_blind_rotate_level(e._h, _ptr(arr["acc_slot"]), _ptr(arr["term_start"]), _ptr(arr["term_wire"]), _ptr(arr["term_coef"]), _ptr(arr["cst"]),
                                               _ptr(arr["sel"]), a["n_out"], a["out_form"], _ptr(arr["out_slot"]), _ptr(arr["out_wires"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode(), a


class _Net:
    """The same for tfhe_mk_rot_net_level, on the two-level network."""

    def __init__(self, eng, net, sel):
        self.eng = eng
        self.args = dict(NET_OK, widths=net.widths, levels=net.levels, nodes=net.nodes, sel=sel)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        arr = {key: None if a[key] is None else np.ascontiguousarray(a[key], np.int32) for key in ("table_first", "widths", "nodes", "sel", "out_wires")}
        rc = e._lib.tfhe_mk_rot_net_level(e._h, _ptr(arr["table_first"]), a["E"], _ptr(arr["widths"]), a["levels"], _ptr(arr["nodes"]), _ptr(arr["sel"]), a["V"],
                                          a["out_form"], a["out_first"], _ptr(arr["out_wires"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode(), a


@pytest.mark.gpu
def test_gpu_refusals_change_nothing_and_the_next_call_is_right(tfhe):
    from tfhe_jl_amd import leveled
    P, N, l, beta = SETS[0]
    s, eng = _setup(tfhe, P, N, l, beta, 9600)
    full, allw = s.full, s.allw
    S, Pn = s.all_tgsw.shape[0], P * N_LWE
    net = _two_level_net(leveled, N)
    sel = s.rng.integers(0, S, (3, 3)).astype(np.int32)
    rot, lvl = _Rotate(eng), _Net(eng, net, sel)
    a = rot.args
    x = form_rows(allw, a["term_start"], a["term_wire"], a["term_coef"], a["cst"])
    want_rot = eng.mk_blind_rotate(full, x, acc_index=a["acc_slot"], in_form=0, out_form=0)
    want_net = eng.mk_rot_net(np.stack([full[f:f + 4] for f in (0, 2, 1)]), net, sel, table_index=[0, 1, 2], out_form=0).reshape(6, P + 1, N)

    def unchanged_and_still_right():
        assert np.array_equal(eng.mk_tlwe_download(0, SLOTS), full) and np.array_equal(eng.wires_download(0, WIRES), allw)
        assert rot()[0] == OK and np.array_equal(eng.mk_tlwe_download(8, 3), want_rot)
        assert lvl()[0] == OK and np.array_equal(eng.mk_tlwe_download(8, 6), want_net)
        eng.mk_tlwe_upload(8, full[8:14])

    unchanged_and_still_right()
    assert rot(B=0)[0] == OK and lvl(B=0)[0] == OK
    for over in ROT_CASES:
        rc, msg, args = rot(**over)
        assert rc == _rot_model(args) == INVALID and msg.startswith("mk_blind_rotate_level:"), (over, rc, msg)
        unchanged_and_still_right()
    assert "slot 9 written twice" in rot(out_slot=[8, 9, 9])[1] and "acc_slot[2] = 2 is an output slot" in rot(out_slot=[8, 9, 2])[1]
    assert "wire 21 written twice" in rot(out_form=2, out_wires=[20, 21, 21])[1] and "reads wire 5, which the same call writes" in rot(out_form=2, out_wires=[20, 21, 5])[1]
    good_sel = list(range(Pn))
    for over in (dict(B=-1), dict(acc_slot=None), dict(term_start=None), dict(out_slot=None), dict(out_form=2), dict(term_wire=None), dict(term_coef=None),
                 dict(sel=good_sel[:-1] + [S]), dict(sel=good_sel[:-1] + [-1])):
        rc, msg, _ = rot(**over)
        assert rc == INVALID and msg.startswith("mk_blind_rotate_level:"), (over, rc, msg)
    for over in NET_CASES:
        rc, msg, args = lvl(**over)
        assert rc == _net_model(args) == INVALID and msg.startswith("mk_rot_net_level:"), (over, rc, msg)
        unchanged_and_still_right()
    assert "meet the slots" in lvl(out_first=5)[1] and "wire 20 written twice" in lvl(out_form=2, out_wires=[20, 21, 22, 23, 24, 20])[1]
    bad_nodes = net.nodes.copy(); bad_nodes[3, 1] = 3
    bad_sel = sel.copy(); bad_sel[1, 1] = S
    for over in (dict(B=-1), dict(widths=None), dict(nodes=None), dict(sel=None), dict(E=0), dict(E=SLOTS + 1), dict(V=0), dict(levels=0), dict(nodes=bad_nodes),
                 dict(sel=bad_sel), dict(out_form=2)):
        rc, msg, _ = lvl(**over)
        assert rc == INVALID and msg.startswith("mk_rot_net_level:"), (over, rc, msg)
    unchanged_and_still_right()
    # the state a level call needs, refused before the arguments are looked at
    eng.set_option("measure_margin", 1)
    for call, over in ((rot, dict(out_slot=[8, 9, 9])), (lvl, dict(out_first=5))):
        rc, msg, _ = call(**over)
        assert rc == STATE and "measure_margin" in msg, (rc, msg)
    eng.set_option("measure_margin", 0)
    unchanged_and_still_right()
    raw = tfhe.Engine(s.p)
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)
    for call in (rot, lvl):
        rc, msg, _ = call(eng=raw)
        assert rc == STATE and "no MK TLWE table" in msg, (rc, msg)
    raw.mk_tlwe_alloc(SLOTS)
    raw.mk_tlwe_upload(0, full)
    rc, msg, _ = rot(eng=raw)
    assert rc == STATE and "no wire table" in msg, (rc, msg)               # the call has terms
    rc, msg, _ = lvl(eng=raw, out_form=2, out_wires=[20, 21, 22, 23, 24, 25])
    assert rc == STATE and "no wire table" in msg, (rc, msg)
    raw.wires_alloc(WIRES)                                                 # a wire table with single-key rows
    for call, over in ((rot, dict()), (lvl, dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 25]))):
        rc, msg, _ = call(eng=raw, **over)
        assert rc == STATE and "single-key rows" in msg, (rc, msg)
    raw.wires_alloc(0)
    rc, msg, _ = rot(eng=raw, term_start=[0, 0, 0, 0], out_slot=[8, 9, 9])
    assert rc == INVALID, (rc, msg)                                        # without terms no wire table is needed: the arguments come next
    for call, over in ((rot, dict(term_start=[0, 0, 0, 0])), (lvl, dict())):
        rc, msg, _ = call(eng=raw, **over)
        assert rc == NO_KEY and "tfhe_mk_tgsw_load" in msg, (rc, msg)      # ... then the selector set
    raw.mk_tgsw_load(s.all_tgsw, s.all_who)
    raw.mk_wires_alloc(WIRES)
    raw.wires_upload(0, allw)
    for call, over in ((rot, dict(out_form=2, out_wires=[20, 21, 22])), (lvl, dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 25]))):
        rc, msg, _ = call(eng=raw, **over)
        assert rc == NO_KEY and "keyswitch" in msg, (rc, msg)
        rc, msg, _ = call(eng=raw, **dict(over, out_wires=[20] * len(over["out_wires"])))
        assert rc == INVALID and "written twice" in msg, (rc, msg)         # the arguments are named before the missing key
    assert np.array_equal(raw.mk_tlwe_download(0, SLOTS), full) and np.array_equal(raw.wires_download(0, WIRES), allw)
    assert rot(eng=raw)[0] == OK and np.array_equal(raw.mk_tlwe_download(8, 3), want_rot)       # forms that need no keyswitch key run
    raw.close()
    multi = s.ck.engine([0, 0])
    for call in (rot, lvl):
        rc, msg, _ = call(eng=multi)
        assert rc == STATE and "multi-device" in msg, (rc, msg)
    assert multi._lib.tfhe_mk_tlwe_alloc(multi._h, 4) == STATE
    assert multi._lib.tfhe_mk_tgsw_update(multi._h, _ptr(s.tgsw), _ptr(s.owners), 0, 1, P) == STATE
    # an injected allocation failure: NOMEM, nothing written, and the context goes on working
    lib = eng._lib
    for call in (rot, lvl):
        assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
        rc, msg, _ = call()
        lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
        assert rc == NOMEM and "memory" in msg, (rc, msg)
        unchanged_and_still_right()
    s.ck.close()


@pytest.mark.gpu
def test_gpu_tables_and_keys_of_another_party_count_are_refused(tfhe):
    """A table, a wire table and a keyswitch key whose parties differ from the bootstrapping key's: TFHE_ERR_STATE each, before the
    arguments are looked at; with all of them for the same parties the calls run."""
    from tfhe_jl_amd import leveled
    s3 = Setup(tfhe, 3, 32, 2, 8, 9650, owners=[0, 1, 2], n=N_LWE)
    ck2 = tfhe.MKCloudKey(s3.parts[:2])
    raw = tfhe.Engine(s3.p)
    raw.mk_load_bootstrap_key(s3.ck.bootstrap_key, 3)
    raw.mk_load_keyswitch_key(s3.ck.keyswitch_key, 3)
    raw.mk_tlwe_alloc(SLOTS)
    raw.mk_wires_alloc(WIRES)
    raw.mk_load_bootstrap_key(ck2.bootstrap_key, 2)                        # now P = 2: the table, the wires and the keyswitch key are 3-party
    net = _two_level_net(leveled, 32)
    rot, lvl = _Rotate(raw), _Net(raw, net, np.zeros((3, 3), np.int32))
    wires6 = dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 25])
    for call in (rot, lvl):
        rc, msg, _ = call()
        assert rc == STATE and "MK TLWE table holds 3-party" in msg, (rc, msg)
    raw.mk_tlwe_alloc(SLOTS)
    for call, over in ((rot, dict()), (lvl, wires6)):
        rc, msg, _ = call(**over)
        assert rc == STATE and "wire table holds 3-party" in msg, (rc, msg)
    raw.mk_wires_alloc(WIRES)
    for call, over in ((rot, dict(out_form=2, out_wires=[20, 21, 22])), (lvl, wires6)):
        rc, msg, _ = call(**over)
        assert rc == STATE and "keyswitch key for 3" in msg, (rc, msg)
    rc, msg, _ = rot()
    assert rc == NO_KEY and "selector" in msg, (rc, msg)                   # out_form 0 does not ask about the keyswitch key
    raw.close()
    ck2.close()
    s3.ck.close()


@pytest.mark.gpu
def test_gpu_single_key_context_refuses_every_new_entry_point(tfhe):
    p1 = tfhe.SchemeParameters(16, 1 / 2**15, 64, 1, 3, 7, 1e-7, 8, 2, 1 / 2**15, 1)
    rng = np.random.default_rng(9700)
    sk1, ck1 = tfhe.make_key_pair(rng, p1)
    e1 = ck1.engine(0)
    lib, h = e1._lib, e1._h
    one, two = np.zeros(1, np.int32), np.zeros(2, np.int32)
    poly = np.zeros(64 * 64, np.int32)
    assert lib.tfhe_mk_tlwe_alloc(h, 4) == STATE and "single-key" in lib.tfhe_last_error(h).decode()
    assert lib.tfhe_mk_tlwe_upload(h, 0, 0, None) == STATE and lib.tfhe_mk_tlwe_download(h, 0, 0, None) == STATE
    assert lib.tfhe_mk_tgsw_update(h, _ptr(poly), _ptr(one), 0, 1, 2) == STATE
    assert lib.tfhe_mk_tgsw_expand_update(h, 2, *[_ptr(poly)] * 1, _ptr(one), *[_ptr(poly)] * 6, 0, 1, None) == STATE
    assert lib.tfhe_mk_blind_rotate_level(h, _ptr(one), _ptr(two), None, None, None, None, 1, 0, _ptr(one), None, 1) == STATE
    widths, nodes = np.ones(1, np.int32), np.zeros(5, np.int32)
    assert lib.tfhe_mk_rot_net_level(h, None, 1, _ptr(widths), 1, _ptr(nodes), _ptr(one), 1, 0, 1, None, 1) == STATE
    assert "single-key" in lib.tfhe_last_error(h).decode()
    bx = tfhe.encrypt(rng, sk1, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk1, e1.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])      # the context still runs its gates
    ck1.close()
