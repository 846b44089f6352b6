"""The leveled half's device-resident table and its level calls (tfhe_tlwe_alloc / _upload / _download, tfhe_tgsw_update,
tfhe_rot_net_level, tfhe_blind_rotate_level; Engine.tlwe_*, tgsw_update, rot_net_level, blind_rotate_level).

Every GPU comparison is word for word against the host-buffer batch call the level call restates (tfhe_blind_rotate_batch,
tfhe_rot_net_batch, tfhe_extern_mul_batch) on the same samples — those are pinned to the integer schoolbook by tests/test_blind_rotate.py
and tests/test_rot_net.py — and one set is compared with that schoolbook (`Rotation`) directly.  The rotating samples x_g are formed on
the host here (`form_rows`: uint32 wrap-around sums of wire rows, tfhe_lut_level's rule).  Two parameter sets, (N, k, l, beta) =
(64, 1, 3, 8) with n = 7 and (128, 2, 2, 10) with n = 6: an odd and an even step count, so both ping-pong samples end up final.

The host-side range and overlap rules of the two level calls are restated as a small model (`model_blind_rotate_level`,
`model_rot_net_level`): checked by hand cases on the CPU and against the library's return codes on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_blind_rotate import Rotation
from test_leveled import _params, _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, NO_KEY, STATE, NOMEM = 0, 1, 3, 5, 6
SETS = [(64, 1, 3, 8, 7), (128, 2, 2, 10, 6)]
NEW = {"tfhe_tlwe_alloc": 2, "tfhe_tlwe_upload": 4, "tfhe_tlwe_download": 4, "tfhe_tgsw_update": 4, "tfhe_rot_net_level": 12, "tfhe_blind_rotate_level": 12}


# ---- the host model -----------------------------------------------------------------------------------------------------------------
def form_rows(wires, term_start, term_wire, term_coef, cst):
    """x_g = sum_t coef[t] * wires[wire[t]] (+ cst[g] on the body) mod 2^32: int32 [B][n+1]."""
    w = np.ascontiguousarray(wires, np.int32).view(np.uint32)
    coef = np.ascontiguousarray(term_coef, np.int32).view(np.uint32)
    B = len(term_start) - 1
    out = np.zeros((B, w.shape[1]), np.uint32)
    for g in range(B):
        for t in range(term_start[g], term_start[g + 1]):
            out[g] += coef[t] * w[term_wire[t]]
        if cst is not None:
            out[g, -1:] += np.ascontiguousarray(cst, np.int32).view(np.uint32)[g:g + 1]
    return out.view(np.int32)


def model_blind_rotate_level(slots, wires, N, acc_slot, term_start, term_wire, n_out, out_form, out_slot, out_wires):
    """TFHE_OK or TFHE_ERR_INVALID_ARG of a tfhe_blind_rotate_level call on a table of `slots` slots and `wires` wires (state and keys
    in order): the ranges, the distinct outputs, no output that the same call reads."""
    B = len(acc_slot)
    if out_form not in (0, 2) or n_out < 1 or n_out > 32 or n_out & (n_out - 1) or (n_out > 1 and n_out > N // 4) or (out_form == 0 and n_out != 1):
        return INVALID
    if len(term_start) != B + 1 or term_start[0] != 0 or any(term_start[g + 1] < term_start[g] for g in range(B)):
        return INVALID
    terms = list(term_wire[:term_start[B]])
    if any(not 0 <= w < wires for w in terms) or any(not 0 <= s < slots for s in acc_slot):
        return INVALID
    if out_form == 0:
        outs = list(out_slot)
        if len(outs) != B or any(not 0 <= s < slots for s in outs) or len(set(outs)) != len(outs) or set(outs) & set(acc_slot):
            return INVALID
    else:
        outs = list(out_wires)
        if len(outs) != B * n_out or any(not 0 <= w < wires for w in outs) or len(set(outs)) != len(outs) or set(outs) & set(terms):
            return INVALID
    return OK


def model_rot_net_level(slots, wires, E, F, B, table_first, out_form, out_first, out_wires):
    """The same for tfhe_rot_net_level with a valid network of E entries and F outputs."""
    if out_form not in (0, 2) or E > slots:
        return INVALID
    first = [0] * B if table_first is None else list(table_first)
    if any(not 0 <= f <= slots - E for f in first):
        return INVALID
    if out_form == 0:
        if out_first < 0 or out_first + B * F > slots:
            return INVALID
        if any(f < out_first + B * F and out_first < f + E for f in first):
            return INVALID
    else:
        outs = list(out_wires)
        if len(outs) != B * F or any(not 0 <= w < wires for w in outs) or len(set(outs)) != len(outs):
            return INVALID
    return OK


# ---- 1. CPU -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_exported(tfhe):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read(), flags=re.S)
    lib = tfhe._lib.load()
    for name, nargs in NEW.items():
        m = re.search(rf"int32_t\s+{name}\s*\(([^)]*)\)", txt)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert m.group(1).lstrip().startswith("tfhe_ctx *ctx"), name
        assert name in tfhe._lib.ABI_SYMBOLS and hasattr(lib, name), name
    for method in ("tlwe_alloc", "tlwe_upload", "tlwe_download", "tgsw_update", "rot_net_level", "blind_rotate_level"):
        assert callable(getattr(tfhe.Engine, method)), method
    assert lib.tfhe_abi_version() == 7


def test_model_of_the_range_and_overlap_rules():
    ok = dict(slots=8, wires=10, N=64, acc_slot=[1, 1, 2], term_start=[0, 0, 1, 3], term_wire=[4, 5, 4], n_out=1, out_form=0, out_slot=[0, 3, 7], out_wires=None)
    assert model_blind_rotate_level(**ok) == OK
    for over in (dict(out_slot=[0, 3, 3]), dict(out_slot=[0, 3, 2]), dict(out_slot=[0, 3, 8]), dict(out_slot=[-1, 3, 4]), dict(acc_slot=[1, 8, 2]),
                 dict(term_wire=[4, 10, 4]), dict(term_start=[1, 1, 1, 3]), dict(term_start=[0, 2, 1, 3]), dict(n_out=2), dict(out_form=1), dict(n_out=0)):
        assert model_blind_rotate_level(**dict(ok, **over)) == INVALID, over
    ok2 = dict(ok, out_form=2, n_out=2, out_slot=None, out_wires=[0, 1, 2, 3, 6, 9])
    assert model_blind_rotate_level(**ok2) == OK
    for over in (dict(out_wires=[0, 1, 2, 3, 6, 6]), dict(out_wires=[0, 1, 2, 3, 6, 5]), dict(out_wires=[0, 1, 2, 3, 6, 10]), dict(n_out=32), dict(n_out=3),
                 dict(out_wires=[0, 1, 2])):
        assert model_blind_rotate_level(**dict(ok2, **over)) == INVALID, over
    assert model_blind_rotate_level(**dict(ok2, term_wire=[4, 5, 9], term_start=[0, 0, 1, 2])) == OK      # wire 9 is past term_start[B]
    net = dict(slots=16, wires=10, E=4, F=2, B=3, table_first=[0, 2, 1], out_form=0, out_first=6, out_wires=None)
    assert model_rot_net_level(**net) == OK
    for over in (dict(out_first=5), dict(out_first=11), dict(out_first=-1), dict(table_first=[0, 13, 1]), dict(table_first=[0, -1, 1]), dict(out_form=1),
                 dict(E=17), dict(table_first=[0, 2, 7], out_first=6), dict(table_first=None, out_first=3)):
        assert model_rot_net_level(**dict(net, **over)) == INVALID, over
    assert model_rot_net_level(**dict(net, table_first=None, out_first=4)) == OK
    assert model_rot_net_level(**dict(net, table_first=[8, 10, 12], out_first=0)) == OK       # outputs below every read range
    net2 = dict(net, out_form=2, out_wires=[9, 0, 3, 2, 1, 4])
    assert model_rot_net_level(**net2) == OK
    for over in (dict(out_wires=[9, 0, 3, 2, 1, 9]), dict(out_wires=[9, 0, 3, 2, 1, 10]), dict(out_wires=[9, 0, 3])):
        assert model_rot_net_level(**dict(net2, **over)) == INVALID, over


def test_form_rows_wraps_like_uint32():
    wires = np.array([[2**31 - 1, -2**31, 5], [-1, 3, 7]], np.int32)
    x = form_rows(wires, [0, 0, 2], [0, 1], [-3, 2**31 - 1], [11, -2**31])
    assert x[0].tolist() == [0, 0, 11]
    want = [(-3 * a + (2**31 - 1) * b) for a, b in zip(wires[0].tolist(), wires[1].tolist())]
    want[2] += -2**31
    assert x[1].tolist() == [((v + 2**31) % 2**32) - 2**31 for v in want]


# ---- 2. GPU: the setup --------------------------------------------------------------------------------------------------------------
SLOTS, WIRES, IN_WIRES = 16, 48, 12


def _setup(tfhe, N, k, l, beta, n, seed, table=True):
    """A key pair's engine with S = n + 2 selectors loaded, a TLWE table of SLOTS slots with samples in slots 0 ... 7 and a wire table
    of WIRES wires with rows in wires 0 ... IN_WIRES - 1; arbitrary words where the set is exact for any words, encryptions otherwise."""
    from tfhe_jl_amd import leveled
    p = _params(tfhe, N, k, l, beta, n=n)
    rng = np.random.default_rng(seed)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    S = n + 2
    if eng.get_option("exact_domain") == 2:
        tgsw = _words(rng, S, l, k + 1, k + 1, N)
        tgsw[0, 0, 0, 0, :] = 2**31 - 1
        tgsw[1, 0, 0, k, :] = -2**31
        tlwe = _words(rng, 8, k + 1, N)
        tlwe[0, :, :] = 2**31 - 1
        tlwe[1, :, :] = -2**31
    else:
        tgsw = leveled.tgsw_encrypt_bits(rng, sk, rng.integers(0, 2, S))
        tlwe = leveled.tlwe_encrypt(rng, sk, _words(rng, 8, N))
    wires = _words(rng, IN_WIRES, n + 1)
    half = 2**32 // (2 * N) // 2                     # the words just below and at a rounding boundary of decode_message(., 2N)
    wires[1, :6] = [2**31 - 1, -2**31, half - 1, half, -half - 1, -half]
    wires[4, n - 1] = 0                              # a skipped last step
    wires[4, n - 2] = 2**30                          # (the step before it is not)
    wires[4, n] = 3 * half - 1
    eng.tgsw_load(tgsw)
    if table:
        eng.tlwe_alloc(SLOTS)
        full = np.concatenate([tlwe, _words(rng, SLOTS - 8, k + 1, N)])
        eng.tlwe_upload(0, full)
        eng.wires_alloc(WIRES)
        allw = np.concatenate([wires, _words(rng, WIRES - IN_WIRES, n + 1)])
        eng.wires_upload(0, allw)
    else:
        full, allw = tlwe, wires
    return rng, sk, ck, eng, tgsw, full, allw


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mem_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    return free.value


# ---- 3. GPU: the table and the selector update --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", SETS)
def test_gpu_tlwe_table_partial_round_trip(tfhe, N, k, l, beta, n):
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9100 + N)
    assert np.array_equal(eng.tlwe_download(0, SLOTS), full)
    part = _words(rng, 3, k + 1, N)
    eng.tlwe_upload(5, part)
    want = full.copy()
    want[5:8] = part
    assert np.array_equal(eng.tlwe_download(4, 5), want[4:9])            # a partial range across the edited one
    assert np.array_equal(eng.tlwe_download(0, SLOTS), want)             # every untouched slot intact
    assert eng.tlwe_download(SLOTS, 0).shape == (0, k + 1, N)            # an empty range at the end of the table
    for first, count in ((-1, 1), (SLOTS, 1), (SLOTS - 1, 2), (0, -1)):
        with pytest.raises(tfhe.EngineError) as e:
            eng.tlwe_download(first, count)
        assert e.value.code == INVALID
    with pytest.raises(tfhe.EngineError) as e:
        eng.tlwe_upload(SLOTS - 2, part)
    assert e.value.code == INVALID and np.array_equal(eng.tlwe_download(0, SLOTS), want)
    eng.tlwe_alloc(4)                                                    # reallocating discards; the new table works
    eng.tlwe_upload(1, part)
    assert np.array_equal(eng.tlwe_download(1, 3), part)
    eng.tlwe_alloc(0)                                                    # freed
    with pytest.raises(tfhe.EngineError) as e:
        eng.tlwe_download(0, 1)
    assert e.value.code == STATE
    ck.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", SETS)
def test_gpu_tgsw_update_equals_a_fresh_load_of_the_edited_set(tfhe, N, k, l, beta, n):
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9200 + N, table=False)
    S = tgsw.shape[0]
    x = np.ascontiguousarray(np.repeat(full[3:4], S, axis=0))
    every = np.arange(S, dtype=np.int32)
    before = eng.extern_mul(x, every)
    new = tgsw[[S - 1, 0, 1]].copy()
    new[0, 0, 0, 0, :5] += 1
    eng.tgsw_update(2, new)                                              # selectors 2, 3, 4 of the middle
    after = eng.extern_mul(x, every)
    edited = tgsw.copy()
    edited[2:5] = new
    eng.tgsw_load(edited)
    fresh = eng.extern_mul(x, every)
    assert np.array_equal(after, fresh)
    untouched = [s for s in range(S) if not 2 <= s < 5]
    assert np.array_equal(after[untouched], before[untouched]) and not np.array_equal(after[2:5], before[2:5])
    for first, count in ((-1, 1), (S, 1), (S - 1, 2)):
        rc = eng._lib.tfhe_tgsw_update(eng._h, _ptr(new), first, count)
        assert rc == INVALID and "tgsw_update" in eng._lib.tfhe_last_error(eng._h).decode()
    assert eng._lib.tfhe_tgsw_update(eng._h, None, 0, 1) == INVALID and eng._lib.tfhe_tgsw_update(eng._h, _ptr(new), 0, 0) == INVALID
    assert np.array_equal(eng.extern_mul(x, every), fresh)
    raw = tfhe.Engine(ck.params)
    assert raw._lib.tfhe_tgsw_update(raw._h, _ptr(new), 0, 1) == NO_KEY
    raw.close()
    ck.close()


# ---- 4. GPU: blind_rotate_level against tfhe_blind_rotate_batch -----------------------------------------------------------------------
ACC_SLOT = np.array([3, 2, 3, 5, 4, 6, 0, 1], np.int32)                  # slot 3 twice; slots 0 and 1 hold the extreme words
OUT_SLOT = np.array([7, 8, 9, 15, 10, 12, 14, 11], np.int32)             # slot 13 is written by nobody
TERM_START = np.array([0, 0, 1, 4, 5, 6, 6, 7, 8], np.int32)
TERM_WIRE = np.array([1, 2, 3, 2, 4, 5, 6, 1], np.int32)                 # row 1: the planted wire; row 2: three terms, wire 2 twice
TERM_COEF = np.array([1, -3, -2**31, 2**31 - 1, 1, -1, 7, -2**31], np.int32)


def _level_rows(rng, allw):
    """Rows of 0 terms (every mask exponent zero), 1 term, 3 terms whose negative coefficients wrap, a skipped last step, a negated
    row, 0 terms and no constant (the trivial zero sample: a plain copy), and two more single terms on the extreme accumulators."""
    cst = _words(rng, len(ACC_SLOT))
    cst[5] = 0
    return cst, form_rows(allw, TERM_START, TERM_WIRE, TERM_COEF, cst)


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", SETS)
def test_gpu_blind_rotate_level_equals_the_batch_call(tfhe, N, k, l, beta, n):
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9300 + N)
    S, B = tgsw.shape[0], len(ACC_SLOT)
    cst, x = _level_rows(rng, allw)
    two_n = 2 * N
    exps = ((x.astype(np.int64) + 2**32 // two_n // 2) >> (32 - two_n.bit_length() + 1)) % two_n
    assert not exps[0, :n].any() and not exps[5].any() and list(exps[1, :6]) == [N, N, 0, 1, 2 * N - 1, 0] and exps[3, n - 1] == 0 and exps[3, n - 2] != 0
    perm = np.random.default_rng(5).permutation(S)[:n].astype(np.int32)
    assert len(set(perm.tolist())) == n
    for sel in (None, perm):
        # out_form 0: the final accumulators into their slots, every other slot as it was
        want = eng.blind_rotate(full, x, sel=sel, acc_index=ACC_SLOT, in_form=0, out_form=0)
        eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, sel=sel, out_form=0, out_slot=OUT_SLOT)
        assert eng.last_kernel_name() == f"tlwe_rotate_level_kernel(N={N},k={k},l={l},steps={n})"
        assert eng.last_rotation_count() == B and eng.last_timing_ms(0) > 0
        table = full.copy()
        table[OUT_SLOT] = want
        got = eng.tlwe_download(0, SLOTS)
        assert np.array_equal(got[OUT_SLOT], want), ("out_form 0", sel)
        assert np.array_equal(got, table) and np.array_equal(eng.wires_download(0, WIRES), allw)
        eng.tlwe_upload(0, full)
        # out_form 2: the keyswitched extractions into permuted wires, every other wire as it was
        for n_out in (1, 4):
            out_wires = (IN_WIRES + rng.permutation(WIRES - IN_WIRES)[:B * n_out]).astype(np.int32)
            want2 = eng.blind_rotate(full, x, sel=sel, acc_index=ACC_SLOT, in_form=0, n_out=n_out, out_form=2)
            eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, sel=sel, n_out=n_out, out_form=2, out_wires=out_wires)
            assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
            wtab = allw.copy()
            wtab[out_wires] = want2.reshape(B * n_out, n + 1)
            assert np.array_equal(eng.wires_gather(out_wires), want2.reshape(B * n_out, n + 1)), ("out_form 2", n_out, sel)
            assert np.array_equal(eng.wires_download(0, WIRES), wtab) and np.array_equal(eng.tlwe_download(0, SLOTS), full)
            eng.wires_upload(0, allw)
    # cst NULL: the rows without their constants
    x0 = form_rows(allw, TERM_START, TERM_WIRE, TERM_COEF, None)
    eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, sel=perm, out_form=0, out_slot=OUT_SLOT)
    assert np.array_equal(eng.tlwe_download(0, SLOTS)[OUT_SLOT], eng.blind_rotate(full, x0, sel=perm, acc_index=ACC_SLOT, in_form=0, out_form=0))
    # the spectrum accumulators in global memory change no word
    eng.tlwe_upload(0, full)
    eng.set_option("anyn_spec", 1)
    eng.blind_rotate_level(ACC_SLOT, TERM_START, TERM_WIRE, TERM_COEF, cst=cst, sel=perm, out_form=0, out_slot=OUT_SLOT)
    assert eng.last_kernel_name() == f"tlwe_rotate_level_kernel(N={N},k={k},l={l},steps={n},spec=global)"
    glob = eng.tlwe_download(0, SLOTS)
    eng.set_option("anyn_spec", -1)
    assert np.array_equal(glob[OUT_SLOT], want)                           # (want: the last out_form 0 of the loop, sel = perm)
    if N == 64:
        # ... and against the integer schoolbook itself
        ref = Rotation(N, k, l, beta, tgsw)
        for g in (1, 2, 3):
            assert np.array_equal(glob[OUT_SLOT[g]], ref.rotate_lwe(full[ACC_SLOT[g]], x[g], perm).astype(np.int32)), g
    ck.close()


# ---- 5. GPU: rot_net_level against tfhe_rot_net_batch ---------------------------------------------------------------------------------
def _two_level_net(leveled, N):
    """E = 4, widths (3, 2): a product with rotations 0 and 1, a rotated copy, a product with rotations N and 2N - 1; then a product of
    rotation 0 and a copy."""
    nodes = [(0, 1, 0, 0, 1), (2, 2, 1, 5, 5), (3, 1, 1, N, 2 * N - 1), (0, 2, 2, 0, 0), (1, 1, 0, 0, 0)]
    return leveled.RotNet([3, 2], nodes, N, entries=4, variables=3)


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", SETS)
def test_gpu_rot_net_level_equals_the_batch_call(tfhe, N, k, l, beta, n):
    from tfhe_jl_amd import leveled
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9400 + N)
    S = tgsw.shape[0]
    net = _two_level_net(leveled, N)
    first = np.array([0, 2, 1], np.int32)                                # different and overlapping read ranges
    B, E, F = 3, 4, 2
    sel = rng.integers(0, S, (B, 3)).astype(np.int32)
    data = np.stack([full[f:f + E] for f in first])
    want = eng.rot_net(data, net, sel, table_index=np.arange(B, dtype=np.int32), out_form=0)
    eng.rot_net_level(net, sel, table_first=first, out_form=0, out_first=8)
    assert eng.last_kernel_name().startswith("rot_net_level_kernel(")
    table = full.copy()
    table[8:8 + B * F] = want.reshape(B * F, k + 1, N)
    assert np.array_equal(eng.tlwe_download(0, SLOTS), table), "out_form 0"
    eng.tlwe_upload(0, full)
    out_wires = (IN_WIRES + rng.permutation(WIRES - IN_WIRES)[:B * F]).astype(np.int32)
    want2 = eng.rot_net(data, net, sel, table_index=np.arange(B, dtype=np.int32), out_form=2)
    eng.rot_net_level(net, sel, table_first=first, out_form=2, out_wires=out_wires)
    wtab = allw.copy()
    wtab[out_wires] = want2.reshape(B * F, n + 1)
    assert np.array_equal(eng.wires_download(0, WIRES), wtab) and np.array_equal(eng.tlwe_download(0, SLOTS), full), "out_form 2"
    eng.wires_upload(0, allw)
    # a packed lookup (a tree level, then rotations by -2^b) at absolute slots: table_first NULL
    depth = N.bit_length()                                               # log2 N + 1: two samples
    packed = leveled.packed_lookup_net(depth, N)
    assert packed.entries == 2 and packed.variables == depth <= S
    selp = np.stack([rng.permutation(S)[:depth] for _ in range(2)]).astype(np.int32)
    wantp = eng.rot_net(full[:2], packed, selp, out_form=0)
    eng.rot_net_level(packed, selp, out_form=0, out_first=SLOTS - 2)
    assert np.array_equal(eng.tlwe_download(SLOTS - 2, 2), wantp[:, 0]) and np.array_equal(eng.tlwe_download(0, SLOTS - 2), full[:SLOTS - 2])
    # a CMUX tree as the rotation-0 case: tfhe_cmux_tree_batch's words
    tree = leveled.tree_net(2)
    selt = rng.integers(0, S, (2, 2)).astype(np.int32)
    wantt = eng.cmux_tree(np.stack([full[2:6], full[3:7]]), selt, table_index=[0, 1], out_form=2)
    eng.rot_net_level(tree, selt, table_first=[2, 3], out_form=2, out_wires=[40, 13])
    assert np.array_equal(eng.wires_gather([40, 13]), wantt)
    ck.close()


# ---- 6. GPU: the chain on the device ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", SETS)
def test_gpu_chain_stays_on_the_device(tfhe, N, k, l, beta, n):
    """wires -> blind_rotate_level (into slots) -> rot_net_level (a depth-1 tree over two of those slots, into wires) -> a NAND level on
    those wires: the words of the same chain through the host-buffer calls."""
    from tfhe_jl_amd import leveled
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9500 + N)
    S = tgsw.shape[0]
    start, wire, coef = np.array([0, 1, 3, 4, 4], np.int32), np.array([7, 8, 9, 10], np.int32), np.array([1, 2, -1, 5], np.int32)
    cst = _words(rng, 4)
    acc = np.array([2, 3, 4, 5], np.int32)
    tree = leveled.tree_net(1)
    selt = np.array([[S - 1], [S - 2]], np.int32)
    # the host chain
    x = form_rows(allw, start, wire, coef, cst)
    stage1 = eng.blind_rotate(full, x, acc_index=acc, in_form=0, out_form=0)
    stage2 = eng.rot_net(stage1.reshape(2, 2, k + 1, N), leveled.RotNet(tree.widths, [(0, 1, 0, 0, 0)], N), selt, table_index=[0, 1], out_form=2)[:, 0]
    want = eng.gates(np.zeros(2, np.uint8), stage2, allw[[0, 1]])
    # the device chain: slots 8 ... 11, wires 20 and 21, wires 30 and 31
    eng.blind_rotate_level(acc, start, wire, coef, cst=cst, out_form=0, out_slot=[8, 9, 10, 11])
    eng.rot_net_level(tree, selt, table_first=[8, 10], out_form=2, out_wires=[20, 21])
    eng.gates_level(np.zeros(2, np.uint8), [20, 21], [0, 1], None, [30, 31])
    assert np.array_equal(eng.wires_gather([20, 21]), stage2)
    assert np.array_equal(eng.wires_gather([30, 31]), want)
    # ... and a level call queued behind an asynchronous level reads what that level wrote
    eng.gates_level(np.array([14, 14], np.uint8), [30, 31], None, None, [32, 33])          # COPY
    eng.blind_rotate_level([2], [0, 1], [32], [1], out_form=2, out_wires=[34])
    assert np.array_equal(eng.wires_gather([34])[0], eng.blind_rotate(full, want[:1], acc_index=[2], in_form=0, out_form=2)[0, 0])
    ck.close()


# ---- 7. GPU: refusals ---------------------------------------------------------------------------------------------------------------
class _Rotate:
    """A valid raw tfhe_blind_rotate_level call whose arguments can be replaced one at a time."""

    def __init__(self, eng):
        self.eng = eng
        self.args = dict(acc_slot=[1, 1, 2], term_start=[0, 0, 1, 3], term_wire=[4, 5, 4], term_coef=[1, -2, 3], cst=[5, 6, 7], sel=None, n_out=1, out_form=0,
                         out_slot=[8, 9, 10], out_wires=None, B=3)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        arr = {key: None if a[key] is None else np.asarray(a[key], np.int32) for key in ("acc_slot", "term_start", "term_wire", "term_coef", "cst", "sel", "out_slot", "out_wires")}
        rc = e._lib.tfhe_blind_rotate_level(e._h, _ptr(arr["acc_slot"]), _ptr(arr["term_start"]), _ptr(arr["term_wire"]), _ptr(arr["term_coef"]), _ptr(arr["cst"]),
                                            _ptr(arr["sel"]), a["n_out"], a["out_form"], _ptr(arr["out_slot"]), _ptr(arr["out_wires"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode(), a


class _Net:
    """The same for tfhe_rot_net_level, on the two-level network."""

    def __init__(self, eng, net, sel):
        self.eng, self.net = eng, net
        self.args = dict(table_first=[0, 2, 1], E=4, widths=net.widths, levels=net.levels, nodes=net.nodes, sel=sel, V=3, out_form=0, out_first=8, out_wires=None, B=3)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        arr = {key: None if a[key] is None else np.ascontiguousarray(a[key], np.int32) for key in ("table_first", "widths", "nodes", "sel", "out_wires")}
        rc = e._lib.tfhe_rot_net_level(e._h, _ptr(arr["table_first"]), a["E"], _ptr(arr["widths"]), a["levels"], _ptr(arr["nodes"]), _ptr(arr["sel"]), a["V"],
                                       a["out_form"], a["out_first"], _ptr(arr["out_wires"]), a["B"])
        return rc, e._lib.tfhe_last_error(e._h).decode(), a


@pytest.mark.gpu
def test_gpu_refusals_change_nothing_and_the_next_call_is_right(tfhe):
    from tfhe_jl_amd import leveled
    N, k, l, beta, n = SETS[0]
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9600)
    S = tgsw.shape[0]
    net = _two_level_net(leveled, N)
    sel = rng.integers(0, S, (3, 3)).astype(np.int32)
    rot, lvl = _Rotate(eng), _Net(eng, net, sel)
    a = rot.args
    x = form_rows(allw, a["term_start"], a["term_wire"], a["term_coef"], a["cst"])
    want_rot = eng.blind_rotate(full, x, acc_index=a["acc_slot"], in_form=0, out_form=0)
    want_net = eng.rot_net(np.stack([full[f:f + 4] for f in (0, 2, 1)]), net, sel, table_index=[0, 1, 2], out_form=0).reshape(6, k + 1, N)

    def unchanged_and_still_right():
        assert np.array_equal(eng.tlwe_download(0, SLOTS), full) and np.array_equal(eng.wires_download(0, WIRES), allw)
        assert rot()[0] == OK and np.array_equal(eng.tlwe_download(8, 3), want_rot)
        assert lvl()[0] == OK and np.array_equal(eng.tlwe_download(8, 6), want_net)
        eng.tlwe_upload(8, full[8:14])

    unchanged_and_still_right()
    assert rot(B=0)[0] == OK and lvl(B=0)[0] == OK
    rot_cases = [dict(out_slot=[8, 9, 9]), dict(out_slot=[8, 9, 2]), dict(out_slot=[8, 9, SLOTS]), dict(out_slot=[-1, 9, 10]), dict(acc_slot=[1, SLOTS, 2]),
                 dict(acc_slot=[1, -1, 2]), dict(term_wire=[4, WIRES, 4]), dict(term_wire=[4, -1, 4]), dict(term_start=[1, 1, 1, 3]), dict(term_start=[0, 2, 1, 3]),
                 dict(n_out=2), dict(n_out=0), dict(out_form=1), dict(out_form=3), dict(out_form=-1),
                 dict(out_form=2, out_wires=[20, 21, 21]), dict(out_form=2, out_wires=[20, 21, 5]), dict(out_form=2, out_wires=[20, 21, WIRES]),
                 dict(out_form=2, n_out=32, out_wires=list(range(12, 12 + 96))), dict(out_form=2, n_out=3, out_wires=list(range(12, 21)))]
    for over in rot_cases:
        rc, msg, args = rot(**over)
        model = model_blind_rotate_level(SLOTS, WIRES, N, args["acc_slot"], args["term_start"], args["term_wire"], args["n_out"], args["out_form"], args["out_slot"],
                                         args["out_wires"])
        assert rc == model == INVALID and msg.startswith("blind_rotate_level:"), (over, rc, model, msg)
        unchanged_and_still_right()
    assert "slot 9 written twice" in rot(out_slot=[8, 9, 9])[1] and "acc_slot[2] = 2 is an output slot" in rot(out_slot=[8, 9, 2])[1]
    assert "wire 21 written twice" in rot(out_form=2, out_wires=[20, 21, 21])[1] and "reads wire 5, which the same call writes" in rot(out_form=2, out_wires=[20, 21, 5])[1]
    for over in (dict(B=-1), dict(acc_slot=None), dict(term_start=None), dict(out_slot=None), dict(out_form=2), dict(term_wire=None), dict(term_coef=None),
                 dict(sel=[0, 1, 2, 3, 4, 5, S]), dict(sel=[0, 1, 2, 3, 4, 5, -1])):
        rc, msg, _ = rot(**over)
        assert rc == INVALID and msg.startswith("blind_rotate_level:"), (over, rc, msg)
    net_cases = [dict(out_first=5), dict(out_first=11), dict(out_first=-1), dict(table_first=[0, 13, 1]), dict(table_first=[0, -1, 1]), dict(out_form=1), dict(out_form=3),
                 dict(table_first=None, out_first=3), dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 20]), dict(out_form=2, out_wires=[20, 21, 22, 23, 24, WIRES]),
                 dict(out_form=2, out_wires=[20, 21, 22, 23, 24, -1])]
    for over in net_cases:
        rc, msg, args = lvl(**over)
        model = model_rot_net_level(SLOTS, WIRES, 4, 2, 3, args["table_first"], args["out_form"], args["out_first"], args["out_wires"])
        assert rc == model == INVALID and msg.startswith("rot_net_level:"), (over, rc, model, msg)
        unchanged_and_still_right()
    assert "meet the slots" in lvl(out_first=5)[1] and "wire 20 written twice" in lvl(out_form=2, out_wires=[20, 21, 22, 23, 24, 20])[1]
    bad_nodes = net.nodes.copy(); bad_nodes[3, 1] = 3
    bad_sel = sel.copy(); bad_sel[1, 1] = S
    for over in (dict(B=-1), dict(widths=None), dict(nodes=None), dict(sel=None), dict(E=0), dict(E=SLOTS + 1), dict(V=0), dict(levels=0), dict(nodes=bad_nodes),
                 dict(sel=bad_sel), dict(out_form=2)):
        rc, msg, _ = lvl(**over)
        assert rc == INVALID and msg.startswith("rot_net_level:"), (over, rc, msg)
    unchanged_and_still_right()
    # the state a level call needs, refused before the arguments are looked at
    eng.set_option("measure_margin", 1)
    assert rot(out_slot=[8, 9, 9])[0] == STATE and lvl(out_first=5)[0] == STATE
    eng.set_option("measure_margin", 0)
    unchanged_and_still_right()
    raw = tfhe.Engine(ck.params)
    raw.load_bootstrap_key(ck.bootstrap_key)
    for call in (rot, lvl):
        rc, msg, _ = call(eng=raw)
        assert rc == STATE and "no TLWE table" in msg, (rc, msg)
    raw.tlwe_alloc(SLOTS)
    raw.tlwe_upload(0, full)
    rc, msg, _ = rot(eng=raw)
    assert rc == STATE and "no wire table" in msg, (rc, msg)               # the call has terms
    rc, msg, _ = lvl(eng=raw, out_form=2, out_wires=[20, 21, 22, 23, 24, 25])
    assert rc == STATE and "no wire table" in msg, (rc, msg)
    rc, msg, _ = rot(eng=raw, term_start=[0, 0, 0, 0], out_slot=[8, 9, 9])
    assert rc == INVALID, (rc, msg)                                        # without terms no wire table is needed: the arguments come next
    for call, over in ((rot, dict(term_start=[0, 0, 0, 0])), (lvl, dict())):
        rc, msg, _ = call(eng=raw, **over)
        assert rc == NO_KEY and "tfhe_tgsw_load" in msg, (rc, msg)         # ... then the selector set
    raw.tgsw_load(tgsw)
    raw.wires_alloc(WIRES)
    raw.wires_upload(0, allw)
    for call, over in ((rot, dict(out_form=2, out_wires=[20, 21, 22])), (lvl, dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 25]))):
        rc, msg, _ = call(eng=raw, **over)
        assert rc == NO_KEY and "keyswitch" in msg, (rc, msg)
    assert np.array_equal(raw.tlwe_download(0, SLOTS), full) and np.array_equal(raw.wires_download(0, WIRES), allw)
    assert rot(eng=raw)[0] == OK and np.array_equal(raw.tlwe_download(8, 3), want_rot)       # forms that need no keyswitch key run
    raw.close()
    multi = ck.engine([0, 0])
    assert rot(eng=multi)[0] == STATE and lvl(eng=multi)[0] == STATE and multi._lib.tfhe_tlwe_alloc(multi._h, 4) == STATE
    assert multi._lib.tfhe_tgsw_update(multi._h, _ptr(tgsw), 0, 1) == STATE
    # an injected allocation failure: NOMEM, nothing written, and the context goes on working
    lib = eng._lib
    for call in (rot, lvl):
        assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
        rc, msg, _ = call()
        lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
        assert rc == NOMEM and "memory" in msg, (rc, msg)
        unchanged_and_still_right()
    ck.close()


@pytest.mark.gpu
def test_gpu_multikey_context_refuses_the_tlwe_table(tfhe):
    from test_independent import _mk_setup
    p, sks, ck, xs, ys, want = _mk_setup(tfhe, 2, 4, 7, 3, 405)
    eng = ck.engine(0)
    one = np.zeros(1, np.int32)
    lib, h = eng._lib, eng._h
    assert lib.tfhe_tlwe_alloc(h, 4) == STATE and "multi-key" in lib.tfhe_last_error(h).decode()
    assert lib.tfhe_tlwe_upload(h, 0, 0, None) == STATE and lib.tfhe_tlwe_download(h, 0, 0, None) == STATE
    assert lib.tfhe_tgsw_update(h, _ptr(one), 0, 1) == STATE
    assert lib.tfhe_blind_rotate_level(h, _ptr(one), _ptr(np.zeros(2, np.int32)), None, None, None, None, 1, 0, _ptr(one), None, 1) == STATE
    widths, nodes = np.ones(1, np.int32), np.zeros(5, np.int32)
    assert lib.tfhe_rot_net_level(h, None, 1, _ptr(widths), 1, _ptr(nodes), _ptr(one), 1, 0, 1, None, 1) == STATE
    assert np.array_equal(eng.mk_gate_nand(xs, ys), want)               # the context still runs its own gates
    ck.close()


@pytest.mark.gpu
def test_gpu_oversized_tlwe_alloc_is_refused_before_allocating(tfhe):
    """2^31 - 1 slots of 512 bytes are a terabyte: TFHE_ERR_NOMEM with hipMemGetInfo unchanged, the present table kept."""
    N, k, l, beta, n = SETS[0]
    rng, sk, ck, eng, tgsw, full, allw = _setup(tfhe, N, k, l, beta, n, 9700)
    before = _mem_free()
    with pytest.raises(tfhe.EngineError) as e:
        eng.tlwe_alloc(2**31 - 1)
    assert e.value.code == NOMEM and "free memory" in str(e.value)
    assert _mem_free() == before
    assert eng._lib.tfhe_tlwe_alloc(eng._h, -1) == INVALID and eng._lib.tfhe_tlwe_alloc(eng._h, 2**31) == INVALID
    assert np.array_equal(eng.tlwe_download(0, SLOTS), full)
    eng.blind_rotate_level([2], [0, 0], [], [], out_form=0, out_slot=[9])                   # a row without terms or constant: a copy
    assert np.array_equal(eng.tlwe_download(9, 1)[0], full[2])
    ck.close()
