"""Multi-key gate set (tfhe_mk_gates_batch): every opcode of gates.jl over multi-key samples.

Expected words come from a helper built on the oracle's exported multi-key pieces: the gates.jl affine prologue in numpy,
then orc_mk_bootstrap_wo_keyswitch (mu = 1/8) and orc_mk_keyswitch; MUX sums its two extracted samples and adds 1/8 to b
before the one keyswitch (gates.jl:163-177).  CPU: the helper's NAND is the oracle's mk_gate_nand word for word and every
opcode decrypts to its truth table.  GPU: the engine equals the helper word for word (decrypt-level multi-key checks are
~0.2 %/gate flaky, SURVEY §4, so parity is asserted on words)."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import DEVICE_PAIRS
from test_mk import MKKeys, _mk_setup

OPS = dict(NAND=0, OR=1, AND=2, XOR=3, XNOR=4, NOT=5, NOR=6, ANDNY=7, ANDYN=8, ORNY=9, ORYN=10,
           MUX=11, CONST0=12, CONST1=13, COPY=14)
P8, P4 = 1 << 29, 1 << 30          # encode_message(1, 8), encode_message(1, 4)
# gates.jl: b constant, sign of x, sign of y, the (x + y) * 2 form of XOR / XNOR
FORMS = {
    OPS["NAND"]: (P8, -1, -1, False), OPS["OR"]: (P8, 1, 1, False), OPS["AND"]: (-P8, 1, 1, False),
    OPS["XOR"]: (P4, 1, 1, True), OPS["XNOR"]: (-P4, -1, -1, True), OPS["NOR"]: (-P8, -1, -1, False),
    OPS["ANDNY"]: (-P8, -1, 1, False), OPS["ANDYN"]: (-P8, 1, -1, False), OPS["ORNY"]: (P8, -1, 1, False),
    OPS["ORYN"]: (P8, 1, -1, False),
}
TRUTH = {
    OPS["NAND"]: lambda x, y, z: not (x and y), OPS["OR"]: lambda x, y, z: x or y, OPS["AND"]: lambda x, y, z: x and y,
    OPS["XOR"]: lambda x, y, z: x != y, OPS["XNOR"]: lambda x, y, z: x == y, OPS["NOT"]: lambda x, y, z: not x,
    OPS["NOR"]: lambda x, y, z: not (x or y), OPS["ANDNY"]: lambda x, y, z: (not x) and y,
    OPS["ANDYN"]: lambda x, y, z: x and not y, OPS["ORNY"]: lambda x, y, z: (not x) or y,
    OPS["ORYN"]: lambda x, y, z: x or not y, OPS["MUX"]: lambda x, y, z: y if x else z,
    OPS["CONST0"]: lambda x, y, z: False, OPS["CONST1"]: lambda x, y, z: True, OPS["COPY"]: lambda x, y, z: x,
}


def _wrap(v):
    return (np.asarray(v, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _affine(cst, sx, sy, mul2, x, y):
    x, y = x.astype(np.int64), y.astype(np.int64)
    t = 2 * (x + y) * sx if mul2 else sx * x + sy * y
    t[-1] += cst
    return _wrap(t)


class MKGateRef:
    """Multi-key gates on the CPU from the oracle library's exported multi-key bootstrap and keyswitch."""

    def __init__(self, orc, o, threads=8):
        self.lib, self.o, self.threads = orc.lib(), o, threads
        self.Pn, self.n, self.N = o.parties, o.n, o.N

    def _bootstrap(self, t):
        """bootstrap_wo_keyswitch of one prologue result, mu = 1/8 -> extracted sample [P N + 1]"""
        t = np.ascontiguousarray(t, np.int32)
        u = np.zeros(self.Pn * self.N + 1, np.int32)
        m = C.c_double(0)
        o = self.o
        rc = self.lib.orc_mk_bootstrap_wo_keyswitch(C.byref(o.P), C.c_int32(self.Pn), o.bk_re.ctypes.data_as(C.c_void_p),
                                                    o.bk_im.ctypes.data_as(C.c_void_p), o.bk_i32.ctypes.data_as(C.c_void_p),
                                                    C.c_int32(0), C.c_int32(P8), t.ctypes.data_as(C.c_void_p),
                                                    u.ctypes.data_as(C.c_void_p), C.byref(m))
        assert rc == 0
        return u

    def _keyswitch(self, u):
        u = np.ascontiguousarray(u, np.int32)
        out = np.zeros(self.Pn * self.n + 1, np.int32)
        self.lib.orc_mk_keyswitch(C.byref(self.o.P), C.c_int32(self.Pn), self.o.ks.ctypes.data_as(C.c_void_p),
                                  u.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out

    def gate(self, op, x, y=None, z=None):
        w = self.Pn * self.n + 1
        if op == OPS["NOT"]:
            return _wrap(-np.asarray(x, np.int64))
        if op == OPS["COPY"]:
            return np.array(x, np.int32)
        if op in (OPS["CONST0"], OPS["CONST1"]):
            out = np.zeros(w, np.int32)
            out[-1] = P8 if op == OPS["CONST1"] else -P8
            return out
        if op == OPS["MUX"]:
            u1 = self._bootstrap(_affine(-P8, 1, 1, False, x, y))        # AND(x, y)       gates.jl:166
            u2 = self._bootstrap(_affine(-P8, -1, 1, False, x, z))       # AND(NOT x, z)   gates.jl:170
            u = u1.astype(np.int64) + u2
            u[-1] += P8                                                  # gates.jl:174
            return self._keyswitch(_wrap(u))
        return self._keyswitch(self._bootstrap(_affine(*FORMS[op], x, y)))

    def batch(self, ops, in0, in1=None, in2=None):
        ops = np.asarray(ops, np.uint8)
        row = lambda a, g: None if a is None else np.asarray(a[g], np.int32)
        with ThreadPoolExecutor(self.threads) as ex:       # (ctypes releases the GIL; the oracle's scratch is per thread)
            rows = list(ex.map(lambda g: self.gate(int(ops[g]), row(in0, g), row(in1, g), row(in2, g)), range(ops.size)))
        return np.stack(rows) if rows else np.zeros((0, self.Pn * self.n + 1), np.int32)


def _rotations(ops):
    ops = np.asarray(ops)
    return int(sum(2 if op == OPS["MUX"] else 0 if op in (OPS["NOT"], OPS["COPY"], OPS["CONST0"], OPS["CONST1"]) else 1
                   for op in ops))


@pytest.fixture(scope="module")
def mk_small(tfhe, orc):
    return MKKeys(tfhe, orc, n=24)


@pytest.fixture(scope="module")
def mk_full(tfhe, orc):
    return MKKeys(tfhe, orc)


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_helper_nand_equals_oracle(orc, tfhe, mk_small):
    K = mk_small
    x = tfhe.mk_encrypt(K.rng, K.sks, [True, False, True])
    y = tfhe.mk_encrypt(K.rng, K.sks, [True, True, False])
    z = K.rng.integers(-2**31, 2**31, size=(2, x.shape[1]), dtype=np.int64).astype(np.int32)
    z[0, :4] = [2**31 - 1, -2**31, 2**20, 0]
    a, b = np.concatenate([x, z]), np.concatenate([y, z[::-1]])
    ref = MKGateRef(orc, K.oracle)
    assert np.array_equal(ref.batch(np.zeros(len(a), np.uint8), a, b), K.oracle.mk_gate_nand(a, b))


def test_helper_truth_tables(orc, tfhe, mk_small):
    """Every opcode on every input combination, 2 parties, n = 24, fixed seed: the helper's outputs decrypt to gates.jl's truth
    tables (XOR / XNOR double signal and noise together, so their margin is NAND's)."""
    K = mk_small
    combos = [(x, y, z) for x in (False, True) for y in (False, True) for z in (False, True)]
    ops = np.repeat(np.arange(15, dtype=np.uint8), len(combos))
    bits = np.array(combos * 15, bool)
    enc = [tfhe.mk_encrypt(K.rng, K.sks, bits[:, i]) for i in range(3)]
    got = tfhe.mk_decrypt(K.sks, MKGateRef(orc, K.oracle).batch(ops, *enc))
    want = np.array([TRUTH[int(op)](*b) for op, b in zip(ops, bits)])
    bad = [(int(op), tuple(b)) for op, b, g, w in zip(ops, bits, got, want) if g != w]
    assert not bad, bad


def test_new_symbols_exported_and_null_context(tfhe):
    lib = tfhe._lib.load()
    for s in ("tfhe_mk_gates_batch", "tfhe_mk_wires_alloc", "tfhe_mk_gates_level"):
        assert s in tfhe._lib.ABI_SYMBOLS
        assert hasattr(lib, s)
    ops = np.zeros(1, np.uint8)
    row = np.zeros((1, 1001), np.int32)
    idx = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tfhe_mk_gates_batch(None, p(ops), p(row), p(row), None, p(row), 1) == 1
    assert lib.tfhe_mk_wires_alloc(None, 4) == 1
    assert lib.tfhe_mk_gates_level(None, p(ops), p(idx), p(idx), None, p(idx), 1) == 1
    for name in ("mk_gate_or", "mk_gate_and", "mk_gate_xor", "mk_gate_xnor", "mk_gate_nor", "mk_gate_andny", "mk_gate_andyn",
                 "mk_gate_orny", "mk_gate_oryn", "mk_gate_mux", "mk_gate_not", "mk_gate_constant", "mk_gates_batch"):
        assert callable(getattr(tfhe, name)) and name in tfhe.__all__


# ---- GPU ------------------------------------------------------------------------------------------------------------

def _mixed_batch(tfhe, rng, sks, width):
    """All 15 opcodes on encryptions of every input pattern, then on arbitrary words with mod-switch edges planted."""
    ops = np.concatenate([np.arange(15, dtype=np.uint8)] * 2)
    bits = rng.integers(0, 2, size=(ops.size // 2, 3)).astype(bool)
    enc = [tfhe.mk_encrypt(rng, sks, bits[:, i]) for i in range(3)]
    raw = [rng.integers(-2**31, 2**31, size=(ops.size // 2, width), dtype=np.int64).astype(np.int32) for _ in range(3)]
    raw[0][0, :4] = [2**31 - 1, -2**31, 2**20, 0]
    raw[1][3, -4:] = [0, -2**31, 2**31 - 1, 1 << 21]
    return ops, [np.concatenate([e, r]) for e, r in zip(enc, raw)], bits


@pytest.mark.gpu
def test_mk_gates_all_opcodes_full_size(orc, tfhe, mk_full):
    K = mk_full
    ops, ins, bits = _mixed_batch(tfhe, K.rng, K.sks, 1001)
    want = MKGateRef(orc, K.oracle).batch(ops, *ins)
    eng = K.ck.engine(0)
    got = eng.mk_gates_batch(ops, *ins)
    assert eng.last_kernel_name().startswith("mk_blind_rotate_kernel_w2")
    assert eng.last_rotation_count() == _rotations(ops)
    assert np.array_equal(got, want)
    half = ops.size // 2
    truth = np.array([TRUTH[int(op)](*b) for op, b in zip(ops[:half], bits)])
    assert (tfhe.mk_decrypt(K.sks, got[:half]) == truth).sum() >= half - 1
    eng.set_option("mk_general", 1)
    try:
        got = eng.mk_gates_batch(ops, *ins)
        assert eng.last_kernel_name().startswith("mk_blind_rotate_kernel_general")
        assert eng.last_rotation_count() == _rotations(ops)
        assert np.array_equal(got, want)
    finally:
        eng.set_option("mk_general", 0)
    # the Python gate functions: flat in, flat out; matrix in, matrix out
    x, y, z = (a[:3] for a in ins)
    assert np.array_equal(tfhe.mk_gate_xor(K.ck, x[0], y[0]), MKGateRef(orc, K.oracle).gate(OPS["XOR"], x[0], y[0]))
    m = tfhe.mk_gate_mux(K.ck, x, y, z)
    assert m.shape == (3, 1001) and np.array_equal(m, MKGateRef(orc, K.oracle).batch([OPS["MUX"]] * 3, x, y, z))
    c1 = tfhe.mk_gate_constant(K.ck, True)
    assert c1.shape == (1001,) and not c1[:-1].any() and c1[-1] == P8
    assert np.array_equal(tfhe.mk_gate_not(K.ck, x[1]), _wrap(-x[1].astype(np.int64)))


@pytest.mark.gpu
@pytest.mark.parametrize("which,parties,n", [("4party", 4, 12), ("4party", 3, 12), ("8party", 8, 6)])
def test_mk_gates_many_parties(orc, tfhe, which, parties, n):
    base = getattr(tfhe, "mktfhe_parameters_" + which)
    p, rng, sks, ck, o = _mk_setup(tfhe, orc, base, parties, n, seed=70 + parties)
    ops, ins, _ = _mixed_batch(tfhe, rng, sks, parties * n + 1)
    sel = np.r_[0:15, 18:27]                # every opcode on encryptions, then XOR .. MUX on arbitrary words
    ops, ins = ops[sel], [a[sel] for a in ins]
    eng = ck.engine(0)
    got = eng.mk_gates_batch(ops, *ins)
    assert eng.last_rotation_count() == _rotations(ops)
    assert np.array_equal(got, MKGateRef(orc, o).batch(ops, *ins))
    ck.close()


@pytest.mark.gpu
def test_mk_gates_nand_equals_nand_batch(tfhe, mk_full):
    K = mk_full
    x = tfhe.mk_encrypt(K.rng, K.sks, K.rng.integers(0, 2, 12).astype(bool))
    y = tfhe.mk_encrypt(K.rng, K.sks, K.rng.integers(0, 2, 12).astype(bool))
    eng = K.ck.engine(0)
    assert np.array_equal(eng.mk_gates_batch(np.zeros(12, np.uint8), x, y), eng.mk_gate_nand(x, y))


@pytest.mark.gpu
def test_mk_gates_error_paths(orc, tfhe, keys80):
    """Each misuse returns its documented code, and the context then still runs a gate correctly."""
    lib = tfhe._lib.load()
    base = tfhe.mktfhe_parameters_4party
    p, rng, sks, ck, o = _mk_setup(tfhe, orc, base, 4, 8, seed=91)
    eng = ck.engine(0)
    ref = MKGateRef(orc, o)
    x, y, z = (tfhe.mk_encrypt(rng, sks, [True, False]) for _ in range(3))
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)

    def still_works(e, r, x, y):
        assert np.array_equal(e.mk_gates_batch(np.array([OPS["XOR"]] * 2, np.uint8), x, y), r.batch([OPS["XOR"]] * 2, x, y))

    # a multi-key entry point on a single-key context
    sk_eng = keys80.ck.engine(0)
    w = np.zeros((1, keys80.params.lwe_size + 1), np.int32)
    assert lib.tfhe_mk_gates_batch(sk_eng._h, ptr(np.zeros(1, np.uint8)), ptr(w), ptr(w), None, ptr(w), 1) == 5
    assert lib.tfhe_mk_wires_alloc(sk_eng._h, 4) == 5
    assert np.array_equal(tfhe.gate_nand(keys80.ck, tfhe.LweSampleArray(w), tfhe.LweSampleArray(w)).data,
                          keys80.oracle.gates(np.zeros(1, np.uint8), w, w))
    # a multi-key level without a table
    one = np.zeros(1, np.int32)
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_gates_level(np.array([OPS["NAND"]], np.uint8), one, one, None, one + 1)
    assert e.value.code == 5
    still_works(eng, ref, x, y)
    # a single-key table given to tfhe_mk_gates_level
    eng.wires_alloc(4)
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_gates_level(np.array([OPS["NAND"]], np.uint8), one, one, None, one + 1)
    assert e.value.code == 5
    # a MUX without a third operand (level and batch)
    eng.mk_wires_alloc(6)
    eng.wires_upload(0, np.concatenate([x, y]))
    assert lib.tfhe_mk_gates_level(eng._h, ptr(np.array([OPS["MUX"]], np.uint8)), ptr(one), ptr(one + 1), None, ptr(one + 4), 1) == 1
    assert lib.tfhe_mk_gates_batch(eng._h, ptr(np.array([OPS["MUX"]], np.uint8)), ptr(x[:1]), ptr(y[:1]), None, ptr(x[:1].copy()), 1) == 1
    # a wire written twice in one level; a level that reads a wire it also writes
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_gates_level(np.array([OPS["AND"], OPS["OR"]], np.uint8), [0, 1], [2, 3], None, [4, 4])
    assert e.value.code == 1
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_gates_level(np.array([OPS["AND"], OPS["OR"]], np.uint8), [0, 4], [2, 3], None, [4, 5])
    assert e.value.code == 1
    # ... the table still runs a level correctly
    eng.mk_gates_level(np.array([OPS["XOR"], OPS["MUX"]], np.uint8), [0, 0], [2, 1], [0, 3], [4, 5])
    assert np.array_equal(eng.wires_download(4, 2), ref.batch([OPS["XOR"], OPS["MUX"]], x[[0, 0]], np.stack([y[0], x[1]]), np.stack([x[0], y[1]])))
    # a table allocated for 4 parties after the keys are reloaded for 3
    sub = tfhe.MKCloudKey(ck._parts[:3])
    eng.mk_load_bootstrap_key(sub.bootstrap_key, 3)
    eng.mk_load_keyswitch_key(sub.keyswitch_key, 3)
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_gates_level(np.array([OPS["NAND"]], np.uint8), [0], [1], None, [4])
    assert e.value.code == 5
    o3 = orc.Oracle(p.lwe_size, 1024, 1, p.bs_decomp_length, p.bs_log2_base, p.ks_decomp_length, p.ks_log2_base, parties=3)
    o3.load_bootstrap_key(sub.bootstrap_key)
    o3.load_keyswitch_key(sub.keyswitch_key)
    x3, y3 = (tfhe.mk_encrypt(rng, sks[:3], [True, False]) for _ in range(2))
    still_works(eng, MKGateRef(orc, o3), x3, y3)
    ck.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", DEVICE_PAIRS)
def test_mk_gates_two_devices(orc, tfhe, mk_full, devices):
    """A multi-device context splits the batch by rotations and gives the one-device words."""
    K = mk_full
    ops, ins, _ = _mixed_batch(tfhe, K.rng, K.sks, 1001)
    one = K.ck.engine(0).mk_gates_batch(ops, *ins)
    eng = K.ck.engine(devices)
    assert np.array_equal(eng.mk_gates_batch(ops, *ins), one)
    assert eng.last_rotation_count() == _rotations(ops)


@pytest.mark.gpu
@pytest.mark.parametrize("which,parties,n", [("2party", 2, 24), ("4party", 3, 12)])
def test_mk_keyswitch_families_agree(orc, tfhe, which, parties, n):
    """The three keyswitch families under a multi-key keyswitch key, through every multi-key caller of the keyswitch launch.
    Keyswitching is exact integer arithmetic in all three, so the tiled integer kernel (ks_variant 3) and the gather kernel (1)
    equal the int8 MFMA default (4, anchored to the references by the tests above) word for word.  Every shipped multi-key set has
    base 4, t = 8, N = 1024, so each variant really gets its own family.  One engine per variant, the option set before the key
    is loaded:
      (a) mk_gates_batch of 19 gates, half of the operand rows encryptions and half arbitrary words: NOT, COPY and CONST1 are
          trivial, the other 16 fill one 16-sample tile of the tiled kernel; the MUXes take the two-operand (e1) path; with
          three parties the third chains the body word a second time;
      (b) the same gates as one mk_gates_level on a multi-key wire table, output wires distinct and in reverse order (dst);
      (c) mk_bootstrap_tv_multi, 3 rows, n_out = 2, with keyswitch: the source is tv_ext, 6 samples in a partly filled tile;
      (d) mk_gate_nand of the 19 rows: 19 samples cross the 16-sample tile and leave a partly filled one.
    (b) equals (a); the NAND rows of (a) and all of (d) equal Oracle.mk_gate_nand."""
    base = getattr(tfhe, "mktfhe_parameters_" + which)
    p, rng, sks, ck, o = _mk_setup(tfhe, orc, base, parties, n, seed=130 + parties)
    w = parties * n + 1
    names = ["NAND", "MUX", "XOR", "NOT", "COPY", "CONST1", "AND", "NAND", "XOR", "AND",
             "NAND", "MUX", "XOR", "AND", "NAND", "XOR", "AND", "NAND", "XOR"]
    ops = np.array([OPS[s] for s in names], np.uint8)
    B, half = ops.size, 10
    assert B == 19 and names.count("MUX") == 2
    ins = []
    for _ in range(3):
        enc = tfhe.mk_encrypt(rng, sks, rng.integers(0, 2, half).astype(bool))
        raw = rng.integers(-2**31, 2**31, size=(B - half, w), dtype=np.int64).astype(np.int32)
        ins.append(np.concatenate([enc, raw]))
    ins[0][half, :4] = [2**31 - 1, -2**31, 2**20, 0]
    tables = rng.integers(-2**31, 2**31, size=(2, 1024), dtype=np.int64).astype(np.int32)
    tv_rows, tv_index = ins[0][[0, 1, half]], np.array([0, 1, 0], np.int32)
    out_wires = np.arange(3 * B, 4 * B, dtype=np.int32)[::-1].copy()

    got = {}
    for variant in (4, 3, 1):
        eng = tfhe._lib.Engine(p, 0)
        try:
            eng.set_option("ks_variant", variant)
            eng.mk_load_bootstrap_key(ck.bootstrap_key, parties)
            eng.mk_load_keyswitch_key(ck.keyswitch_key, parties)
            a = eng.mk_gates_batch(ops, *ins)
            assert eng.last_rotation_count() == _rotations(ops)
            eng.mk_wires_alloc(4 * B)
            eng.wires_upload(0, np.concatenate(ins))
            idx = np.arange(B, dtype=np.int32)
            eng.mk_gates_level(ops, idx, idx + B, idx + 2 * B, out_wires)
            b = eng.wires_gather(out_wires)
            c = eng.mk_bootstrap_tv_multi(tables, tv_rows, 2, tv_index, with_keyswitch=True)
            d = eng.mk_gate_nand(ins[0], ins[1])
            got[variant] = (a, b, c, d)
        finally:
            eng.close()
    ck.close()

    for variant in (3, 1):
        for part, x, y in zip("abcd", got[variant], got[4]):
            assert x.shape == y.shape and np.array_equal(x, y), (variant, part)
    a, b, c, d = got[4]
    assert c.shape == (3, 2, w)
    assert np.array_equal(b, a)
    nand = np.flatnonzero(ops == OPS["NAND"])
    assert nand.size == 5
    want = o.mk_gate_nand(ins[0], ins[1])
    assert np.array_equal(a[nand], want[nand])
    assert np.array_equal(d, want)
