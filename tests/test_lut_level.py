"""Programmable bootstrapping on the device-resident wire table: tfhe_lut_level / tfhe_linear_level, Engine.lut_level / linear_level,
and the integer nodes of Circuit (lut, lut_multi, linear).

CPU: the entry points in the header, ABI_SYMBOLS and the library; levelisation, folding of linear nodes, table sharing and the level
arrays of run / run_batch; Circuit's argument errors.  GPU: word for word against the host-buffer path (bootstrap_tv /
bootstrap_tv_multi of the same combinations formed in numpy) and, for one small case, against tests/pbs_ref/pbs_ref.c; the linear
level; staging of the caller's arrays; the 16-bit LUT adder as a circuit; a mixed LUT / gate circuit; multi-device contexts; every
error path."""
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import DEVICE_PAIRS, KeySet
from test_pbs_multi import _p, _set, _words, checkers, small80  # noqa: F401  (session fixtures shared with the PBS tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_NO_KEY, ERR_STATE = 1, 3, 5


def _wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) % 2**32 - 2**31).astype(np.int32)


def _adder_module():
    spec = importlib.util.spec_from_file_location("lut_adder_example", os.path.join(ROOT, "examples", "lut_adder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_exist(tfhe):
    from tfhe_jl_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read()
    assert re.search(r"int32_t tfhe_lut_level\(tfhe_ctx \*ctx, const int32_t \*tv, int32_t n_tv, const int32_t \*tv_index, int32_t n_out,\s+"
                     r"const int32_t \*term_start, const int32_t \*term_wire, const int32_t \*term_coef, const int32_t \*cst,\s+"
                     r"const int32_t \*out, int64_t B\);", header)
    assert re.search(r"int32_t tfhe_linear_level\(tfhe_ctx \*ctx, const int32_t \*term_start, const int32_t \*term_wire, const int32_t \*term_coef,\s+"
                     r"const int32_t \*cst, const int32_t \*out, int64_t B\);", header)
    lib = L.load()
    for name in ("tfhe_lut_level", "tfhe_linear_level"):
        assert name in L.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.tfhe_abi_version() == 7 and L.ABI_VERSION == 7
    assert callable(tfhe.Engine.lut_level) and callable(tfhe.Engine.linear_level)
    for name in ("lut", "lut_multi", "linear", "level_plan"):
        assert callable(getattr(tfhe.Circuit, name))
    assert tfhe.GATE_BIT_TO_Z2 == 1 << 30 and "make_gate_test_vector" in tfhe.__all__


def test_levels_folding_and_tables(tfhe):
    from tfhe_jl_amd.lut import make_multi_test_vector, make_test_vector
    c = tfhe.Circuit()
    x, y, z = c.inputs(3)
    f, g = (lambda m: (m + 1) % 8), (lambda m: m // 2)
    lin = c.linear([(x, 3), (y, -1)], const=5)
    lin2 = c.linear([(lin, 2**31 + 1), z], const=2**31)        # folds through lin: coefficients composed mod 2^32
    u = c.lut(f, [lin2, (x, 2**31)], 8)
    v = c.lut(f, [lin], 8)                                      # same (f, p, q): one table
    w = c.lut(g, [(z, 4)], 8, q=16)
    m0, m1 = c.lut_multi([f, g], [u, v], 4, 8, const=-7)
    gate = c.nand(lin, u)
    c.set_outputs([gate, m0, m1, w])
    assert [c._level[wr] for wr in (lin, lin2, u, v, w, m0, m1, gate)] == [1, 1, 1, 1, 1, 2, 2, 2]
    # lin2 = (2^31 + 1)(3x - y + 5) + z + 2^31 = (2^31 + 3) x + (2^31 - 1) y + z + (2^31 + 5 + 2^31) mod 2^32
    assert c._linear[lin2] == ({x: (3 * (2**31 + 1)) % 2**32, y: (-(2**31 + 1)) % 2**32, z: 1}, (5 * (2**31 + 1) + 2**31) % 2**32)
    # u's terms: lin2's plus 2^31 x: x's coefficient 2^31 + 3 + 2^31 = 3
    plan = c.level_plan(1024)
    assert len(plan) == 2
    (K1, tv1, idx1, st1, tw1, tc1, cs1, o1), = plan[0]["lut"]
    assert K1 == 1 and tv1.shape == (2, 1024)
    assert np.array_equal(tv1[0], make_test_vector(f, 8, 1024)) and np.array_equal(tv1[1], make_test_vector(g, 8, 1024, 16))
    assert idx1.tolist() == [0, 0, 1] and o1.tolist() == [u, v, w]
    assert st1.tolist() == [0, 3, 5, 6]
    assert tw1.tolist() == [x, y, z, x, y, z]
    assert tc1.tolist() == _wrap32([3, 2**31 - 1, 1, 3, -1, 4]).tolist()
    assert cs1.tolist() == _wrap32([(5 * (2**31 + 1) + 2**31) % 2**32, 5, 0]).tolist()
    # lin is read by a gate: computed; lin2 is read only by a LUT: folded, never computed
    assert plan[0]["linear"][4].tolist() == [lin] and plan[0]["gates"] is None
    ops, a, b, cc, out = plan[1]["gates"]
    assert ops.tolist() == [tfhe.OPCODES["NAND"]] and a.tolist() == [lin] and b.tolist() == [u] and out.tolist() == [gate]
    (K2, tv2, idx2, st2, tw2, tc2, cs2, o2), = plan[1]["lut"]
    assert K2 == 2 and np.array_equal(tv2[0], make_multi_test_vector([f, g], 4, 1024, 8))
    assert tw2.tolist() == [u, v] and tc2.tolist() == [1, 1] and cs2.tolist() == [-7] and o2.tolist() == [m0, m1]
    assert plan[1]["linear"] is None
    # run_batch: wire w of instance i is row w M + i, instance fastest; outputs of a K-output row grouped per row
    M = 3
    pb = c.level_plan(1024, M)
    K, tv, idx, st, tw, tc, cs, o = pb[0]["lut"][0]
    assert idx.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1]
    assert st.tolist() == [0, 3, 6, 9, 11, 13, 15, 16, 17, 18]
    assert tw[:9].tolist() == [x * M, y * M, z * M, x * M + 1, y * M + 1, z * M + 1, x * M + 2, y * M + 2, z * M + 2]
    assert tc[:3].tolist() == tc1[:3].tolist() and tc[3:6].tolist() == tc1[:3].tolist()
    assert o.tolist() == [u * M, u * M + 1, u * M + 2, v * M, v * M + 1, v * M + 2, w * M, w * M + 1, w * M + 2]
    assert cs.tolist() == np.repeat(cs1, M).tolist()
    o2 = pb[1]["lut"][0][7]
    assert o2.tolist() == [m0 * M, m1 * M, m0 * M + 1, m1 * M + 1, m0 * M + 2, m1 * M + 2]
    gm = pb[1]["gates"]
    assert gm[1].tolist() == [lin * M + i for i in range(M)] and gm[4].tolist() == [gate * M + i for i in range(M)]


def test_gate_only_circuit_plan_is_the_gate_arrays(tfhe):
    c = tfhe.Circuit()
    a, b, s = c.inputs(3)
    x = c.xor(a, b)
    c.set_outputs([c.mux(s, x, a), c.not_(x)])
    for lv, (ops, aa, bb, cc, out) in zip(c.level_plan(1024), c.level_arrays()):
        assert lv["lut"] == [] and lv["linear"] is None
        for got, want in zip(lv["gates"], (ops, aa, bb, cc, out)):
            assert np.array_equal(got, want)


def test_circuit_argument_errors(tfhe):
    c = tfhe.Circuit()
    x, y = c.inputs(2)
    f = lambda m: m
    with pytest.raises(ValueError):
        c.lut(f, [x, 17], 8)                    # unknown wire
    with pytest.raises(ValueError):
        c.linear([(x, 1), (99, 2)])
    with pytest.raises(ValueError):
        c.lut(f, [(x, 1.5)], 8)                 # non-integer coefficient
    with pytest.raises(ValueError):
        c.linear([(x, "2")])
    with pytest.raises(ValueError):
        c.lut(f, [x], 8, const=0.25)
    with pytest.raises(ValueError):
        c.lut_multi([f, f, f], [x], 4)          # K not a power of two
    with pytest.raises(ValueError):
        c.lut(f, [x], 6)                        # p not a power of two
    c.lut_multi([f] * 4, [x, y], 256)          # p K = 1024 > N / 2: refused once N is known
    with pytest.raises(ValueError):
        c.level_plan(1024)
    c2 = tfhe.Circuit()
    z = c2.input()
    c2.lut(np.zeros(512, np.int32), [z], 2)    # a raw table of the wrong length
    with pytest.raises(ValueError):
        c2.level_plan(1024)


def test_gate_test_vector(tfhe):
    from tfhe_jl_amd.lut import make_gate_test_vector
    v = make_gate_test_vector(lambda m: m >= 2, 4, 1024)
    assert v.dtype == np.int32 and v.shape == (1024,)
    assert (v[:512] == -(1 << 29)).all() and (v[512:] == 1 << 29).all()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def keys128k2(tfhe, orc):
    return KeySet(tfhe, orc, tfhe.tfhe_parameters_128(2), seed=128)


@pytest.fixture(scope="session")
def keys2048(tfhe, orc):
    return _set(tfhe, orc, 2048, 1, 3, 7)


def _random_level(rng, n_in, B, n_out, width, max_terms=4):
    """Random input words [n_in][width] and a level of B rows of 0 .. max_terms terms over them (int32 coefficients, some small);
    outputs a permutation of wires n_in .. n_in + B n_out."""
    rows = _words(rng, n_in, width)
    counts = rng.integers(0, max_terms + 1, size=B)
    counts[0] = max(counts[0], 1)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    T = int(start[-1])
    wire = rng.integers(0, n_in, size=T).astype(np.int32)
    coef = np.where(rng.random(T) < 0.5, rng.integers(-3, 4, size=T), rng.integers(-2**31, 2**31, size=T)).astype(np.int32)
    cst = rng.integers(-2**31, 2**31, size=B).astype(np.int32)
    out = (n_in + rng.permutation(B * n_out)).astype(np.int32)
    return rows, start, wire, coef, cst, out


def _combine(rows, start, wire, coef, cst):
    """x_g = sum coef * row + cst on the body, mod 2^32, in numpy."""
    B = start.size - 1
    x = np.zeros((B, rows.shape[1]), np.int64)
    for g in range(B):
        for t in range(start[g], start[g + 1]):
            x[g] += int(coef[t]) * rows[wire[t]].astype(np.int64)
            x[g] %= 2**32
        if cst is not None:
            x[g, -1] += int(cst[g])
    return _wrap32(x)


def _combine_fast(rows, start, wire, coef, cst):
    B, T = start.size - 1, int(start[-1])
    row_of = np.repeat(np.arange(B), np.diff(start))
    x = np.zeros((B, rows.shape[1]), np.uint64)
    contrib = (rows[wire].astype(np.int64).astype(np.uint64) * coef[:T].astype(np.int64).astype(np.uint64)[:, None]) & 0xFFFFFFFF
    np.add.at(x, row_of, contrib)
    x &= 0xFFFFFFFF
    if cst is not None:
        x[:, -1] = (x[:, -1] + cst.astype(np.int64).astype(np.uint64)) & 0xFFFFFFFF
    return x.astype(np.uint32).astype(np.int32)


def test_combine_helpers_agree():
    rng = np.random.default_rng(3)
    rows, start, wire, coef, cst, _ = _random_level(rng, 20, 30, 1, 9)
    assert np.array_equal(_combine(rows, start, wire, coef, cst), _combine_fast(rows, start, wire, coef, cst))


def _keys(request, which):
    return request.getfixturevalue({"80": "keys80", "128k2": "keys128k2", "2048": "keys2048"}[which])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["80", "128k2", "2048"])
@pytest.mark.parametrize("B", [1, 300, 4096])
@pytest.mark.parametrize("n_out", [1, 2, 4])
def test_lut_level_is_the_host_path(request, which, B, n_out):
    K = _keys(request, which)
    eng = K.ck.engine(0)
    n1, N = K.params.lwe_size + 1, K.params.tlwe_polynomial_degree
    rng = np.random.default_rng(B + 10 * n_out + len(which))
    n_in = min(B + 3, 700)
    rows, start, wire, coef, cst, out = _random_level(rng, n_in, B, n_out, n1)
    tables = _words(rng, 3, N)
    index = rng.integers(0, 3, size=B).astype(np.int32)
    x = _combine_fast(rows, start, wire, coef, cst)
    want = eng.bootstrap_tv(tables, x, index=index)[:, None] if n_out == 1 else eng.bootstrap_tv_multi(tables, x, n_out, index=index)
    eng.wires_alloc(n_in + B * n_out)
    eng.wires_upload(0, rows)
    eng.lut_level(tables, start, wire, coef, cst, out, index=index, n_out=n_out)
    assert eng.last_rotation_count() == B
    got = eng.wires_gather(out).reshape(B, n_out, n1)
    assert np.array_equal(got, want)
    # tv_index NULL (table 0) and cst NULL
    eng.lut_level(tables, start, wire, coef, None, out, n_out=n_out)
    x0 = _combine_fast(rows, start, wire, coef, None)
    want0 = eng.bootstrap_tv_multi(tables[:1], x0, n_out)
    assert np.array_equal(eng.wires_gather(out).reshape(B, n_out, n1), want0)


@pytest.mark.gpu
def test_small_level_against_pbs_ref(checkers, small80):  # noqa: F811
    """One small level against tests/pbs_ref/pbs_ref.c (CPU): the check does not rest on the GPU's own host path."""
    import ctypes as C
    K = small80
    o = K.oracle
    lib = checkers["pbs_ref"]
    eng = K.ck.engine(0)
    rng = np.random.default_rng(77)
    rows, start, wire, coef, cst, out = _random_level(rng, 10, 7, 1, K.params.lwe_size + 1)
    tables = _words(rng, 2, 1024)
    index = rng.integers(0, 2, size=7).astype(np.int32)
    x = _combine(rows, start, wire, coef, cst)
    want = np.zeros((7, o.n + 1), np.int32)
    assert lib.orc_init(C.c_int32(o.N)) == 0
    assert lib.pbs_bootstrap_batch(C.byref(o.P), _p(o.bk_re), _p(o.bk_im), _p(o.bk_i32), _p(o.ks), 0, _p(tables), _p(index), _p(x),
                                   _p(want), 7, 1) == 0
    eng.wires_alloc(20)
    eng.wires_upload(0, rows)
    eng.lut_level(tables, start, wire, coef, cst, out, index=index)
    assert np.array_equal(eng.wires_gather(out), want)


@pytest.mark.gpu
def test_linear_level_is_numpy(keys80):
    eng = keys80.ck.engine(0)
    n1 = keys80.params.lwe_size + 1
    rng = np.random.default_rng(5)
    rows, start, wire, coef, cst, out = _random_level(rng, 50, 400, 1, n1, max_terms=6)
    eng.wires_alloc(450)
    eng.wires_upload(0, rows)
    eng.linear_level(start, wire, coef, cst, out)
    assert eng.last_rotation_count() == 0
    assert np.array_equal(eng.wires_gather(out), _combine(rows, start, wire, coef, cst))
    eng.linear_level(start, wire, coef, None, out)
    assert np.array_equal(eng.wires_gather(out), _combine(rows, start, wire, coef, None))
    # rows without terms are the trivial samples (0, cst)
    empty = np.zeros(4, np.int32)
    eng.linear_level(empty, np.zeros(0, np.int32), np.zeros(0, np.int32), np.array([7, -1, 2**30], np.int32), out[:3])
    triv = eng.wires_gather(out[:3])
    assert (triv[:, :-1] == 0).all() and triv[:, -1].tolist() == [7, -1, 2**30]


@pytest.mark.gpu
def test_caller_arrays_are_staged(keys80):
    """Every host array is copied before lut_level returns: overwriting them at once changes nothing."""
    eng = keys80.ck.engine(0)
    n1 = keys80.params.lwe_size + 1
    rng = np.random.default_rng(6)
    B = 4096
    rows, start, wire, coef, cst, out = _random_level(rng, 600, B, 2, n1)
    tables = _words(rng, 3, 1024)
    index = rng.integers(0, 3, size=B).astype(np.int32)
    want = eng.bootstrap_tv_multi(tables, _combine_fast(rows, start, wire, coef, cst), 2, index=index)
    keep_out = out.copy()
    eng.wires_alloc(600 + 2 * B)
    eng.wires_upload(0, rows)
    eng.lut_level(tables, start, wire, coef, cst, out, index=index, n_out=2)
    for a in (tables, start, wire, coef, cst, out, index):
        a[...] = rng.integers(-2**31, 2**31, size=a.shape, dtype=np.int64).astype(np.int32)
    assert np.array_equal(eng.wires_gather(keep_out).reshape(B, 2, n1), want)


@pytest.mark.gpu
def test_lut_adder_circuit(keys80):
    """The 16-bit LUT adder of examples/lut_adder.py as a Circuit, run_batch over 1024 instances in Z_8: every sum right and the words
    those of the host-orchestrated adder."""
    ex = _adder_module()
    sk, ck = keys80.sk, keys80.ck
    rng = np.random.default_rng(2024)
    M = 1024
    x, y = rng.integers(0, 2**16, size=M), rng.integers(0, 2**16, size=M)
    a, b = ex.encrypt_digits(rng, sk, x), ex.encrypt_digits(rng, sk, y)
    host = ex.lut_add16(ck, a, b)
    circ = ex.lut_adder_circuit()
    assert len(circ.levels()) == ex.DIGITS
    res = circ.run_batch(ck, ex.circuit_inputs(a, b))
    assert res.shape == (M, ex.DIGITS + 1, keys80.params.lwe_size + 1)
    assert np.array_equal(ex.decrypt_sum(sk, [_arr(res[:, i]) for i in range(ex.DIGITS + 1)]), x + y)
    assert np.array_equal(res, np.stack([d.data for d in host], axis=1))


def _arr(words):
    import tfhe_jl_amd as tfhe
    return tfhe.LweSampleArray(np.ascontiguousarray(words))


@pytest.mark.gpu
def test_lut_adder_circuit_multi_output_matches_the_host_loop(keys80):
    ex = _adder_module()
    sk, ck = keys80.sk, keys80.ck
    rng = np.random.default_rng(16)
    M = 256
    x, y = rng.integers(0, 2**16, size=M), rng.integers(0, 2**16, size=M)
    a, b = ex.encrypt_digits(rng, sk, x, ex.P_MULTI), ex.encrypt_digits(rng, sk, y, ex.P_MULTI)
    host = ex.lut_add16_multi(ck, a, b)
    res = ex.lut_adder_circuit(True).run_batch(ck, ex.circuit_inputs(a, b))
    assert np.array_equal(res, np.stack([d.data for d in host], axis=1))


def _mixed_circuit(tfhe, N):
    """c = x >= y (a LUT comparator on Z_8 digits, output a gate bit), then MUX(c, u, v) on gate bits; and the same bit back in Z_2
    (GATE_BIT_TO_Z2) through a LUT, and NOT c as a linear node read by a gate."""
    from tfhe_jl_amd.lut import GATE_BIT_TO_Z2, lut_encode, make_gate_test_vector
    c = tfhe.Circuit()
    x, y, u, v = c.inputs(4)
    ge = c.lut(make_gate_test_vector(lambda s: s >= 4, 8, N), [x, (y, -1)], 8, const=int(lut_encode(4, 8)))
    mux = c.mux(ge, u, v)
    back = c.lut(lambda b: 1 - b, [ge], 2, 8, const=GATE_BIT_TO_Z2)
    not_ge = c.linear([(ge, -1)])
    both = c.and_(not_ge, u)
    c.set_outputs([ge, mux, back, both])
    return c


@pytest.mark.gpu
def test_mixed_lut_and_gate_circuit(tfhe, keys80):
    from tfhe_jl_amd.lut import GATE_BIT_TO_Z2, lut_decrypt, lut_encode, lut_encrypt, make_gate_test_vector, make_test_vector
    sk, ck = keys80.sk, keys80.ck
    eng = ck.engine(0)
    rng = np.random.default_rng(31)
    M = 64
    xv, yv = rng.integers(0, 4, size=M), rng.integers(0, 4, size=M)
    uv, vv = rng.integers(0, 2, size=M).astype(bool), rng.integers(0, 2, size=M).astype(bool)
    ex, ey = lut_encrypt(rng, sk, xv, 8), lut_encrypt(rng, sk, yv, 8)
    eu, ev = tfhe.encrypt(rng, sk, uv), tfhe.encrypt(rng, sk, vv)
    c = _mixed_circuit(tfhe, 1024)
    res = c.run_batch(ck, np.stack([ex.data, ey.data, eu.data, ev.data], axis=1))
    ge = xv >= yv
    assert np.array_equal(tfhe.decrypt(sk, _arr(res[:, 0])), ge)
    assert np.array_equal(tfhe.decrypt(sk, _arr(res[:, 1])), np.where(ge, uv, vv))
    assert np.array_equal(lut_decrypt(sk, res[:, 2], 8), 1 - ge)
    assert np.array_equal(tfhe.decrypt(sk, _arr(res[:, 3])), ~ge & uv)
    # the same computation call by call on host buffers
    s = _wrap32(ex.data.astype(np.int64) - ey.data.astype(np.int64))
    s[:, -1] = _wrap32(s[:, -1].astype(np.int64) + int(lut_encode(4, 8)))
    bit = eng.bootstrap_tv(make_gate_test_vector(lambda t: t >= 4, 8, 1024), s)
    assert np.array_equal(res[:, 0], bit)
    assert np.array_equal(res[:, 1], eng.gates(np.full(M, tfhe.OPCODES["MUX"], np.uint8), bit, eu.data, ev.data))
    z2 = bit.copy()
    z2[:, -1] = _wrap32(z2[:, -1].astype(np.int64) + GATE_BIT_TO_Z2)
    assert np.array_equal(res[:, 2], eng.bootstrap_tv(make_test_vector(lambda b: 1 - b, 2, 1024, 8), z2))
    assert np.array_equal(res[:, 3], eng.gates(np.full(M, tfhe.OPCODES["AND"], np.uint8), _wrap32(-bit.astype(np.int64)), eu.data))
    # run (one instance) gives instance 0's words
    one = c.run(ck, [ex.data[0], ey.data[0], eu.data[0], ev.data[0]])
    assert np.array_equal(one.data, res[0])


@pytest.mark.gpu
@pytest.mark.parametrize("devices", DEVICE_PAIRS)
def test_multi_device_levels(keys80, devices):
    """A narrow level (first device only) and a wide one above level_split_min (sharded), then a level reading the outputs of both
    shards (pulled between the devices), and a linear level: the words of a one-device context."""
    K = keys80
    n1 = K.params.lwe_size + 1
    one, multi = K.ck.engine(0), K.ck.engine(devices)
    rng = np.random.default_rng(41)
    rows, start, wire, coef, cst, out = _random_level(rng, 100, 300, 2, n1)
    tables = _words(rng, 2, 1024)
    index = rng.integers(0, 2, size=300).astype(np.int32)
    s2 = np.arange(0, 301, dtype=np.int32)
    w2 = out[::2].copy()                                        # level 2: one term per row, reading level 1's outputs on both shards
    c2 = rng.integers(-3, 4, size=300).astype(np.int32)
    o2 = (700 + np.arange(300)).astype(np.int32)
    ol = (1000 + np.arange(300)).astype(np.int32)
    results = []
    for eng, split in ((one, None), (multi, 4096), (multi, 64)):
        if split is not None:
            eng.set_option("level_split_min", split)
        eng.wires_alloc(1300)
        eng.wires_upload(0, rows)
        eng.lut_level(tables, start, wire, coef, cst, out, index=index, n_out=2)
        if split is not None:
            assert eng.last_device_count() == (1 if split > 300 else len(devices))
        eng.lut_level(tables, s2, w2, c2, None, o2, index=index[::-1].copy())
        eng.linear_level(s2, o2, c2, cst, ol)
        results.append(eng.wires_gather(np.concatenate([out, o2, ol])))
    multi.set_option("level_split_min", 4096)
    assert np.array_equal(results[1], results[0]) and np.array_equal(results[2], results[0])


@pytest.mark.gpu
def test_error_paths_leave_the_context_sound(tfhe, keys80):
    from tfhe_jl_amd import _lib as L
    lib = L.load()
    K = keys80
    eng = K.ck.engine(0)
    n1 = K.params.lwe_size + 1
    rng = np.random.default_rng(12)
    rows, start, wire, coef, cst, out = _random_level(rng, 10, 6, 2, n1)
    tables = _words(rng, 2, 1024)
    index = rng.integers(0, 2, size=6).astype(np.int32)
    eng.wires_alloc(30)
    eng.wires_upload(0, rows)

    def lut(h=eng._h, tv=tables, n_tv=2, idx=index, n_out=2, st=start, tw=wire, tc=coef, cs=cst, o=out, B=6):
        return lib.tfhe_lut_level(h, _p(tv), n_tv, _p(idx), n_out, _p(st), _p(tw), _p(tc), _p(cs), _p(o), B)

    def linear(h=eng._h, st=start, tw=wire, tc=coef, cs=cst, o=out[:6], B=6):
        return lib.tfhe_linear_level(h, _p(st), _p(tw), _p(tc), _p(cs), _p(o), B)

    bad_start = start.copy(); bad_start[0] = 1
    dec_start = start.copy(); dec_start[3] = dec_start[2] - 1
    far = wire.copy(); far[0] = 30
    neg = wire.copy(); neg[-1] = -1
    dup = out.copy(); dup[3] = dup[0]
    reads_own = wire.copy(); reads_own[0] = out[5]
    oob = out.copy(); oob[1] = 30
    bad_idx = index.copy(); bad_idx[2] = 2
    for kw in (dict(st=None), dict(o=None), dict(B=-1), dict(tv=None), dict(st=bad_start), dict(st=dec_start), dict(tw=far), dict(tw=neg),
               dict(o=dup), dict(tw=reads_own), dict(o=oob), dict(n_out=3), dict(n_out=64), dict(n_out=0), dict(n_tv=0), dict(idx=bad_idx),
               dict(tw=None), dict(tc=None)):
        assert lut(**kw) == ERR_INVALID, kw
    for kw in (dict(st=None), dict(o=None), dict(B=-1), dict(st=bad_start), dict(tw=far), dict(o=dup[:6]), dict(tw=reads_own),
               dict(o=np.array([1, 2, 3, 4, 5, 30], np.int32)), dict(tc=None)):
        assert linear(**kw) == ERR_INVALID, kw
    eng.set_option("measure_margin", 1)
    try:
        assert lut() == ERR_STATE
        assert linear(o=out[6:]) == 0
    finally:
        eng.set_option("measure_margin", 0)
    bare = tfhe.Engine(K.params, 0)
    try:
        assert lut(h=bare._h) == ERR_STATE and linear(h=bare._h) == ERR_STATE          # no wire table
        bare.wires_alloc(30)
        assert lut(h=bare._h) == ERR_NO_KEY
        assert linear(h=bare._h) == 0                                                  # no key needed
    finally:
        bare.close()
    mk = tfhe.Engine(tfhe.mktfhe_parameters_2party, 0)
    try:
        assert lut(h=mk._h) == ERR_STATE and linear(h=mk._h) == ERR_STATE
    finally:
        mk.close()
    assert lut(B=0) == 0 and linear(B=0) == 0
    with pytest.raises(tfhe.EngineError):
        eng.lut_level(tables, start, wire, coef, cst, np.arange(10, 28, dtype=np.int32), index=index, n_out=3)
    # the context goes on
    eng.lut_level(tables, start, wire, coef, cst, out, index=index, n_out=2)
    want = eng.bootstrap_tv_multi(tables, _combine(rows, start, wire, coef, cst), 2, index=index)
    assert np.array_equal(eng.wires_gather(out).reshape(6, 2, n1), want)
