"""Multi-key programmable bootstrapping: tfhe_mk_bootstrap_tv_batch / tfhe_mk_bootstrap_tv_multi_batch, tfhe_mk_lut_level /
tfhe_mk_linear_level, and LUT / linear nodes of a Circuit under an MKCloudKey.

The multi-key blind rotation starts its body from X^{-barb} tv[tv_index[g]] instead of X^{-barb} (mu, ..., mu); sample j is the final
accumulator extracted at coefficient j N / n_out (one mask column per party), then mk_keyswitch.  Expected words come from the
test-only checker tests/pbs_ref/mk_pbs_ref.c (the oracle's source plus that rotation).  CPU: symbols and declarations, the checker
against the oracle's orc_mk_bootstrap_wo_keyswitch with a constant table, the shift rule on P mask polynomials, the TV kernels in
resource_usage_mk_tv.txt and the schedule of the 2-party TV kernel.  GPU: every multi-key family word for word, a multi-device
context, the error paths, the levels, a mixed Circuit and the decryption rate."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DEVICE_PAIRS
from test_mk import MKKeys, _mk_setup
from test_mk_gates import MKGateRef, OPS
from test_pbs_multi import _extract_at, _shift

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["gcc", "-O3", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-std=c11", "-shared"]
P8 = 1 << 29
NEW = ("tfhe_mk_bootstrap_tv_batch", "tfhe_mk_bootstrap_tv_multi_batch", "tfhe_mk_lut_level", "tfhe_mk_linear_level")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="session")
def mkref(tmp_path_factory, orc):
    """tests/pbs_ref/mk_pbs_ref.c compiled with the oracle's flags into pytest's temporary directory."""
    so = str(tmp_path_factory.mktemp("mk_pbs_ref") / "libmk_pbs_ref.so")
    subprocess.check_call(CFLAGS + ["-o", so, os.path.join(ROOT, "tests", "pbs_ref", "mk_pbs_ref.c"), "-lm"])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.mk_pbs_multi_batch.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int64, C.c_int32]
    lib.mk_pbs_multi_batch.restype = C.c_int
    lib.orc_mk_bootstrap_wo_keyswitch.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]

    def run(o, tables, index, x, n_out, with_keyswitch=True):
        assert lib.orc_init(C.c_int32(o.N)) == 0
        x = np.ascontiguousarray(np.atleast_2d(x), np.int32)
        tables = np.ascontiguousarray(np.atleast_2d(tables), np.int32)
        idx = None if index is None else np.ascontiguousarray(index, np.int32)
        B, P = x.shape[0], o.parties
        out = np.zeros((B, n_out, P * o.n + 1 if with_keyswitch else P * o.N + 1), np.int32)
        rc = lib.mk_pbs_multi_batch(C.byref(o.P), P, _p(o.bk_re), _p(o.bk_im), _p(o.bk_i32), _p(o.ks), 0, _p(tables), _p(idx), n_out,
                                    _p(x), _p(out), B, 1 if with_keyswitch else 0)
        assert rc == 0
        return out
    run.lib = lib
    return run


@pytest.fixture(scope="module")
def mk_small(tfhe, orc):
    return MKKeys(tfhe, orc, n=24)


def _rows(tfhe, K, B, seed):
    """B multi-key rows: encryptions of both bits, then arbitrary words (the rotation is the same function of them)."""
    rng = np.random.default_rng(seed)
    w = len(K.sks) * K.params.lwe_size + 1
    x = rng.integers(-2**31, 2**31, size=(B, w), dtype=np.int64).astype(np.int32)
    x[:2] = tfhe.mk_encrypt(rng, K.sks, [True, False])
    return x


def _tables(N, n_tv, seed):
    return np.random.default_rng(seed).integers(-2**31, 2**31, size=(n_tv, N), dtype=np.int64).astype(np.int32)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exported_and_declared(tfhe):
    from tfhe_jl_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read()
    lib = L.load()
    for name in NEW:
        assert name in L.ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(r"int32_t " + name + r"\(tfhe_ctx \*ctx,", header), name
    for name in ("mk_bootstrap_tv", "mk_bootstrap_tv_multi", "mk_lut_level", "mk_linear_level"):
        assert callable(getattr(tfhe.Engine, name))
    import tfhe_jl_amd.lut as lut
    assert callable(lut.mk_lut_encrypt) and callable(lut.mk_lut_decrypt)
    assert lib.tfhe_mk_bootstrap_tv_batch(None, None, 1, None, None, None, 0, 1) == 1          # NULL context


def test_mk_lut_encrypt_roundtrip(tfhe, mk_small):
    from tfhe_jl_amd.lut import mk_lut_decrypt, mk_lut_encrypt
    K = mk_small
    for p in (2, 4):                    # (p = 8: a window of +-1/32 is 2.5 standard deviations of a fresh encryption's noise)
        m = K.rng.integers(0, p, 64)
        x = mk_lut_encrypt(K.rng, K.sks, m, p)
        assert x.shape == (64, 2 * K.params.lwe_size + 1) and np.array_equal(mk_lut_decrypt(K.sks, x, p), m)
    with pytest.raises(ValueError):
        mk_lut_encrypt(K.rng, K.sks, [4], 4)


def test_checker_constant_table_equals_oracle(orc, tfhe, mk_small, mkref):
    """With the constant table (1/8, ..., 1/8) and n_out = 1 the checker is orc_mk_bootstrap_wo_keyswitch(mu = 1/8), word for word."""
    K = mk_small
    o = K.oracle
    x = _rows(tfhe, K, 4, 1)
    got = mkref(o, np.full(o.N, P8, np.int32), None, x, 1, with_keyswitch=False)[:, 0]
    lib = mkref.lib
    for g in range(x.shape[0]):
        u = np.zeros(2 * o.N + 1, np.int32)
        m = C.c_double(0)
        xg = np.ascontiguousarray(x[g])
        assert lib.orc_mk_bootstrap_wo_keyswitch(C.byref(o.P), 2, _p(o.bk_re), _p(o.bk_im), _p(o.bk_i32), 0, P8, _p(xg), _p(u),
                                                 C.byref(m)) == 0
        assert np.array_equal(got[g], u), g
    # ... and keyswitched, the NAND helper's bootstrap + keyswitch of the same rows
    ks = mkref(o, np.full(o.N, P8, np.int32), None, x, 1)[:, 0]
    ref = MKGateRef(orc, o)
    assert np.array_equal(ks, np.stack([ref._keyswitch(u) for u in got]))


@pytest.mark.parametrize("P,N", [(2, 64), (3, 32), (2, 1024)])
def test_shift_rule_multi_key(P, N):
    """The engine's rule (extract_shift_kernel with W = P N + 1) is the direct extraction at c of each party's mask column."""
    rng = np.random.default_rng(P * N)
    acc = rng.integers(-2**31, 2**31, size=(P + 1, N), dtype=np.int64)
    e0 = _extract_at(acc, P, N, 0)
    for K in (1, 2, 4):
        for j in range(K):
            c = j * N // K
            assert np.array_equal(_shift(e0, P, N, c, acc[P][c]), _extract_at(acc, P, N, c)), (K, j)


def _report(name):
    """test_tv_kernels' reading of a compiler report, plus each kernel's SGPR spills."""
    from test_tv_kernels import BUILD, _report as rep
    rows = rep(name)
    spills = {}
    for block in re.split(r"remark: Function Name: ", open(os.path.join(BUILD, name)).read())[1:]:
        m = re.search(r"SGPRs Spill: (\d+)", block)
        spills[block.split()[0]] = int(m.group(1)) if m else None
    dem = subprocess.run(["c++filt"], input="\n".join(spills), capture_output=True, text=True, check=True).stdout.split("\n")
    for mangled, d in zip(spills, dem):
        rows[d]["sgpr_spill"] = spills[mangled]
    return rows


def test_every_multi_key_family_has_its_tv_kernels():
    """resource_usage_mk_tv.txt: one TV kernel per non-DIAG multi-key instantiation the dispatcher can select, none spilling more
    scratch, VGPRs or SGPRs than its mu kernel, each at its mu kernel's occupancy; no multi-key TV kernel in the other reports."""
    tv, mu = _report("resource_usage_mk_tv.txt"), _report("resource_usage.txt")
    assert not [k for k in mu if "_tv<" in k] and not [k for k in _report("resource_usage_tv.txt") if "mk_" in k]
    counts = {}
    for k, v in tv.items():
        m = re.match(r"void (?:anyn::)?(mk_blind_rotate_kernel\w*)_tv<", k)
        assert m, k
        counts[m.group(1)] = counts.get(m.group(1), 0) + 1
        base = re.sub(r"_tv<", "<", k).replace("WithTv<", "").replace(">)", ")")
        assert base in mu, (k, base)
        assert v["occ"] >= mu[base]["occ"] and v["vgpr"] + v["agpr"] <= 512, (k, v, mu[base])
        assert v["scratch"] <= mu[base]["scratch"] and v["vgpr_spill"] <= mu[base]["vgpr_spill"], (k, v, mu[base])
        # (the untuned any-N kernel, which spills scalars in its mu form too, holds the table pointer through its first loop: 43
        #  spilled SGPRs against 41; every tuned family spills no more scalars than its mu kernel)
        extra = 2 if k.startswith("void anyn::") else 0
        assert v["sgpr_spill"] is not None and v["sgpr_spill"] <= mu[base]["sgpr_spill"] + extra, (k, v, mu[base])
    assert counts == {"mk_blind_rotate_kernel_w2": 2, "mk_blind_rotate_kernel_general": 4, "mk_blind_rotate_kernel_g2": 4,
                      "mk_blind_rotate_kernel": 1}, counts
    # the non-DIAG instantiations only (MARGIN = false)
    assert sorted(re.sub(r"\(.*", "", k) for k in tv) == sorted([
        "void anyn::mk_blind_rotate_kernel_tv<false>", "void mk_blind_rotate_kernel_w2_tv<4, false, 1>", "void mk_blind_rotate_kernel_w2_tv<4, false, 2>",
        "void mk_blind_rotate_kernel_general_tv<false, 1, false>", "void mk_blind_rotate_kernel_general_tv<false, 1, true>",
        "void mk_blind_rotate_kernel_general_tv<false, 2, false>", "void mk_blind_rotate_kernel_general_tv<false, 2, true>",
        "void mk_blind_rotate_kernel_g2_tv<4, 5, false, 2, true>", "void mk_blind_rotate_kernel_g2_tv<4, 5, false, 4, true>",
        "void mk_blind_rotate_kernel_g2_tv<8, 8, false, 2, false>", "void mk_blind_rotate_kernel_g2_tv<8, 8, false, 4, false>"])


def test_two_party_tv_kernel_keeps_the_schedule():
    """mk_w2 sits at the 102-SGPR limit: its TV form meets the signature of the mu form — no scalar spills
    (v_readlane), at most 8 scratch instructions, at most 140 LDS-queue drains."""
    from test_resource_usage import _disassemble
    _report("resource_usage_mk_tv.txt")          # (builds the library if it is stale)
    mk = _disassemble(os.path.join(ROOT, "tfhe.jl_amd", "build", "engine_mk_tv.o"))
    w2 = {k: v for k, v in mk.items() if "mk_blind_rotate_kernel_w2_tv" in k}
    assert len(w2) == 2, list(w2)
    for k, body in w2.items():
        st = {"drains": sum("lgkmcnt(0)" in l for l in body), "readlane": sum("v_readlane" in l for l in body),
              "scratch": sum("scratch_" in l for l in body)}
        assert st["readlane"] == 0 and st["scratch"] <= 8 and st["drains"] <= 140, (k, st)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _check_family(tfhe, eng, o, K, mkref, name, seed):
    x = _rows(tfhe, K, 5, seed)
    tables = _tables(o.N, 3, seed)
    idx = np.array([0, 1, 2, 1, 0], np.int32)
    for n_out in (1, 2, 4):
        for ks in (True, False):
            want = mkref(o, tables, idx, x, n_out, with_keyswitch=ks)
            if n_out == 1:
                got = eng.mk_bootstrap_tv(tables, x, index=idx, with_keyswitch=ks)[:, None]
            else:
                got = eng.mk_bootstrap_tv_multi(tables, x, n_out, index=idx, with_keyswitch=ks)
            assert eng.last_kernel_name() == name + "+tv", eng.last_kernel_name()
            assert eng.last_rotation_count() == x.shape[0]
            assert np.array_equal(got, want), (name, n_out, ks)


class _Keys:
    def __init__(self, p, rng, sks, ck, o):
        self.params, self.rng, self.sks, self.ck, self.oracle = p, rng, sks, ck, o


@pytest.mark.gpu
@pytest.mark.parametrize("option", [None, "mk_general", "mkg_rw", "mkg_acc"])
def test_two_party_families_word_for_word(tfhe, mk_small, mkref, option):
    K = mk_small
    eng = K.ck.engine(0)
    names = {None: "mk_blind_rotate_kernel_w2<4>", "mk_general": "mk_blind_rotate_kernel_general(P=2,L=4)",
             "mkg_rw": "mk_blind_rotate_kernel_general(P=2,L=4)", "mkg_acc": "mk_blind_rotate_kernel_general(P=2,L=4,acc=global)"}
    opts = {None: {}, "mk_general": {"mk_general": 1}, "mkg_rw": {"mk_general": 1, "mkg_rw": 1}, "mkg_acc": {"mk_general": 1, "mkg_acc": 1}}[option]
    before = {k: eng.get_option(k) for k in opts}
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        _check_family(tfhe, eng, K.oracle, K, mkref, names[option], 10)
    finally:
        for k, v in before.items():
            eng.set_option(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("which,parties,n", [("4party", 4, 12), ("8party", 8, 6)])
def test_many_party_families_word_for_word(tfhe, orc, mkref, which, parties, n):
    base = getattr(tfhe, "mktfhe_parameters_" + which)
    K = _Keys(*_mk_setup(tfhe, orc, base, parties, n, seed=170 + parties))
    eng = K.ck.engine(0)
    name = "mk_blind_rotate_kernel_g2<4,5,acc=lds>" if parties == 4 else "mk_blind_rotate_kernel_g2<8,8>"
    try:
        for rw in (2, 4):
            eng.set_option("mkg_rw", rw)
            _check_family(tfhe, eng, K.oracle, K, mkref, name, 20 + rw)
    finally:
        eng.set_option("mkg_rw", 0)
        K.ck.close()


@pytest.mark.gpu
def test_any_n_family_word_for_word(tfhe, orc, mkref):
    from test_any_params import _mk, _mk_oracle
    p, rng, sks, ck = _mk(tfhe, orc, 2, 512, 4, 7, 6)
    K = _Keys(p, rng, sks, ck, _mk_oracle(orc, p, 2, ck))
    _check_family(tfhe, ck.engine(0), K.oracle, K, mkref, "mk_blind_rotate_kernel_anyn(N=512,P=2,l=4)", 30)
    ck.close()


@pytest.mark.gpu
@pytest.mark.parametrize("devices", DEVICE_PAIRS)
def test_multi_device_equals_one_device(tfhe, mk_small, devices):
    K = mk_small
    x = _rows(tfhe, K, 9, 40)
    tables = _tables(K.oracle.N, 2, 40)
    idx = np.arange(9, dtype=np.int32) % 2
    one = K.ck.engine(0).mk_bootstrap_tv_multi(tables, x, 2, index=idx)
    eng = K.ck.engine(devices)
    assert np.array_equal(eng.mk_bootstrap_tv_multi(tables, x, 2, index=idx), one)
    assert np.array_equal(eng.mk_bootstrap_tv(tables, x, index=idx, with_keyswitch=False),
                          K.ck.engine(0).mk_bootstrap_tv(tables, x, index=idx, with_keyswitch=False))


@pytest.mark.gpu
def test_error_paths_leave_the_context_usable(tfhe, orc, mk_small, mkref, keys80):
    K = mk_small
    lib = tfhe._lib.load()
    eng = K.ck.engine(0)
    x = _rows(tfhe, K, 2, 50)
    tables = _tables(K.oracle.N, 2, 50)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    out = np.zeros((2, 4, 2 * K.oracle.N + 1), np.int32)

    def works():
        assert np.array_equal(eng.mk_bootstrap_tv(tables, x, index=[1, 0]), mkref(K.oracle, tables, [1, 0], x, 1)[:, 0])

    h = eng._h
    assert lib.tfhe_mk_bootstrap_tv_batch(h, None, 2, None, ptr(x), ptr(out), 2, 1) == 1                          # NULL tables
    assert lib.tfhe_mk_bootstrap_tv_batch(h, ptr(tables), 0, None, ptr(x), ptr(out), 2, 1) == 1                   # n_tv < 1
    assert lib.tfhe_mk_bootstrap_tv_batch(h, ptr(tables), 2, ptr(np.array([0, 2], np.int32)), ptr(x), ptr(out), 2, 1) == 1
    for n_out in (0, 3, 64):
        assert lib.tfhe_mk_bootstrap_tv_multi_batch(h, ptr(tables), 2, None, n_out, ptr(x), ptr(out), 2, 1) == 1
    works()
    eng.set_option("measure_margin", 1)
    try:
        assert lib.tfhe_mk_bootstrap_tv_batch(h, ptr(tables), 2, None, ptr(x), ptr(out), 2, 1) == 5
    finally:
        eng.set_option("measure_margin", 0)
    works()
    # the single-key entry points keep refusing a multi-key context; the multi-key ones refuse a single-key context
    assert lib.tfhe_bootstrap_tv_batch(h, ptr(tables), 2, None, ptr(x), ptr(out), 2, 1) == 5
    assert lib.tfhe_lut_level(h, ptr(tables), 2, None, 1, ptr(np.array([0, 1], np.int32)), ptr(np.zeros(1, np.int32)),
                              ptr(np.ones(1, np.int32)), None, ptr(np.ones(1, np.int32)), 1) == 5
    sk = keys80.ck.engine(0)
    w = np.zeros((1, keys80.params.lwe_size + 1), np.int32)
    assert lib.tfhe_mk_bootstrap_tv_batch(sk._h, ptr(tables), 1, None, ptr(w), ptr(out), 1, 1) == 5
    assert lib.tfhe_mk_linear_level(sk._h, ptr(np.array([0, 1], np.int32)), ptr(np.zeros(1, np.int32)), ptr(np.ones(1, np.int32)), None,
                                    ptr(np.ones(1, np.int32)), 1) == 5
    # a context without multi-key keys
    bare = tfhe.Engine(K.params)
    assert lib.tfhe_mk_bootstrap_tv_batch(bare._h, ptr(tables), 2, None, ptr(x), ptr(out), 2, 1) == 3
    bare.close()
    # levels: no table, a single-key table, bad indices
    one = np.array([0, 1], np.int32)
    eng.wires_alloc(4)
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_lut_level(tables, one, [0], [1], None, [1])
    assert e.value.code == 5
    eng.mk_wires_alloc(4)
    eng.wires_upload(0, x)
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_lut_level(tables, one, [0], [1], None, [0])          # reads the wire it writes
    assert e.value.code == 1
    with pytest.raises(tfhe.EngineError) as e:
        eng.mk_linear_level(one, [9], [1], None, [2])                # outside the table
    assert e.value.code == 1
    works()


def _replay_level(o, mkref, rows, tables, index, term_start, wire, coef, cst, n_out):
    """The rows a tfhe_mk_lut_level computes: the integer combinations, then the checker."""
    B = len(term_start) - 1
    xs = np.zeros((B, rows.shape[1]), np.int64)
    for g in range(B):
        for t in range(term_start[g], term_start[g + 1]):
            xs[g] += int(coef[t]) * rows[wire[t]].astype(np.int64)
        xs[g, -1] += 0 if cst is None else int(cst[g])
    xs = ((xs + 2**31) % 2**32 - 2**31).astype(np.int32)
    return xs, (None if tables is None else mkref(o, tables, index, xs, n_out))


@pytest.mark.gpu
def test_levels_equal_the_checker(tfhe, mk_small, mkref):
    K = mk_small
    eng = K.ck.engine(0)
    x = _rows(tfhe, K, 4, 60)
    tables = _tables(K.oracle.N, 2, 60)
    eng.mk_wires_alloc(16)
    eng.wires_upload(0, x)
    start, wire, coef, cst = [0, 2, 3, 3], [0, 1, 2, 3, 0][:3], [1, -2, 3], [5, P8, -7]
    _, want = _replay_level(K.oracle, mkref, x, tables, [1, 0, 1], start, wire, coef, cst, 2)
    eng.mk_lut_level(tables, start, wire, coef, cst, [4, 5, 6, 7, 8, 9], index=[1, 0, 1], n_out=2)
    assert eng.last_rotation_count() == 3
    assert np.array_equal(eng.wires_download(4, 6), want.reshape(6, -1))
    lin, _ = _replay_level(K.oracle, mkref, x, None, None, [0, 2, 3], [0, 3, 1], [2, 1, -1], [0, 9], 1)
    eng.mk_linear_level([0, 2, 3], [0, 3, 1], [2, 1, -1], [0, 9], [10, 11])
    assert np.array_equal(eng.wires_download(10, 2), lin)


def _circuit(tfhe):
    from tfhe_jl_amd.lut import GATE_BIT_TO_Z2
    c = tfhe.Circuit()
    a, b, d = c.inputs(3)
    g = c.nand(a, b)
    maj = c.lut(np.full(1024, P8, np.int32), [a, b, d], 2)                  # majority of three gate bits in one rotation
    s = c.lut(lambda m: m ^ 1, [(g, 1)], 2, const=GATE_BIT_TO_Z2)
    pair = c.lut_multi([lambda m: m, lambda m: 1 - m], [(maj, 2)], 2)
    lin = c.linear([(maj, 1), (g, 1)], const=P8)
    x = c.xor(lin, a)
    c.set_outputs([g, maj, s, pair[0], pair[1], x])
    return c


def _replay_circuit(orc, o, mkref, rows):
    """The circuit of _circuit, node by node, on the gate helper and the checker."""
    from tfhe_jl_amd.lut import GATE_BIT_TO_Z2, make_multi_test_vector, make_test_vector
    ref = MKGateRef(orc, o)
    w32 = lambda v: ((np.asarray(v, np.int64) + 2**31) % 2**32 - 2**31).astype(np.int32)
    a, b, d = (rows[i] for i in range(3))
    g = ref.gate(OPS["NAND"], a, b)
    maj = mkref(o, np.full(o.N, P8, np.int32), None, w32(a.astype(np.int64) + b + d), 1)[0, 0]
    gs = g.astype(np.int64)
    gs[-1] += GATE_BIT_TO_Z2
    s = mkref(o, make_test_vector(lambda m: m ^ 1, 2, o.N), None, w32(gs), 1)[0, 0]
    pair = mkref(o, make_multi_test_vector([lambda m: m, lambda m: 1 - m], 2, o.N), None, w32(2 * maj.astype(np.int64)), 2)[0]
    lin = maj.astype(np.int64) + g
    lin[-1] += P8
    x = ref.gate(OPS["XOR"], w32(lin), a)
    return np.stack([g, maj, s, pair[0], pair[1], x])


@pytest.mark.gpu
def test_mixed_circuit_under_a_multi_key_cloud_key(orc, tfhe, mk_small, mkref):
    K = mk_small
    c = _circuit(tfhe)
    rows = tfhe.mk_encrypt(K.rng, K.sks, [True, False, True])
    got = c.run(K.ck, rows)
    assert np.array_equal(got, _replay_circuit(orc, K.oracle, mkref, rows))
    batch = np.stack([tfhe.mk_encrypt(K.rng, K.sks, K.rng.integers(0, 2, 3).astype(bool)) for _ in range(3)])
    got = c.run_batch(K.ck, batch)
    for i in range(3):
        assert np.array_equal(got[i], _replay_circuit(orc, K.oracle, mkref, batch[i])), i


@pytest.mark.gpu
def test_python_helpers_under_a_multi_key_cloud_key(tfhe, mk_small, mkref):
    from tfhe_jl_amd.lut import make_multi_test_vector, make_test_vector, programmable_bootstrap, programmable_bootstrap_multi
    K = mk_small
    x = _rows(tfhe, K, 3, 70)
    f = lambda m: (m + 1) % 4
    got = programmable_bootstrap(K.ck, x, f, p=4)
    assert np.array_equal(got, mkref(K.oracle, make_test_vector(f, 4, 1024), None, x, 1)[:, 0])
    outs = programmable_bootstrap_multi(K.ck, x, [f, lambda m: m], 2)
    want = mkref(K.oracle, make_multi_test_vector([f, lambda m: m], 2, 1024), None, x, 2)
    assert all(np.array_equal(outs[j], want[:, j]) for j in range(2))


@pytest.mark.gpu
def test_decryption_rate_two_parties(tfhe, orc):
    """mktfhe_parameters_2party, fresh inputs: lookups of the identity of Z_p decrypt.  The bound is for p = 2 (tolerance 1/8); p = 4
    and 8 are measured and printed."""
    from tfhe_jl_amd.lut import make_test_vector, mk_lut_decrypt, mk_lut_encrypt
    p2 = tfhe.mktfhe_parameters_2party
    rng = np.random.default_rng(808)
    sks = [tfhe.SecretKey(rng, p2) for _ in range(2)]
    shared = tfhe.SharedKey(rng, p2)
    ck = tfhe.MKCloudKey([tfhe.CloudKeyPart(rng, sk, shared) for sk in sks])
    eng = ck.engine(0)
    B = 1024
    for p in (2, 4, 8):
        m = rng.integers(0, p, B)
        out = eng.mk_bootstrap_tv(make_test_vector(lambda v: v, p, 1024), mk_lut_encrypt(rng, sks, m, p))
        fails = int((mk_lut_decrypt(sks, out, p) != m).sum())
        print(f"  2 parties, p = {p}: {fails} of {B} lookups fail")
        if p == 2:
            assert fails <= B // 50, fails        # (6 of 1024 measured on an MI355X)
    ck.close()


def test_julia_shim_binds_multi_key_pbs():
    """The Julia shim's mk_bootstrap_tv / mk_bootstrap_tv_multi on a GpuMKCloudKey, and its ccall of tfhe_mk_bootstrap_tv_multi_batch
    with the header's argument kinds (checked statically, as test_julia_shim.py checks the others)."""
    from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia
    src = strip_julia(open(JULIA[0]).read())
    assert re.search(r"\nmk_bootstrap_tv\(mck::GpuMKCloudKey, tables::AbstractMatrix\{Int32\}, xs::MKVec", src)
    assert re.search(r"\nfunction mk_bootstrap_tv_multi\(mck::GpuMKCloudKey, tables::AbstractMatrix\{Int32\}, xs::MKVec, n_out::Integer", src)
    calls = [(types, nargs) for sym, types, nargs in ccalls(src) if sym == "tfhe_mk_bootstrap_tv_multi_batch"]
    want = c_prototypes()["tfhe_mk_bootstrap_tv_multi_batch"]
    assert len(calls) == 1 and [julia_kind(t) for t in calls[0][0]] == want and calls[0][1] == len(want), (calls, want)
