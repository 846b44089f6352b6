"""Programmable bootstrapping: tfhe_bootstrap_tv_batch / Engine.bootstrap_tv / tfhe_jl_amd.lut.

CPU: the entry point and the module exist, the extraction rule the kernels implement (numpy), and the test-only checker
tests/pbs_ref/pbs_ref.c (the oracle's source with blind_rotate_and_extract for any test polynomial, bootstrap.jl:50-59) against
the oracle's own bootstrap.  GPU: every kernel family word for word against the checker, constant tables against
tfhe_bootstrap_batch, what the functions decrypt to, chained lookups (the 16-bit digit adder of examples/lut_adder.py), a
multi-device context and every error path."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import DEVICE_PAIRS, KeySet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU = 2**29


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_entry_point_and_module_exist(tfhe):
    from tfhe_jl_amd import _lib as L
    assert "tfhe_bootstrap_tv_batch" in L.ABI_SYMBOLS
    assert hasattr(L.load(), "tfhe_bootstrap_tv_batch")
    import tfhe_jl_amd.lut as lut
    for name in ("lut_encode", "lut_decode", "lut_encrypt", "lut_decrypt", "make_test_vector", "programmable_bootstrap"):
        assert callable(getattr(lut, name)) and getattr(tfhe, name) is getattr(lut, name)


def _rotate_body(v, barb):
    """Body of (0, .., 0, X^{-barb} v) the way the kernels fill it: coefficient j = v[idx mod N], negated when idx & N,
    idx = (j + barb) mod 2N."""
    N = v.size
    idx = (np.arange(N) + barb) % (2 * N)
    x = v[idx % N].astype(np.int64)
    return np.where(idx & N, -x, x)


@pytest.mark.parametrize("N", [512, 1024, 2048])
@pytest.mark.parametrize("p", [2, 4, 8, 16])
def test_extraction_rule_selects_the_table_entry(tfhe, N, p):
    """After the rotation by the phase sum(bara_i s_i) the extracted body is coefficient 0 of X^{-phi} v, phi = barb - sum: v[phi]
    for phi in [0, N), -v[phi - N] above.  On make_test_vector's output every noiseless phi of message m's window gives
    lut_encode(f(m), q), and lut_decode recovers f(m)."""
    from tfhe_jl_amd.lut import lut_decode, lut_encode, make_test_vector
    rng = np.random.default_rng(N + p)
    for q in (p, 2 * p):
        table = rng.integers(0, q, size=p)
        v = make_test_vector(lambda m: table[m], p, N, q)
        # explicit negacyclic monomial product against the index rule, for a few phases
        for phi in rng.integers(0, 2 * N, size=8):
            Xv = np.zeros(N, np.int64)
            for j in range(N):                  # X^{-phi} v: coefficient (j - phi) mod 2N of v, the sign of the wrap
                e = (j - phi) % (2 * N)
                Xv[e % N] += -v[j] if e >= N else v[j]
            assert np.array_equal(np.int32(Xv[0]), np.int32(_rotate_body(v, phi)[0]))
        for m in range(p):
            for phi in range(m * N // p, (m + 1) * N // p):
                body = _rotate_body(v, phi)[0]
                assert body == lut_encode(table[m], q)
                assert lut_decode(body, q) == table[m]
        # the padding half returns the negation
        assert _rotate_body(v, N)[0] == np.int32(-np.int64(v[0]))


@pytest.fixture(scope="session")
def pbs_ref(tmp_path_factory, orc):
    """tests/pbs_ref/pbs_ref.c compiled with the oracle's flags into pytest's temporary directory."""
    d = tmp_path_factory.mktemp("pbs_ref")
    so = str(d / "libpbs_ref.so")
    src = os.path.join(ROOT, "tests", "pbs_ref", "pbs_ref.c")
    subprocess.check_call(["gcc", "-O3", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-std=c11",
                           "-shared", "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.pbs_bootstrap_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int64, C.c_int32]
    lib.pbs_bootstrap_batch.restype = C.c_int

    def run(K, tables, index, x, with_keyswitch=True):
        o = K.oracle
        assert lib.orc_init(C.c_int32(o.N)) == 0
        x = np.ascontiguousarray(x, np.int32)
        tables = np.ascontiguousarray(np.atleast_2d(tables), np.int32)
        idx = None if index is None else np.ascontiguousarray(index, np.int32)
        B = x.shape[0]
        out = np.zeros((B, o.n + 1 if with_keyswitch else o.k * o.N + 1), np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(vp)
        rc = lib.pbs_bootstrap_batch(C.byref(o.P), p(o.bk_re), p(o.bk_im), p(o.bk_i32), p(o.ks), 0, p(tables), p(idx), p(x), p(out),
                                     B, 1 if with_keyswitch else 0)
        assert rc == 0
        return out
    return run


@pytest.fixture(scope="session")
def small80(tfhe, orc):
    """tfhe_parameters_80's ring and decomposition with a short LWE key (CPU checks stay quick)."""
    return KeySet(tfhe, orc, tfhe.SchemeParameters(40, 1 / 2**15, 1024, 1, 2, 10, 9e-9, 8, 2, 1 / 2**15, 1), seed=80)


def test_checker_is_the_oracle_bootstrap_for_a_constant_table(pbs_ref, small80, keys80):
    """v = (mu, ..., mu): the checker gives orc_bootstrap's words, with and without keyswitch (tfhe_parameters_80 and a short key)."""
    for K, B in ((small80, 16), (keys80, 3)):
        rng = np.random.default_rng(B)
        x = rng.integers(-2**31, 2**31, size=(B, K.params.lwe_size + 1), dtype=np.int64).astype(np.int32)
        tv = np.full((1, K.params.tlwe_polynomial_degree), MU, np.int32)
        for ks in (True, False):
            assert np.array_equal(pbs_ref(K, tv, None, x, ks), K.oracle.bootstrap(MU, x, with_keyswitch=ks)), ks


def test_lwe_arithmetic_wraps(tfhe):
    from tfhe_jl_amd.lwe import LweSampleArray
    a = LweSampleArray(np.array([[2**31 - 1, 5, -2**31]], np.int32))
    b = LweSampleArray(np.array([[1, -7, -1]], np.int32))
    assert (a + b).data.tolist() == [[-2**31, -2, 2**31 - 1]]
    assert (a - b).data.tolist() == [[2**31 - 2, 12, -2**31 + 1]]
    assert (3 * b).data.tolist() == [[3, -21, -3]] and (-b).data.tolist() == [[-1, 7, 1]]
    assert a.add_constant(1).data.tolist() == [[2**31 - 1, 5, -2**31 + 1]]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _words(rng, rows, width):
    return rng.integers(-2**31, 2**31, size=(rows, width), dtype=np.int64).astype(np.int32)


def _set(tfhe, orc, N, k, l, beta, n=8, seed=0):
    return KeySet(tfhe, orc, tfhe.SchemeParameters(n, 1 / 2**15, N, k, l, beta, 9e-9, 8, 2, 1 / 2**15, 1), seed=7000 + N + 10 * k + l + seed)


# (family, N, k, l, beta, options, rows): each forces the kernel the dispatcher takes for a mu batch of that size
FAMILIES = [
    ("h2", 1024, 1, 2, 10, {}, 6),
    ("w2", 1024, 1, 2, 10, {"br_tiny": -1}, 6),
    ("w2_rw2", 1024, 1, 3, 7, {"br_tiny": -1, "w2_rw": 2}, 7),
    ("v3", 1024, 1, 2, 10, {"br_tiny": -1, "br_small": -1, "v3_rw": 1}, 6),
    ("v3_rw4", 1024, 1, 3, 7, {"br_tiny": -1, "br_small": -1, "v3_rw": 4}, 7),
    ("v3_rt_l", 1024, 1, 4, 7, {"br_tiny": -1, "br_small": -1}, 5),
    ("general", 1024, 1, 2, 10, {"br_general": 1}, 5),
    ("k2_w3", 1024, 2, 2, 7, {"k2_w3": 1}, 5),
    ("k2_rw", 1024, 2, 3, 7, {"k2_w3": 0, "k2_rw": 7}, 9),
    ("k2_single", 1024, 2, 2, 7, {"k2_w3": 0, "k2_rw": 1}, 5),
    ("n512_w2", 512, 1, 2, 7, {"n512_w2": 1}, 6),
    ("n512", 512, 1, 2, 7, {"n512_w2": 0, "n512_rw": 1}, 6),
    ("n512_rw", 512, 1, 3, 7, {"n512_w2": 0, "n512_rw": 4}, 7),
    ("n2048_rw1", 2048, 1, 3, 7, {"n2048_rw": 1}, 4),
    ("n2048_rw", 2048, 1, 3, 7, {"n2048_rw": 2}, 5),
    ("anyn", 256, 1, 2, 7, {}, 5),
]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_family_matches_the_checker(tfhe, orc, pbs_ref, fam):
    """Several tables with a per-row index, tv_index = NULL, and tables of arbitrary Int32 words: the engine's words are the
    checker's, with and without keyswitch, and the kernel is the one a mu batch of the same size takes, named "+tv"."""
    name, N, k, l, beta, opts, rows = fam
    K = _set(tfhe, orc, N, k, l, beta)
    eng = K.ck.engine(0)
    for o, v in opts.items():
        eng.set_option(o, v)
    rng = np.random.default_rng(len(name) + rows)
    x = _words(rng, rows, K.params.lwe_size + 1)
    eng.bootstrap(MU, x, with_keyswitch=False)
    mu_kernel = eng.last_kernel_name()
    tables = _words(rng, 3, N)
    index = rng.integers(0, 3, size=rows).astype(np.int32)
    for idx in (index, None):
        for ks in (True, False):
            got = eng.bootstrap_tv(tables, x, index=idx, with_keyswitch=ks)
            assert eng.last_kernel_name() == mu_kernel + "+tv", (name, eng.last_kernel_name(), mu_kernel)
            assert np.array_equal(got, pbs_ref(K, tables, idx, x, ks)), (name, idx is None, ks)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["80", "128"])
def test_shipped_sets_match_the_checker(tfhe, pbs_ref, keys80, keys128, which):
    K = keys80 if which == "80" else keys128
    eng = K.ck.engine(0)
    rng = np.random.default_rng(int(which))
    x = _words(rng, 6, K.params.lwe_size + 1)
    tables = _words(rng, 4, K.params.tlwe_polynomial_degree)
    index = np.array([3, 0, 1, 2, 2, 3], np.int32)
    for ks in (True, False):
        assert np.array_equal(eng.bootstrap_tv(tables, x, index=index, with_keyswitch=ks), pbs_ref(K, tables, index, x, ks)), ks
    assert eng.last_kernel_name().endswith("+tv")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 257, 1100, 2100, 2500, 4096])
def test_constant_table_is_tfhe_bootstrap_batch(keys80, pbs_ref, B):
    """v = (mu, ..., mu): every row equals tfhe_bootstrap_batch(mu), ragged sizes and split launches included; a sample of the
    rows also equals the checker."""
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(B)
    x = _words(rng, B, K.params.lwe_size + 1)
    want = eng.bootstrap(MU, x)
    name = eng.last_kernel_name()
    tv = np.full((2, 1024), MU, np.int32)
    got = eng.bootstrap_tv(tv, x, index=rng.integers(0, 2, size=B).astype(np.int32))
    assert eng.last_kernel_name() == " + ".join(s + "+tv" for s in name.split(" + ")), (eng.last_kernel_name(), name)
    assert np.array_equal(got, want)
    rows = rng.choice(B, size=min(B, 3), replace=False)
    assert np.array_equal(got[rows], pbs_ref(K, tv[:1], None, x[rows]))


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [f for f in FAMILIES if f[0] in ("h2", "w2_rw2", "v3_rw4", "general", "k2_rw", "k2_w3", "n512_rw", "n2048_rw", "anyn")],
                         ids=lambda f: f[0])
def test_constant_table_identity_per_family(tfhe, orc, fam):
    name, N, k, l, beta, opts, rows = fam
    K = _set(tfhe, orc, N, k, l, beta, seed=1)
    eng = K.ck.engine(0)
    for o, v in opts.items():
        eng.set_option(o, v)
    rng = np.random.default_rng(3)
    for B in (rows, rows + 3):
        x = _words(rng, B, K.params.lwe_size + 1)
        assert np.array_equal(eng.bootstrap_tv(np.full(N, MU, np.int32), x, with_keyswitch=False), eng.bootstrap(MU, x, with_keyswitch=False)), (name, B)


@pytest.mark.gpu
def test_functions_decrypt_to_f_of_m(tfhe, keys80):
    """4096 fresh encryptions, random f, p = 2, 4, 8 at tfhe_parameters_80: every output decrypts to f(m).  (Estimate: the
    modulus switch adds sigma ~ 2.2e-3 against a window of 1/32 at p = 8, ~14 sigma.)  p = 16 and 32: failures reported only."""
    from tfhe_jl_amd.lut import lut_decrypt, lut_encrypt, programmable_bootstrap
    K = keys80
    rng = np.random.default_rng(6)
    for p in (2, 4, 8, 16, 32):
        m = rng.integers(0, p, size=4096)
        f = rng.integers(0, p, size=p)
        out = programmable_bootstrap(K.ck, lut_encrypt(rng, K.sk, m, p), lambda v: f[v], p=p)
        bad = int(np.sum(lut_decrypt(K.sk, out, p) != f[m]))
        print(f"p = {p}: {bad} of 4096 decrypt wrongly")
        if p <= 8:
            assert bad == 0, p


def _example():
    spec = importlib.util.spec_from_file_location("lut_adder", os.path.join(ROOT, "examples", "lut_adder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_chained_digit_adder(keys80):
    """16-bit addition of 1024 random pairs from base-4 digits, both lookups of a digit in one call: the integer sums."""
    ex = _example()
    rng = np.random.default_rng(16)
    a, b = rng.integers(0, 2**16, size=1024), rng.integers(0, 2**16, size=1024)
    got = ex.decrypt_sum(keys80.sk, ex.lut_add16(keys80.ck, ex.encrypt_digits(rng, keys80.sk, a), ex.encrypt_digits(rng, keys80.sk, b)))
    assert np.array_equal(got, a + b)


@pytest.mark.gpu
@pytest.mark.parametrize("devices", DEVICE_PAIRS)
def test_multi_device_context_gives_the_same_words(keys80, devices):
    K = keys80
    rng = np.random.default_rng(8)
    x = _words(rng, 301, K.params.lwe_size + 1)
    tables = _words(rng, 3, 1024)
    index = rng.integers(0, 3, size=301).astype(np.int32)
    one = K.ck.engine(0).bootstrap_tv(tables, x, index=index)
    multi = K.ck.engine(devices)
    assert np.array_equal(multi.bootstrap_tv(tables, x, index=index), one)
    assert np.array_equal(multi.bootstrap_tv(tables, x, with_keyswitch=False), K.ck.engine(0).bootstrap_tv(tables, x, with_keyswitch=False))


@pytest.mark.gpu
def test_error_paths_leave_the_context_sound(tfhe, keys80, pbs_ref):
    from tfhe_jl_amd import _lib as L
    lib = L.load()
    K = keys80
    eng = K.ck.engine(0)
    vp = C.c_void_p
    rng = np.random.default_rng(9)
    x = _words(rng, 4, K.params.lwe_size + 1)
    out = np.zeros_like(x)
    tables = _words(rng, 2, 1024)
    p = lambda a: a.ctypes.data_as(vp)

    def call(tv, n_tv, idx, xin, o, B=4, ks=1):
        return lib.tfhe_bootstrap_tv_batch(eng._h, tv, n_tv, idx, xin, o, B, ks)
    assert call(None, 2, None, p(x), p(out)) == 1
    assert call(p(tables), 2, None, None, p(out)) == 1
    assert call(p(tables), 2, None, p(x), None) == 1
    assert call(p(tables), 0, None, p(x), p(out)) == 1
    bad = np.array([0, 1, 2, 0], np.int32)
    assert call(p(tables), 2, p(bad), p(x), p(out)) == 1
    assert "tv_index[2]" in lib.tfhe_last_error(eng._h).decode()
    neg = np.array([0, -1, 0, 0], np.int32)
    assert call(p(tables), 2, p(neg), p(x), p(out)) == 1
    eng.set_option("measure_margin", 1)
    try:
        assert call(p(tables), 2, None, p(x), p(out)) == 5
        assert "measure_margin" in lib.tfhe_last_error(eng._h).decode()
    finally:
        eng.set_option("measure_margin", 0)
    mk = tfhe.Engine(tfhe.mktfhe_parameters_2party, 0)
    try:
        xm = np.zeros((1, mk.n + 1), np.int32)
        om = np.zeros_like(xm)
        tm = np.zeros((1, mk.N), np.int32)
        assert lib.tfhe_bootstrap_tv_batch(mk._h, p(tm), 1, None, p(xm), p(om), 1, 1) == 5
    finally:
        mk.close()
    bare = tfhe.Engine(K.params, 0)
    try:
        assert lib.tfhe_bootstrap_tv_batch(bare._h, p(tables), 2, None, p(x), p(out), 4, 1) == 3
    finally:
        bare.close()
    index = np.array([1, 0, 1, 1], np.int32)
    assert np.array_equal(eng.bootstrap_tv(tables, x, index=index), pbs_ref(K, tables, index, x))


@pytest.mark.gpu
def test_allocation_failures_return_nomem_and_the_context_goes_on(keys80, pbs_ref):
    """A debug_fail_alloc_after walk through the entry point (tests/test_abi_nomem.py): every armed call returns TFHE_ERR_NOMEM
    until the countdown passes the last checkpoint, and the context then computes the right words."""
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(10)
    x = _words(rng, 5, K.params.lwe_size + 1)
    tables = _words(rng, 2, 1024)
    index = np.array([1, 0, 1, 0, 0], np.int32)
    want = pbs_ref(K, tables, index, x)
    import tfhe_jl_amd as tfhe
    for n in range(1, 40):
        eng.set_option("debug_fail_alloc_after", n)
        try:
            got = eng.bootstrap_tv(tables, x, index=index)
        except tfhe.EngineError as e:
            assert e.code == 6, str(e)
            continue
        finally:
            eng.set_option("debug_fail_alloc_after", 0)
        assert np.array_equal(got, want)
        break
    else:
        pytest.fail("the countdown never ran past the entry point's checkpoints")
    assert n > 1
    assert np.array_equal(eng.bootstrap_tv(tables, x, index=index), want)
