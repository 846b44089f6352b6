"""Multi-output programmable bootstrapping: tfhe_bootstrap_tv_multi_batch / Engine.bootstrap_tv_multi / lut.make_multi_test_vector.

One blind rotation, n_out = K samples per row: sample j is the final accumulator extracted at coefficient j N / K (tlwe.jl:55-59
generalised).  CPU: the entry point, the helpers, the packed-table rule and the shift rule the engine applies (numpy and the test-only
checker tests/pbs_ref/pbs_multi_ref.c), and the checker against tests/pbs_ref/pbs_ref.c.  GPU: every kernel family word for word
against the checker, sample 0 against tfhe_bootstrap_tv_batch, the shipped sets at full and split batch sizes, decryption, one step
of the digit adder, a multi-device context and every error path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import DEVICE_PAIRS, KeySet
from test_pbs import FAMILIES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["gcc", "-O3", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-std=c11", "-shared"]


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_entry_point_and_helpers_exist(tfhe):
    from tfhe_jl_amd import _lib as L
    assert "tfhe_bootstrap_tv_multi_batch" in L.ABI_SYMBOLS
    assert hasattr(L.load(), "tfhe_bootstrap_tv_multi_batch")
    assert L.load().tfhe_abi_version() == 7
    header = open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read()
    assert re.search(r"int32_t tfhe_bootstrap_tv_multi_batch\(tfhe_ctx \*ctx, const int32_t \*tv, int32_t n_tv, const int32_t \*tv_index, "
                     r"int32_t n_out,\s+const int32_t \*in, int32_t \*out, int64_t B, int32_t with_keyswitch\);", header)
    import tfhe_jl_amd.lut as lut
    for name in ("make_multi_test_vector", "programmable_bootstrap_multi"):
        assert callable(getattr(lut, name)) and getattr(tfhe, name) is getattr(lut, name) and name in tfhe.__all__
    assert callable(tfhe.Engine.bootstrap_tv_multi)


def _rotate_body(v, barb):
    """Body of (0, .., 0, X^{-barb} v): coefficient j = v[idx mod N], negated when idx & N, idx = (j + barb) mod 2N."""
    N = v.size
    idx = (np.arange(N) + barb) % (2 * N)
    x = v[idx % N].astype(np.int64)
    return np.where(idx & N, -x, x)


PK = [(p, K) for p in (2, 4, 8, 16) for K in (1, 2, 4, 8) if p * K <= 16]


@pytest.mark.parametrize("N", [512, 1024, 2048])
@pytest.mark.parametrize("p,K", PK, ids=[f"p{p}K{K}" for p, K in PK])
def test_packed_table_rule(tfhe, N, p, K):
    """For every noiseless phase phi of message m in Z_{pK} (m < p), coefficient j N / K of X^{-phi} v is lut_encode(f_j(m), q),
    v = make_multi_test_vector(f, p, N, q)."""
    from tfhe_jl_amd.lut import lut_encode, make_multi_test_vector, make_test_vector
    rng = np.random.default_rng(N + 10 * p + K)
    for q in (p, 2 * p):
        f = rng.integers(0, q, size=(K, p))
        v = make_multi_test_vector([lambda m, j=j: f[j][m] for j in range(K)], p, N, q)
        assert np.array_equal(v, make_test_vector(lambda x: f[x // p][x % p], p * K, N, q))
        for m in range(p):
            for phi in range(m * N // (p * K), (m + 1) * N // (p * K)):
                body = _rotate_body(v, phi)
                for j in range(K):
                    assert body[j * N // K] == lut_encode(f[j][m], q), (m, phi, j)


def test_make_multi_test_vector_refuses_bad_shapes(tfhe):
    from tfhe_jl_amd.lut import make_multi_test_vector
    f = lambda m: m
    with pytest.raises(ValueError):
        make_multi_test_vector([f, f, f], 4, 1024)          # K = 3
    with pytest.raises(ValueError):
        make_multi_test_vector([f] * 4, 4, 16)              # p K = 16 > N / 2
    with pytest.raises(ValueError):
        make_multi_test_vector([], 4, 1024)


def _negacyclic(a, b):
    """a * b mod X^N + 1, int64 (exact for the small test sizes, then wrapped)."""
    N = a.size
    full = np.convolve(a.astype(np.int64), b.astype(np.int64))
    out = full[:N].copy()
    out[: full.size - N] -= full[N:]
    return out


def _extract_at(acc, k, N, c):
    """The sample extracted at coefficient c from a TLWE sample acc [(k+1)][N] (tlwe.jl:55-59 with 0 -> c)."""
    u = np.arange(N)
    out = np.empty(k * N + 1, np.int64)
    for i in range(k):
        p = acc[i].astype(np.int64)
        out[i * N:(i + 1) * N] = np.where(u <= c, p[(c - u) % N], -p[(N + c - u) % N])
    out[k * N] = acc[k][c]
    return out


def _w32(v):
    return (int(v) + 2**31) % 2**32 - 2**31


def _shift(e, k, N, c, body):
    """The engine's rule: X^c times each mask polynomial of the index-0 extraction e, body replaced."""
    u = np.arange(N)
    out = np.empty(k * N + 1, np.int64)
    for i in range(k):
        x = e[i * N:(i + 1) * N].astype(np.int64)
        out[i * N:(i + 1) * N] = np.where(u >= c, x[(u - c) % N], -x[(N + u - c) % N])
    out[k * N] = body
    return out


@pytest.mark.parametrize("k,N", [(1, 64), (2, 32), (1, 1024)])
def test_shift_rule(k, N):
    """X^c applied to the index-0 extraction is the direct extraction at c, on random TLWE words; and the direct extraction at c
    decrypts to coefficient c of the TLWE phase body - sum_i a_i s_i."""
    rng = np.random.default_rng(N + k)
    for _ in range(3):
        acc = rng.integers(-2**31, 2**31, size=(k + 1, N), dtype=np.int64)
        e0 = _extract_at(acc, k, N, 0)
        s = rng.integers(0, 2, size=(k, N))
        phase = acc[k] - sum(_negacyclic(acc[i], s[i]) for i in range(k))
        for c in sorted({0, 1, N // 4, N // 2, N - 1, int(rng.integers(0, N))}):
            ec = _extract_at(acc, k, N, c)
            assert np.array_equal(_shift(e0, k, N, c, acc[k][c]).astype(np.int32), ec.astype(np.int32)), c
            lwe_phase = int(ec[k * N]) - sum(int(np.dot(ec[i * N:(i + 1) * N], s[i])) for i in range(k))
            assert _w32(lwe_phase) == _w32(phase[c]), c


@pytest.fixture(scope="session")
def checkers(tmp_path_factory, orc):
    """tests/pbs_ref/pbs_multi_ref.c and tests/pbs_ref/pbs_ref.c compiled with the oracle's flags into pytest's temporary directory."""
    d = tmp_path_factory.mktemp("pbs_multi_ref")
    libs = {}
    for name in ("pbs_multi_ref", "pbs_ref"):
        so = str(d / f"lib{name}.so")
        subprocess.check_call(CFLAGS + ["-o", so, os.path.join(ROOT, "tests", "pbs_ref", f"{name}.c"), "-lm"])
        libs[name] = C.CDLL(so)
    vp = C.c_void_p
    libs["pbs_multi_ref"].pbs_multi_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int64, C.c_int32]
    libs["pbs_multi_ref"].pbs_multi_batch.restype = C.c_int
    libs["pbs_multi_ref"].pbs_shift_extraction.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int32, vp]
    libs["pbs_multi_ref"].pbs_extract_at.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    libs["pbs_ref"].pbs_bootstrap_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp, vp, vp, C.c_int64, C.c_int32]
    libs["pbs_ref"].pbs_bootstrap_batch.restype = C.c_int
    return libs


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="session")
def multi_ref(checkers):
    lib = checkers["pbs_multi_ref"]

    def run(K, tables, index, x, n_out, with_keyswitch=True):
        o = K.oracle
        assert lib.orc_init(C.c_int32(o.N)) == 0
        x = np.ascontiguousarray(x, np.int32)
        tables = np.ascontiguousarray(np.atleast_2d(tables), np.int32)
        idx = None if index is None else np.ascontiguousarray(index, np.int32)
        B = x.shape[0]
        out = np.zeros((B, n_out, o.n + 1 if with_keyswitch else o.k * o.N + 1), np.int32)
        rc = lib.pbs_multi_batch(C.byref(o.P), _p(o.bk_re), _p(o.bk_im), _p(o.bk_i32), _p(o.ks), 0, _p(tables), _p(idx), n_out, _p(x),
                                 _p(out), B, 1 if with_keyswitch else 0)
        assert rc == 0
        return out
    return run


def test_checker_shift_rule_agrees_with_its_extraction(checkers):
    """The checker's pbs_shift_extraction (the engine's rule) and its pbs_extract_at (the direct extraction) on random words."""
    lib = checkers["pbs_multi_ref"]
    rng = np.random.default_rng(5)
    for k, N in ((1, 1024), (2, 256), (1, 512)):
        acc = rng.integers(-2**31, 2**31, size=(k + 1, N), dtype=np.int64).astype(np.int32)
        e0 = np.zeros(k * N + 1, np.int32)
        lib.pbs_extract_at(_p(acc), k, N, 0, _p(e0))
        assert np.array_equal(e0, _extract_at(acc, k, N, 0).astype(np.int32))
        for c in (0, 3, N // 8, N // 2, N - 5):
            direct, shifted = np.zeros_like(e0), np.zeros_like(e0)
            lib.pbs_extract_at(_p(acc), k, N, c, _p(direct))
            lib.pbs_shift_extraction(_p(e0), k, N, c, int(acc[k][c]), _p(shifted))
            assert np.array_equal(direct, shifted), (k, N, c)


@pytest.fixture(scope="session")
def small80(tfhe, orc):
    """tfhe_parameters_80's ring and decomposition with a short LWE key (CPU checks stay quick)."""
    return KeySet(tfhe, orc, tfhe.SchemeParameters(40, 1 / 2**15, 1024, 1, 2, 10, 9e-9, 8, 2, 1 / 2**15, 1), seed=81)


def test_checker_with_one_output_is_pbs_ref(checkers, multi_ref, small80):
    """n_out = 1: pbs_multi_ref.c gives pbs_ref.c's words, with and without keyswitch; n_out = 4: its output 0 is the same."""
    K = small80
    o = K.oracle
    lib = checkers["pbs_ref"]
    rng = np.random.default_rng(11)
    B = 12
    x = rng.integers(-2**31, 2**31, size=(B, K.params.lwe_size + 1), dtype=np.int64).astype(np.int32)
    tables = rng.integers(-2**31, 2**31, size=(3, 1024), dtype=np.int64).astype(np.int32)
    index = rng.integers(0, 3, size=B).astype(np.int32)
    for ks in (True, False):
        want = np.zeros((B, o.n + 1 if ks else o.k * o.N + 1), np.int32)
        assert lib.orc_init(C.c_int32(o.N)) == 0
        assert lib.pbs_bootstrap_batch(C.byref(o.P), _p(o.bk_re), _p(o.bk_im), _p(o.bk_i32), _p(o.ks), 0, _p(tables), _p(index), _p(x),
                                       _p(want), B, 1 if ks else 0) == 0
        assert np.array_equal(multi_ref(K, tables, index, x, 1, ks)[:, 0], want), ks
        assert np.array_equal(multi_ref(K, tables, index, x, 4, ks)[:, 0], want), ks


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _words(rng, rows, width):
    return rng.integers(-2**31, 2**31, size=(rows, width), dtype=np.int64).astype(np.int32)


def _set(tfhe, orc, N, k, l, beta, n=8, seed=0):
    return KeySet(tfhe, orc, tfhe.SchemeParameters(n, 1 / 2**15, N, k, l, beta, 9e-9, 8, 2, 1 / 2**15, 1), seed=9000 + N + 10 * k + l + seed)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_family_matches_the_checker(tfhe, orc, multi_ref, fam):
    """K = 2, 4, 8 outputs; several tables with a per-row index and tv_index = NULL; with and without keyswitch: the engine's words
    are the checker's, the kernel is the one a mu batch of the same size takes, named "+tv", and B rotations are counted."""
    name, N, k, l, beta, opts, rows = fam
    K = _set(tfhe, orc, N, k, l, beta)
    eng = K.ck.engine(0)
    for o, v in opts.items():
        eng.set_option(o, v)
    rng = np.random.default_rng(len(name) + rows + 1)
    x = _words(rng, rows, K.params.lwe_size + 1)
    eng.bootstrap(2**29, x, with_keyswitch=False)
    mu_kernel = eng.last_kernel_name()
    tables = _words(rng, 3, N)
    index = rng.integers(0, 3, size=rows).astype(np.int32)
    for n_out in (2, 4, 8):
        assert n_out <= N // 4
        for idx in (index, None):
            for ks in (True, False):
                got = eng.bootstrap_tv_multi(tables, x, n_out, index=idx, with_keyswitch=ks)
                assert eng.last_kernel_name() == mu_kernel + "+tv", (name, eng.last_kernel_name(), mu_kernel)
                assert eng.last_rotation_count() == rows
                assert np.array_equal(got, multi_ref(K, tables, idx, x, n_out, ks)), (name, n_out, idx is None, ks)


@pytest.mark.gpu
def test_output_zero_and_one_output_are_bootstrap_tv(keys80):
    eng = keys80.ck.engine(0)
    rng = np.random.default_rng(21)
    x = _words(rng, 37, keys80.params.lwe_size + 1)
    tables = _words(rng, 2, 1024)
    index = rng.integers(0, 2, size=37).astype(np.int32)
    for ks in (True, False):
        want = eng.bootstrap_tv(tables, x, index=index, with_keyswitch=ks)
        one = eng.bootstrap_tv_multi(tables, x, 1, index=index, with_keyswitch=ks)
        assert one.shape == (37, 1, want.shape[1]) and np.array_equal(one[:, 0], want), ks
        for n_out in (2, 4, 32):
            assert np.array_equal(eng.bootstrap_tv_multi(tables, x, n_out, index=index, with_keyswitch=ks)[:, 0], want), (n_out, ks)


def _check_rows(eng, K, multi_ref, tables, index, x, n_out, rng):
    """Every row: sample 0 is bootstrap_tv's, the masks of samples j > 0 are X^{j N / n_out} times sample 0's; a sample of the rows
    (first, last and random ones) against the checker, keyswitched and not."""
    B, N, k = x.shape[0], K.params.tlwe_polynomial_degree, K.params.tlwe_mask_size
    raw = eng.bootstrap_tv_multi(tables, x, n_out, index=index, with_keyswitch=False)
    assert eng.last_rotation_count() == B
    assert np.array_equal(raw[:, 0], eng.bootstrap_tv(tables, x, index=index, with_keyswitch=False))
    for j in range(1, n_out):
        c = j * N // n_out
        for i in range(k):
            e = raw[:, 0, i * N:(i + 1) * N]
            want = np.concatenate([-e[:, N - c:].astype(np.int64), e[:, :N - c]], axis=1)
            assert np.array_equal(raw[:, j, i * N:(i + 1) * N], want.astype(np.int32)), (j, i)
    ks = eng.bootstrap_tv_multi(tables, x, n_out, index=index)
    rows = np.unique(np.concatenate([[0, B - 1], rng.choice(B, size=min(B, 30), replace=False)]))
    idx = None if index is None else index[rows]
    assert np.array_equal(raw[rows], multi_ref(K, tables, idx, x[rows], n_out, False))
    assert np.array_equal(ks[rows], multi_ref(K, tables, idx, x[rows], n_out, True))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["80", "128"])
def test_shipped_sets_match_the_checker(keys80, keys128, multi_ref, which):
    K = keys80 if which == "80" else keys128
    eng = K.ck.engine(0)
    rng = np.random.default_rng(int(which))
    x = _words(rng, 4096, K.params.lwe_size + 1)
    tables = _words(rng, 4, K.params.tlwe_polynomial_degree)
    index = rng.integers(0, 4, size=4096).astype(np.int32)
    _check_rows(eng, K, multi_ref, tables, index, x, 4, rng)
    assert eng.last_kernel_name().endswith("+tv")


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 7, 2100, 3072])
def test_split_launches_offset_the_bodies(keys80, multi_ref, B):
    """Batch sizes the dispatcher may split into several launches: the bodies of every part land in their rows."""
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(B + 3)
    x = _words(rng, B, K.params.lwe_size + 1)
    tables = _words(rng, 3, 1024)
    _check_rows(eng, K, multi_ref, tables, rng.integers(0, 3, size=B).astype(np.int32), x, 2, rng)
    _check_rows(eng, K, multi_ref, tables, None, x, 8, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("p,K", [(4, 2), (2, 4)])
def test_functions_decrypt_to_f_of_m(keys80, p, K):
    """4096 fresh encryptions of m in Z_p as messages of Z_{pK}, K random functions: every output j decrypts to f_j(m)."""
    from tfhe_jl_amd.lut import lut_decrypt, lut_encrypt, programmable_bootstrap_multi
    rng = np.random.default_rng(10 * p + K)
    m = rng.integers(0, p, size=4096)
    f = rng.integers(0, p, size=(K, p))
    outs = programmable_bootstrap_multi(keys80.ck, lut_encrypt(rng, keys80.sk, m, p * K), [lambda v, j=j: f[j][v] for j in range(K)], p)
    assert len(outs) == K
    for j in range(K):
        assert np.array_equal(lut_decrypt(keys80.sk, outs[j], p), f[j][m]), j


@pytest.mark.gpu
def test_digit_and_carry_from_one_rotation(keys80):
    """One chained step of a base-2 adder in Z_8: s = a + b + carry (0 .. 3, p = 4, K = 2), digit s mod 2 and carry s >= 2 from one
    rotation, both in Z_8 and usable in the next sum, the carry of the first step bootstrapped; all 4096 correct."""
    from tfhe_jl_amd.lut import lut_decrypt, lut_encode, lut_encrypt, programmable_bootstrap_multi
    rng = np.random.default_rng(44)
    a, b, a2, b2 = (rng.integers(0, 2, size=4096) for _ in range(4))
    fs = [lambda s: s % 2, lambda s: s >= 2]
    sk, ck = keys80.sk, keys80.ck
    ea, eb, ea2, eb2 = (lut_encrypt(rng, sk, v, 8) for v in (a, b, a2, b2))
    digit0, carry0 = programmable_bootstrap_multi(ck, (ea + eb).add_constant(-int(lut_encode(0, 8))), fs, 4, q=8)
    assert np.array_equal(lut_decrypt(sk, digit0, 8), (a + b) % 2) and np.array_equal(lut_decrypt(sk, carry0, 8), (a + b) >= 2)
    s = (ea2 + eb2 + carry0).add_constant(-2 * int(lut_encode(0, 8)))
    digit1, carry1 = programmable_bootstrap_multi(ck, s, fs, 4, q=8)
    t = a2 + b2 + ((a + b) >= 2)
    assert np.array_equal(lut_decrypt(sk, digit1, 8), t % 2) and np.array_equal(lut_decrypt(sk, carry1, 8), t >= 2)


@pytest.mark.gpu
def test_base4_digit_step_in_z16_reports_its_failures(keys80):
    """The base-4 step of examples/lut_adder.py's one-rotation adder: digit sums of Z_8 in Z_16 (p = 8, K = 2).  Its noise headroom
    is half that of Z_8: the failures of 4096 are printed, and only a gross excess (> 1 %) fails the test."""
    from tfhe_jl_amd.lut import lut_decrypt, lut_encode, lut_encrypt, programmable_bootstrap_multi
    rng = np.random.default_rng(45)
    a, b, c = rng.integers(0, 4, size=4096), rng.integers(0, 4, size=4096), rng.integers(0, 2, size=4096)
    fs = [lambda s: s % 4, lambda s: s >= 4]
    sk, ck = keys80.sk, keys80.ck
    ea, eb, ec = lut_encrypt(rng, sk, a, 16), lut_encrypt(rng, sk, b, 16), lut_encrypt(rng, sk, c, 16)
    digit, carry = programmable_bootstrap_multi(ck, (ea + eb + ec).add_constant(-2 * int(lut_encode(0, 16))), fs, 8, q=16)
    s = a + b + c
    bad = int(np.sum((lut_decrypt(sk, digit, 16) != s % 4) | (lut_decrypt(sk, carry, 16) != (s >= 4))))
    print(f"Z_16 digit step: {bad} of 4096 wrong")
    assert bad <= 40, bad


@pytest.mark.gpu
@pytest.mark.parametrize("devices", DEVICE_PAIRS)
def test_multi_device_context_gives_the_same_words(keys80, devices):
    K = keys80
    rng = np.random.default_rng(8)
    x = _words(rng, 301, K.params.lwe_size + 1)
    tables = _words(rng, 3, 1024)
    index = rng.integers(0, 3, size=301).astype(np.int32)
    one = K.ck.engine(0)
    multi = K.ck.engine(devices)
    for ks in (True, False):
        assert np.array_equal(multi.bootstrap_tv_multi(tables, x, 4, index=index, with_keyswitch=ks),
                              one.bootstrap_tv_multi(tables, x, 4, index=index, with_keyswitch=ks)), ks
    assert np.array_equal(multi.bootstrap_tv_multi(tables, x, 2), one.bootstrap_tv_multi(tables, x, 2))


@pytest.mark.gpu
def test_error_paths_leave_the_context_sound(tfhe, keys80, multi_ref):
    # (return codes only: after an injected TFHE_ERR_NOMEM earlier in the session on this context, tfhe_last_error keeps reporting
    #  that message on this thread)
    from tfhe_jl_amd import _lib as L
    lib = L.load()
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(9)
    x = _words(rng, 4, K.params.lwe_size + 1)
    out = np.zeros((4, 32, K.params.lwe_size + 1), np.int32)
    tables = _words(rng, 2, 1024)

    def call(h, n_out, idx=None, tv=tables, xin=x, o=out, B=4, ks=1, n_tv=2):
        return lib.tfhe_bootstrap_tv_multi_batch(h, _p(tv), n_tv, _p(idx), n_out, _p(xin), _p(o), B, ks)
    for n_out in (0, 3, 64, -2, 33):
        assert call(eng._h, n_out) == 1, n_out
    assert call(eng._h, 2, tv=None) == 1
    assert call(eng._h, 2, xin=None) == 1
    assert call(eng._h, 2, o=None) == 1
    assert call(eng._h, 2, n_tv=0) == 1
    bad = np.array([0, 1, 2, 0], np.int32)
    assert call(eng._h, 2, idx=bad) == 1
    eng.set_option("measure_margin", 1)
    try:
        assert call(eng._h, 2) == 5
    finally:
        eng.set_option("measure_margin", 0)
    mk = tfhe.Engine(tfhe.mktfhe_parameters_2party, 0)
    try:
        xm = np.zeros((1, mk.n + 1), np.int32)
        om = np.zeros((1, 2, mk.n + 1), np.int32)
        tm = np.zeros((1, mk.N), np.int32)
        assert lib.tfhe_bootstrap_tv_multi_batch(mk._h, _p(tm), 1, None, 2, _p(xm), _p(om), 1, 1) == 5
    finally:
        mk.close()
    bare = tfhe.Engine(K.params, 0)
    try:
        assert call(bare._h, 2) == 3
    finally:
        bare.close()
    # n_out > N / 4: N = 64 allows at most 16 outputs (refused before the missing key is noticed)
    tiny = tfhe.Engine(tfhe.SchemeParameters(8, 1 / 2**15, 64, 1, 2, 7, 9e-9, 8, 2, 1 / 2**15, 1), 0)
    try:
        xt = np.zeros((1, 9), np.int32)
        ot = np.zeros((1, 32, 9), np.int32)
        tt = np.zeros((1, 64), np.int32)
        assert lib.tfhe_bootstrap_tv_multi_batch(tiny._h, _p(tt), 1, None, 32, _p(xt), _p(ot), 1, 1) == 1
        assert lib.tfhe_bootstrap_tv_multi_batch(tiny._h, _p(tt), 1, None, 16, _p(xt), _p(ot), 1, 1) == 3
    finally:
        tiny.close()
    with pytest.raises(tfhe.EngineError):
        eng.bootstrap_tv_multi(tables, x, 3)
    index = np.array([1, 0, 1, 1], np.int32)
    assert np.array_equal(eng.bootstrap_tv_multi(tables, x, 4, index=index), multi_ref(K, tables, index, x, 4))


@pytest.mark.gpu
def test_allocation_failures_return_nomem_and_the_context_goes_on(keys80, multi_ref):
    """A debug_fail_alloc_after walk through the entry point: every armed call returns TFHE_ERR_NOMEM until the countdown passes
    the last checkpoint, and the context then computes the right words."""
    import tfhe_jl_amd as tfhe
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(10)
    x = _words(rng, 5, K.params.lwe_size + 1)
    tables = _words(rng, 2, 1024)
    index = np.array([1, 0, 1, 0, 0], np.int32)
    want = multi_ref(K, tables, index, x, 4)
    for n in range(1, 40):
        eng.set_option("debug_fail_alloc_after", n)
        try:
            got = eng.bootstrap_tv_multi(tables, x, 4, index=index)
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
    assert np.array_equal(eng.bootstrap_tv_multi(tables, x, 4, index=index), want)
