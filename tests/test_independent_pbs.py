"""Programmable bootstrapping, levels and the multi-key gate set against the integer schoolbook of tests/test_independent.py.

Everything added after the mu bootstrap (tfhe_bootstrap_tv_batch, tfhe_bootstrap_tv_multi_batch, tfhe_lut_level / tfhe_linear_level,
their tfhe_mk_* forms and tfhe_mk_gates_batch) was checked through oracle/tfhe_oracle.c only: tests/pbs_ref/*.c include its source.
Here the expected words come from `Schoolbook` / `MKSchoolbook` (exact int64 products, written from the reference's text):

    rotate(v, x)          blind_rotate_and_extract up to the final accumulator, any Int32 test polynomial (bootstrap.jl:50-57, 69-75)
    extract_at(acc, c)    tlwe_extract_sample (tlwe.jl:55-59) at coefficient c: word u = coefficient c of X^u p, from the phase
    bootstrap_tv          the two, n_out samples at c_j = j N / n_out, keyswitch (keyswitch.jl:45-80, bootstrap.jl:92-95)
    mk_rotate / mk_extract_at / mk_keyswitch / mk_bootstrap_tv / mk_gate      mk_internals.jl:464-509, :88-95, :397-411; gates.jl
    combine               a level row: sum coef * wire + cst on the body, every word mod 2^32 (lwe.jl:67-82)

CPU tests pin the test-only checkers (pbs_ref.c, pbs_multi_ref.c, mk_pbs_ref.c, both product back-ends) and the oracle's multi-key
gate pieces to these values.  GPU tests compare the engine with the same values and call no function of oracle/ and no checker.  The
inputs are the edge rows and tables below (zero exponents, exponent -N, the rounding boundary of the modulus switch, extreme table
words) next to random words; section 5 needs no reference at all (delta tables on zero masks: the answer is one monomial).  Every
comparison is np.array_equal on Int32 words."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_independent import CASES, MKSchoolbook, Schoolbook, _keys, monomial, negacyclic, wrap32
from test_mk_gates import MKGateRef, OPS
from test_mk_pbs import mkref  # noqa: F401  (the compile recipe of tests/pbs_ref/mk_pbs_ref.c)
from test_pbs import FAMILIES
from test_pbs_multi import checkers  # noqa: F401  (the compile recipe of pbs_ref.c and pbs_multi_ref.c)

MU = 2**29


def _i32(a):
    return np.ascontiguousarray(wrap32(a), np.int32)


# ---- 4. edge inputs ------------------------------------------------------------------------------------------------------------------
def edge_rows(rng, w, N, random_rows=3):
    """Sample rows [R][w + 1] (w mask words, then the body).  With s = 32 - log2(2N) a word b 2^s decodes to exponent b
    (numeric-functions.jl:30-33).  Rows with different zero patterns alternate, so kernels that put two or more rows in one
    workgroup (h2, w2 pairs, rw groups) see them together."""
    s = 32 - (2 * N).bit_length() + 1
    one, half = 1 << s, 1 << (s - 1)
    rows = []

    def row(mask=None, body=0):
        r = np.zeros(w + 1, np.int64)
        for i, v in (mask or {}).items():
            r[i] = v
        r[w] = body
        rows.append(r)

    row()                                           # every word zero: every bara is 0 (the skip at bootstrap.jl:34), barb = 0: trivial extraction of v
    row({0: one})                                   # body zero, exactly one non-zero bara: +1 at index 0
    row(body=-N * one)                              # mask zero, barb = -N: X^N v = -v
    row({i: -2**31 for i in range(w)}, 3 * one + 5)  # every mask word decodes to -N: X^-N - 1 = -2, a doubling that wraps, at every step
    row(body=-one)                                  # barb = -1: v[N-1] wraps to coefficient 0 with a sign change
    row({w - 1: -one})                              # one bara = -1 at the last index
    row(body=one)                                   # barb = 1
    row({0: -2**31})                                # one bara = -N at index 0
    row(body=(N - 1) * one)                         # barb = N - 1, the last exponent before the wrap
    row({w - 1: one})                               # one bara = +1 at the last index
    row({0: -one})                                  # one bara = -1 at index 0
    row({w - 1: -2**31})                            # one bara = -N at the last index
    if w > 2:
        row({w // 2: 5 * one})                      # one bara in the middle (the first word of party 1 when w = 2 n)
    for b in (0, -1, 5, -N, N - 1):                 # rounding boundary of the modulus switch on the body
        row(body=b * one + half - 1)                #   decodes to b
        row(body=b * one + half)                    #   decodes to b + 1 (b = N - 1: wraps to -N)
    row(body=2**31 - 1)                             # the largest word: wraps to barb = -N
    row({0: half - 1})                              # a non-zero mask word that decodes to 0: still skipped
    row({0: half})                                  # ... and the next word up decodes to 1
    row({w - 1: 2**31 - 1})                         # mask word 2^31 - 1 wraps to bara = -N
    row({1 % w: -half})                             # -2^(s-1) decodes to 0
    row({1 % w: -half - 1}, 7 * one)                # -2^(s-1) - 1 decodes to -1
    for _ in range(random_rows):
        rows.append(rng.integers(-2**31, 2**31, size=w + 1, dtype=np.int64))
    return _i32(np.stack(rows))


def edge_tables(rng, N):
    """Test polynomials [8][N]."""
    t = np.zeros((8, N), np.int64)
    t[0] = rng.integers(-2**31, 2**31, size=N, dtype=np.int64)     # uniform random Int32
    t[1] = -2**31                                                  # every entry -2^31: its negation is itself
    t[2] = 2**31 - 1                                               # every entry 2^31 - 1
    t[3, 0::2], t[3, 1::2] = -2**31, 2**31 - 1                     # alternating extremes
    t[4, 0] = 2**29 + 12345                                        # deltas: one non-zero coefficient at 0, 1 and N - 1
    t[5, 1] = -2**31
    t[6, N - 1] = 1
    t[7] = rng.integers(-2**31, 2**31, size=N, dtype=np.int64)
    return _i32(t)


def table_index(rows, n_tv=8):
    return ((3 * np.arange(rows) + 1) % n_tv).astype(np.int32)      # 3 and 8 coprime: every table is used, neighbours differ


def combine(rows, start, wire, coef, cst):
    """The samples a level bootstraps, in Python integers mod 2^32: row g = sum over its terms of coef * wire (LweSample * Integer,
    lwe.jl:77-80, every word wraps), summed (lwe.jl:67-68), plus the trivial sample (0, cst[g]) (lwe.jl:63-64: the body only)."""
    B, width = len(start) - 1, len(rows[0])
    out = []
    for g in range(B):
        acc = [0] * width
        for t in range(int(start[g]), int(start[g + 1])):
            c, r = int(coef[t]), rows[int(wire[t])]
            acc = [(a + c * int(v)) % 2**32 for a, v in zip(acc, r)]
        if cst is not None:
            acc[-1] = (acc[-1] + int(cst[g])) % 2**32
        out.append(acc)
    return _i32(np.array(out, dtype=object).astype(np.int64).reshape(B, width))


def edge_level(rng, rows, N):
    """A level over the wires `rows` that hits the coefficient edges: returns (start, wire, coef, cst)."""
    s = 32 - (2 * N).bit_length() + 1
    one, half = 1 << s, 1 << (s - 1)
    n_in = len(rows)
    terms, cst = [], []

    def add(ts, c):
        terms.append(ts)
        cst.append(c)

    add([(0, -2**31), (1, -1), (2, 0), (3, 1), (4, 2**31 - 1)], 12345)        # every extreme coefficient in one row
    add([(n_in - 1, 3), (n_in - 1, -2**31)], -one)                            # the same wire twice in one row
    add([], 5 * one)                                                          # a LUT row with no terms: a pure barb rotation
    add([(int(rng.integers(0, n_in)), int(rng.integers(-2**31, 2**31))) for _ in range(70)], 0)       # many terms (>= 64)
    add([], -N * one)                                                         # no terms, barb = -N
    add([(n_in - 2, 2**31 - 1), (n_in - 3, 2**31 - 1)], 3 * one + half - 1)   # cst just below the rounding boundary (on zero-mask wires it decides barb)
    add([], 3 * one + half)                                                   # ... and on it: barb = 4
    add([], 3 * one + half - 1)                                               # ... just below: barb = 3
    add([(n_in - 1, 1)], 2**31 - 1)                                           # cst the largest word
    add([(5, -1), (5, 1)], (N - 1) * one)                                     # a wire that cancels itself
    add([(int(rng.integers(0, n_in)), int(rng.integers(-3, 4))) for _ in range(5)], int(rng.integers(-2**31, 2**31)))
    start = np.concatenate([[0], np.cumsum([len(t) for t in terms])]).astype(np.int32)
    wire = np.array([t[0] for ts in terms for t in ts], np.int32)
    coef = _i32(np.array([t[1] for ts in terms for t in ts], np.int64))
    return start, wire, coef, _i32(np.array(cst, np.int64))


# ---- expected words --------------------------------------------------------------------------------------------------------------------
def coefficient_of(j, N, n_out):
    """c_j: the accumulator coefficient at which sample j of n_out is extracted (a function of its own so that
    tests/test_pbs_fuzz.py can replace it by a wrong one and see the expected words move)."""
    return j * (N // n_out)


def table_of(tables, index, g):
    """Row g's test polynomial: tables[index[g]], table 0 without an index (its own function for the same reason)."""
    return tables[0 if index is None else index[g]]


def expected(sb, tables, index, x, n_outs, mk=False):
    """{(n_out, with_keyswitch): int32 [B][n_out][width]} from one schoolbook rotation per row: bootstrap_tv / mk_bootstrap_tv for every
    n_out at once (the accumulator and the samples at shared coefficients are computed once)."""
    rotate, extract, keyswitch = (sb.mk_rotate, sb.mk_extract_at, sb.mk_keyswitch) if mk else (sb.rotate, sb.extract_at, sb.keyswitch)
    N = sb.N
    cs = sorted({coefficient_of(j, N, K) for K in n_outs for j in range(K)})
    per_row = []
    for g, row in enumerate(x):
        acc = rotate(table_of(tables, index, g), row)
        ext = {c: extract(acc, c) for c in cs}
        per_row.append((ext, {c: keyswitch(ext[c]) for c in cs}))
    return {(K, ks): _i32(np.array([[r[ks][coefficient_of(j, N, K)] for j in range(K)] for r in per_row])) for K in n_outs for ks in (False, True)}


class _Case:
    """One single-key set with its schoolbook, edge rows, edge tables and expected words."""

    def __init__(self, tfhe, N, k, l, beta, n, n_outs, seed, random_rows=3):
        self.p, self.rng, self.sk, self.ck = _keys(tfhe, N, k, l, beta, n, seed)
        self.sb = Schoolbook(n, N, k, l, beta, 8, 2, self.ck.bootstrap_key, self.ck.keyswitch_key)
        self.x = edge_rows(self.rng, n, N, random_rows)
        self.tables = edge_tables(self.rng, N)
        self.index = table_index(len(self.x))
        self.n_outs = n_outs
        self.want = expected(self.sb, self.tables, self.index, self.x, n_outs)


def _short_n(i):
    return 3 + i % 6            # short keys: n between 3 and 8


def _n_outs(N, anyn=False):
    return (1, 2, 8) + ((32,) if N == 1024 else ()) + ((N // 4,) if anyn and N in (32, 64) else ())


# every family of test_pbs, and the any-N kernel at a degree where n_out = N / 4 is small enough to run
ALL_FAMILIES = list(FAMILIES) + [("anyn64", 64, 1, 2, 7, {}, 5)]
# what tfhe_last_kernel_name must contain (and must not) for the family to have run: the names engine_dispatch.hip gives
KERNEL_OF = {
    "h2": ("_kernel_h2<", None), "w2": ("_kernel_w2<", ",rw2"), "w2_rw2": ("_kernel_w2<3,rw2", None), "v3": ("_kernel_v3<", "rw4"),
    "v3_rw4": ("_kernel_v3<3,8,tw2reg,rw4", None), "v3_rt_l": ("_kernel_v3<0", "rw4"), "general": ("_kernel_general(", None),
    "k2_w3": ("_kernel_k2w3<", None), "k2_rw": ("_kernel_k2<3,rw7", None), "k2_single": ("_kernel_k2<2>", None),
    "n512_w2": ("_kernel_n512w2<", None), "n512": ("_kernel_n512<", "rw4"), "n512_rw": ("_kernel_n512<3,rw4", None),
    "n2048_rw1": ("_kernel_n2048x<3,rw1", None), "n2048_rw": ("_kernel_n2048x<3,rw2", None), "anyn": ("_kernel_anyn(N=256", None),
    "anyn64": ("_kernel_anyn(N=64", None),
}


def _family_case(i):
    import tfhe_jl_amd as tfhe
    name, N, k, l, beta, opts, rows = ALL_FAMILIES[i]
    return _Case(tfhe, N, k, l, beta, _short_n(i), _n_outs(N, name.startswith("anyn")), 4000 + i)


# ---- 2. CPU: the checkers and the oracle's multi-key pieces against the schoolbook ----------------------------------------------------------
class _Orc:
    """An oracle object holding a cloud key (the checkers take their key arrays from it)."""

    def __init__(self, orc, p, ck, parties=1):
        self.oracle = orc.Oracle(p.lwe_size, p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length, p.bs_log2_base,
                                 p.ks_decomp_length, p.ks_log2_base, parties=parties)
        self.oracle.load_bootstrap_key(ck.bootstrap_key)
        self.oracle.load_keyswitch_key(ck.keyswitch_key)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pbs_ref(lib, o, mode, tables, index, x, ks):
    assert lib.orc_init(C.c_int32(o.N)) == 0
    out = np.zeros((len(x), o.n + 1 if ks else o.k * o.N + 1), np.int32)
    assert lib.pbs_bootstrap_batch(C.byref(o.P), _ptr(o.bk_re), _ptr(o.bk_im), _ptr(o.bk_i32), _ptr(o.ks), mode, _ptr(tables), _ptr(index),
                                   _ptr(x), _ptr(out), len(x), int(ks)) == 0
    return out


def _pbs_multi_ref(lib, o, mode, tables, index, x, n_out, ks):
    assert lib.orc_init(C.c_int32(o.N)) == 0
    out = np.zeros((len(x), n_out, o.n + 1 if ks else o.k * o.N + 1), np.int32)
    assert lib.pbs_multi_batch(C.byref(o.P), _ptr(o.bk_re), _ptr(o.bk_im), _ptr(o.bk_i32), _ptr(o.ks), mode, _ptr(tables), _ptr(index), n_out,
                               _ptr(x), _ptr(out), len(x), int(ks)) == 0
    return out


def _mk_pbs_ref(lib, o, mode, tables, index, x, n_out, ks):
    assert lib.orc_init(C.c_int32(o.N)) == 0
    P = o.parties
    out = np.zeros((len(x), n_out, P * o.n + 1 if ks else P * o.N + 1), np.int32)
    assert lib.mk_pbs_multi_batch(C.byref(o.P), P, _ptr(o.bk_re), _ptr(o.bk_im), _ptr(o.bk_i32), _ptr(o.ks), mode, _ptr(tables), _ptr(index),
                                  n_out, _ptr(x), _ptr(out), len(x), int(ks)) == 0
    return out


def test_extract_at_is_the_phase_coefficient():
    """extract_at against the definition it is written from, word by word: with the TLWE key s = X^u (one bit set) the phase
    body - p s has coefficient c equal to body[c] - (X^u p)[c], so the extracted mask word u is coefficient c of X^u p (monomial());
    with a random binary key the extracted sample's LWE phase is coefficient c of body - sum p_i s_i (negacyclic())."""
    rng = np.random.default_rng(55)
    for k, N in ((1, 32), (2, 16), (1, 64)):
        sb = Schoolbook(1, N, k, 2, 7, 8, 2, np.zeros((1, 2, k + 1, k + 1, N), np.int32))
        acc = [rng.integers(-2**31, 2**31, size=N, dtype=np.int64) for _ in range(k + 1)]
        s = rng.integers(0, 2, size=(k, N))
        phase = wrap32(acc[k] - sum(negacyclic(acc[i], s[i], N) for i in range(k)))
        for c in range(N):
            e = sb.extract_at(acc, c)
            for i in range(k):
                assert [int(e[i * N + u]) for u in range(N)] == [int(wrap32(monomial(acc[i], u, N)[c])) for u in range(N)], (k, N, c, i)
            assert e[k * N] == acc[k][c]
            assert int(wrap32(int(e[k * N]) - int(np.dot(e[:k * N], s.reshape(-1))))) == int(phase[c]), (k, N, c)
        # coefficient 0 is tlwe_extract_sample as the mu path has always written it (tlwe.jl:55-59)
        e0 = sb.extract_at(acc, 0)
        for i in range(k):
            assert e0[i * N] == acc[i][0] and np.array_equal(e0[i * N + 1:(i + 1) * N], wrap32(-acc[i][:0:-1]))


def test_edge_rows_decode_as_documented(tfhe):
    """The edge rows really produce the exponents their comments name (the schoolbook's decode is numeric-functions.jl:30-33)."""
    for N in (64, 512, 1024, 2048):
        w = 5
        sb = Schoolbook(w, N, 1, 2, 7, 8, 2, np.zeros((w, 2, 2, 2, N), np.int32))
        x = edge_rows(np.random.default_rng(1), w, N, 0)
        ex = np.array([sb.modswitch(r) for r in x])
        assert not ex[0].any()
        assert ex[1].tolist() == [1, 0, 0, 0, 0, 0] and ex[2].tolist() == [0, 0, 0, 0, 0, -N]
        assert ex[3].tolist() == [-N] * w + [3] and ex[4, w] == -1 and ex[5, w - 1] == -1 and ex[6, w] == 1
        assert ex[7, 0] == -N and ex[8, w] == N - 1 and ex[9, w - 1] == 1 and ex[10, 0] == -1 and ex[11, w - 1] == -N
        assert ex[13:23, w].tolist() == [0, 1, -1, 0, 5, 6, -N, -N + 1, N - 1, -N] and not ex[13:23, :w].any()
        assert ex[23, w] == -N
        assert not ex[24].any() and ex[25].tolist() == [1, 0, 0, 0, 0, 0] and ex[26, w - 1] == -N
        assert not ex[27].any() and ex[28].tolist() == [0, -1, 0, 0, 0, 7]
        zero_masks = [g for g in range(len(x)) if not ex[g, :w].any()]
        assert len(zero_masks) >= 17 and 0 < len(zero_masks) < len(x)


def test_combine_wraps_every_word():
    rows = _i32(np.array([[2**31 - 1, -2**31, 7], [1, -1, 2**31 - 1]], np.int64))
    got = combine(rows, [0, 2, 2, 3], [0, 1, 1], _i32(np.array([2, -2**31, 2**31 - 1], np.int64)), _i32(np.array([1, -5, 2**31 - 1], np.int64)))
    # row 0: 2 (2^31 - 1) - 2^31 = 2^31 - 2; -2^32 + 2^31 -> -2^31; 14 - 2^31 (2^31 - 1) -> 14 - 2^31, + 1.  row 2: (2^31 - 1)^2 = 1 mod 2^32
    assert got.tolist() == [[2**31 - 2, -2**31, 15 - 2**31], [0, 0, -5], [2**31 - 1, -2**31 + 1, -2**31]]


CPU_SETS = [(1024, 1, 2, 10, 5), (256, 2, 2, 8, 3), (2048, 1, 3, 7, 3)]          # N, k, l, beta, n


@pytest.mark.parametrize("N,k,l,beta,n", CPU_SETS)
def test_checkers_equal_schoolbook(orc, tfhe, checkers, N, k, l, beta, n):  # noqa: F811
    """tests/pbs_ref/pbs_ref.c and pbs_multi_ref.c (n_out = 1, 2, 8, 32), both product back-ends, with and without keyswitch, on the
    edge rows and edge tables: the schoolbook's words."""
    c = _Case(tfhe, N, k, l, beta, n, (1, 2, 8, 32), 3000 + N + k)
    o = _Orc(orc, c.p, c.ck).oracle
    # the shared-coefficient helper is bootstrap_tv itself
    for g in (3, len(c.x) - 1):
        for ks in (False, True):
            assert np.array_equal(c.want[8, ks][g], _i32(c.sb.bootstrap_tv(c.tables[c.index[g]], c.x[g], 8, ks))), (g, ks)
    for mode in (orc.MODE_FFT, orc.MODE_EXACT):
        for ks in (False, True):
            assert np.array_equal(_pbs_ref(checkers["pbs_ref"], o, mode, c.tables, c.index, c.x, ks), c.want[1, ks][:, 0]), (mode, ks)
            for n_out in (1, 2, 8, 32):
                got = _pbs_multi_ref(checkers["pbs_multi_ref"], o, mode, c.tables, c.index, c.x, n_out, ks)
                assert np.array_equal(got, c.want[n_out, ks]), (mode, ks, n_out)
    c.ck.close()


def _mk_keys(tfhe, parties, l, beta, n, seed, N=1024, t=8, gamma=2):
    p = tfhe.SchemeParameters(n, 0.012467, N, 1, l, beta, 3.29e-10, t, gamma, 2.44e-5, parties)
    rng = np.random.default_rng(seed)
    sks = [tfhe.SecretKey(rng, p) for _ in range(parties)]
    shared = tfhe.SharedKey(rng, p)
    ck = tfhe.MKCloudKey([tfhe.CloudKeyPart(rng, sk, shared) for sk in sks])
    return p, rng, sks, ck, MKSchoolbook(n, N, l, beta, t, gamma, parties, ck.bootstrap_key, ck.keyswitch_key)


class _MKCase:
    def __init__(self, parties, l, beta, n, N, n_outs, random_rows):
        import tfhe_jl_amd as tfhe
        self.parties, self.n, self.N = parties, n, N
        self.p, self.rng, self.sks, self.ck, self.sb = _mk_keys(tfhe, parties, l, beta, n, 6000 + parties + N, N)
        self.x = edge_rows(self.rng, parties * n, N, random_rows)
        self.tables = edge_tables(self.rng, N)
        self.index = table_index(len(self.x))
        self.n_outs = n_outs
        self.want = expected(self.sb, self.tables, self.index, self.x, n_outs, mk=True)


# parties -> (l, beta, n, N, random rows): the gadget shapes of mktfhe_parameters_2party / _4party / _8party (mk_api.jl:4-34), short keys
MK_SETS = {2: (4, 7, 3, 1024, 3), 4: (5, 6, 3, 1024, 2), 8: (8, 4, 2, 1024, 1), "anyn": (4, 7, 3, 512, 3)}


@functools.lru_cache(maxsize=None)
def _mk_case(which):
    l, beta, n, N, rnd = MK_SETS[which]
    return _MKCase(2 if which == "anyn" else which, l, beta, n, N, (1, 2, 8), rnd)


@pytest.mark.parametrize("which", [2, 4])
def test_mk_checker_equals_schoolbook(orc, mkref, which):  # noqa: F811
    """tests/pbs_ref/mk_pbs_ref.c (n_out = 1, 2, 8), both product back-ends, with and without keyswitch, at 2 and 4 parties."""
    c = _mk_case(which)
    o = _Orc(orc, c.p, c.ck, c.parties).oracle
    g = len(c.x) - 1
    assert np.array_equal(c.want[2, True][g], _i32(c.sb.mk_bootstrap_tv(c.tables[c.index[g]], c.x[g], 2, True)))
    for mode in (orc.MODE_FFT, orc.MODE_EXACT):
        for ks in (False, True):
            for n_out in c.n_outs:
                got = _mk_pbs_ref(mkref.lib, o, mode, c.tables, c.index, c.x, n_out, ks)
                assert np.array_equal(got, c.want[n_out, ks]), (mode, ks, n_out)


class _MKGateCase:
    """Every opcode of tfhe_mk_gates_batch, twice: on arbitrary words, and on rows taken from the edge set."""

    def __init__(self, parties):
        import tfhe_jl_amd as tfhe
        l, beta, n, N, _ = MK_SETS[parties]
        n = 2 if parties == 4 else n
        self.parties = parties
        self.p, rng, self.sks, self.ck, self.sb = _mk_keys(tfhe, parties, l, beta, n, 6500 + parties)
        self.names = list(OPS) + list(OPS)
        B, w = len(self.names), parties * n + 1
        self.ops = np.array([OPS[nm] for nm in self.names], np.uint8)
        edges = edge_rows(rng, w - 1, N, 0)
        self.x, self.y, self.z = (rng.integers(-2**31, 2**31, size=(B, w), dtype=np.int64).astype(np.int32) for _ in range(3))
        pick = rng.permutation(len(edges))
        for i in range(B // 2, B):                       # second half: edge rows as operands (sums and doublings of them reach the wraps)
            self.x[i], self.y[i] = edges[pick[i % len(edges)]], edges[pick[(i + 7) % len(edges)]]
        self.z[B // 2:] = edges[3]                       # (every mask word -2^31)
        self.want = _i32(np.stack([self.sb.mk_gate(nm, self.x[g], self.y[g], self.z[g]) for g, nm in enumerate(self.names)]))


@functools.lru_cache(maxsize=None)
def _mk_gate_case(parties):
    return _MKGateCase(parties)


@pytest.mark.parametrize("parties", [2, 4])
def test_oracle_mk_gates_equal_schoolbook(orc, parties):
    """The oracle's multi-key gate layer (its exported orc_mk_bootstrap_wo_keyswitch and orc_mk_keyswitch under the gates.jl prologues of
    tests/test_mk_gates.py's MKGateRef, which every multi-key gate test compares with) against mk_gate, all 15 opcodes."""
    c = _mk_gate_case(parties)
    ref = MKGateRef(orc, _Orc(orc, c.p, c.ck, parties).oracle)
    got = ref.batch(c.ops, c.x, c.y, c.z)
    for g, nm in enumerate(c.names):
        assert np.array_equal(got[g], c.want[g]), (nm, g)
    assert np.array_equal(c.want[0], _i32(c.sb.mk_gate_nand(c.x[0], c.y[0])))


# ---- 3. GPU: the engine against the schoolbook (no oracle, no checker) ----------------------------------------------------------------------
def _run_tv(eng, c, mk=False):
    """Every n_out of the case, with and without keyswitch, through the single-output and the multi-output entry points."""
    one, multi = (eng.mk_bootstrap_tv, eng.mk_bootstrap_tv_multi) if mk else (eng.bootstrap_tv, eng.bootstrap_tv_multi)
    names = set()
    for ks in (False, True):
        got = one(c.tables, c.x, index=c.index, with_keyswitch=ks)
        names.add(eng.last_kernel_name())
        assert np.array_equal(got, c.want[1, ks][:, 0]), ("one", ks, np.nonzero((got != c.want[1, ks][:, 0]).any(axis=1))[0])
        for n_out in c.n_outs:
            got = multi(c.tables, c.x, n_out, index=c.index, with_keyswitch=ks)
            names.add(eng.last_kernel_name())
            assert eng.last_rotation_count() == len(c.x)
            assert np.array_equal(got, c.want[n_out, ks]), (n_out, ks, np.nonzero((got != c.want[n_out, ks]).any(axis=(1, 2)))[0])
    return names


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(ALL_FAMILIES)), ids=[f[0] for f in ALL_FAMILIES])
def test_gpu_tv_families_equal_schoolbook(tfhe, i):
    """tfhe_bootstrap_tv_batch and tfhe_bootstrap_tv_multi_batch, every kernel family, on the edge rows and tables with a per-row index,
    n_out = 1, 2, 8 (32 at N = 1024, N / 4 on the any-N kernel at N = 64), with and without keyswitch."""
    name, N, k, l, beta, opts, rows = ALL_FAMILIES[i]
    c = _family_case(i)
    eng = c.ck.engine(0)
    for o, v in opts.items():
        eng.set_option(o, v)
    eng.bootstrap(MU, c.x, with_keyswitch=False)
    mu_kernel = eng.last_kernel_name()
    has, has_not = KERNEL_OF[name]
    assert has in mu_kernel and (has_not is None or has_not not in mu_kernel), (name, mu_kernel)
    assert _run_tv(eng, c) == {mu_kernel + "+tv"}, name
    c.ck.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", [cs for cs in CASES if cs[:4] in ((4096, 1, 3, 7), (256, 2, 2, 8), (1024, 5, 1, 8))])
def test_gpu_tv_other_shapes_equal_schoolbook(tfhe, N, k, l, beta, n):
    """The shapes of test_independent.CASES that no family reaches, through the TV entry points."""
    c = _Case(tfhe, N, k, l, beta, n, (1, 2, 8), 900 + N + k + l)
    eng = c.ck.engine(0)
    names = _run_tv(eng, c)
    assert len(names) == 1 and names.pop().endswith("+tv")
    c.ck.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["80", "128"])
def test_gpu_tv_full_size_equals_schoolbook(tfhe, keys80, keys128, which):
    """The shipped parameter sets at full size: one random row and one edge row (every mask word decodes to -N: 500 / 630 doublings,
    body 2^31 - 1), one table of random words, n_out = 4, with and without keyswitch."""
    K = keys80 if which == "80" else keys128
    p = K.params
    n, N = p.lwe_size, p.tlwe_polynomial_degree
    sb = Schoolbook(n, N, p.tlwe_mask_size, p.bs_decomp_length, p.bs_log2_base, p.ks_decomp_length, p.ks_log2_base, K.ck.bootstrap_key,
                    K.ck.keyswitch_key)
    rng = np.random.default_rng(4040 + int(which))
    x = rng.integers(-2**31, 2**31, size=(2, n + 1), dtype=np.int64).astype(np.int32)
    x[1, :n], x[1, n] = -2**31, 2**31 - 1
    table = rng.integers(-2**31, 2**31, size=(1, N), dtype=np.int64).astype(np.int32)
    want = expected(sb, table, None, x, (4,))
    eng = K.ck.engine(0)
    for ks in (False, True):
        assert np.array_equal(eng.bootstrap_tv_multi(table, x, 4, with_keyswitch=ks), want[4, ks]), ks
        assert eng.last_kernel_name().endswith("+tv")
        assert np.array_equal(eng.bootstrap_tv(table, x, with_keyswitch=ks), want[4, ks][:, 0]), ks


def _level_case(tfhe, mk):
    if mk:
        c = _mk_case("anyn")
        rows = c.x[-3:]                                  # a 3-row level over the random rows ...
        start, wire, coef = np.array([0, 2, 2, 5], np.int32), np.array([0, 1, 2, 2, 0], np.int32), _i32(np.array([1, -2**31, 2**31 - 1, -1, 3], np.int64))
        s = 32 - (2 * c.N).bit_length() + 1
        cst = _i32(np.array([12345, -c.N << s, (3 << s) + (1 << (s - 1))], np.int64))       # ... one row without terms (barb = -N), cst on the boundary
        return c, rows, start, wire, coef, cst
    c = _Case(tfhe, 1024, 1, 2, 10, 4, (1, 4), 7100, random_rows=3)
    start, wire, coef, cst = edge_level(c.rng, c.x, 1024)
    return c, c.x, start, wire, coef, cst


@pytest.mark.gpu
def test_gpu_levels_equal_schoolbook(tfhe):
    """tfhe_lut_level (n_out = 1, 4) and tfhe_linear_level over a wire table holding the edge rows, on a level of edge terms: the
    integer combination, and the schoolbook's bootstrap_tv of it."""
    c, rows, start, wire, coef, cst = _level_case(tfhe, False)
    B, n_in = len(start) - 1, len(rows)
    x = combine(rows, start, wire, coef, cst)
    index = table_index(B)
    want = expected(c.sb, c.tables, index, x, (1, 4))
    eng = c.ck.engine(0)
    eng.wires_alloc(n_in + 5 * B)
    eng.wires_upload(0, rows)
    out_lin = np.arange(n_in, n_in + B, dtype=np.int32)
    eng.linear_level(start, wire, coef, cst, out_lin)
    assert np.array_equal(eng.wires_gather(out_lin), x)
    eng.linear_level(start, wire, coef, None, out_lin)
    assert np.array_equal(eng.wires_gather(out_lin), combine(rows, start, wire, coef, None))
    for n_out in (1, 4):
        out = (n_in + B + np.random.default_rng(n_out).permutation(B * n_out)).astype(np.int32)
        eng.lut_level(c.tables, start, wire, coef, cst, out, index=index, n_out=n_out)
        assert eng.last_rotation_count() == B and eng.last_kernel_name().endswith("+tv")
        assert np.array_equal(eng.wires_gather(out).reshape(B, n_out, -1), want[n_out, True]), n_out
    c.ck.close()


MK_NAMES = {2: "mk_blind_rotate_kernel_w2<4>", 4: "mk_blind_rotate_kernel_g2<4,5,acc=lds>", 8: "mk_blind_rotate_kernel_g2<8,8>",
            "anyn": "mk_blind_rotate_kernel_anyn(N=512,P=2,l=4)"}
MK_OPTIONS = {                                           # 2 parties: the options as tests/test_mk_pbs.py forces them (and lockstep pairs of w2)
    "w2": ({}, MK_NAMES[2]), "w2_pairs": ({"mk_rw": 2}, MK_NAMES[2]),
    "mk_general": ({"mk_general": 1}, "mk_blind_rotate_kernel_general(P=2,L=4)"),
    "mkg_rw": ({"mk_general": 1, "mkg_rw": 1}, "mk_blind_rotate_kernel_general(P=2,L=4)"),
    "mkg_acc": ({"mk_general": 1, "mkg_acc": 1}, "mk_blind_rotate_kernel_general(P=2,L=4,acc=global)"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("option", list(MK_OPTIONS))
def test_gpu_mk_tv_two_parties_equal_schoolbook(option):
    c = _mk_case(2)
    opts, name = MK_OPTIONS[option]
    eng = c.ck.engine(0)
    before = {k: eng.get_option(k) for k in opts}
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        assert _run_tv(eng, c, mk=True) == {name + "+tv"}
    finally:
        for k, v in before.items():
            eng.set_option(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [4, 8, "anyn"])
def test_gpu_mk_tv_many_parties_and_any_n_equal_schoolbook(which):
    """4 and 8 parties (mk_blind_rotate_kernel_g2, both row groupings) and a 2-party set at N = 512 (the any-N kernel)."""
    c = _mk_case(which)
    eng = c.ck.engine(0)
    try:
        for rw in ((2, 4) if which != "anyn" else (0,)):
            eng.set_option("mkg_rw", rw)
            assert _run_tv(eng, c, mk=True) == {MK_NAMES[which] + "+tv"}, rw
    finally:
        eng.set_option("mkg_rw", 0)


@pytest.mark.gpu
def test_gpu_mk_levels_equal_schoolbook(tfhe):
    """tfhe_mk_lut_level (n_out = 1, 2) and tfhe_mk_linear_level on a 3-row level of the any-N multi-key set."""
    c, rows, start, wire, coef, cst = _level_case(tfhe, True)
    x = combine(rows, start, wire, coef, cst)
    index = np.array([0, 5, 3], np.int32)
    want = expected(c.sb, c.tables, index, x, (1, 2), mk=True)
    eng = c.ck.engine(0)
    eng.mk_wires_alloc(16)
    eng.wires_upload(0, rows)
    eng.mk_linear_level(start, wire, coef, cst, [3, 4, 5])
    assert np.array_equal(eng.wires_download(3, 3), x)
    for n_out, out in ((1, [8, 6, 7]), (2, [9, 10, 11, 12, 13, 14])):
        eng.mk_lut_level(c.tables, start, wire, coef, cst, out, index=index, n_out=n_out)
        assert eng.last_kernel_name() == MK_NAMES["anyn"] + "+tv" and eng.last_rotation_count() == 3
        assert np.array_equal(eng.wires_gather(out).reshape(3, n_out, -1), want[n_out, True]), n_out


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [2, 4])
def test_gpu_mk_gates_equal_schoolbook(parties):
    """tfhe_mk_gates_batch, all 15 opcodes (MUX: two rotations, one keyswitch) on arbitrary words and on edge rows."""
    c = _mk_gate_case(parties)
    eng = c.ck.engine(0)
    got = eng.mk_gates_batch(c.ops, c.x, c.y, c.z)
    assert eng.last_kernel_name().startswith({2: "mk_blind_rotate_kernel_w2<4", 4: "mk_blind_rotate_kernel_g2<4,5"}[parties]), eng.last_kernel_name()
    assert eng.last_rotation_count() == sum(2 if nm == "MUX" else 0 if nm in ("NOT", "COPY", "CONST0", "CONST1") else 1 for nm in c.names)
    for g, nm in enumerate(c.names):
        assert np.array_equal(got[g], c.want[g]), (nm, g)


# ---- 5. closed form: a delta table on zero masks ----------------------------------------------------------------------------------------
DELTA, DELTA_AT = -2**31 + 3, 1                          # v = DELTA X^1


@functools.lru_cache(maxsize=4)
def _delta_rotations(N, exponents):
    """X^{-e} v for the delta table v and every exponent e of the tuple: int64 [len(exponents)][N], shared by the n_out of one set."""
    v = np.zeros(N, np.int64)
    v[DELTA_AT] = DELTA
    return v, np.stack([wrap32(monomial(v, -int(e), N)) for e in exponents])


@functools.lru_cache(maxsize=None)
def closed_form(N, n_out, exponents=None):
    """All 2N body values b 2^s, b in [-N, N) (or the exponents of the tuple `exponents`, for degrees at which 2N rows are too many),
    and the un-keyswitched bodies they must give: the mask is zero, so nothing rotates after testvectbis = X^{-barb} v
    (bootstrap.jl:54) and sample j's body is coefficient j N / n_out of that monomial product."""
    s = 32 - (2 * N).bit_length() + 1
    b = np.arange(-N, N) if exponents is None else np.array(exponents, np.int64)
    v, rotated = _delta_rotations(N, tuple(int(e) for e in b))
    bodies = rotated[:, [j * (N // n_out) for j in range(n_out)]]
    return _i32(v), _i32(b << s), _i32(bodies)


def _assert_closed_form(got, bodies):
    """got [2N][n_out][width]: zero masks and the bodies of the monomial; each is +-DELTA or 0."""
    assert not got[:, :, :-1].any()
    assert np.array_equal(got[:, :, -1], bodies)
    assert set(np.unique(bodies)) == {int(wrap32(-DELTA)), 0, DELTA}


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [(1024, 1, 2, 10), (512, 1, 2, 7), (2048, 1, 3, 7), (128, 1, 2, 7)])
def test_gpu_delta_table_closed_form(tfhe, N, k, l, beta):
    """tfhe_bootstrap_tv_batch / _multi_batch, un-keyswitched, and tfhe_lut_level (rows without terms, cst = b 2^s; the keyswitch of
    a sample with a zero mask subtracts nothing, keyswitch.jl:66-68, so the wire is (0, body)): 2N rows, one per exponent."""
    n = 4
    p, rng, sk, ck = _keys(tfhe, N, k, l, beta, n, 5000 + N)
    eng = ck.engine(0)
    for n_out in (1, 4):
        v, body, want = closed_form(N, n_out)
        x = np.zeros((2 * N, n + 1), np.int32)
        x[:, n] = body
        if n_out == 1:
            _assert_closed_form(eng.bootstrap_tv(v, x, with_keyswitch=False)[:, None], want)
        _assert_closed_form(eng.bootstrap_tv_multi(v, x, n_out, with_keyswitch=False), want)
        eng.wires_alloc(2 * N * n_out)
        eng.lut_level(v, np.zeros(2 * N + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), body,
                      np.arange(2 * N * n_out, dtype=np.int32), n_out=n_out)
        _assert_closed_form(eng.wires_download(0, 2 * N * n_out).reshape(2 * N, n_out, n + 1), want)
    ck.close()


@pytest.mark.gpu
def test_gpu_mk_delta_table_closed_form():
    """The same through tfhe_mk_bootstrap_tv_multi_batch at 2 parties (N = 1024, 2048 rows)."""
    c = _mk_case(2)
    eng = c.ck.engine(0)
    for n_out in (1, 4):
        v, body, want = closed_form(c.N, n_out)
        x = np.zeros((2 * c.N, 2 * c.n + 1), np.int32)
        x[:, -1] = body
        _assert_closed_form(eng.mk_bootstrap_tv_multi(v, x, n_out, with_keyswitch=False), want)
