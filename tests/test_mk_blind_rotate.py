"""Multi-key blind rotation of the caller's MK TLWE accumulators (tfhe_mk_blind_rotate_batch; Engine.mk_blind_rotate; tfhe_jl_amd.leveled's
mk_bootstrap_key_selectors, mk_private_lut_encrypt, mk_blind_rotate_lookup, mk_two_stage_lookup, mk_pbs_to_tlwe) against an integer
schoolbook.

The reference of every word comparison is `MKRotation` below: tests/test_mk_leveled.py's `MKTree` (mk_tgsw_extern_mul, mk_internals.jl:348-391,
as exact int64 np.convolve) with three additions written from the reference — `rotate`, mk_blind_rotate (:473-485) from a FULL accumulator
(mk_mul_by_monomial, :79-85, on all P + 1 polynomials, then cmux(s, A, X^e A) = mk_mux_rotate, :464-470, per live step), `rotate_lwe`
with the modulus switch of :502-503 (decode_message(v, 2N), numeric-functions.jl:31-34) and `extract_at`, mk_tlwe_extract_sample (:88-95)
at a coefficient c.  It never touches the engine, and of the oracle only the gadget constants MKTree reads.  At full size the expected
words come from the test-only checker tests/pbs_ref/mk_rotate_ref.c (the oracle's source plus that rotation), which is itself checked on
the CPU against tests/pbs_ref/mk_pbs_ref.c for a trivial accumulator and by decryption of all of its rows.

Noise (why "every row decrypts" is a condition, not a measurement): the accumulator's own noise passes through unrefreshed (one MK TLWE
encryption at bs_noise_stddev for a private table, d MK CMUX levels for a two-stage lookup), the rotation adds what a multi-key bootstrap's
rotation adds, and the input's modulus switch adds sqrt((P n + 1) / 12) / 2N.  A fresh multi-key encryption carries lwe_noise_stddev =
0.0125 of the torus, so the lookups here use p = 4 (input window +-1/8, ten standard deviations).  The schoolbook alone, on the CPU, at
n = 4 and p = q = 4 (output window +-2^29; the tests ask for half of it, 2^28):
  private table, (2, 64, 3, 7), 8 rows: all correct, worst phase 2^25.8 from its window's centre
  private table, (2, 256, 4, 6), 8 rows: all correct, worst phase 2^24.9
  two-stage lookup, (2, 64, 3, 7), d = 2: all 16 addresses correct, worst phase 2^26.0
  rotation result as a tree entry, (2, 64, 3, 7): all 4 cases correct, worst phase 2^24.8
At mktfhe_parameters_2party one multi-key external product adds 1.8e-3 of the torus (tests/test_mk_leveled.py) and a row has about 1000
live steps: a standard deviation near 0.06 of the torus, which is the multi-key bootstrap's own (its gates sit at +-1/8).  The full-size
private table therefore has binary outputs (p = 4, q = 2: window +-1/8), and the seed of its four rows was picked among eight on the CPU
through the C checker so that all four decrypt: worst phase 0.078 of the torus from its window's centre at out_form 1, 0.077 at out_form
2 (five of the eight seeds had all four rows inside the window; the worst row of the eight was 0.234 away).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_independent import monomial
from test_mk_leveled import MKTree, Setup, _words, wrap32
from test_mk_pbs import CFLAGS, mk_small, mkref          # noqa: F401  (fixtures: the 2-party N = 1024, n = 24 keys; the mk_pbs_ref.c checker)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6
NAME = "tfhe_mk_blind_rotate_batch"
SETS = [(2, 64, 3, 7), (3, 32, 2, 8), (2, 256, 4, 6), (4, 64, 2, 10)]


class MKRotation(MKTree):
    """The multi-key blind rotation of a full MK TLWE accumulator in exact integer arithmetic over the selector set of an MKTree."""

    def rotate(self, acc, exps, barb, sel=None):
        """acc [P+1][N]; exps: the steps' exponents (any integers, taken mod 2N); sel[i]: the selector of step i (None: i)."""
        N = self.N
        a = np.stack([wrap32(monomial(np.asarray(p, np.int64), -int(barb), N)) for p in acc])         # mk_mul_by_monomial, :79-85
        for i, e in enumerate(exps):                                                                  # :476-483
            if int(e) % (2 * N) == 0:                                                                 # :478-480
                continue
            rotated = np.stack([wrap32(monomial(x, int(e), N)) for x in a])
            a = self.cmux(i if sel is None else int(sel[i]), a, rotated)                              # mk_mux_rotate, :464-470
        return a

    def modswitch(self, x):
        """decode_message(v, 2N) of every word (:502-503; numeric-functions.jl:31-34): round(v 2N / 2^32) mod 2N."""
        shift = 32 - (2 * self.N).bit_length() + 1
        v = np.asarray(x, np.int64) & 0xFFFFFFFF
        return ((v + (1 << (shift - 1))) >> shift) & (2 * self.N - 1)

    def rotate_lwe(self, acc, x, sel=None):
        w = self.modswitch(x)
        return self.rotate(acc, w[:-1], w[-1], sel)

    def extract_at(self, sample, c):
        """mk_tlwe_extract_sample (:88-95) at coefficient c: per party a'[u] = coefficient c of X^u a; b = body[c]."""
        P, N = self.P, self.N
        ext = np.empty(P * N + 1, np.int64)
        for p in range(P):
            poly = np.asarray(sample[p], np.int64)
            for u in range(N):
                ext[p * N + u] = poly[c - u] if u <= c else -poly[N + c - u]
        ext[P * N] = sample[P][c]
        return wrap32(ext)


def _key_ref(tfhe, orc, s, with_ks=False):
    """MKRotation over s's bootstrapping key as selectors 0 ... P n - 1 (party-major) with s's own selector bits behind them."""
    from tfhe_jl_amd import leveled
    tg, who = leveled.mk_bootstrap_key_selectors(s.ck)
    assert tg.shape == (s.P * s.n, 2 * s.l * s.P + 2 * s.l, s.N) and tg.dtype == np.int32 and list(who) == [i for i in range(s.P) for _ in range(s.n)]
    assert np.array_equal(tg.reshape(-1), np.asarray(s.ck.bootstrap_key).reshape(-1))
    ks = s.ck.keyswitch_key if with_ks else None
    return MKRotation(orc, s.N, s.l, s.beta, s.P, np.concatenate([tg, s.tgsw]), np.concatenate([who, s.owners]), ks=ks, n=s.n)


def _rot(s, orc, with_ks=False):
    """MKRotation over s's own selectors (what Setup.tree gives as an MKTree)."""
    return MKRotation(orc, s.N, s.l, s.beta, s.P, s.tgsw, s.owners, ks=s.ck.keyswitch_key if with_ks else None, n=s.n)


def _dist(phase, want):
    return abs(int(wrap32(int(phase) - int(want))))


# ---- 1. CPU: the symbol, and the reference with the host helpers -------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported(tfhe):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+" + NAME + r"\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == 12
    assert NAME in tfhe._lib.ABI_SYMBOLS
    lib = tfhe._lib.load()
    assert hasattr(lib, NAME) and lib.tfhe_abi_version() == 7
    assert getattr(lib, NAME)(None, None, 1, None, None, 1, 0, None, 1, None, 0, 0) == INVALID          # NULL context
    assert callable(getattr(tfhe.Engine, "mk_blind_rotate"))
    for fn in ("mk_bootstrap_key_selectors", "mk_private_lut_encrypt", "mk_blind_rotate_lookup", "mk_two_stage_lookup", "mk_pbs_to_tlwe"):
        assert callable(getattr(tfhe, fn)) and fn in tfhe.__all__, fn


@pytest.mark.parametrize("P,N,l,beta", [SETS[0], SETS[2]])
def test_schoolbook_rotation_of_a_private_table_decrypts_every_row(tfhe, orc, P, N, l, beta):
    """p = 4, n = 4: the schoolbook rotation of mk_private_lut_encrypt(f) by mk_lut_encrypt(m) under the bootstrapping key as selectors
    decrypts (mk_tlwe_phase, coefficient 0) to f(m) for every one of 8 rows, within half the window of its centre (window +-2^29)."""
    from tfhe_jl_amd import leveled, lut
    s = Setup(tfhe, P, N, l, beta, 6100 + N, owners=[0])
    f = [3, 0, 2, 1]
    acc = leveled.mk_private_lut_encrypt(s.rng, s.tlwe_keys, s.p.bs_noise_stddev, lambda m: f[m], 4)
    assert acc.shape == (1, P + 1, N) and acc.dtype == np.int32 and all(np.any(acc[0, i] != 0) for i in range(P))      # an encryption
    ref = _key_ref(tfhe, orc, s)
    m = np.arange(8) % 4
    x = lut.mk_lut_encrypt(s.rng, s.sks, m, 4)
    worst = 0
    for g in range(8):
        got = ref.rotate_lwe(acc[0], x[g])
        phase = leveled.mk_tlwe_phase(s.tlwe_keys, got.astype(np.int32))[0]
        assert lut.lut_decode(phase[0], 4) == f[m[g]], (g, phase[0])
        worst = max(worst, _dist(phase[0], lut.lut_encode(f[m[g]], 4)))
    print(f"private table ({P}, {N}, {l}, {beta}): worst phase 2^{np.log2(worst):.1f} from the window's centre")
    assert worst < 2**28
    s.ck.close()


def test_schoolbook_two_stage_lookup_decrypts_all_16_addresses(tfhe, orc):
    """A 16-entry table as 2^2 test polynomials of p = 4 entries at (2, 64, 3, 7): a depth-2 schoolbook tree over uni-encrypted high
    bits (party 0 owns bit 0, party 1 bit 1; selectors behind the key's P n), then the rotation by the low digit's multi-key LWE sample,
    decrypts at all 16 addresses."""
    from tfhe_jl_amd import leveled, lut
    P, N, l, beta = SETS[0]
    highs = [(a >> 2) for a in range(16)]
    s = Setup(tfhe, P, N, l, beta, 6200, owners=[0, 1] * 16, bits=[(h >> v) & 1 for h in highs for v in range(2)])
    table = [int(v) for v in np.random.default_rng(5).integers(0, 4, 16)]
    tables = np.concatenate([leveled.mk_tlwe_trivial(lut.make_test_vector(lambda m, h=h: table[4 * h + m], 4, N), P) for h in range(4)])
    ref = _key_ref(tfhe, orc, s)
    Pn = P * s.n
    x = lut.mk_lut_encrypt(s.rng, s.sks, np.arange(16) & 3, 4)
    worst = 0
    for address in range(16):
        picked = ref.tree(tables, [Pn + 2 * address, Pn + 2 * address + 1])
        got = ref.rotate_lwe(picked, x[address], sel=range(Pn))
        phase = leveled.mk_tlwe_phase(s.tlwe_keys, got.astype(np.int32))[0]
        assert lut.lut_decode(phase[0], 4) == table[address], (address, phase[0])
        worst = max(worst, _dist(phase[0], lut.lut_encode(table[address], 4)))
    print(f"two-stage lookup: worst phase 2^{np.log2(worst):.1f} from the window's centre")
    assert worst < 2**28
    s.ck.close()


def test_schoolbook_rotation_result_is_a_table_entry_of_a_tree(tfhe, orc):
    """What mk_pbs_to_tlwe returns (the final accumulator of the trivial (0, ..., 0, test vector)) for two samples, used as the two
    entries of a depth-1 MKTree.tree, decrypts at coefficient 0 to f of the selected sample's message."""
    from tfhe_jl_amd import leveled, lut
    P, N, l, beta = SETS[0]
    cases = [(0, 3, 0), (0, 3, 1), (2, 1, 1), (1, 1, 0)]
    s = Setup(tfhe, P, N, l, beta, 6300, owners=[0, 1, 1, 0], bits=[c[2] for c in cases])
    f = [1, 3, 0, 2]
    acc = leveled.mk_tlwe_trivial(lut.make_test_vector(lambda m: f[m], 4, N), P)[0]
    ref = _key_ref(tfhe, orc, s)
    Pn = P * s.n
    worst = 0
    for i, (m0, m1, bit) in enumerate(cases):
        entries = [ref.rotate_lwe(acc, lut.mk_lut_encrypt(s.rng, s.sks, [m], 4)[0], sel=range(Pn)) for m in (m0, m1)]
        got = ref.tree(entries, [Pn + i])
        phase = leveled.mk_tlwe_phase(s.tlwe_keys, got.astype(np.int32))[0]
        assert lut.lut_decode(phase[0], 4) == f[(m0, m1)[bit]], (m0, m1, bit, phase[0])
        worst = max(worst, _dist(phase[0], lut.lut_encode(f[(m0, m1)[bit]], 4)))
    print(f"rotation result as a tree entry: worst phase 2^{np.log2(worst):.1f} from the window's centre")
    assert worst < 2**28
    s.ck.close()


# ---- 2. the C checker (tests/pbs_ref/mk_rotate_ref.c) -------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def rotref(tmp_path_factory, orc):
    so = str(tmp_path_factory.mktemp("mk_rotate_ref") / "libmk_rotate_ref.so")
    subprocess.check_call(CFLAGS + ["-o", so, os.path.join(ROOT, "tests", "pbs_ref", "mk_rotate_ref.c"), "-lm"])
    lib = C.CDLL(so)
    vp = C.c_void_p
    lib.mk_rotate_batch.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, C.c_int64, C.c_int32]
    lib.mk_rotate_batch.restype = C.c_int

    def run(o, accs, index, x, n_out, out_form):
        assert lib.orc_init(C.c_int32(o.N)) == 0
        x = np.ascontiguousarray(np.atleast_2d(x), np.int32)
        accs = np.ascontiguousarray(accs, np.int32)
        idx = None if index is None else np.ascontiguousarray(index, np.int32)
        B, P = x.shape[0], o.parties
        assert accs.ndim == 3 and accs.shape[1:] == (P + 1, o.N)
        shape = {0: (B, P + 1, o.N), 1: (B, n_out, P * o.N + 1), 2: (B, n_out, P * o.n + 1)}[out_form]
        out = np.zeros(shape, np.int32)
        rc = lib.mk_rotate_batch(C.byref(o.P), P, _p(o.bk_re), _p(o.bk_im), _p(o.bk_i32), _p(o.ks), 0, _p(accs), _p(idx), n_out, _p(x), _p(out), B, out_form)
        assert rc == 0
        return out
    return run


def test_checker_trivial_accumulator_equals_mk_pbs_checker(tfhe, mk_small, mkref, rotref):
    """With the accumulator (0, 0, tv) the new checker is mk_pbs_multi_batch (tests/pbs_ref/mk_pbs_ref.c), word for word, extracted and
    keyswitched, n_out 1 and 4; and its out_form 0 is what the extraction reads."""
    from tfhe_jl_amd import leveled
    K = mk_small
    o = K.oracle
    rng = np.random.default_rng(77)
    x = _words(rng, 3, 2 * o.n + 1)
    x[:2] = tfhe.mk_encrypt(rng, K.sks, [True, False])
    tv = _words(rng, 2, o.N)
    idx = np.array([1, 0, 1], np.int32)
    accs = leveled.mk_tlwe_trivial(tv, 2)
    for n_out in (1, 4):
        for form in (1, 2):
            assert np.array_equal(rotref(o, accs, idx, x, n_out, form), mkref(o, tv, idx, x, n_out, with_keyswitch=form == 2)), (n_out, form)
    full = rotref(o, accs, idx, x, 1, 0)
    ext = rotref(o, accs, idx, x, 4, 1)
    assert np.array_equal(ext[:, 1, -1], full[:, 2, o.N // 4]) and np.array_equal(ext[:, 0, 0], full[:, 0, 0])
    assert np.array_equal(ext[:, 0, 1], -full[:, 0, o.N - 1]) and np.array_equal(ext[:, 2, o.N], full[:, 1, o.N // 2])


class _Full:
    """mktfhe_parameters_2party with kept TLWE keys: a private table Z_4 -> Z_2 and B = 4 rows, the expected words from the C checker on
    the host-expanded key (RGSW.Expand on the device gives the same words: tests/test_mk_leveled.py)."""
    F = [1, 0, 0, 1]

    def __init__(self, tfhe, orc, rotref):
        from tfhe_jl_amd import leveled, lut
        p = self.p = tfhe.mktfhe_parameters_2party
        rng = np.random.default_rng(2025)
        self.sks = [tfhe.SecretKey(rng, p) for _ in range(2)]
        shared = tfhe.SharedKey(rng, p)
        self.parts = [tfhe.CloudKeyPart(rng, sk, shared, keep_tlwe_key=True) for sk in self.sks]
        self.tlwe_keys = [part.tlwe_key for part in self.parts]
        host = tfhe.MKCloudKey(self.parts)
        o = orc.Oracle(p.lwe_size, 1024, 1, p.bs_decomp_length, p.bs_log2_base, p.ks_decomp_length, p.ks_log2_base, parties=2)
        o.load_bootstrap_key(host.bootstrap_key)
        o.load_keyswitch_key(host.keyswitch_key)
        self.m = np.arange(4)
        rng = np.random.default_rng(3003)                           # (the rows' seed: see the module's docstring)
        self.acc = leveled.mk_private_lut_encrypt(rng, self.tlwe_keys, p.bs_noise_stddev, lambda v: self.F[v], 4, 2)
        self.x = lut.mk_lut_encrypt(rng, self.sks, self.m, 4)
        self.want = {form: rotref(o, self.acc, None, self.x, 1, form) for form in (1, 2)}


@pytest.fixture(scope="module")
def full(tfhe, orc, rotref):
    return _Full(tfhe, orc, rotref)


def test_checker_full_size_private_table_decrypts_all_four_rows(tfhe, full):
    """The checker's own outputs decrypt to f(m) for all four rows, extracted (under the TLWE keys) and keyswitched."""
    from tfhe_jl_amd import lut
    from tfhe_jl_amd.mk_keys import mk_phase
    want = [full.F[v] for v in full.m]
    assert list(lut.mk_lut_decrypt(full.sks, full.want[2][:, 0], 2)) == want
    s = np.stack([k.key[0] for k in full.tlwe_keys]).astype(np.int64)                                # the extracted keys are the TLWE keys
    ext = full.want[1][:, 0].astype(np.int64)
    phase = wrap32(ext[:, -1] - np.einsum("bpn,pn->b", ext[:, :-1].reshape(4, 2, 1024), s))
    assert list(lut.lut_decode(phase, 2)) == want
    for name, ph in (("out_form 1", phase), ("out_form 2", mk_phase(full.sks, full.want[2][:, 0]))):
        worst = max(_dist(v, lut.lut_encode(w, 2)) for v, w in zip(ph, want))
        print(f"full size, {name}: worst phase {worst / 2**32:.4f} of the torus from the window's centre")


# ---- 3. GPU: word for word against the schoolbook -----------------------------------------------------------------------------------
B_ROWS = 5
ACC_INDEX = np.array([2, 0, 2, 1, 0], np.int32)                      # a repeated accumulator; rows 1 and 4 read accumulator 0
SEL7 = [0, 1, 2, 3, 0, 1, 4]                                         # parties 0, P-1, 0, P-1, 0, P-1, 1: selectors 0 and 1 repeat


def _owners(P):
    return [0, P - 1, 0, P - 1, 1 % P]


def _planted_exponents(rng, N, steps):
    rows = rng.integers(0, 2 * N, (B_ROWS, steps + 1)).astype(np.int32)
    plant = [0, 1, N, 2 * N - 1]
    rows[0, :steps] = [plant[i % 4] for i in range(steps)]          # (steps = 1: the one exponent is 0, the result a rotated copy)
    rows[0, steps] = 0
    rows[1, steps] = 2 * N - 1
    rows[2, :steps] = [plant[(i + 1) % 4] for i in range(steps)]
    rows[3, steps - 1] = 0                                          # a skipped last step: the other ping-pong sample is the final one
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 6, 7])
@pytest.mark.parametrize("P,N,l,beta", SETS)
def test_gpu_mk_blind_rotate_equals_schoolbook(tfhe, orc, P, N, l, beta, steps):
    s = Setup(tfhe, P, N, l, beta, 7300 + P + N + l + steps, _owners(P))
    eng = s.ck.engine(0)
    acc = s.encrypt(_words(s.rng, 3, N))                            # T = 3
    rows = _planted_exponents(s.rng, N, steps)
    sel = np.array(SEL7[:steps], np.int32)
    if steps > 1:
        assert {int(s.owners[v]) for v in sel} >= {0, P - 1} and all(s.owners[sel[i]] != s.owners[sel[i + 1]] for i in range(min(steps, 6) - 1))
    ref = _rot(s, orc, with_ks=True)
    want = np.stack([ref.rotate(acc[ACC_INDEX[g]], rows[g, :steps], rows[g, steps], sel) for g in range(B_ROWS)])
    eng.mk_tgsw_load(s.tgsw, s.owners)
    got0 = eng.mk_blind_rotate(acc, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, out_form=0)
    assert got0.shape == (B_ROWS, P + 1, N) and np.array_equal(got0, want.astype(np.int32)), "out_form 0"
    assert eng.last_kernel_name() == f"mk_tlwe_rotate_kernel(N={N},P={P},l={l},steps={steps})"
    assert eng.last_rotation_count() == B_ROWS and eng.last_timing_ms(0) > 0
    # NULL acc_index = accumulator 0 for every row: rows 1 and 4 of the call above
    got = eng.mk_blind_rotate(acc, rows[[1, 4]], sel=sel, in_form=1, out_form=0)
    assert np.array_equal(got, want[[1, 4]].astype(np.int32)), "NULL acc_index"
    for n_out in (1, 4):
        want_ext = np.stack([[ref.extract_at(w, j * (N // n_out)) for j in range(n_out)] for w in want])
        got1 = eng.mk_blind_rotate(acc, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, n_out=n_out, out_form=1)
        assert got1.shape == (B_ROWS, n_out, P * N + 1) and np.array_equal(got1, want_ext.astype(np.int32)), ("out_form 1", n_out)
        got2 = eng.mk_blind_rotate(acc, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, n_out=n_out, out_form=2)
        assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
        want_ks = np.stack([[ref.keyswitch(e) for e in row] for row in want_ext])
        assert got2.shape == (B_ROWS, n_out, P * s.n + 1) and np.array_equal(got2, want_ks.astype(np.int32)), ("out_form 2", n_out)
    if eng.get_option("exact_domain") == 2:                         # exact for ANY words: arbitrary accumulators and the extremes
        arb = _words(s.rng, 3, P + 1, N)
        arb[0, 0], arb[0, P], arb[1, P - 1] = 2**31 - 1, -2**31, -2**31
        want = np.stack([ref.rotate(arb[ACC_INDEX[g]], rows[g, :steps], rows[g, steps], sel) for g in range(B_ROWS)])
        got = eng.mk_blind_rotate(arb, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, out_form=0)
        assert np.array_equal(got, want.astype(np.int32)), "arbitrary accumulators"
    s.ck.close()


# ---- 4. GPU: in_form 0 is in_form 1 of the modulus-switched words -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [SETS[0], SETS[2]])
def test_gpu_in_form_0_equals_in_form_1_of_modswitch(tfhe, orc, P, N, l, beta):
    steps = 6
    s = Setup(tfhe, P, N, l, beta, 7500 + N, [0, 1, 1, 0, 1, 0])
    eng = s.ck.engine(0)
    x = _words(s.rng, 4, steps + 1)
    half = 2**32 // (2 * N) // 2                                    # the words just below and at a rounding boundary of decode_message(., 2N)
    x[0, :6] = [2**31 - 1, -2**31, half - 1, half, -half - 1, -half]
    x[1, steps] = 2**31 - 1
    x[2, steps] = -2**31
    x[3, steps] = 3 * half - 1
    ref = _rot(s, orc)
    exps = np.array([ref.modswitch(row) for row in x], np.int64)
    assert list(exps[0, :6]) == [N, N, 0, 1, 2 * N - 1, 0] and exps[1, steps] == N and exps[2, steps] == N and exps[3, steps] == 1
    eng.mk_tgsw_load(s.tgsw, s.owners)
    acc, idx = s.encrypt(_words(s.rng, 3, N)), np.array([0, 1, 2, 1], np.int32)
    for form, n_out in ((0, 1), (1, 4)):
        a = eng.mk_blind_rotate(acc, x, acc_index=idx, in_form=0, n_out=n_out, out_form=form)
        b = eng.mk_blind_rotate(acc, exps.astype(np.int32), acc_index=idx, in_form=1, n_out=n_out, out_form=form)
        assert np.array_equal(a, b), form
    want = ref.rotate_lwe(acc[0], x[0])
    assert np.array_equal(eng.mk_blind_rotate(acc, x[:1], in_form=0, out_form=0)[0], want.astype(np.int32))
    s.ck.close()


# ---- 5. GPU: a trivial accumulator is the multi-key programmable bootstrap ------------------------------------------------------------
def _trivial_equals_tv_multi(tfhe, ck, eng, sks, N, n, family):
    from tfhe_jl_amd import leveled
    rng = np.random.default_rng(7600 + N)
    eng.mk_tgsw_load(*leveled.mk_bootstrap_key_selectors(ck))
    tv = _words(rng, 2, N)
    x = _words(rng, 4, 2 * n + 1)
    x[0, :] = 0                                                     # every exponent zero
    x[1, :2] = [2**31 - 1, -2**31]
    x[2] = tfhe.mk_encrypt(rng, sks, True)
    idx = np.array([0, 1, 1, 0], np.int32)
    for n_out in (1, 4):
        for ks in (False, True):
            want = eng.mk_bootstrap_tv_multi(tv, x, n_out, index=idx, with_keyswitch=ks)
            assert eng.last_kernel_name().startswith(family), eng.last_kernel_name()
            got = eng.mk_blind_rotate(leveled.mk_tlwe_trivial(tv, 2), x, acc_index=idx, in_form=0, n_out=n_out, out_form=2 if ks else 1)
            assert eng.last_kernel_name() == f"mk_tlwe_rotate_kernel(N={N},P=2,l=4,steps={2 * n})"
            assert got.shape == want.shape and np.array_equal(got, want), (n_out, ks)


@pytest.mark.gpu
def test_gpu_trivial_accumulator_equals_mk_bootstrap_tv_multi_tuned_family(tfhe, mk_small):
    """(0, 0, tv), in_form 0, sel NULL, the cloud key's own bootstrapping key as selectors: tfhe_mk_bootstrap_tv_multi_batch word for
    word, with and without keyswitch, n_out 1 and 4, against the tuned 2-party family."""
    K = mk_small
    _trivial_equals_tv_multi(tfhe, K.ck, K.ck.engine(0), K.sks, 1024, K.params.lwe_size, "mk_blind_rotate_kernel_w2<4>")


@pytest.mark.gpu
def test_gpu_trivial_accumulator_equals_mk_bootstrap_tv_multi_any_n_family(tfhe, orc):
    from test_any_params import _mk
    p, rng, sks, ck = _mk(tfhe, orc, 2, 512, 4, 7, 6)
    _trivial_equals_tv_multi(tfhe, ck, ck.engine(0), sks, 512, 6, "mk_blind_rotate_kernel_anyn(N=512,P=2,l=4)")
    ck.close()


# ---- 6. GPU: one launch for the mk_rot_net chain ------------------------------------------------------------------------------------
def _chain(leveled, N, exps, barb):
    r = (2 * N - int(barb)) % (2 * N)
    nodes = [(0, 0, 0, r, r)] + [(0, 0, i, 0, int(e)) for i, e in enumerate(exps)]
    return leveled.RotNet([1] * len(nodes), nodes, N, entries=1, variables=len(exps))


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [SETS[0], SETS[3]])
def test_gpu_one_row_equals_the_mk_rot_net_chain(tfhe, orc, P, N, l, beta):
    """B = 1, out_form 0: the tfhe_mk_rot_net_batch network "a rotated copy by 2N - barb, then `steps` levels of width 1 with records
    (0, 0, i, 0, e_i)", word for word."""
    from tfhe_jl_amd import leveled
    steps = 7
    s = Setup(tfhe, P, N, l, beta, 7700 + N + P, _owners(P))
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    acc = s.encrypt(_words(s.rng, 1, N))
    sel = np.array(SEL7, np.int32)
    for barb in (0, 2 * N - 1, N + 3):
        exps = s.rng.integers(1, 2 * N, steps)
        exps[2] = 0                                                 # (the chain's node is then a copy)
        want = eng.mk_rot_net(acc[None], _chain(leveled, N, exps, barb), sel[None, :], out_form=0)
        assert eng.last_kernel_name().startswith("mk_rot_net_level_kernel(")
        rows = np.array([list(exps) + [barb]], np.int32)
        got = eng.mk_blind_rotate(acc, rows, sel=sel, in_form=1, out_form=0)
        assert np.array_equal(got, want[:, 0]), barb
    s.ck.close()


# ---- 7. GPU: spectrum accumulators in global memory ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_rotate_accumulators_in_global_memory_small(tfhe, orc):
    """The option anyn_spec = 1 at (2, 64, 3, 7) changes where the three spectrum accumulators live and no word."""
    P, N, l, beta = SETS[0]
    s = Setup(tfhe, P, N, l, beta, 7800, [1, 0, 1])
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    acc = s.encrypt(_words(s.rng, 4, N))
    rows = s.rng.integers(1, 2 * N, (3, 4)).astype(np.int32)
    lds = eng.mk_blind_rotate(acc, rows, acc_index=[3, 1, 0], in_form=1, n_out=2, out_form=1)
    assert "spec=global" not in eng.last_kernel_name()
    eng.set_option("anyn_spec", 1)
    glob = eng.mk_blind_rotate(acc, rows, acc_index=[3, 1, 0], in_form=1, n_out=2, out_form=1)
    assert eng.last_kernel_name() == f"mk_tlwe_rotate_kernel(N={N},P={P},l={l},steps=3,spec=global)"
    assert np.array_equal(glob, lds)
    ref = _rot(s, orc)
    assert np.array_equal(glob[0, 1], ref.extract_at(ref.rotate(acc[3], rows[0, :3], rows[0, 3]), N // 2).astype(np.int32))
    s.ck.close()


@pytest.mark.gpu
def test_gpu_mk_rotate_accumulators_in_global_memory_n4096(tfhe, orc):
    """(2, 4096, 2, 6): buf + 3 accumulators + tmp pass 160 KB (tests/test_mk_leveled.py), so the accumulators are in global memory
    without the option; steps 2, B = 2: row 0 against the schoolbook, row 1 against the mk_rot_net chain."""
    from tfhe_jl_amd import leveled
    P, N, l, beta = 2, 4096, 2, 6
    s = Setup(tfhe, P, N, l, beta, 7801, owners=[1, 0], n=2)
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    acc = s.encrypt(_words(s.rng, 2, N))
    rows = np.array([[5, 2 * N - 1, N + 1], [N, 77, 2 * N - 1]], np.int32)
    got = eng.mk_blind_rotate(acc, rows, acc_index=[0, 1], in_form=1, out_form=0)
    assert eng.last_kernel_name() == f"mk_tlwe_rotate_kernel(N={N},P={P},l={l},steps=2,spec=global)"
    ref = _rot(s, orc)
    assert np.array_equal(got[0], ref.rotate(acc[0], rows[0, :2], rows[0, 2]).astype(np.int32))
    want = eng.mk_rot_net(acc[1:2][None], _chain(leveled, N, rows[1, :2], rows[1, 2]), np.array([[0, 1]], np.int32), out_form=0)
    assert np.array_equal(got[1], want[0, 0])
    s.ck.close()


# ---- 8. GPU: mktfhe_parameters_2party at full size ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_private_table_full_size_equals_checker(tfhe, full):
    """B = 4 rows of a private table Z_4 -> Z_2, the key expanded on the device: out_form 1 and 2 equal the C checker word for word (whose
    outputs decrypt: test_checker_full_size_private_table_decrypts_all_four_rows), through mk_blind_rotate_lookup."""
    from tfhe_jl_amd import leveled, lut
    ck = tfhe.MKCloudKey(full.parts, expand="device")
    got1 = leveled.mk_blind_rotate_lookup(ck, full.acc, full.x, out_form=1)
    eng = ck.engine(0)
    assert eng.last_kernel_name() == f"mk_tlwe_rotate_kernel(N=1024,P=2,l=4,steps={2 * full.p.lwe_size})" and eng.last_rotation_count() == 4
    assert got1.shape == (4, 1, 2 * 1024 + 1) and np.array_equal(got1, full.want[1])
    got2 = leveled.mk_blind_rotate_lookup(ck, full.acc, full.x)
    assert got2.shape == (4, 2 * full.p.lwe_size + 1) and np.array_equal(got2, full.want[2][:, 0])
    assert list(lut.mk_lut_decrypt(full.sks, got2, 2)) == [full.F[v] for v in full.m]
    ck.close()


# ---- 9. GPU: the helpers -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("expand", ["device", "host"])
def test_gpu_two_stage_lookup_and_pbs_to_tlwe_equal_schoolbook(tfhe, orc, expand):
    """mk_two_stage_lookup and mk_pbs_to_tlwe at (2, 64, 3, 7) against the schoolbook tree and rotation, word for word, with the key and
    the address bits expanded on the device and on the host; every one of the 16 addresses decrypts."""
    from tfhe_jl_amd import leveled, lut
    P, N, l, beta = SETS[0]
    highs = [(a >> 2) for a in range(16)]
    s = Setup(tfhe, P, N, l, beta, 6200, owners=[0, 1] * 16, bits=[(h >> v) & 1 for h in highs for v in range(2)])
    table = [int(v) for v in np.random.default_rng(5).integers(0, 4, 16)]
    tables = np.concatenate([leveled.mk_tlwe_trivial(lut.make_test_vector(lambda m, h=h: table[4 * h + m], 4, N), P) for h in range(4)])
    ref = _key_ref(tfhe, orc, s, with_ks=True)
    Pn = P * s.n
    x = lut.mk_lut_encrypt(s.rng, s.sks, np.arange(16) & 3, 4)
    uni = [a.reshape(16, 2, l, N) for a in s.uni]
    got = leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, 4, out_form=0, expand=expand)
    want = np.stack([ref.rotate_lwe(ref.tree(tables, [Pn + 2 * a, Pn + 2 * a + 1]), x[a], sel=range(Pn)) for a in range(16)])
    assert np.array_equal(got, want.astype(np.int32))
    out = leveled.mk_two_stage_lookup(s.ck, tables, uni, [0, 1], x, 4, expand=expand)
    assert np.array_equal(out, np.stack([ref.keyswitch(ref.extract_at(w, 0)) for w in want]).astype(np.int32))
    assert list(lut.mk_lut_decrypt(s.sks, out, 4)) == table
    t = leveled.mk_pbs_to_tlwe(s.ck, x[:4], lambda m: table[m], 4)
    acc = leveled.mk_tlwe_trivial(lut.make_test_vector(lambda m: table[m], 4, N), P)[0]
    assert t.shape == (4, P + 1, N) and np.array_equal(t, np.stack([ref.rotate_lwe(acc, x[g], sel=range(Pn)) for g in range(4)]).astype(np.int32))
    # extra address bits behind the key through mk_blind_rotate_lookup: the rotation names the key's selectors itself
    extra = [a[:3] for a in s.uni]
    got = leveled.mk_blind_rotate_lookup(s.ck, acc, x[:2], extra_uni_bits=extra, extra_party_of=s.owners[:3], out_form=0, expand=expand)
    assert np.array_equal(got, t[:2])
    s.ck.close()


# ---- 10. GPU: the contract -----------------------------------------------------------------------------------------------------------
def _mem_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    return free.value


class _Call:
    """A valid raw call of tfhe_mk_blind_rotate_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, acc, rows, sel):
        self.eng = eng
        self.args = dict(acc=acc, T=acc.shape[0], acc_index=np.zeros(rows.shape[0], np.int32), rows=rows, steps=rows.shape[1] - 1, in_form=1, sel=sel,
                         n_out=1, B=rows.shape[0], out_form=0)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        out = np.zeros((self.args["B"], 4, self.args["acc"].shape[1] * self.args["acc"].shape[2]), np.int32)
        rc = e._lib.tfhe_mk_blind_rotate_batch(e._h, _p(a["acc"]), a["T"], _p(a["acc_index"]), _p(a["rows"]), a["steps"], a["in_form"], _p(a["sel"]),
                                               a["n_out"], _p(a.get("out", out)), a["B"], a["out_form"])
        return rc, e._lib.tfhe_last_error(e._h).decode(), out


@pytest.mark.gpu
def test_gpu_mk_rotate_contract_refusals_leave_the_context_usable(tfhe, orc):
    P, N, l, beta = SETS[0]
    s = Setup(tfhe, P, N, l, beta, 9700, owners=[0, 1, 0])
    eng = s.ck.engine(0)
    acc = s.encrypt(_words(s.rng, 2, N))
    rows = np.array([[1, 0, 127, 5], [64, 3, 2, 0]], np.int32)
    sel = np.array([2, 0, 1], np.int32)
    ref = _rot(s, orc, with_ks=True)
    want = np.stack([ref.rotate(acc[0], r[:3], r[3], sel) for r in rows]).astype(np.int32)
    want_ext = np.stack([ref.extract_at(w, 0) for w in want])[:, None]
    want_ks = np.stack([ref.keyswitch(e[0]) for e in want_ext])[:, None].astype(np.int32)
    call = _Call(eng, acc, rows, sel)
    xs, ys = tfhe.mk_encrypt(s.rng, s.sks, [True, False, True]), tfhe.mk_encrypt(s.rng, s.sks, [True, True, False])

    def nand_works(e):
        assert np.array_equal(tfhe.mk_decrypt(s.sks, e.mk_gate_nand(xs, ys)), [False, True, True])

    def still_right():
        rc, msg, out = call()
        assert rc == 0 and np.array_equal(out.reshape(-1)[:want.size], want.reshape(-1)), msg
        nand_works(eng)

    def refused(code, word, **over):
        rc, msg, _ = call(**over)
        assert rc == code and word in msg and msg.startswith("mk_blind_rotate_batch:"), (list(over), rc, msg)
        still_right()

    rc, msg, _ = call()
    assert rc == NO_KEY and "selector" in msg                       # no selector set yet
    nand_works(eng)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    still_right()
    assert call(B=0)[0] == 0 and call(B=0, acc=None, rows=None, out=None)[0] == 0          # B = 0 is TFHE_OK
    refused(INVALID, "negative", B=-1)
    for name in ("acc", "rows", "out"):
        refused(INVALID, "NULL", **{name: None})
    for steps in (0, -1, 65537):
        refused(INVALID, f"steps = {steps}", steps=steps)
    for form in (2, -1):
        refused(INVALID, f"in_form = {form}", in_form=form)
    for form in (3, -1):
        refused(INVALID, f"out_form = {form}", out_form=form)
    refused(INVALID, "T = 0", T=0)
    refused(INVALID, "n_out = 0", n_out=0)
    refused(INVALID, "n_out = 3", n_out=3, out_form=1)
    refused(INVALID, "n_out = 64", n_out=64, out_form=1)
    refused(INVALID, "n_out = 32", n_out=32, out_form=1)            # a power of two <= 32, but above N / 4 = 16
    refused(INVALID, "n_out = 4 with out_form 0", n_out=4)          # out_form 0 returns one sample
    refused(INVALID, "sel[1] = 3", sel=np.array([0, 3, 1], np.int32))
    refused(INVALID, "sel[1] = -1", sel=np.array([0, -1, 1], np.int32))
    refused(INVALID, "steps = 4, 3 selectors", sel=None, steps=4, rows=np.zeros((2, 5), np.int32))       # selector i for step i needs four
    refused(INVALID, "acc_index[1] = 2", acc_index=np.array([0, 2], np.int32))
    refused(INVALID, "acc_index[0] = -1", acc_index=np.array([-1, 0], np.int32))
    bad_rows = rows.copy(); bad_rows[1, 2] = 2 * N
    neg_rows = rows.copy(); neg_rows[0, 3] = -1
    refused(INVALID, "rows[1][2] = 128", rows=bad_rows)             # the message names row and column
    refused(INVALID, "rows[0][3] = -1", rows=neg_rows)
    rc, msg, _ = call(rows=bad_rows, in_form=0)                     # LWE samples are any words
    assert rc == 0, msg
    # the scalars come before the selectors, the selectors before the accumulator indices, those before the words
    assert "steps" in call(steps=0, sel=np.array([9, 9, 9], np.int32))[1] and "sel[0]" in call(sel=np.array([9, 0, 0], np.int32), acc_index=np.array([5, 5], np.int32))[1]
    assert "acc_index[0]" in call(acc_index=np.array([5, 5], np.int32), rows=bad_rows)[1]
    # sel NULL on the loaded three selectors
    assert np.array_equal(eng.mk_blind_rotate(acc, rows, in_form=1, out_form=0)[0], ref.rotate(acc[0], rows[0, :3], rows[0, 3]).astype(np.int32))
    eng.set_option("measure_margin", 1)
    rc, msg, _ = call()
    assert rc == STATE and "measure_margin" in msg
    eng.set_option("measure_margin", 0)
    still_right()
    assert np.array_equal(eng.mk_blind_rotate(acc, rows, sel=sel, acc_index=[0, 0], in_form=1, out_form=1), want_ext.astype(np.int32))
    assert np.array_equal(eng.mk_blind_rotate(acc, rows, sel=sel, acc_index=[0, 0], in_form=1), want_ks)
    # no multi-key bootstrapping key, then no selector set, then out_form 2 without the multi-key keyswitch key; forms 0 and 1 do not
    # need it, and a bad scalar is named before the missing keyswitch key
    raw = tfhe.Engine(s.p)
    rc, msg, _ = call(raw)
    assert rc == NO_KEY and "bootstrapping key" in msg
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)
    rc, msg, _ = call(raw)
    assert rc == NO_KEY and "selector" in msg
    raw.mk_tgsw_load(s.tgsw, s.owners)
    rc, msg, _ = call(raw, out_form=2)
    assert rc == NO_KEY and "keyswitch" in msg
    rc, msg, _ = call(raw, out_form=2, steps=0)
    assert rc == INVALID and "steps" in msg
    assert np.array_equal(raw.mk_blind_rotate(acc, rows, sel=sel, in_form=1, out_form=0), want)
    raw.mk_load_keyswitch_key(s.ck.keyswitch_key, P)
    assert np.array_equal(raw.mk_blind_rotate(acc, rows, sel=sel, in_form=1), want_ks)
    raw.close()
    # out_form 2 with a keyswitch key made for another party count: TFHE_ERR_STATE, before the selectors are looked at
    s3 = Setup(tfhe, 3, 32, 2, 8, 9701, owners=[0, 1, 2])
    ck2 = tfhe.MKCloudKey(s3.parts[:2])
    acc3 = s3.encrypt(_words(s3.rng, 2, 32))
    rows3 = np.array([[1, 0, 63, 5], [32, 3, 2, 0]], np.int32)
    raw3 = tfhe.Engine(s3.p)
    raw3.mk_load_bootstrap_key(s3.ck.bootstrap_key, 3)
    raw3.mk_tgsw_load(s3.tgsw, s3.owners)
    raw3.mk_load_keyswitch_key(ck2.keyswitch_key, 2)
    call3 = _Call(raw3, acc3, rows3, sel)
    rc, msg, _ = call3(out_form=2, sel=np.array([9, 0, 0], np.int32))
    assert rc == STATE and "parties" in msg and "mk_blind_rotate_batch" in msg, (rc, msg)
    ref3 = _rot(s3, orc, with_ks=True)
    want3 = np.stack([ref3.rotate(acc3[0], r[:3], r[3], sel) for r in rows3])
    rc, msg, out = call3()
    assert rc == 0 and np.array_equal(out.reshape(-1)[:want3.size], want3.reshape(-1).astype(np.int32)), msg
    raw3.mk_load_keyswitch_key(s3.ck.keyswitch_key, 3)
    assert np.array_equal(raw3.mk_blind_rotate(acc3, rows3, sel=sel, acc_index=[0, 0], in_form=1)[:, 0],
                          np.stack([ref3.keyswitch(ref3.extract_at(w, 0)) for w in want3]).astype(np.int32))
    raw3.close()
    ck2.close()
    s3.ck.close()
    # a single-key context: the new call is refused, its gates go on; and the single-key call keeps refusing a multi-key context
    p1 = tfhe.SchemeParameters(16, 1 / 2**15, N, 1, l, beta, 1e-7, 8, 2, 1 / 2**15, 1)
    sk1, ck1 = tfhe.make_key_pair(s.rng, p1)
    e1 = ck1.engine(0)
    rc, msg, _ = call(e1)
    assert rc == STATE and "single-key" in msg
    bx = tfhe.encrypt(s.rng, sk1, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk1, e1.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    ck1.close()
    with pytest.raises(tfhe.EngineError) as err:
        eng.blind_rotate(np.zeros((1, 2, N), np.int32), np.zeros((1, 4), np.int32), in_form=1, out_form=0)
    assert err.value.code == STATE and "multi-key" in str(err.value)
    still_right()
    # a multi-device context
    multi = s.ck.engine([0, 0])
    rc, msg, _ = call(multi)
    assert rc == STATE and "multi-device" in msg
    nand_works(multi)
    # an injected allocation failure through the new entry point: NOMEM, and the context goes on working
    lib = eng._lib
    assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
    rc, msg, _ = call()
    lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
    assert rc == NOMEM and "memory" in msg, (rc, msg)
    still_right()
    s.ck.close()


@pytest.mark.gpu
def test_gpu_mk_rotate_oversized_batch_is_refused_before_allocating(tfhe, orc):
    """B = 2^31 - 1 rows of two samples each at (2, 64, 3, 7): the ping-pong workspace alone is 3 TB.  TFHE_ERR_NOMEM, computed and
    refused before any allocation (hipMemGetInfo reads unchanged; the rows are never read), and the context goes on working."""
    P, N, l, beta = SETS[0]
    s = Setup(tfhe, P, N, l, beta, 9800, owners=[1], bits=[1])
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    acc = s.encrypt(_words(s.rng, 1, N))
    rows = np.array([[3, 1]], np.int32)
    ref = _rot(s, orc)
    want = ref.rotate(acc[0], [3], 1).astype(np.int32)
    assert np.array_equal(eng.mk_blind_rotate(acc, rows, in_form=1, out_form=0)[0], want)
    before = _mem_free()
    rc = eng._lib.tfhe_mk_blind_rotate_batch(eng._h, _p(acc), 1, None, _p(rows), 1, 0, None, 1, _p(np.zeros(1, np.int32)), 2**31 - 1, 0)
    assert rc == NOMEM and "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    assert _mem_free() == before
    assert np.array_equal(eng.mk_blind_rotate(acc, rows, in_form=1, out_form=0)[0], want)
    s.ck.close()
