"""Blind rotation of the caller's TLWE accumulators (tfhe_blind_rotate_batch; Engine.blind_rotate; tfhe_jl_amd.leveled's
bootstrap_key_selectors, private_lut_encrypt, blind_rotate_lookup, two_stage_lookup, pbs_to_tlwe) against an integer schoolbook.

The reference of every word comparison is `Rotation` below: tests/test_independent.py's `Schoolbook.rotate` restated with two changes — it
starts from a full TLWE accumulator (monomial(a, -barb, N) on every polynomial, the mask included) and it looks the key up as bk[sel[i]] —
on top of `Schoolbook.extern_mul` / `decompose` (exact int64 np.convolve, no transform, no rounding), with tests/test_leveled.py's `Tree`
for the CMUX trees around it.  It never touches the engine or the oracle.

Noise (why "all decrypt" in the full-size test is a condition, not a measurement): the rotation adds what a bootstrap's rotation adds, and
the accumulator's own noise passes through unrefreshed — for a private table one TLWE encryption at bs_noise_stddev (9e-9 at
tfhe_parameters_80), for the two-stage lookup three CMUX levels at about 3e-4 of the torus each (tests/test_leveled.py).  About n / 2 steps
of 3e-4 each give a standard deviation of 4.7e-3 of the torus against an output window of +-1/32 at q = 8; the input's modulus switch at
n = 500 has a standard deviation of sqrt(n / 24) / 2N = 2.2e-3 against the +-1/32 input window of p = 8.  The schoolbook alone was run over
the 16 rows of the full-size test on the CPU (3.3 s per row; not part of the suite): 8 of 8 private-table rows and 8 of 8 two-stage rows
correct, the worst phase 6.3e-3 of the torus from its window's centre (a two-stage row; 5.7e-3 for the private table), five times inside
the +-1/32 window.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_independent import Schoolbook, monomial, wrap32
from test_leveled import LWE_N, Tree, _params, _setup, _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6
SETS = [(64, 1, 3, 8), (1024, 1, 2, 10), (1024, 2, 2, 10), (1024, 1, 4, 6), (2048, 1, 3, 7)]


class Rotation(Tree):
    """The blind rotation of a full TLWE accumulator in exact integer arithmetic over a selector set int32 [S][l][k+1][k+1][N]."""

    def rotate(self, acc, exps, barb, sel=None):
        """acc [k+1][N]; exps: the steps' exponents (any integers, taken mod 2N); sel[i]: the selector of step i (None: i)."""
        N = self.N
        a = [wrap32(monomial(np.asarray(p, np.int64), -int(barb), N)) for p in acc]           # bootstrap.jl:54-56, on every polynomial
        for i, e in enumerate(exps):                                                        # bootstrap.jl:32-39
            if int(e) % (2 * N) == 0:
                continue
            temp = [wrap32(monomial(x, int(e), N) - x) for x in a]                          # bootstrap.jl:21
            prod = self.sb.extern_mul(temp, i if sel is None else int(sel[i]))
            a = [wrap32(x + q) for x, q in zip(a, prod)]                                    # bootstrap.jl:22
        return np.stack(a)

    def rotate_lwe(self, acc, x, sel=None):
        """The same from an LWE sample x [steps+1], switched to Z_2N as bootstrap.jl:74-75 does."""
        w = self.sb.modswitch(x)
        return self.rotate(acc, w[:-1], w[-1], sel)

    def extract_at(self, tlwe, c):
        return self.sb.extract_at(list(np.asarray(tlwe, np.int64)), c)


def _small_keys(tfhe, seed):
    p = _params(tfhe, 64, 1, 3, 8, bs_noise=1e-7)
    rng = np.random.default_rng(seed)
    sk, ck = tfhe.make_key_pair(rng, p)
    return p, rng, sk, ck


# ---- 1. CPU: the reference with the host helpers ----------------------------------------------------------------------------------
def test_schoolbook_rotation_of_a_private_table_decrypts(tfhe):
    """N = 64, k = 1, l = 3, beta = 8, n = LWE_N, p = 4: the schoolbook rotation of private_lut_encrypt(f) by lut_encrypt(m) under the
    bootstrapping key as selectors decrypts (tlwe_phase, coefficient 0) to f(m) for all four m."""
    from tfhe_jl_amd import leveled, lut
    p, rng, sk, ck = _small_keys(tfhe, 61)
    N, k, l, beta = 64, 1, 3, 8
    f = [3, 0, 2, 1]
    acc = leveled.private_lut_encrypt(rng, sk, lambda m: f[m], 4)
    assert acc.shape == (1, k + 1, N) and acc.dtype == np.int32 and np.any(acc[0, 0] != 0)          # an encryption: the mask is not zero
    sels = leveled.bootstrap_key_selectors(ck)
    assert sels.shape == (LWE_N, l, k + 1, k + 1, N) and sels.dtype == np.int32 and np.array_equal(sels.reshape(-1), np.asarray(ck.bootstrap_key).reshape(-1))
    ref = Rotation(N, k, l, beta, sels)
    for m in range(4):
        x = lut.lut_encrypt(rng, sk, [m], 4).data[0]
        got = ref.rotate_lwe(acc[0], x)
        phase = leveled.tlwe_phase(sk, got.astype(np.int32))[0]
        assert lut.lut_decode(phase[0], 4) == f[m], (m, phase[0])
        assert abs(int(wrap32(int(phase[0]) - int(lut.lut_encode(f[m], 4))))) < 2**26            # ... and close to the window's centre
    ck.close()


def test_schoolbook_two_stage_lookup_decrypts_all_16_addresses(tfhe):
    """A 16-entry table as 2^2 test polynomials of p = 4 entries: a depth-2 schoolbook tree over TGSW high bits (selectors behind the
    key's n), then the rotation by the low digit's LWE sample, decrypts at all 16 addresses."""
    from tfhe_jl_amd import leveled, lut
    p, rng, sk, ck = _small_keys(tfhe, 62)
    N, k, l, beta = 64, 1, 3, 8
    table = [int(v) for v in np.random.default_rng(5).integers(0, 4, 16)]
    tables = np.concatenate([leveled.tlwe_trivial(lut.make_test_vector(lambda m, h=h: table[4 * h + m], 4, N), k) for h in range(4)])
    for address in range(16):
        high, low = address >> 2, address & 3
        tg = leveled.tgsw_encrypt_bits(rng, sk, [(high >> v) & 1 for v in range(2)])
        ref = Rotation(N, k, l, beta, np.concatenate([leveled.bootstrap_key_selectors(ck), tg]))
        picked = ref.tree(tables, [LWE_N, LWE_N + 1])
        got = ref.rotate_lwe(picked, lut.lut_encrypt(rng, sk, [low], 4).data[0], sel=range(LWE_N))
        phase = leveled.tlwe_phase(sk, got.astype(np.int32))[0]
        assert lut.lut_decode(phase[0], 4) == table[address], (address, phase[0])
    ck.close()


def test_schoolbook_rotation_result_is_a_table_entry_of_a_tree(tfhe):
    """The out_form 0 result (the final accumulator of a trivial (0, test vector) accumulator) of two samples, used as the two entries of
    a depth-1 schoolbook Tree, decrypts at coefficient 0 to f of the selected sample's message."""
    from tfhe_jl_amd import leveled, lut
    p, rng, sk, ck = _small_keys(tfhe, 63)
    N, k, l, beta = 64, 1, 3, 8
    f = [1, 3, 0, 2]
    acc = leveled.tlwe_trivial(lut.make_test_vector(lambda m: f[m], 4, N), k)[0]
    for m0, m1, bit in [(0, 3, 0), (0, 3, 1), (2, 1, 1), (1, 1, 0)]:
        tg = leveled.tgsw_encrypt_bits(rng, sk, [bit])
        ref = Rotation(N, k, l, beta, np.concatenate([leveled.bootstrap_key_selectors(ck), tg]))
        entries = [ref.rotate_lwe(acc, lut.lut_encrypt(rng, sk, [m], 4).data[0], sel=range(LWE_N)) for m in (m0, m1)]
        got = ref.tree(entries, [LWE_N])
        phase = leveled.tlwe_phase(sk, got.astype(np.int32))[0]
        assert lut.lut_decode(phase[0], 4) == f[(m0, m1)[bit]], (m0, m1, bit, phase[0])
    ck.close()


def test_entry_point_is_declared_and_exported(tfhe):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read(), flags=re.S)
    m = re.search(r"int32_t\s+tfhe_blind_rotate_batch\s*\(([^)]*)\)", txt)
    assert m and len(m.group(1).split(",")) == 12
    assert "tfhe_blind_rotate_batch" in tfhe._lib.ABI_SYMBOLS
    assert hasattr(tfhe._lib.load(), "tfhe_blind_rotate_batch")
    assert callable(getattr(tfhe.Engine, "blind_rotate"))


# ---- 2. GPU: word for word against the schoolbook ---------------------------------------------------------------------------------
S_SEL, B_ROWS = 5, 5
ACC_INDEX = np.array([2, 0, 2, 1, 0], np.int32)                      # a repeated accumulator; rows 1 and 4 read accumulator 0


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
@pytest.mark.parametrize("N,k,l,beta", SETS)
def test_gpu_blind_rotate_equals_schoolbook(tfhe, N, k, l, beta, steps):
    from leveled_ref import ks_ref, ks_schoolbook
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7300 + N + k + l + steps, S_SEL, 5)
    acc = np.ascontiguousarray(tlwe[[1, 3, 4]])                     # T = 3; where the words are arbitrary, accumulator 0 is all -2^31
    rows = _planted_exponents(rng, N, steps)
    sel = np.array([(2 * i + 1) % S_SEL for i in range(steps)], np.int32)
    ref = Rotation(N, k, l, beta, tgsw)
    want = np.stack([ref.rotate(acc[ACC_INDEX[g]], rows[g, :steps], rows[g, steps], sel) for g in range(B_ROWS)])
    eng.tgsw_load(tgsw)
    got0 = eng.blind_rotate(acc, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, out_form=0)
    assert got0.shape == (B_ROWS, k + 1, N) and np.array_equal(got0, want.astype(np.int32)), "out_form 0"
    assert eng.last_kernel_name().startswith(f"tlwe_rotate_kernel(N={N},k={k},l={l},steps={steps}")
    assert eng.last_rotation_count() == B_ROWS and eng.last_timing_ms(0) > 0
    # NULL acc_index = accumulator 0 for every row: rows 1 and 4 of the call above
    got = eng.blind_rotate(acc, rows[[1, 4]], sel=sel, in_form=1, out_form=0)
    assert np.array_equal(got, want[[1, 4]].astype(np.int32)), "NULL acc_index"
    sbk = ks_schoolbook(ck.params, ck.keyswitch_key)
    for n_out in (1, 4):
        want_ext = np.stack([[ref.extract_at(w, j * (N // n_out)) for j in range(n_out)] for w in want]).astype(np.int32)
        got1 = eng.blind_rotate(acc, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, n_out=n_out, out_form=1)
        assert got1.shape == (B_ROWS, n_out, k * N + 1) and np.array_equal(got1, want_ext), ("out_form 1", n_out)
        got2 = eng.blind_rotate(acc, rows, sel=sel, acc_index=ACC_INDEX, in_form=1, n_out=n_out, out_form=2)
        assert eng.last_timing_ms(1) > 0 and eng.last_timing_ms(2) >= eng.last_timing_ms(0)
        assert got2.shape == (B_ROWS, n_out, LWE_N + 1) and np.array_equal(got2, ks_ref(sbk, want_ext)), ("out_form 2", n_out)
    ck.close()


# ---- 3. GPU: in_form 0 is in_form 1 of the modulus-switched words -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [SETS[0], SETS[1]])
def test_gpu_in_form_0_equals_in_form_1_of_modswitch(tfhe, N, k, l, beta):
    steps = 6
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7500 + N, steps, 4)
    x = _words(rng, 4, steps + 1)
    half = 2**32 // (2 * N) // 2                                    # the words just below and at a rounding boundary of decode_message(., 2N)
    x[0, :6] = [2**31 - 1, -2**31, half - 1, half, -half - 1, -half]
    x[1, steps] = 2**31 - 1
    x[2, steps] = -2**31
    x[3, steps] = 3 * half - 1
    sb = Schoolbook(steps, N, k, l, beta, 8, 2, tgsw)
    exps = np.array([sb.modswitch(row) for row in x], np.int64) % (2 * N)
    assert list(exps[0, :6]) == [N, N, 0, 1, 2 * N - 1, 0] and exps[1, steps] == N and exps[2, steps] == N and exps[3, steps] == 1
    eng.tgsw_load(tgsw)
    acc, idx = tlwe[1:], np.array([0, 1, 2, 1], np.int32)
    for form, n_out in ((0, 1), (1, 4)):
        a = eng.blind_rotate(acc, x, acc_index=idx, in_form=0, n_out=n_out, out_form=form)
        b = eng.blind_rotate(acc, exps.astype(np.int32), acc_index=idx, in_form=1, n_out=n_out, out_form=form)
        assert np.array_equal(a, b), form
    want = Rotation(N, k, l, beta, tgsw).rotate(acc[0], exps[0, :steps], exps[0, steps])
    assert np.array_equal(eng.blind_rotate(acc, x[:1], in_form=0, out_form=0)[0], want.astype(np.int32))
    ck.close()


# ---- 4. GPU: a trivial accumulator is the programmable bootstrap --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [SETS[1], SETS[0]])
def test_gpu_trivial_accumulator_equals_bootstrap_tv_multi(tfhe, N, k, l, beta):
    """(0, tv), in_form 0, sel NULL, the key pair's own bootstrapping key as selectors: tfhe_bootstrap_tv_multi_batch word for word, with
    and without keyswitch, n_out 1 and 4.  At N = 1024 a tuned family serves the comparison side, at N = 64 the any-N family."""
    from tfhe_jl_amd import leveled
    p = _params(tfhe, N, k, l, beta)
    rng = np.random.default_rng(7600 + N)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    eng.tgsw_load(leveled.bootstrap_key_selectors(ck))
    tv = _words(rng, 2, N)
    x = _words(rng, 4, LWE_N + 1)
    x[0, :] = 0                                                     # every exponent zero
    x[1, :2] = [2**31 - 1, -2**31]
    idx = np.array([0, 1, 1, 0], np.int32)
    for n_out in (1, 4):
        for ks in (False, True):
            want = eng.bootstrap_tv_multi(tv, x, n_out, index=idx, with_keyswitch=ks)
            assert ("anyn" in eng.last_kernel_name()) == (N == 64), eng.last_kernel_name()
            got = eng.blind_rotate(leveled.tlwe_trivial(tv, k), x, acc_index=idx, in_form=0, n_out=n_out, out_form=2 if ks else 1)
            assert eng.last_kernel_name().startswith("tlwe_rotate_kernel(")
            assert got.shape == want.shape and np.array_equal(got, want), (n_out, ks)
    ck.close()


# ---- 5. GPU: one launch for the rot_net chain ---------------------------------------------------------------------------------------
def _chain(leveled, N, exps, barb):
    r = (2 * N - int(barb)) % (2 * N)
    nodes = [(0, 0, 0, r, r)] + [(0, 0, i, 0, int(e)) for i, e in enumerate(exps)]
    return leveled.RotNet([1] * len(nodes), nodes, N, entries=1, variables=len(exps))


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [SETS[0], SETS[1]])
def test_gpu_one_row_equals_the_rot_net_chain(tfhe, N, k, l, beta):
    """B = 1, out_form 0: the tfhe_rot_net_batch network "a rotated copy by 2N - barb, then `steps` levels of width 1 with records
    (0, 0, i, 0, e_i)", word for word."""
    from tfhe_jl_amd import leveled
    steps = 7
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7700 + N, S_SEL, 4)
    eng.tgsw_load(tgsw)
    sel = np.array([(3 * i + 2) % S_SEL for i in range(steps)], np.int32)
    for barb in (0, 2 * N - 1, N + 3):
        exps = rng.integers(1, 2 * N, steps)
        exps[2] = 0                                                 # (the chain's node is then a copy)
        want = eng.rot_net(tlwe[3:4], _chain(leveled, N, exps, barb), sel[None, :], out_form=0)
        assert eng.last_kernel_name().startswith("rot_net_level_kernel(")
        rows = np.array([list(exps) + [barb]], np.int32)
        got = eng.blind_rotate(tlwe[3:4], rows, sel=sel, in_form=1, out_form=0)
        assert np.array_equal(got, want[:, 0]), barb
    ck.close()


# ---- 6. GPU: spectrum accumulators in global memory ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_anyn_spec_global_at_n64_and_n8192(tfhe):
    """The option anyn_spec = 1 at N = 64 changes where the spectrum accumulators live and no word; at N = 8192 they do not fit LDS and
    one row of two steps equals the rot_net chain (the same arithmetic, also there in global memory)."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = SETS[0]
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7800, 3, 4)
    eng.tgsw_load(tgsw)
    rows = rng.integers(1, 2 * N, (3, 4)).astype(np.int32)
    lds = eng.blind_rotate(tlwe, rows, acc_index=[3, 1, 0], in_form=1, n_out=2, out_form=1)
    assert "spec=global" not in eng.last_kernel_name()
    eng.set_option("anyn_spec", 1)
    glob = eng.blind_rotate(tlwe, rows, acc_index=[3, 1, 0], in_form=1, n_out=2, out_form=1)
    assert eng.last_kernel_name() == f"tlwe_rotate_kernel(N={N},k={k},l={l},steps=3,spec=global)"
    assert np.array_equal(glob, lds)
    ref = Rotation(N, k, l, beta, tgsw)
    assert np.array_equal(glob[0, 1], ref.extract_at(ref.rotate(tlwe[3], rows[0, :3], rows[0, 3]), N // 2).astype(np.int32))
    ck.close()
    N, k, l, beta = 8192, 1, 2, 10
    p = _params(tfhe, N, k, l, beta)
    rng = np.random.default_rng(7801)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    tgsw = leveled.tgsw_encrypt_bits(rng, sk, [1, 0])
    acc = leveled.tlwe_encrypt(rng, sk, _words(rng, 1, N))
    eng.tgsw_load(tgsw)
    exps, barb = [5, 2 * N - 1], N + 1
    want = eng.rot_net(acc, _chain(leveled, N, exps, barb), np.array([[0, 1]], np.int32), out_form=0)
    got = eng.blind_rotate(acc, np.array([exps + [barb]], np.int32), in_form=1, out_form=0)
    assert eng.last_kernel_name() == f"tlwe_rotate_kernel(N={N},k={k},l={l},steps=2,spec=global)"
    assert np.array_equal(got, want[:, 0])
    ck.close()


# ---- 7. GPU: the 80-bit set at full size --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_private_table_and_two_stage_lookup_full_size(tfhe, keys80):
    """8 rows of a private p = 8 table and 8 rows of a 2^3 * 8-entry two-stage lookup, all decrypting; a constant-table row equals
    tfhe_bootstrap_tv_batch word for word."""
    from tfhe_jl_amd import leveled, lut
    K = keys80
    prm = K.params
    N, k, l = prm.tlwe_polynomial_degree, prm.tlwe_mask_size, prm.bs_decomp_length
    rng = np.random.default_rng(8080)
    f = [int(v) for v in rng.integers(0, 8, 8)]
    m = np.arange(8)
    acc = leveled.private_lut_encrypt(rng, K.sk, lambda v: f[v], 8)
    out = leveled.blind_rotate_lookup(K.ck, acc, lut.lut_encrypt(rng, K.sk, m, 8))
    assert list(lut.lut_decrypt(K.sk, out, 8)) == [f[v] for v in m]
    table = [int(v) for v in rng.integers(0, 8, 64)]
    tables = np.concatenate([leveled.tlwe_trivial(lut.make_test_vector(lambda v, h=h: table[8 * h + v], 8, N), k) for h in range(8)])
    addr = rng.integers(0, 64, 8)
    hbits = ((addr >> 3)[:, None] >> np.arange(3)[None, :]) & 1
    tg = leveled.tgsw_encrypt_bits(rng, K.sk, hbits.reshape(-1)).reshape(8, 3, l, k + 1, k + 1, N)
    out = leveled.two_stage_lookup(K.ck, tables, tg, lut.lut_encrypt(rng, K.sk, addr & 7, 8), 8)
    assert list(lut.lut_decrypt(K.sk, out, 8)) == [table[a] for a in addr]
    # the constant test polynomial of the gates: the bootstrap itself
    eng = K.ck.engine(0)
    x = tfhe.encrypt(rng, K.sk, [True, False]).data
    tv = np.full((1, N), 2**29, np.int32)
    for ks in (False, True):
        got = leveled.blind_rotate_lookup(K.ck, leveled.tlwe_trivial(tv, k), x, out_form=2 if ks else 1)
        got = got.data if ks else got[:, 0]
        assert np.array_equal(got, eng.bootstrap_tv(tv, x, with_keyswitch=ks)), ks
    # pbs_to_tlwe: the lookup's result as a TLWE sample whose coefficient 0 carries f(m)
    t = leveled.pbs_to_tlwe(K.ck, lut.lut_encrypt(rng, K.sk, m, 8), lambda v: f[v], 8)
    assert t.shape == (8, k + 1, N)
    assert list(lut.lut_decode(leveled.tlwe_phase(K.sk, t)[:, 0], 8)) == [f[v] for v in m]


# ---- 8. GPU: the contract -----------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _mem_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    return free.value


class _Call:
    """A valid raw call of tfhe_blind_rotate_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, acc, rows, sel):
        self.eng = eng
        self.args = dict(acc=acc, T=acc.shape[0], acc_index=np.zeros(rows.shape[0], np.int32), rows=rows, steps=rows.shape[1] - 1, in_form=1, sel=sel,
                         n_out=1, out=np.empty((rows.shape[0], 4, acc.shape[1] * acc.shape[2]), np.int32), B=rows.shape[0], out_form=0)

    def __call__(self, eng=None, **over):
        a = dict(self.args, **over)
        e = eng or self.eng
        rc = e._lib.tfhe_blind_rotate_batch(e._h, _ptr(a["acc"]), a["T"], _ptr(a["acc_index"]), _ptr(a["rows"]), a["steps"], a["in_form"], _ptr(a["sel"]),
                                            a["n_out"], _ptr(a["out"]), a["B"], a["out_form"])
        return rc, e._lib.tfhe_last_error(e._h).decode()


@pytest.mark.gpu
def test_gpu_contract_refusals_leave_the_context_usable(tfhe):
    from tfhe_jl_amd import leveled
    N, k, l, beta = 64, 1, 3, 8
    p = _params(tfhe, N, k, l, beta, n=16, bs_noise=1e-7)
    rng = np.random.default_rng(97)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    tg = leveled.tgsw_encrypt_bits(rng, sk, [1, 0, 1])
    acc = leveled.tlwe_encrypt(rng, sk, _words(rng, 2, N))
    rows = np.array([[1, 0, 127, 5], [64, 3, 2, 0]], np.int32)
    sel = np.array([2, 0, 1], np.int32)
    want = np.stack([Rotation(N, k, l, beta, tg).rotate(acc[0], r[:3], r[3], sel) for r in rows]).astype(np.int32)
    call = _Call(eng, acc, rows, sel)

    def still_right():
        assert np.array_equal(eng.blind_rotate(acc, rows, sel=sel, in_form=1, out_form=0), want)

    rc, msg = call()                                                # no selector set yet
    assert rc == NO_KEY and "tfhe_tgsw_load" in msg, (rc, msg)
    eng.tgsw_load(tg)
    still_right()
    assert call(B=0)[0] == 0                                        # B = 0 is TFHE_OK
    bad_rows = rows.copy(); bad_rows[1, 2] = 2 * N
    neg_rows = rows.copy(); neg_rows[0, 3] = -1
    refusals = [dict(B=-1), dict(acc=None), dict(rows=None), dict(out=None), dict(steps=0), dict(steps=65537), dict(in_form=2), dict(in_form=-1),
                dict(out_form=3), dict(out_form=-1), dict(T=0), dict(n_out=0), dict(n_out=3, out_form=1), dict(n_out=64, out_form=1),
                dict(n_out=32, out_form=1),                         # a power of two <= 32, but above N / 4 = 16
                dict(n_out=4),                                      # out_form 0 returns one sample
                dict(sel=np.array([0, 3, 1], np.int32)), dict(sel=np.array([0, -1, 1], np.int32)),
                dict(sel=None, steps=4, rows=np.zeros((2, 5), np.int32)),          # selector i for step i needs four selectors
                dict(acc_index=np.array([0, 2], np.int32)), dict(acc_index=np.array([-1, 0], np.int32)), dict(rows=bad_rows), dict(rows=neg_rows)]
    for over in refusals:
        rc, msg = call(**over)
        assert rc == INVALID and msg.startswith("blind_rotate_batch:"), (over, rc, msg)
        still_right()
    assert "rows[1][2] = 128" in call(rows=bad_rows)[1] and "rows[0][3] = -1" in call(rows=neg_rows)[1]      # the message names row and column
    rc, msg = call(rows=bad_rows, in_form=0)                        # LWE samples are any words
    assert rc == 0, msg
    assert np.array_equal(eng.blind_rotate(acc, rows, in_form=1, out_form=0)[0], Rotation(N, k, l, beta, tg).rotate(acc[0], rows[0, :3], rows[0, 3]).astype(np.int32))
    eng.set_option("measure_margin", 1)
    assert call()[0] == STATE
    eng.set_option("measure_margin", 0)
    still_right()
    # out_form 2 without a keyswitch key: NO_KEY; forms 0 and 1 do not need it
    raw = tfhe.Engine(p)
    raw.load_bootstrap_key(ck.bootstrap_key)
    raw.tgsw_load(tg)
    rc, msg = call(eng=raw, out_form=2)
    assert rc == NO_KEY and "keyswitch" in msg, (rc, msg)
    assert np.array_equal(raw.blind_rotate(acc, rows, sel=sel, in_form=1, out_form=0), want)
    raw.load_keyswitch_key(ck.keyswitch_key)
    assert np.array_equal(raw.blind_rotate(acc, rows, sel=sel, in_form=1), eng.blind_rotate(acc, rows, sel=sel, in_form=1))
    raw.close()
    # a multi-device context
    multi = ck.engine([0, 0])
    assert call(eng=multi)[0] == STATE
    bx = tfhe.encrypt(rng, sk, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk, multi.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    # an injected allocation failure through the new entry point: NOMEM, and the context goes on working
    lib = eng._lib
    assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
    rc, msg = call()
    lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
    assert rc == NOMEM and "memory" in msg, (rc, msg)
    still_right()
    ck.close()


@pytest.mark.gpu
def test_gpu_multikey_context_refuses_blind_rotate(tfhe):
    from test_independent import _mk_setup
    p, sks, ck, xs, ys, want = _mk_setup(tfhe, 2, 4, 7, 3, 404)
    eng = ck.engine(0)
    with pytest.raises(tfhe.EngineError) as e:
        eng.blind_rotate(np.zeros((1, 2, 1024), np.int32), np.zeros((1, 4), np.int32), in_form=1, out_form=0)
    assert e.value.code == STATE and "multi-key" in str(e.value)
    assert np.array_equal(eng.mk_gate_nand(xs, ys), want)            # the context still runs its own gates
    ck.close()


@pytest.mark.gpu
def test_gpu_oversized_batch_is_refused_before_allocating(tfhe):
    """B = 2^31 - 1 rows of two samples each at N = 64: the ping-pong workspace alone is 2 TB.  TFHE_ERR_NOMEM, computed and refused
    before any allocation (hipMemGetInfo reads unchanged; the rows are never read), and the context goes on working."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = 64, 1, 3, 8
    p = _params(tfhe, N, k, l, beta, n=16, bs_noise=1e-7)
    rng = np.random.default_rng(15)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    tg = leveled.tgsw_encrypt_bits(rng, sk, [1])
    eng.tgsw_load(tg)
    acc = leveled.tlwe_encrypt(rng, sk, _words(rng, 1, N))
    rows = np.array([[3, 1]], np.int32)
    want = Rotation(N, k, l, beta, tg).rotate(acc[0], [3], 1).astype(np.int32)
    assert np.array_equal(eng.blind_rotate(acc, rows, in_form=1, out_form=0)[0], want)
    before = _mem_free()
    rc = eng._lib.tfhe_blind_rotate_batch(eng._h, _ptr(acc), 1, None, _ptr(rows), 1, 0, None, 1, _ptr(np.zeros(1, np.int32)), 2**31 - 1, 0)
    assert rc == NOMEM and "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    assert _mem_free() == before
    assert np.array_equal(eng.blind_rotate(acc, rows, in_form=1, out_form=0)[0], want)
    ck.close()
