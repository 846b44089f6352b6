"""Leveled mode (tfhe_tgsw_load, tfhe_extern_mul_batch, tfhe_cmux_tree_batch; tfhe_jl_amd.leveled) against an integer schoolbook.

The reference of every word comparison is `Tree` below: the CMUX d0 + C (.) (d1 - d0) (bootstrap.jl:19-23) and its tree restated on top of
tests/test_independent.py's exact int64 `Schoolbook.extern_mul` / `decompose` (tgsw.jl:99-129) with the selector set in the place of the
bootstrapping key (n := S) — np.convolve on int64, no transform, no rounding, and never the engine.

Noise at the shipped sets (why "all 32 addresses correct" is a condition, not a measurement): one external product adds about
sqrt((k+1) l N) 2^(beta-1) bs_noise_stddev of fresh noise plus the gadget truncation 2^-(l beta) sqrt((1 + k N / 2) / 12): 3e-4 of the
torus per level at tfhe_parameters_80 (l beta = 20), 2^-24 at tfhe_parameters_128 (l beta = 21 and a 1e-9 noise) — eight levels stay
two orders of magnitude inside the +-1/8 window, and the keyswitch adds what it adds to every gate.  The schoolbook tree alone was run
over the 32 addresses of the full-size tests on the CPU (1.5 s per row; not part of the suite): 32 of 32 correct at both sets, the worst
phase 1.6e-3 of the torus from +-1/8.
"""
import ctypes as C

import numpy as np
import pytest

from test_independent import Schoolbook, wrap32

SETS = [  # N, k, l, beta
    (1024, 1, 2, 10),
    (1024, 2, 2, 10),
    (2048, 1, 3, 7),
    (512, 1, 2, 10),
    (64, 1, 3, 8),
    (1024, 1, 4, 6),                  # run-time l
]
LWE_N = 6                             # lwe_size of the small key pairs: only the keyswitch reads it


class Tree:
    """CMUX trees in exact integer arithmetic over a selector set int32 [S][l][k+1][k+1][N]."""

    def __init__(self, N, k, l, beta, tgsw):
        S = np.asarray(tgsw).reshape(-1, l, k + 1, k + 1, N).shape[0]
        self.sb = Schoolbook(S, N, k, l, beta, 8, 2, tgsw)
        self.N, self.k = N, k

    def extern_mul(self, tlwe, s):                                   # tgsw.jl:125-129
        return np.stack(self.sb.extern_mul([np.asarray(p, np.int64) for p in tlwe], int(s)))

    def cmux(self, s, d0, d1):                                       # bootstrap.jl:19-23: d0 + C (.) (d1 - d0), every word wrapping
        d0, d1 = np.asarray(d0, np.int64), np.asarray(d1, np.int64)
        return wrap32(d0 + self.extern_mul(wrap32(d1 - d0), s))

    def tree(self, table, sels):
        """table: [2^d][k+1][N]; sels: d selector indices, level 0 = the lowest address bit."""
        cur = [np.asarray(t, np.int64) for t in table]
        for s in sels:
            cur = [self.cmux(s, cur[2 * i], cur[2 * i + 1]) for i in range(len(cur) // 2)]
        assert len(cur) == 1
        return cur[0]

    def extract(self, tlwe):                                         # tlwe.jl:55-59
        return self.sb.extract_at(list(np.asarray(tlwe, np.int64)), 0)


def _params(tfhe, N, k, l, beta, n=LWE_N, bs_noise=9e-9):
    return tfhe.SchemeParameters(n, 1 / 2**15, N, k, l, beta, bs_noise, 8, 2, 1 / 2**15, 1)


def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


# ---- 1. CPU: the reference itself and the host helpers ---------------------------------------------------------------------------
def test_schoolbook_tree_decrypts_every_address(tfhe):
    """N = 64, k = 1, l = 3, beta = 8, depth 3: the schoolbook tree over tgsw_encrypt_bits selectors and a table_to_tlwe table decrypts
    (tlwe_phase, coefficient 0) to table[address] for all 8 addresses, for a trivial and for an encrypted table."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = 64, 1, 3, 8
    p = _params(tfhe, N, k, l, beta, bs_noise=1e-7)
    rng = np.random.default_rng(31)
    sk, ck = tfhe.make_key_pair(rng, p)
    assert sk.tlwe_key is not None and sk.tlwe_key.key.shape == (k, N)
    bits = [True, False, False, True, True, True, False, True]
    for table in (leveled.table_to_tlwe(bits, N, k), leveled.table_to_tlwe(bits, N, k, rng=rng, secret_key=sk)):
        assert table.shape == (8, k + 1, N) and table.dtype == np.int32
        for address in range(8):
            abits = [(address >> v) & 1 for v in range(3)]
            tg = leveled.tgsw_encrypt_bits(rng, sk, abits)
            assert tg.shape == (3, l, k + 1, k + 1, N) and tg.dtype == np.int32
            got = Tree(N, k, l, beta, tg).tree(table, [0, 1, 2])
            phase = leveled.tlwe_phase(sk, got.astype(np.int32))[0]
            assert (phase[0] > 0) == bits[address], (address, phase[0])
            assert abs(int(phase[0]) - (2**29 if bits[address] else -2**29)) < 2**26      # ... and close to +-1/8, not just its sign
            assert np.abs(phase[1:].astype(np.int64)).max() < 2**26                      # the other coefficients carry no message
    # the helpers against each other: a trivial sample's phase is its message; an encryption's is the message plus small noise
    mu = _words(rng, 2, N)
    assert np.array_equal(leveled.tlwe_phase(sk, leveled.tlwe_trivial(mu, k)), mu)
    err = wrap32(leveled.tlwe_phase(sk, leveled.tlwe_encrypt(rng, sk, mu)).astype(np.int64) - mu)
    assert 0 < np.abs(err).max() < 2**14                                                  # 1e-7 * 2^32 = 430, 6 sigma far below 2^14
    ck.close()


def test_keeping_the_tlwe_key_draws_nothing(tfhe):
    """CloudKey keeps the TLWE key on the secret side without consuming a draw: ck.bootstrap_key for a fixed seed equals
    make_bootstrap_key replayed from the same generator state with a TLWE key drawn as CloudKey draws it."""
    from tfhe_jl_amd import keys
    p = _params(tfhe, 64, 1, 3, 8)
    rng = np.random.default_rng(77)
    sk = tfhe.SecretKey(rng, p)
    assert sk.tlwe_key is None
    state = rng.bit_generator.state
    ck = tfhe.CloudKey(rng, sk)
    after = rng.bit_generator.state
    replay = np.random.default_rng(0)
    replay.bit_generator.state = state
    tk = keys.TLweKey(replay, 64, 1)
    bk = keys.make_bootstrap_key(replay, p.bs_noise_stddev, sk.key, tk, 3, 8)
    ks = keys.make_keyswitch_key(replay, p.ks_noise_stddev, 8, 2, sk.key, tk)
    assert np.array_equal(ck.bootstrap_key, bk) and np.array_equal(ck.keyswitch_key, ks)
    assert np.array_equal(sk.tlwe_key.key, tk.key)
    assert replay.bit_generator.state == after                                            # not one draw more, not one less
    ck.close()


# ---- operands for the GPU comparisons --------------------------------------------------------------------------------------------
def _setup(tfhe, N, k, l, beta, seed, S, n_tlwe):
    """A key pair's engine, S selectors and n_tlwe TLWE samples: arbitrary Int32 words with the extreme rows planted where the set is
    exact for ANY words (exact_domain 2), real encryptions otherwise."""
    from tfhe_jl_amd import leveled
    p = _params(tfhe, N, k, l, beta)
    rng = np.random.default_rng(seed)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    if eng.get_option("exact_domain") == 2:
        tgsw = _words(rng, S, l, k + 1, k + 1, N)
        tgsw[0, 0, 0, 0, :] = 2**31 - 1
        tgsw[1 % S, 0, 0, k, :] = -2**31
        tgsw[S - 1, l - 1, k, k, :] = 0
        tlwe = _words(rng, n_tlwe, k + 1, N)
        tlwe[0, :, :] = 2**31 - 1
        tlwe[1, :, :] = -2**31
        tlwe[2, :, :] = 0
    else:
        tgsw = leveled.tgsw_encrypt_bits(rng, sk, rng.integers(0, 2, S))
        tlwe = leveled.tlwe_encrypt(rng, sk, _words(rng, n_tlwe, N))
    return rng, sk, ck, eng, tgsw, tlwe


# ---- 2. GPU: extern_mul word for word --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", SETS)
def test_gpu_extern_mul_equals_schoolbook(tfhe, N, k, l, beta):
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 4100 + N + k + l, 3, 5)
    sel = np.array([0, 2, 1, 2, 0], np.int32)                      # three selectors, two of them used twice
    ref = Tree(N, k, l, beta, tgsw)
    want = np.stack([ref.extern_mul(tlwe[g], sel[g]) for g in range(5)]).astype(np.int32)
    eng.tgsw_load(tgsw)
    got = eng.extern_mul(tlwe, sel)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert eng.last_kernel_name().startswith(f"cmux_level_kernel(N={N},k={k},l={l}")
    assert eng.last_rotation_count() == 0 and eng.last_timing_ms(0) > 0
    ck.close()


# ---- 3. GPU: cmux_tree word for word ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("N,k,l,beta", [SETS[0], SETS[1], SETS[4]])
def test_gpu_cmux_tree_equals_schoolbook(tfhe, N, k, l, beta, depth):
    B, T, W = 3, 2, 1 << depth
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 5200 + N + k + l + depth, 4, T * W)
    data = tlwe.reshape(T, W, k + 1, N)
    sel = rng.integers(0, 4, (B, depth)).astype(np.int32)
    ref = Tree(N, k, l, beta, tgsw)
    eng.tgsw_load(tgsw)
    for index in (np.array([1, 0, 1], np.int32), None):            # mixed tables, and NULL = table 0 for every row
        rows = [0] * B if index is None else index
        want = np.stack([ref.tree(data[rows[g]], sel[g]) for g in range(B)])
        want_ext = np.stack([ref.extract(w) for w in want]).astype(np.int32)
        got0 = eng.cmux_tree(data, sel, table_index=index, out_form=0)
        assert np.array_equal(got0, want.astype(np.int32)), ("out_form 0", index)
        got1 = eng.cmux_tree(data, sel, table_index=index, out_form=1)
        assert np.array_equal(got1, want_ext), ("out_form 1", index)
        got2 = eng.cmux_tree(data, sel, table_index=index, out_form=2)
        assert eng.last_timing_ms(1) > 0
        assert np.array_equal(got2, eng.keyswitch(got1)), ("out_form 2", index)
        from leveled_ref import ks_ref, ks_schoolbook                  # (imported here: leveled_ref imports Tree from this module)
        assert np.array_equal(got2, ks_ref(ks_schoolbook(ck.params, ck.keyswitch_key), want_ext)), ("out_form 2 against the integer keyswitch", index)
    if depth == 1:                                                  # d0 = 0: the CMUX is the plain external product of d1
        zero = data.copy()
        zero[:, 0] = 0
        got = eng.cmux_tree(zero, sel, table_index=np.array([1, 0, 1], np.int32), out_form=0)
        assert np.array_equal(got, eng.extern_mul(zero[[1, 0, 1], 1], sel[:, 0]))
    ck.close()


# ---- 4. GPU: the shipped sets at full size ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["80", "128"])
def test_gpu_encrypted_rom_full_size(tfhe, keys80, keys128, which):
    """Depth 8: 256 random table bits read at 32 random encrypted addresses (8 fresh TGSW each), out_form 2.  All 32 decrypt to
    table[address]; NANDed with fresh encryptions through the gates they still do; two rows equal the schoolbook tree word for word."""
    from tfhe_jl_amd import leveled
    K = keys80 if which == "80" else keys128
    p = K.params
    N, k, l, beta = p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length, p.bs_log2_base
    rng = np.random.default_rng(8800 + int(which))
    bits = rng.integers(0, 2, 256).astype(bool)
    addr = rng.integers(0, 256, 32)
    table = leveled.table_to_tlwe(bits, N, k)
    abits = (addr[:, None] >> np.arange(8)[None, :]) & 1
    tgsw = leveled.tgsw_encrypt_bits(rng, K.sk, abits.reshape(-1)).reshape(32, 8, l, k + 1, k + 1, N)
    out = leveled.cmux_lookup(K.ck, table, tgsw)
    assert np.array_equal(tfhe.decrypt(K.sk, out), bits[addr])
    y = rng.integers(0, 2, 32).astype(bool)
    nand = tfhe.gate_nand(K.ck, out, tfhe.encrypt(rng, K.sk, y))
    assert np.array_equal(tfhe.decrypt(K.sk, nand), ~(bits[addr] & y))
    ext = leveled.cmux_lookup(K.ck, table, tgsw[:2], out_form=1)
    for g in range(2):
        ref = Tree(N, k, l, beta, tgsw[g])
        assert np.array_equal(ext[g], ref.extract(ref.tree(table, range(8))).astype(np.int32)), g


# ---- 5. GPU: the contract --------------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    try:
        fn(*args)
    except Exception as e:                                          # EngineError carries the TFHE_ERR_* code
        return getattr(e, "code", repr(e))
    return 0


def _nand_works(tfhe, rng, sk, ck):
    x, y = np.array([True, False, True]), np.array([True, True, False])
    got = tfhe.decrypt(sk, tfhe.gate_nand(ck, tfhe.encrypt(rng, sk, x), tfhe.encrypt(rng, sk, y)))
    assert np.array_equal(got, ~(x & y))


INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6


@pytest.mark.gpu
def test_gpu_contract_errors_leave_the_context_usable(tfhe):
    from tfhe_jl_amd import leveled
    N, k, l, beta = 64, 1, 3, 8
    p = _params(tfhe, N, k, l, beta, n=16, bs_noise=1e-7)
    rng = np.random.default_rng(99)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    table = leveled.table_to_tlwe([True, False, False, True], N, k)
    sel = np.zeros((2, 2), np.int32)
    # no selector set yet
    assert _rc(eng.cmux_tree, table, sel) == NO_KEY
    assert _rc(eng.extern_mul, table[:2], [0, 0]) == NO_KEY
    _nand_works(tfhe, rng, sk, ck)
    tg = leveled.tgsw_encrypt_bits(rng, sk, [1, 0, 1])
    eng.tgsw_load(tg)
    lib, h = eng._lib, eng._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.empty((2, 17), np.int32)
    for depth in (0, 13, -1):                                       # (the binding derives depth from sel: the raw call for these)
        assert lib.tfhe_cmux_tree_batch(h, ptr(table), 1, None, depth, ptr(sel), ptr(out), 2, 2) == INVALID
        _nand_works(tfhe, rng, sk, ck)
    for bad in (3, -1):                                             # three selectors loaded
        s = sel.copy(); s[1, 1] = bad
        assert _rc(eng.cmux_tree, table, s) == INVALID
        assert _rc(eng.extern_mul, table[:2], [0, bad]) == INVALID
        _nand_works(tfhe, rng, sk, ck)
    for bad in (1, -1):                                             # one table
        assert _rc(eng.cmux_tree, table, sel, np.array([0, bad])) == INVALID
        _nand_works(tfhe, rng, sk, ck)
    assert _rc(eng.cmux_tree, table, sel, None, 3) == INVALID       # out_form
    eng.set_option("measure_margin", 1)
    assert _rc(eng.cmux_tree, table, sel) == STATE and _rc(eng.extern_mul, table[:2], [0, 0]) == STATE
    eng.set_option("measure_margin", 0)
    _nand_works(tfhe, rng, sk, ck)
    # a second load replaces the first: one selector now, index 1 is out of range, index 0 is the new sample
    tg2 = leveled.tgsw_encrypt_bits(rng, sk, [0])
    x = leveled.tlwe_encrypt(rng, sk, _words(rng, 1, N))
    before = eng.extern_mul(x, [0])
    eng.tgsw_load(tg2)
    assert _rc(eng.extern_mul, x, [1]) == INVALID
    after = eng.extern_mul(x, [0])
    assert np.array_equal(after[0], Tree(N, k, l, beta, tg2).extern_mul(x[0], 0).astype(np.int32)) and not np.array_equal(after, before)
    assert np.array_equal(before[0], Tree(N, k, l, beta, tg).extern_mul(x[0], 0).astype(np.int32))
    # out_form 2 without a keyswitch key: NO_KEY; forms 0 and 1 do not need it
    raw = tfhe.Engine(p)
    raw.load_bootstrap_key(ck.bootstrap_key)
    raw.tgsw_load(tg2)
    s1 = np.zeros((1, 2), np.int32)
    assert _rc(raw.cmux_tree, table, s1, None, 2) == NO_KEY
    assert np.array_equal(raw.cmux_tree(table, s1, out_form=1), eng.cmux_tree(table, s1, out_form=1))
    raw.load_keyswitch_key(ck.keyswitch_key)
    assert np.array_equal(raw.cmux_tree(table, s1), eng.cmux_tree(table, s1))
    raw.close()
    # a multi-device context
    multi = ck.engine([0, 0])
    assert _rc(multi.tgsw_load, tg2) == STATE and _rc(multi.cmux_tree, table, s1) == STATE and _rc(multi.extern_mul, x, [0]) == STATE
    bx = tfhe.encrypt(rng, sk, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk, multi.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    assert lib.tfhe_abi_version() == 7
    ck.close()


@pytest.mark.gpu
def test_gpu_multikey_context_refuses_leveled_calls(tfhe):
    from test_independent import _mk_setup
    p, sks, ck, xs, ys, want = _mk_setup(tfhe, 2, 4, 7, 3, 402)
    eng = ck.engine(0)
    N, l = 1024, 4
    tg = np.zeros((1, l, 2, 2, N), np.int32)
    x = np.zeros((1, 2, N), np.int32)
    assert _rc(eng.tgsw_load, tg) == STATE and _rc(eng.extern_mul, x, [0]) == STATE
    assert _rc(eng.cmux_tree, np.zeros((2, 2, N), np.int32), np.zeros((1, 1), np.int32)) == STATE
    assert np.array_equal(eng.mk_gate_nand(xs, ys), want)          # the context still runs its own gates
    ck.close()


@pytest.mark.gpu
def test_gpu_oversized_request_is_refused_before_allocating(tfhe):
    """depth 12 with B one row more than the device's free memory holds in the first workspace buffer alone: TFHE_ERR_NOMEM, computed and
    refused before any allocation (no HIP fault), and the context goes on working."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = 64, 1, 3, 8
    p = _params(tfhe, N, k, l, beta, n=16, bs_noise=1e-7)
    rng = np.random.default_rng(12)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    eng.tgsw_load(leveled.tgsw_encrypt_bits(rng, sk, [1]))
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    per_row = (1 << 11) * (k + 1) * N * 4                           # B 2^(depth-1) TLWE samples in the first buffer
    B = free.value // per_row + 1
    table = leveled.table_to_tlwe([False] * 4096, N, k)
    sel = np.zeros((B, 12), np.int32)
    assert _rc(eng.cmux_tree, table, sel) == NOMEM
    assert "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    small = eng.cmux_tree(leveled.table_to_tlwe([True, False], N, k), np.zeros((1, 1), np.int32))
    assert list(tfhe.decrypt(sk, small)) == [False]                # selector bit 1 picks entry 1
    _nand_works(tfhe, rng, sk, ck)
    ck.close()
