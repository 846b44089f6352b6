"""Leveled mode under a multi-key cloud key (tfhe_mk_tgsw_load, tfhe_mk_tgsw_expand_load, tfhe_mk_extern_mul_batch,
tfhe_mk_cmux_tree_batch; the mk_* functions of tfhe_jl_amd.leveled) against an integer schoolbook.

The reference of every word comparison is `MKTree` below, written from mk_internals.jl:348-391 (mk_tgsw_extern_mul), :464-471 (the CMUX
form of mk_mux_rotate, without the monomial), :88-95 (mk_tlwe_extract_sample) and :397-411 with keyswitch.jl:45-80 (mk_keyswitch):
negacyclic products as np.convolve on int64, every sum reduced mod 2^32, the oracle's orc_tgsw_constants for the gadget and nothing
else of the oracle, and never the engine.  The reference inverse-transforms every product separately, the engine sums spectra; both are
the integer sum when exact, so every comparison is word for word, with no tolerance.

Noise (why "every address decrypts" is a condition, not a measurement).  In one multi-key external product with a selector of party i
the dominant term is the x / y rows of the OTHER parties: RGSW.Expand builds them as sum_u g^-1(b_q - b_i)[u] (*) f[u], l N products of
a digit (rms 2^(beta-1) / sqrt 3) with the noise of f, and the product then multiplies them by the l N digits of the operand's mask.
At mktfhe_parameters_2party (N = 1024, l = 4, beta = 7, bs_noise_stddev 3.29e-10 = 1.4 units of 2^-32) that is
sqrt(l N) 37 * 1.4 = 3.3e3 units per row word and sqrt(l N) 37 * 3.3e3 = 7.8e6 units = 1.8e-3 of the torus per level; the gadget
truncation 2^-(l beta + 1) sqrt(1 + P N / 2) = 6e-8 is far below it.  A depth-4 tree therefore stays near 4e-3, against the +-1/8 of a
gate-encoded bit and the 2 x 500 such products of one rotation.  test_schoolbook_tree_decrypts_every_address runs the schoolbook alone
at the small sets; the full-size shape (depth 4, each party owning two bits) was run through the same schoolbook on the CPU (12 s,
not part of the suite): 16 of 16 addresses correct, the worst phase 6.3e-3 of the torus from +-1/8.
"""
import ctypes as C

import numpy as np
import pytest

MASK32 = (1 << 32) - 1


def wrap32(v):
    v = np.asarray(v, dtype=np.int64) & MASK32
    return np.where(v >= 2**31, v - 2**32, v).astype(np.int64)


def negacyclic(a, b, N):
    """a * b mod (X^N + 1) over the integers, int64 schoolbook."""
    full = np.convolve(np.asarray(a, np.int64), np.asarray(b, np.int64))
    out = full[:N].copy()
    out[: N - 1] -= full[N:]
    return out


class MKTree:
    """mk_tgsw_extern_mul and CMUX trees in exact integer arithmetic over expanded samples int32 [S][2 l P + 2 l][N] (per sample
    x[l][P] | y[l][P] | c0[l] | c1[l]) with party_of [S]; MK TLWE samples are [P + 1][N] = a_0 ... a_{P-1}, b."""

    def __init__(self, orc, N, l, beta, P, tgsw, party_of, ks=None, n=None, t=8, gamma=2):
        self.N, self.l, self.beta, self.P = N, l, beta, P
        gadget, self.offset = orc.tgsw_constants(l, beta)                        # tgsw.jl:8-21
        assert [int(g) & MASK32 for g in gadget] == [(1 << (32 - p * beta)) & MASK32 for p in range(1, l + 1)]      # (as 32-bit words: 2^31 at beta = 1)
        # |digit| <= 2^(beta-1), |key word| <= 2^31, N terms, up to l P + l products summed before the reduction: no int64 overflow
        assert (beta - 1) + 31 + (N.bit_length() - 1) + (l * P + l - 1).bit_length() < 63
        self.tg = np.asarray(tgsw, np.int64).reshape(-1, 2 * l * P + 2 * l, N)
        self.party_of = [int(v) for v in np.asarray(party_of).reshape(-1)]
        assert len(self.party_of) == self.tg.shape[0]
        self.n, self.t, self.gamma = n, t, gamma
        self.ks = None if ks is None else np.asarray(ks, np.int64).reshape(P, N, t, (1 << gamma) - 1, n + 1)

    def decompose(self, poly):                                                   # tgsw.jl:99-117
        l, beta = self.l, self.beta
        c = wrap32(np.asarray(poly, np.int64) + self.offset)
        half, mask = 1 << (beta - 1), (1 << beta) - 1
        return [((c >> (32 - p * beta)) & mask) - half for p in range(1, l + 1)]

    def extern_mul(self, sample, s):                                             # mk_internals.jl:348-391
        P, l, N = self.P, self.l, self.N
        key, party = self.tg[int(s)], self.party_of[int(s)]
        x = lambda p, q: key[p * P + q]
        y = lambda p, q: key[l * P + p * P + q]
        c0 = lambda p: key[2 * l * P + p]
        c1 = lambda p: key[2 * l * P + l + p]
        da = [self.decompose(sample[i]) for i in range(P)]                       # :361
        db = self.decompose(sample[P])                                           # :362
        out = []
        for i in range(P):                                                       # :373-380
            if i == party:
                acc = sum(negacyclic(da[j][p], y(p, j), N) for p in range(l) for j in range(P))
                acc = acc + sum(negacyclic(db[p], c1(p), N) for p in range(l))
            else:
                acc = sum(negacyclic(da[i][p], y(p, party), N) for p in range(l))
            out.append(wrap32(acc))
        body = sum(negacyclic(da[i][p], x(p, i), N) for p in range(l) for i in range(P))      # :383-386
        body = body + sum(negacyclic(db[p], c0(p), N) for p in range(l))
        out.append(wrap32(body))
        return np.stack(out)

    def cmux(self, s, d0, d1):                                                   # mk_mux_rotate (:464-471) without the monomial
        d0, d1 = np.asarray(d0, np.int64), np.asarray(d1, np.int64)
        return wrap32(d0 + self.extern_mul(wrap32(d1 - d0), s))

    def tree(self, table, sels):
        cur = [np.asarray(t, np.int64) for t in table]
        for s in sels:                                                           # level 0 = the lowest address bit
            cur = [self.cmux(s, cur[2 * i], cur[2 * i + 1]) for i in range(len(cur) // 2)]
        assert len(cur) == 1
        return cur[0]

    def extract(self, sample):                                                   # mk_tlwe_extract_sample, mk_internals.jl:88-95
        P, N = self.P, self.N
        ext = np.empty(P * N + 1, np.int64)
        for p in range(P):                                                       # reverse_polynomial (polynomials.jl:32-35): p[0], -p[N-1], ..., -p[1]
            ext[p * N] = sample[p][0]
            ext[p * N + 1:(p + 1) * N] = -np.asarray(sample[p], np.int64)[:0:-1]
        ext[P * N] = sample[P][0]
        return wrap32(ext)

    def keyswitch(self, ext):                                                    # mk_keyswitch (:397-411) over keyswitch.jl:45-80
        P, N, n, t, gamma = self.P, self.N, self.n, self.t, self.gamma
        res = np.zeros(P * n + 1, np.int64)
        res[P * n] = ext[P * N]
        for p in range(P):
            abar = wrap32(np.asarray(ext[p * N:(p + 1) * N], np.int64) + (1 << (32 - (1 + gamma * t))))
            d = (abar[:, None] >> (32 - gamma * np.arange(1, t + 1))) & ((1 << gamma) - 1)
            i, j = np.nonzero(d)
            part = -self.ks[p][i, j, d[i, j] - 1].sum(axis=0)
            res[p * n:(p + 1) * n] = part[:n]
            res[P * n] += part[n]
        return wrap32(res)


def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


class Setup:
    """P parties with kept TLWE keys, an MKCloudKey at a tiny lwe_size (only the keyswitch and the key's party count read it), and S
    selector bits uni-encrypted by the parties `owners` names, expanded on the host."""

    def __init__(self, tfhe, P, N, l, beta, seed, owners, bits=None, n=4, bs_noise=3.29e-10, device_key=False):
        from tfhe_jl_amd import leveled
        self.p = tfhe.SchemeParameters(n, 0.012467, N, 1, l, beta, bs_noise, 8, 2, 2.44e-5, P)
        self.P, self.N, self.l, self.beta, self.n = P, N, l, beta, n
        self.rng = rng = np.random.default_rng(seed)
        self.sks = [tfhe.SecretKey(rng, self.p) for _ in range(P)]
        self.shared = tfhe.SharedKey(rng, self.p)
        self.parts = [tfhe.CloudKeyPart(rng, sk, self.shared, keep_tlwe_key=True) for sk in self.sks]
        self.ck = tfhe.MKCloudKey(self.parts, expand="device" if device_key else "host")
        self.tlwe_keys = [part.tlwe_key for part in self.parts]
        self.pub = np.stack([part.public_b for part in self.parts])
        self.owners = np.asarray(owners, np.int32)
        S = self.owners.size
        self.bits = rng.integers(0, 2, S) if bits is None else np.asarray(bits)
        self.uni = [np.zeros((S, l, N), np.int32) for _ in range(6)]
        self.tgsw = np.zeros((S, 2 * l * P + 2 * l, N), np.int32)
        for i in range(P):
            mine = np.nonzero(self.owners == i)[0]
            if mine.size == 0:
                continue
            arrs = leveled.mk_tgsw_uni_encrypt_bits(rng, self.tlwe_keys[i], self.shared, self.pub[i], self.bits[mine])
            for dst, a in zip(self.uni, arrs):
                dst[mine] = a
            self.tgsw[mine] = leveled.mk_tgsw_expand(self.p, self.pub, i, *arrs)

    def tree(self, orc, with_ks=False):
        ks = self.ck.keyswitch_key if with_ks else None
        return MKTree(orc, self.N, self.l, self.beta, self.P, self.tgsw, self.owners, ks=ks, n=self.n)

    def encrypt(self, polys):
        from tfhe_jl_amd import leveled
        return leveled.mk_tlwe_encrypt(self.rng, self.tlwe_keys, self.p.bs_noise_stddev, polys)


def _gate_table(bits, N, P):
    from tfhe_jl_amd import leveled
    mu = np.zeros((len(bits), N), np.int32)
    mu[:, 0] = [leveled.encode_gate_bit(b) for b in bits]
    return leveled.mk_tlwe_trivial(mu, P)


# ---- 1. CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported(tfhe):
    import os
    names = ["tfhe_mk_tgsw_load", "tfhe_mk_tgsw_expand_load", "tfhe_mk_extern_mul_batch", "tfhe_mk_cmux_tree_batch"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfhe_mi355x.h")).read()
    lib = tfhe._lib.load()
    for name in names:
        assert name in tfhe._lib.ABI_SYMBOLS and f"int32_t {name}(tfhe_ctx *ctx" in header and hasattr(lib, name), name
    assert lib.tfhe_abi_version() == 7
    for fn in ("mk_tgsw_load", "mk_tgsw_expand_load", "mk_extern_mul", "mk_cmux_tree"):
        assert callable(getattr(tfhe.Engine, fn))


def test_keep_tlwe_key_changes_no_draw_and_no_key_word(tfhe):
    p = tfhe.SchemeParameters(4, 0.012467, 64, 1, 3, 7, 3.29e-10, 8, 2, 2.44e-5, 2)
    made = []
    for keep in (False, True):
        rng = np.random.default_rng(606)
        sk = tfhe.SecretKey(rng, p)
        part = tfhe.CloudKeyPart(rng, sk, tfhe.SharedKey(rng, p), **({"keep_tlwe_key": True} if keep else {}))
        made.append((part, rng.bit_generator.state))
    (a, sa), (b, sb) = made
    assert sa == sb                                                              # not one draw more, not one less
    for name in ("public_b", "c0", "c1", "d0", "d1", "f0", "f1", "ks"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a.tlwe_key is None and b.tlwe_key.key.shape == (1, 64)
    # the kept key is the one the public key was made with: b - s (*) a is the small noise e (mk_internals.jl:131-136)
    rng = np.random.default_rng(606)
    sk = tfhe.SecretKey(rng, p)
    shared = tfhe.SharedKey(rng, p)
    from tfhe_jl_amd.numeric import negacyclic_mul_small
    e = wrap32(b.public_b.astype(np.int64) - negacyclic_mul_small(b.tlwe_key.key[0], shared.a).astype(np.int64))
    assert np.abs(e).max() < 2**8                                                # 3.29e-10 * 2^32 = 1.4


def test_mk_tgsw_expand_equals_the_cloud_keys_host_expansion(tfhe):
    from tfhe_jl_amd import leveled
    s = Setup(tfhe, 3, 32, 2, 8, 11, owners=[0])
    bk = s.ck._expand_on_host()
    assert bk.shape == (3, 4, 2 * 2 * 3 + 4, 32) and np.array_equal(bk, s.ck.bootstrap_key)
    for i, part in enumerate(s.parts):
        got = leveled.mk_tgsw_expand(s.p, s.pub, i, part.c0, part.c1, part.d0, part.d1, part.f0, part.f1)
        assert got.dtype == np.int32 and np.array_equal(got, bk[i]), i
        assert np.array_equal(got[1:3], leveled.mk_tgsw_expand(s.p, s.pub, i, *[getattr(part, a)[1:3] for a in ("c0", "c1", "d0", "d1", "f0", "f1")]))
    # structure (mk_internals.jl:328-336): the party's own x / y columns are d0 / d1, the c rows are copies
    l, P = 2, 3
    assert np.array_equal(bk[1][:, 0 * P + 1], s.parts[1].d0[:, 0]) and np.array_equal(bk[1][:, l * P + 1 * P + 1], s.parts[1].d1[:, 1])
    assert np.array_equal(bk[2][:, 2 * l * P:2 * l * P + l], s.parts[2].c0)
    s.ck.close()


@pytest.mark.parametrize("P,N,l,beta", [(2, 64, 3, 7), (3, 32, 3, 8)])
def test_schoolbook_tree_decrypts_every_address(tfhe, orc, P, N, l, beta):
    """The reference path alone: depth 3, address bits spread over the parties (party 0 owns bit 0, party P - 1 bit 2), a trivial and an
    encrypted table: the schoolbook tree decrypts (mk_tlwe_phase, coefficient 0) to table[address] for all 8 addresses.  The bound on
    the phase error is 1/16 of the torus: a gate's prologue adds two such samples and needs the sum within 1/8 of +-1/4.  Measured
    through this schoolbook: 2^25.3 at (2, 64, 3, 7), 2^22.9 at (3, 32, 3, 8).  The 16-bit gadget (3, 32, 2, 8) of the GPU sets is NOT
    a decrypting set and is compared word for word only: RGSW.Expand's own truncation of b_q - b_i, 2^16 per coefficient, is multiplied
    by r and then by the digits of the operand, 0.3 of the torus after three levels (5 of 16 lookups wrong through this schoolbook)."""
    from tfhe_jl_amd import leveled
    table_bits = [True, False, False, True, True, True, False, True]
    owners = [0, 1 % P, P - 1]
    for address in range(8):
        abits = [(address >> v) & 1 for v in range(3)]
        s = Setup(tfhe, P, N, l, beta, 700 + address, owners, bits=abits)
        ref = s.tree(orc)
        for table in (_gate_table(table_bits, N, P), s.encrypt(_gate_table(table_bits, N, P)[:, P, :])):
            assert table.shape == (8, P + 1, N) and table.dtype == np.int32
            got = ref.tree(table, [0, 1, 2])
            phase = leveled.mk_tlwe_phase(s.tlwe_keys, got.astype(np.int32))[0]
            assert (phase[0] > 0) == table_bits[address], (address, phase[0])
            assert abs(int(phase[0]) - (2**29 if table_bits[address] else -2**29)) < 2**28
            assert np.abs(phase[1:]).max() < 2**28                              # the other coefficients carry no message
        s.ck.close()
    mu = _words(np.random.default_rng(1), 2, N)
    assert np.array_equal(leveled.mk_tlwe_phase(s.tlwe_keys, leveled.mk_tlwe_trivial(mu, P)), mu)
    err = wrap32(leveled.mk_tlwe_phase(s.tlwe_keys, s.encrypt(mu)).astype(np.int64) - mu)
    assert 0 < np.abs(err).max() < 2**8


# ---- 2. GPU: extern_mul word for word ----------------------------------------------------------------------------------------------
EXT_SETS = [(2, 64, 3, 7), (3, 32, 2, 8), (2, 256, 4, 6), (4, 64, 2, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", EXT_SETS)
def test_gpu_mk_extern_mul_equals_schoolbook(tfhe, orc, P, N, l, beta):
    owners = list(range(P)) + [0]                                               # selectors of every party
    s = Setup(tfhe, P, N, l, beta, 4300 + P + N + l, owners)
    eng = s.ck.engine(0)
    rows = s.encrypt(_words(s.rng, 5, N))
    sel = np.array([(g % len(owners)) for g in range(5)], np.int32)
    if P > 2:
        sel[4] = P - 1
    if eng.get_option("exact_domain") == 2:                                     # exact for ANY words: arbitrary rows and the extremes
        extra = _words(s.rng, 4, P + 1, N)
        extra[1], extra[2], extra[3] = 2**31 - 1, -2**31, 0
        rows = np.concatenate([rows, extra])
        sel = np.concatenate([sel, np.array([1, 0, P - 1, len(owners) - 1], np.int32)])
    assert set(s.owners[sel]) == set(range(P))
    ref = s.tree(orc)
    want = np.stack([ref.extern_mul(rows[g], sel[g]) for g in range(len(sel))]).astype(np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    got = eng.mk_extern_mul(rows, sel)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert eng.last_kernel_name() == f"mk_cmux_level_kernel(N={N},P={P},l={l})"
    assert eng.last_rotation_count() == 0 and eng.last_timing_ms(0) > 0
    s.ck.close()


# ---- 3. GPU: the tree word for word ------------------------------------------------------------------------------------------------
TREE_CASES = [c + (d,) for c in EXT_SETS[:2] for d in (1, 2, 3)] + [EXT_SETS[3] + (2,)]      # (4, 64) at depth 2 covers P >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta,depth", TREE_CASES)
def test_gpu_mk_cmux_tree_equals_schoolbook(tfhe, orc, P, N, l, beta, depth):
    B, T, W = 3, 2, 1 << depth
    owners = list(range(P)) + [P - 1, 0]
    s = Setup(tfhe, P, N, l, beta, 5400 + P + N + depth, owners)
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, T * W, N)).reshape(T, W, P + 1, N)
    sel = s.rng.integers(0, len(owners), (B, depth)).astype(np.int32)
    sel[0, :] = [v % P for v in range(depth)]                                   # row 0: its levels use selectors of different parties
    ref = s.tree(orc, with_ks=True)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    for index in (np.array([1, 0, 1], np.int32), None):                         # mixed tables, and NULL = table 0 for every row
        rows = [0] * B if index is None else index
        want = np.stack([ref.tree(data[rows[g]], sel[g]) for g in range(B)])
        got0 = eng.mk_cmux_tree(data, sel, table_index=index, out_form=0)
        assert np.array_equal(got0, want.astype(np.int32)), ("out_form 0", index)
        got1 = eng.mk_cmux_tree(data, sel, table_index=index, out_form=1)
        assert np.array_equal(got1, np.stack([ref.extract(w) for w in want]).astype(np.int32)), ("out_form 1", index)
        got2 = eng.mk_cmux_tree(data, sel, table_index=index, out_form=2)
        assert eng.last_timing_ms(1) > 0
        assert np.array_equal(got2, np.stack([ref.keyswitch(ref.extract(w)) for w in want]).astype(np.int32)), ("out_form 2", index)
    if depth == 1:                                                              # d0 = 0: the CMUX is the plain external product of d1
        zero = data.copy()
        zero[:, 0] = 0
        got = eng.mk_cmux_tree(zero, sel, table_index=np.array([1, 0, 1], np.int32), out_form=0)
        assert np.array_equal(got, eng.mk_extern_mul(zero[[1, 0, 1], 1], sel[:, 0]))
    s.ck.close()


# ---- 4. GPU: spectrum accumulators in global memory --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_global_spectrum_path(tfhe, orc):
    """N = 4096 is the smallest degree at which buf + 3 accumulators + tmp (anyn::lds_bytes(N, 3) = 163856 bytes) pass 160 KB = 163840."""
    P, N, l, beta = 2, 4096, 2, 6
    assert (1 + 3) * (N // 2 + N // 16) * 16 + 4 * N + 16 > 160 * 1024 >= (1 + 3) * (N // 4 + N // 32) * 16 + 2 * N + 16
    s = Setup(tfhe, P, N, l, beta, 6100, owners=[1, 0], n=2)
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, 2, N)).reshape(1, 2, P + 1, N)
    ref = s.tree(orc)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    got = eng.mk_cmux_tree(data, np.array([[0]], np.int32), out_form=0)
    assert eng.last_kernel_name() == f"mk_cmux_level_kernel(N={N},P={P},l={l},spec=global)"
    assert np.array_equal(got[0], ref.tree(data[0], [0]).astype(np.int32))
    s.ck.close()


# ---- 5. GPU: RGSW.Expand on the device ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_tgsw_expand_load_equals_host_expansion(tfhe, orc):
    P, N, l, beta = 3, 32, 2, 8
    owners = [2, 0, 2, 2, 1]                                                    # S = 5, unevenly over the 3 parties, not grouped
    s = Setup(tfhe, P, N, l, beta, 7100, owners)
    eng = s.ck.engine(0)
    got = eng.mk_tgsw_expand_load(s.pub, s.owners, *s.uni, want_expanded=True)
    assert got.shape == s.tgsw.shape and np.array_equal(got, s.tgsw)
    data = s.encrypt(_words(s.rng, 8, N)).reshape(1, 8, P + 1, N)
    sel = np.array([[0, 1, 4], [3, 2, 1]], np.int32)
    ref = s.tree(orc)
    want = np.stack([ref.tree(data[0], sel[g]) for g in range(2)]).astype(np.int32)
    assert np.array_equal(eng.mk_cmux_tree(data, sel, out_form=0), want)
    eng.mk_tgsw_load(s.tgsw, s.owners)                                          # the same store from the host expansion
    assert np.array_equal(eng.mk_cmux_tree(data, sel, out_form=0), want)
    s.ck.close()


# ---- 6. GPU: the shipped 2-party set at full size ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_rom_full_size_two_parties(tfhe, orc):
    """mktfhe_parameters_2party, depth 4, B = 8, two address bits per party, gate-encoded table bits, out_form 2: mk_decrypt returns
    table[address] for every row, the results NANDed with fresh encryptions decrypt too, row 0 equals the schoolbook word for word."""
    from tfhe_jl_amd import leveled
    p = tfhe.mktfhe_parameters_2party
    N, l, beta, P = p.tlwe_polynomial_degree, p.bs_decomp_length, p.bs_log2_base, 2
    rng = np.random.default_rng(8802)
    sks = [tfhe.SecretKey(rng, p) for _ in range(P)]
    shared = tfhe.SharedKey(rng, p)
    parts = [tfhe.CloudKeyPart(rng, sk, shared, keep_tlwe_key=True) for sk in sks]
    ck = tfhe.MKCloudKey(parts, expand="device")
    bits = rng.integers(0, 2, 16).astype(bool)
    addr = rng.integers(0, 16, 8)
    owners = np.array([0, 1, 0, 1], np.int32)                                   # bits 0, 2: party 0; bits 1, 3: party 1
    abits = (addr[:, None] >> np.arange(4)[None, :]) & 1
    uni = [np.zeros((8, 4, l, N), np.int32) for _ in range(6)]
    for i in range(P):
        cols = np.nonzero(owners == i)[0]
        arrs = leveled.mk_tgsw_uni_encrypt_bits(rng, parts[i].tlwe_key, shared, parts[i].public_b, abits[:, cols].reshape(-1))
        for dst, a in zip(uni, arrs):
            dst[:, cols] = a.reshape(8, cols.size, l, N)
    table = _gate_table(bits, N, P)
    out = leveled.mk_cmux_lookup(ck, table, uni, owners)
    assert out.shape == (8, P * p.lwe_size + 1)
    assert np.array_equal(tfhe.mk_decrypt(sks, out), bits[addr])
    y = rng.integers(0, 2, 8).astype(bool)
    nand = tfhe.mk_gate_nand(ck, out, tfhe.mk_encrypt(rng, sks, y))
    assert np.array_equal(tfhe.mk_decrypt(sks, nand), ~(bits[addr] & y))
    pub = np.stack([part.public_b for part in parts])
    tg = np.zeros((4, 2 * l * P + 2 * l, N), np.int32)
    for v in range(4):
        tg[v] = leveled.mk_tgsw_expand(p, pub, owners[v], *[a[0, v:v + 1] for a in uni])[0]
    ref = MKTree(orc, N, l, beta, P, tg, owners)
    ext = leveled.mk_cmux_lookup(ck, table, [a[:1] for a in uni], owners, out_form=1, expand="host")
    assert np.array_equal(ext[0], ref.extract(ref.tree(table, range(4))).astype(np.int32))
    ck.close()


# ---- 7. GPU: the contract ----------------------------------------------------------------------------------------------------------
def _rc(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except Exception as e:                                                      # EngineError carries the TFHE_ERR_* code
        return getattr(e, "code", repr(e))
    return 0


INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6


@pytest.mark.gpu
def test_gpu_mk_contract_errors_leave_the_context_usable(tfhe):
    P, N, l, beta = 2, 64, 3, 7
    s = Setup(tfhe, P, N, l, beta, 9100, owners=[0, 1, 0])
    eng = s.ck.engine(0)
    xs, ys = tfhe.mk_encrypt(s.rng, s.sks, [True, False, True]), tfhe.mk_encrypt(s.rng, s.sks, [True, True, False])

    def nand_works(e=eng):
        assert np.array_equal(tfhe.mk_decrypt(s.sks, e.mk_gate_nand(xs, ys)), [False, True, True])

    table = _gate_table([True, False, False, True], N, P)
    sel = np.zeros((2, 2), np.int32)
    # no selector set yet
    assert _rc(eng.mk_cmux_tree, table, sel) == NO_KEY and _rc(eng.mk_extern_mul, table[:2], [0, 0]) == NO_KEY
    nand_works()
    # parties != the key's P, party_of out of range
    lib, h = eng._lib, eng._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.tfhe_mk_tgsw_load(h, ptr(s.tgsw), ptr(s.owners), 3, 3) == STATE
    for bad in (2, -1):
        who = s.owners.copy(); who[1] = bad
        assert _rc(eng.mk_tgsw_load, s.tgsw, who) == INVALID
        assert _rc(eng.mk_tgsw_expand_load, s.pub, who, *s.uni) == INVALID
    assert lib.tfhe_mk_tgsw_load(h, ptr(s.tgsw), ptr(s.owners), 0, 2) == INVALID
    assert _rc(eng.mk_cmux_tree, table, sel) == NO_KEY                           # none of them left a set behind
    nand_works()
    eng.mk_tgsw_load(s.tgsw, s.owners)
    out = np.empty((2, P * s.n + 1), np.int32)
    for depth in (0, 13, -1):                                                   # (the binding derives depth from sel: the raw call for these)
        assert lib.tfhe_mk_cmux_tree_batch(h, ptr(table), 1, None, depth, ptr(sel), ptr(out), 2, 2) == INVALID
        nand_works()
    for bad in (3, -1):                                                         # three selectors loaded
        b = sel.copy(); b[1, 1] = bad
        assert _rc(eng.mk_cmux_tree, table, b) == INVALID and _rc(eng.mk_extern_mul, table[:2], [0, bad]) == INVALID
        nand_works()
    for bad in (1, -1):                                                         # one table
        assert _rc(eng.mk_cmux_tree, table, sel, np.array([0, bad])) == INVALID
    assert _rc(eng.mk_cmux_tree, table, sel, None, 3) == INVALID                # out_form
    eng.set_option("measure_margin", 1)
    assert _rc(eng.mk_cmux_tree, table, sel) == STATE and _rc(eng.mk_extern_mul, table[:2], [0, 0]) == STATE
    eng.set_option("measure_margin", 0)
    nand_works()
    assert list(tfhe.mk_decrypt(s.sks, eng.mk_cmux_tree(table, np.array([[0, 1]], np.int32)))) == [[True, False, False, True][s.bits[0] + 2 * s.bits[1]]]
    # the single-key trio still refuses this context
    assert _rc(eng.tgsw_load, np.zeros((1, l, 2, 2, N), np.int32)) == STATE and _rc(eng.extern_mul, np.zeros((1, 2, N), np.int32), [0]) == STATE
    assert _rc(eng.cmux_tree, np.zeros((2, 2, N), np.int32), np.zeros((1, 1), np.int32)) == STATE
    # out_form 2 without the keyswitch key: NO_KEY; forms 0 and 1 do not need it
    raw = tfhe.Engine(s.p)
    assert _rc(raw.mk_tgsw_load, s.tgsw, s.owners) == NO_KEY                    # (the binding: no multi-key keys at all)
    assert raw._lib.tfhe_mk_tgsw_load(raw._h, ptr(s.tgsw), ptr(s.owners), 3, 2) == NO_KEY
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)
    raw.mk_tgsw_load(s.tgsw, s.owners)
    s1 = np.array([[0, 1]], np.int32)
    assert _rc(raw.mk_cmux_tree, table, s1, None, 2) == NO_KEY
    assert np.array_equal(raw.mk_cmux_tree(table, s1, out_form=1), eng.mk_cmux_tree(table, s1, out_form=1))
    raw.mk_load_keyswitch_key(s.ck.keyswitch_key, P)
    assert np.array_equal(raw.mk_cmux_tree(table, s1), eng.mk_cmux_tree(table, s1))
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)                            # the same party count keeps the selector set ...
    assert _rc(raw.mk_cmux_tree, table, s1) == 0
    raw.close()
    # ... another party count drops it
    p3 = tfhe.SchemeParameters(s.n, 0.012467, N, 1, l, beta, 3.29e-10, 8, 2, 2.44e-5, 3)
    e3 = tfhe.Engine(p3)
    bk2 = s.ck.bootstrap_key
    e3.mk_load_bootstrap_key(bk2, 2)
    e3.mk_tgsw_load(s.tgsw, s.owners)
    assert _rc(e3.mk_extern_mul, table[:1], [0]) == 0
    e3.mk_load_bootstrap_key(np.zeros((3, s.n, 2 * l * 3 + 2 * l, N), np.int32), 3)
    assert _rc(e3.mk_extern_mul, np.zeros((1, 4, N), np.int32), [0]) == NO_KEY
    e3.close()
    # a single-key context, a multi-device context
    p1 = tfhe.SchemeParameters(16, 1 / 2**15, N, 1, l, beta, 1e-7, 8, 2, 1 / 2**15, 1)
    sk1, ck1 = tfhe.make_key_pair(s.rng, p1)
    e1 = ck1.engine(0)
    e1._mk_parties = 2                                                          # (past the binding's own check: the library's answer)
    assert _rc(e1.mk_tgsw_load, s.tgsw, s.owners) == STATE and _rc(e1.mk_extern_mul, table[:2], [0, 0]) == STATE
    assert _rc(e1.mk_cmux_tree, table, sel) == STATE and _rc(e1.mk_tgsw_expand_load, s.pub, s.owners, *s.uni) == STATE
    bx = tfhe.encrypt(s.rng, sk1, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk1, e1.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    ck1.close()
    multi = s.ck.engine([0, 0])
    assert _rc(multi.mk_tgsw_load, s.tgsw, s.owners) == STATE and _rc(multi.mk_cmux_tree, table, sel) == STATE
    assert _rc(multi.mk_extern_mul, table[:2], [0, 0]) == STATE
    nand_works(multi)
    s.ck.close()


@pytest.mark.gpu
def test_gpu_mk_oversized_request_is_refused_before_allocating(tfhe):
    """depth 12 with B one row more than the device's free memory holds in the first workspace buffer alone: TFHE_ERR_NOMEM, computed and
    refused before any allocation, and the context goes on working."""
    P, N, l, beta = 2, 64, 3, 7
    s = Setup(tfhe, P, N, l, beta, 9200, owners=[1], bits=[1])
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    per_row = (1 << 11) * (P + 1) * N * 4                                       # B 2^(depth-1) MK TLWE samples in the first buffer
    B = free.value // per_row + 1
    table = _gate_table([False] * 4096, N, P)
    assert _rc(eng.mk_cmux_tree, table, np.zeros((B, 12), np.int32)) == NOMEM
    assert "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    small = eng.mk_cmux_tree(_gate_table([True, False], N, P), np.zeros((1, 1), np.int32))
    assert list(tfhe.mk_decrypt(s.sks, small)) == [False]                       # selector bit 1 picks entry 1
    xs = tfhe.mk_encrypt(s.rng, s.sks, [True, False])
    assert np.array_equal(tfhe.mk_decrypt(s.sks, eng.mk_gate_nand(xs, xs)), [False, True])
    s.ck.close()
