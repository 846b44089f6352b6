"""Programmable bootstrapping: any function of a small encrypted integer in one blind rotation.

A message m of the space Z_p (p a power of two, 2 <= p <= N/2) is encrypted at the phase (2m + 1)/(4p): the centre of the m-th
of 2p equal windows of the torus, in the half [0, 1/2) (the other half is the padding).  A phase within +-1/(4p) of that centre
still decodes to m.  The blind rotation of a sample with the test polynomial v (Engine.bootstrap_tv, tfhe_bootstrap_tv_batch;
bootstrap.jl:50-59) returns the body v[phi] for phi in [0, N) and -v[phi - N] for phi in [N, 2N), phi = the modulus-switched
phase; make_test_vector(f, p, N, q) fills the N / p coefficients of window m with lut_encode(f(m), q), so the result encrypts f(m)
in Z_q.  The output's noise is that of a fresh bootstrap, whatever the input's was, and samples combine linearly in between
(LweSampleArray's +, -, integer scale and add_constant), which is how the functions chain.

Several functions of one input from one blind rotation (Engine.bootstrap_tv_multi, tfhe_bootstrap_tv_multi_batch): sample j of K
(a power of two) is extracted at the accumulator's coefficient j N / K, so its body is v[phi + j N / K].  The input m of Z_p must
then be encrypted as a message of Z_{pK} (lut_encrypt(rng, sk, m, p * K), or any sample whose phase is within +-1/(4pK) of
lut_encode(m, p * K)): phi lies in window m of Z_{pK}, phi + j N / K in window j p + m, below N, so no negacyclic sign enters.
make_multi_test_vector([f_0, ..., f_{K-1}], p, N, q) is the table of g(j p + m) = f_j(m); output j encrypts f_j(m) in Z_q.
The price is log2 K bits of message space: the input's noise must stay within a window K times narrower, and p K <= N / 2.

On the device-resident wire table (Circuit.lut / lut_multi / linear, Engine.lut_level, tfhe_lut_level) LUTs and gates mix in one
circuit through two conversions:
  - a gate-encoded bit (+-1/8, gates.jl) is the message lut_encode(b, 2) = (2b + 1)/8 of Z_2 once GATE_BIT_TO_Z2 = +1/4 is added:
    c.lut(f, [bit_wire], 2, q, const=GATE_BIT_TO_Z2) (or as one term among others of a sum in Z_2);
  - a LUT whose table holds the raw values +-1/8 returns a gate-encoded bit: make_gate_test_vector(pred, p, N) (pred(m) true: +1/8),
    passed to Circuit.lut as a raw table; its output is an operand of any gate.
The coefficients of a combination are the caller's choice, as with LweSampleArray arithmetic: a term of coefficient c multiplies its
sample's noise by |c|, and nothing checks that the sum still decodes.

Under an MKCloudKey the same holds for multi-key samples int32 [P n + 1] (mk_lut_encrypt, mk_lut_decrypt; Engine.mk_bootstrap_tv,
tfhe_mk_bootstrap_tv_batch): the multi-key blind rotation starts its body from the test polynomial, and the result is keyswitched
back to the parties' LWE keys.  programmable_bootstrap and programmable_bootstrap_multi then return int32 arrays rather than
LweSampleArrays, and Circuit runs its LUT and linear nodes on the multi-key wire table.  The multi-key bootstrap is noisier than the
single-key one: under the shipped 2-party set p = 2 is the safe message space.
"""
import numpy as np

from .lwe import LweSampleArray, lwe_encrypt_many, lwe_phase
from .mk_keys import MKCloudKey, MKLweSample, mk_encrypt_torus, mk_phase
from .numeric import wrap32


def _log2(p, what="p"):
    p = int(p)
    if p < 2 or p & (p - 1):
        raise ValueError(f"{what} = {p}: a power of two >= 2")
    return p.bit_length() - 1


GATE_BIT_TO_Z2 = 1 << 30      # +1/4: a gate-encoded bit (+-1/8) plus this is lut_encode(b, 2)


def make_gate_test_vector(pred, p, N):
    """The test polynomial of m -> gate-encoded bit pred(m), Z_p -> {+-1/8}: v[j] = +2^29 where pred(floor(j p / N)) else -2^29,
    int32 [N] (the encoding of gate_* outputs, so the result feeds any gate).  2 <= p <= N / 2, a power of two."""
    _log2(p)
    if p > N // 2:
        raise ValueError(f"p = {p} > N/2 = {N // 2}")
    vals = np.array([1 if pred(m) else -1 for m in range(p)], np.int64) << 29
    return vals[(np.arange(N) * p) // N].astype(np.int32)


def lut_encode(m, p):
    """The Torus32 phase of message m in Z_p: encode_message(2m + 1, 4p) (numeric-functions.jl:42-45) — the centre of the
    m-th window of width 1/(2p); anything within +-1/(4p) of it decodes to m."""
    s = 32 - (_log2(p) + 2)
    return wrap32((2 * np.asarray(m, np.int64) + 1) << s)


def lut_decode(phase, p):
    """The window a Torus32 phase lies in: (uint32(phase) >> (32 - log2 2p)) & (2p - 1).  A value >= p means the phase
    crossed into the padding half: the noise broke the padding bit."""
    s = 32 - (_log2(p) + 1)
    return ((np.asarray(phase, np.int64) & 0xFFFFFFFF) >> s) & (2 * int(p) - 1)


def lut_encrypt(rng, secret_key, m, p):
    """Messages m (ints in [0, p)) of Z_p encrypted under `secret_key` (a SecretKey) with its LWE noise: LweSampleArray."""
    m = np.atleast_1d(np.asarray(m, np.int64))
    if np.any((m < 0) | (m >= p)):
        raise ValueError(f"messages must lie in [0, {p})")
    return LweSampleArray(lwe_encrypt_many(rng, lut_encode(m, p).astype(np.int64), secret_key.params.lwe_noise_stddev, secret_key.key))


def lut_decrypt(secret_key, samples, p):
    """lut_decode of each sample's phase; values >= p flag a broken padding bit."""
    data = samples.data if isinstance(samples, LweSampleArray) else np.asarray(samples, np.int32)
    return lut_decode(lwe_phase(data, secret_key.key), p)


def mk_lut_encrypt(rng, secret_keys, m, p):
    """Messages m of Z_p as multi-key samples under the parties' secret keys (mk_encrypt at the phases lut_encode(m, p)):
    int32 [B][P n + 1]."""
    m = np.atleast_1d(np.asarray(m, np.int64))
    if m.min(initial=0) < 0 or m.max(initial=0) >= p:
        raise ValueError(f"messages must lie in [0, {p})")
    return mk_encrypt_torus(rng, secret_keys, lut_encode(m, p).astype(np.int64))


def mk_lut_decrypt(secret_keys, flat, p):
    """The messages of Z_p of multi-key samples int32 [B][P n + 1] (mk_phase, lut_decode)."""
    return lut_decode(mk_phase(secret_keys, flat), p)


def _samples(data):
    """An LweSampleArray, a list of MKLweSample (as Circuit.run takes them) or int32 rows, as int32 rows."""
    if isinstance(data, LweSampleArray):
        return data.data
    if isinstance(data, (list, tuple)) and data and all(isinstance(x, MKLweSample) for x in data):
        return np.stack([x.flat() for x in data])
    return np.asarray(data, np.int32)


def make_test_vector(f, p, N, q=None):
    """The test polynomial of x -> f(x), Z_p -> Z_q (q defaults to p): v[j] = lut_encode(f(floor(j p / N)), q), int32 [N].
    2 <= p <= N / 2, both powers of two."""
    q = p if q is None else q
    _log2(p)
    _log2(q, "q")
    if p > N // 2:
        raise ValueError(f"p = {p} > N/2 = {N // 2}")
    vals = np.array([int(f(m)) % q for m in range(p)], np.int64)
    return lut_encode(vals[(np.arange(N) * p) // N], q).astype(np.int32)


def programmable_bootstrap(ck, samples, tables_or_functions, index=None, p=8, q=None, with_keyswitch=True, device=0):
    """f(m) for every sample of m in Z_p, in one batch of blind rotations on the GPU.

    `tables_or_functions`: one or a list of callables Z_p -> Z_q (made into test polynomials by make_test_vector) or int32
    test polynomials [N]; `index[g]` picks row g's (None: the first for every row).  p, q: powers of two, 2 <= p <= N/2; an input
    phase must lie within +-1/(4p) of its message's centre.  Returns an LweSampleArray of messages in Z_q (keyswitched back to
    the LWE key unless with_keyswitch is False, then [B][k N + 1] words under the extracted TLWE key).  Under an MKCloudKey the
    samples are multi-key (int32 [B][P n + 1] or a list of MKLweSample), and the result is int32 [B][P n + 1] ([B][P N + 1] without
    keyswitch), the form every multi-key gate function returns."""
    eng = ck.engine(device)
    items = tables_or_functions if isinstance(tables_or_functions, (list, tuple)) else [tables_or_functions]
    tables = np.stack([make_test_vector(t, p, eng.N, q) if callable(t) else np.asarray(t, np.int32) for t in items])
    if isinstance(ck, MKCloudKey):
        return eng.mk_bootstrap_tv(tables, np.atleast_2d(_samples(samples)), index=index, with_keyswitch=with_keyswitch)
    return LweSampleArray(eng.bootstrap_tv(tables, _samples(samples), index=index, with_keyswitch=with_keyswitch))


def make_multi_test_vector(fs, p, N, q=None):
    """The packed test polynomial of the K = len(fs) functions fs[j]: Z_p -> Z_q (q defaults to p) for one multi-output blind
    rotation: make_test_vector(g, p K, N, q) with g(j p + m) = fs[j](m).  K a power of two, p >= 2 a power of two, p K <= N / 2."""
    fs = list(fs)
    K = len(fs)
    if K < 1 or K & (K - 1):
        raise ValueError(f"K = {K} functions: a power of two >= 1")
    _log2(p)
    if p * K > N // 2:
        raise ValueError(f"p K = {p * K} > N/2 = {N // 2}")
    return make_test_vector(lambda x: fs[x // p](x % p), p * K, N, p if q is None else q)


def programmable_bootstrap_multi(ck, samples, fs_or_tables, p, q=None, index=None, with_keyswitch=True, device=0, n_out=None):
    """[f_0(m), ..., f_{K-1}(m)] for every sample of m in Z_p encrypted in Z_{pK}, from one batch of blind rotations on the GPU:
    a list of K LweSampleArrays (keyswitched back to the LWE key unless with_keyswitch is False, then [B][k N + 1] words under the
    extracted TLWE key).

    `fs_or_tables`: a list of K callables Z_p -> Z_q (one packed table, make_multi_test_vector), a list of such lists with the same
    K (`index[g]` picks row g's, None: the first), or int32 packed tables [N] / [n_tv][N], for which `n_out` gives K.  Under an
    MKCloudKey the samples are multi-key, int32 [B][P n + 1], and the K results are int32 arrays."""
    eng = ck.engine(device)
    items = list(fs_or_tables) if isinstance(fs_or_tables, (list, tuple)) else [fs_or_tables]
    if items and all(callable(f) for f in items):
        items = [items]
    tables, ks = [], set()
    for t in items:
        if isinstance(t, (list, tuple)) and all(callable(f) for f in t):
            ks.add(len(t))
            tables.append(make_multi_test_vector(t, p, eng.N, q))
        else:
            tables.extend(np.atleast_2d(np.asarray(t, np.int32)))
    if n_out is not None:
        ks.add(int(n_out))
    if len(ks) != 1:
        raise ValueError(f"the number of outputs is ambiguous: {sorted(ks) or 'not given'} (pass n_out with raw tables)")
    K = ks.pop()
    if isinstance(ck, MKCloudKey):
        out = eng.mk_bootstrap_tv_multi(np.stack(tables), np.atleast_2d(_samples(samples)), K, index=index, with_keyswitch=with_keyswitch)
        return [np.ascontiguousarray(out[:, j]) for j in range(K)]
    out = eng.bootstrap_tv_multi(np.stack(tables), _samples(samples), K, index=index, with_keyswitch=with_keyswitch)
    return [LweSampleArray(np.ascontiguousarray(out[:, j])) for j in range(K)]
