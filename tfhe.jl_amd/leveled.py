"""Leveled mode: external products and CMUX trees on the caller's own TLWE / TGSW samples, no blind rotation.

A table of 2^d TLWE samples is folded by d levels of CMUXes d0 + C (.) (d1 - d0) (the form of bootstrap.jl:19-23, with
tgsw_extern_mul, tgsw.jl:125-129), level v selecting by the TGSW encryption C of address bit v (bit 0 = the lowest): what is
left is table[address], at 2^d - 1 external products.  Each level adds the noise of one external product (about
sqrt((k+1) l N) 2^(beta-1) bs_noise_stddev plus the gadget truncation 2^-(l beta + 1) (1 + k N / 2)^(1/2): 3e-4 of the torus per
level at tfhe_parameters_80) to a message window of 1/8, so d = 8 is far inside it; extracted at coefficient 0 and keyswitched
(out_form 2) the result is an LWE sample under the gate key and an operand of any gate_* / Circuit.

The host side mirrors the reference's constructors under the TLWE key that CloudKey draws and now keeps as
`secret_key.tlwe_key`: tlwe_encrypt (tlwe.jl:63-73 plus a message on the body), tgsw_encrypt_bits (tgsw.jl:84-88 at
bs_noise_stddev).  The device side is Engine.tgsw_load / extern_mul / cmux_tree (tfhe_tgsw_load, tfhe_extern_mul_batch,
tfhe_cmux_tree_batch); cmux_lookup strings them together.
"""
import numpy as np

from .keys import _tlwe_encrypt_zero_many, make_bootstrap_key
from .lwe import LweKey, LweSampleArray
from .numeric import negacyclic_mul_binary, wrap32


def _tlwe_key(secret_key):
    key = getattr(secret_key, "tlwe_key", None)
    if key is None:
        raise ValueError("this SecretKey has no tlwe_key yet: CloudKey(rng, secret_key) draws it and keeps it there")
    return key


def tlwe_trivial(polys, k=1):
    """tlwe_noiseless_trivial (tlwe.jl:77-81) of each message polynomial: int32 [..., N] -> int32 [count][k+1][N], zero masks."""
    mu = np.atleast_2d(np.asarray(polys, np.int32))
    out = np.zeros((mu.shape[0], k + 1, mu.shape[1]), np.int32)
    out[:, k, :] = mu
    return out


def tlwe_encrypt(rng, secret_key, polys):
    """tlwe_encrypt_zero (tlwe.jl:63-73) at bs_noise_stddev plus the message polynomial on the body: int32 [..., N] Torus32
    messages -> int32 [count][k+1][N] under secret_key.tlwe_key."""
    key = _tlwe_key(secret_key)
    mu = np.atleast_2d(np.asarray(polys, np.int32))
    if mu.shape[1] != key.N:
        raise ValueError(f"message polynomials must have {key.N} coefficients, got {mu.shape[1]}")
    out = _tlwe_encrypt_zero_many(rng, secret_key.params.bs_noise_stddev, key, mu.shape[0]).astype(np.int32)
    out[:, key.k, :] = wrap32(out[:, key.k, :].astype(np.int64) + mu)
    return out


def tlwe_phase(secret_key, samples):
    """body - sum_c a_c (*) key_c (negacyclic) of TLWE samples int32 [count][k+1][N]: the noisy message polynomials [count][N]."""
    key = _tlwe_key(secret_key)
    s = np.asarray(samples, np.int32)
    if s.ndim == 2:
        s = s[None]
    ph = s[:, key.k, :].astype(np.int64)
    for c in range(key.k):
        ph = ph - negacyclic_mul_binary(key.key[c], s[:, c, :]).astype(np.int64)
    return wrap32(ph)


def tgsw_encrypt_bits(rng, secret_key, bits):
    """tgsw_encrypt (tgsw.jl:84-88) of each bit at bs_noise_stddev under secret_key.tlwe_key, in the flat layout the engine takes:
    int32 [S][l][k+1][k+1][N] = samples[p, j].a[c] — S entries of the bootstrapping key's canonical form (bootstrap.jl:6-15 makes
    exactly these of the LWE key's bits)."""
    key = _tlwe_key(secret_key)
    p = secret_key.params
    b = np.asarray(bits).astype(bool).reshape(-1).astype(np.int32)
    return make_bootstrap_key(rng, p.bs_noise_stddev, LweKey(None, b.size, key=b), key, p.bs_decomp_length, p.bs_log2_base)


def encode_gate_bit(value):
    """A table entry as the gate encoding of a bit: +1/8 for true, -1/8 for false (gates.jl)."""
    return (1 << 29) if value else -(1 << 29)


def table_to_tlwe(values, N, k=1, encode=encode_gate_bit, rng=None, secret_key=None):
    """A table as TLWE samples int32 [len(values)][k+1][N]: entry i carries encode(values[i]) (a Torus32 word) on coefficient 0 of
    its message polynomial, which is where tlwe_extract_sample (tlwe.jl:55-59) reads.  Trivial (noiseless, public) samples, or —
    with rng and secret_key — encryptions under secret_key.tlwe_key (a private table)."""
    mu = np.zeros((len(values), N), np.int32)
    mu[:, 0] = wrap32(np.array([int(encode(v)) for v in values], np.int64))
    if secret_key is None:
        return tlwe_trivial(mu, k)
    if rng is None:
        raise ValueError("an encrypted table needs rng as well as secret_key")
    return tlwe_encrypt(rng, secret_key, mu)


def cmux_lookup(ck, tables, address_tgsw, out_form=2, device=0, table_index=None):
    """table[address] for B encrypted addresses.  tables: int32 [2^d][k+1][N] (table_to_tlwe) or [T][2^d][k+1][N] with table_index
    [B]; address_tgsw: int32 [B][d][l][k+1][k+1][N], bit v of address g encrypted by tgsw_encrypt_bits (bit 0 = the lowest).
    out_form 2 (default): an LweSampleArray under the gate key, ready for gate_* / Circuit; 1: the extracted samples int32
    [B][k N + 1]; 0: the TLWE samples int32 [B][k+1][N]."""
    a = np.asarray(address_tgsw, np.int32)
    if a.ndim != 6:
        raise ValueError(f"address_tgsw must be [B][depth][l][k+1][k+1][N], got {a.shape}")
    B, depth = a.shape[:2]
    eng = ck.engine(device)
    eng.tgsw_load(a.reshape((B * depth,) + a.shape[2:]))
    sel = np.arange(B * depth, dtype=np.int32).reshape(B, depth)
    out = eng.cmux_tree(tables, sel, table_index=table_index, out_form=out_form)
    return LweSampleArray(out) if out_form == 2 else out
