#!/usr/bin/env python3
"""Encrypted 16-bit addition with programmable bootstrapping, against the ripple-carry adder built from gates.

Each operand is 8 base-4 digits, each digit encrypted as a message of Z_8 (tfhe_jl_amd.lut, p = 8).  Per digit the sum
s = a + b + carry (0 .. 7) is a plain sum of LWE samples; the three encodings (2x + 1)/32 add up to (2s + 3)/32, so a trivial
constant of -2/32 puts it at lut_encode(s, 8).  One tfhe_bootstrap_tv_batch call then evaluates both s mod 4 (the digit) and
s >= 4 (the next carry) through tv_index: 8 calls of 2 x 1024 rotations add 1024 pairs.  The gate adder (5 gates per bit,
a 32-level carry chain) runs as Circuit.run_batch over the same 1024 instances.

The third variant encrypts every digit as a message of Z_16 (p = 8 messages in a space of p K = 16, K = 2) and takes digit and
carry from ONE rotation per sum (tfhe_bootstrap_tv_multi_batch, make_multi_test_vector): 8 calls of 1024 rotations.  Its noise
headroom is half the Z_8 adder's, so it reports its wrong sums instead of asserting that there are none.

Both LUT adders also run as a Circuit of lut / lut_multi nodes (lut_adder_circuit) with run_batch over the same 1024 instances: the
digit sums are formed on the device from the wire table (tfhe_lut_level), nothing crosses PCIe between the digits, and the result
words are those of the host-orchestrated adders."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe
from tfhe_jl_amd.lut import lut_decrypt, lut_encode, lut_encrypt, make_multi_test_vector, make_test_vector

P = 8            # message space of a digit sum
DIGITS = 8       # base-4 digits of a 16-bit operand
P_MULTI = 16     # the one-rotation adder: digit sums of Z_8 encrypted in Z_16, two outputs per rotation


def encrypt_digits(rng, sk, values, space=P):
    """int [M] -> [DIGITS] LweSampleArrays of M samples (digit i of every value, in Z_space)."""
    values = np.asarray(values, np.int64)
    return [lut_encrypt(rng, sk, (values >> (2 * i)) & 3, space) for i in range(DIGITS)]


def lut_add16(ck, a, b, device=0):
    """Digit-wise sums with carries: [DIGITS + 1] LweSampleArrays (the last one: the carry out, a digit 0 / 1)."""
    eng = ck.engine(device)
    tables = np.stack([make_test_vector(lambda s: s % 4, P, eng.N), make_test_vector(lambda s: s >= 4, P, eng.N)])
    M = len(a[0])
    index = np.repeat(np.array([0, 1], np.int32), M)
    out, carry = [], None
    for i in range(DIGITS):
        s = a[i] + b[i]
        s = s.add_constant(-int(lut_encode(0, P))) if carry is None else (s + carry).add_constant(-2 * int(lut_encode(0, P)))
        both = eng.bootstrap_tv(tables, np.concatenate([s.data, s.data]), index=index)
        out.append(tfhe.LweSampleArray(both[:M]))
        carry = tfhe.LweSampleArray(both[M:])
    return out + [carry]


def lut_add16_multi(ck, a, b, device=0):
    """lut_add16 on digits encrypted in Z_16 (encrypt_digits(..., P_MULTI)): digit s mod 4 and carry s >= 4 of every sum from one
    multi-output rotation, both again in Z_16."""
    eng = ck.engine(device)
    table = make_multi_test_vector([lambda s: s % 4, lambda s: s >= 4], P, eng.N, P_MULTI)
    out, carry = [], None
    for i in range(DIGITS):
        s = a[i] + b[i]
        s = s.add_constant(-int(lut_encode(0, P_MULTI))) if carry is None else (s + carry).add_constant(-2 * int(lut_encode(0, P_MULTI)))
        both = eng.bootstrap_tv_multi(table, s.data, 2)
        out.append(tfhe.LweSampleArray(both[:, 0]))
        carry = tfhe.LweSampleArray(both[:, 1])
    return out + [carry]


DIGIT = lambda s: s % 4                       # (one callable each: equal (f, p, q) share a table per level)
CARRY = lambda s: s >= 4


def lut_adder_circuit(multi=False):
    """lut_add16 (multi=False: two lut nodes per digit, Z_8) or lut_add16_multi (one lut_multi node per digit, Z_16) as a Circuit:
    inputs a_0 .. a_7, b_0 .. b_7 (digit samples), outputs the 8 digits and the carry out.  Row sums a + b + carry - const are the
    host adders' (LweSampleArray + and add_constant, mod 2^32), so the words are the same."""
    space = P_MULTI if multi else P
    c = tfhe.Circuit()
    a, b = c.inputs(DIGITS), c.inputs(DIGITS)
    outs, carry = [], None
    for i in range(DIGITS):
        terms = [a[i], b[i]] + ([] if carry is None else [carry])
        const = -(1 if carry is None else 2) * int(lut_encode(0, space))
        if multi:
            digit, carry = c.lut_multi([DIGIT, CARRY], terms, P, space, const=const)
        else:
            digit, carry = c.lut(DIGIT, terms, P, const=const), c.lut(CARRY, terms, P, const=const)
        outs.append(digit)
    c.set_outputs(outs + [carry])
    return c


def circuit_inputs(a, b):
    """[DIGITS] LweSampleArrays of M samples, twice -> run_batch's inputs [M][2 DIGITS][n + 1]."""
    return np.ascontiguousarray(np.stack([d.data for d in a + b], axis=1))


def decrypt_sum(sk, digits, space=P):
    return sum(lut_decrypt(sk, d, space).astype(np.int64) << (2 * i) for i, d in enumerate(digits))


def gate_adder():
    """Ripple-carry adder: sum_i = a_i ^ b_i ^ c_i, c_{i+1} = (a_i & b_i) | (c_i & (a_i ^ b_i)); 17 output bits."""
    c = tfhe.Circuit()
    a, b = c.inputs(16), c.inputs(16)
    outs, carry = [], None
    for i in range(16):
        x = c.xor(a[i], b[i])
        if carry is None:
            outs.append(x)
            carry = c.and_(a[i], b[i])
        else:
            outs.append(c.xor(x, carry))
            carry = c.or_(c.and_(a[i], b[i]), c.and_(carry, x))
    c.set_outputs(outs + [carry])
    return c


def main(M=1024):
    rng = np.random.default_rng(2024)
    sk, ck = tfhe.make_key_pair(rng)
    x, y = rng.integers(0, 2**16, size=M), rng.integers(0, 2**16, size=M)

    a, b = encrypt_digits(rng, sk, x), encrypt_digits(rng, sk, y)
    lut_add16(ck, a, b)                                            # (warm-up: first launches, LDS attributes)
    t0 = time.perf_counter()
    digits = lut_add16(ck, a, b)
    t_lut = time.perf_counter() - t0
    assert np.array_equal(decrypt_sum(sk, digits), x + y), "LUT adder: wrong sums"

    a16, b16 = encrypt_digits(rng, sk, x, P_MULTI), encrypt_digits(rng, sk, y, P_MULTI)
    lut_add16_multi(ck, a16, b16)
    t0 = time.perf_counter()
    digits16 = lut_add16_multi(ck, a16, b16)
    t_multi = time.perf_counter() - t0
    wrong_multi = int(np.sum(decrypt_sum(sk, digits16, P_MULTI) != x + y))

    res_words = {}
    t_circ = {}
    for multi, (da, db, host) in ((False, (a, b, digits)), (True, (a16, b16, digits16))):
        lc = lut_adder_circuit(multi)
        inp = circuit_inputs(da, db)
        lc.run_batch(ck, inp)                                     # (warm-up: workspaces and staging blocks at full size)
        t0 = time.perf_counter()
        res = lc.run_batch(ck, inp)
        t_circ[multi] = time.perf_counter() - t0
        assert np.array_equal(res, np.stack([d.data for d in host], axis=1)), "LUT circuit: words differ from the host adder's"
        res_words[multi] = res
    assert np.array_equal(decrypt_sum(sk, [tfhe.LweSampleArray(res_words[False][:, i]) for i in range(DIGITS + 1)]), x + y)

    circ = gate_adder()
    bits = lambda v: np.stack([(v >> i) & 1 for i in range(16)], axis=1).astype(bool)
    inputs = np.stack([tfhe.encrypt(rng, sk, np.concatenate([bits(x)[m], bits(y)[m]])).data for m in range(M)])
    circ.run_batch(ck, inputs[:8])
    t0 = time.perf_counter()
    res = circ.run_batch(ck, inputs)
    t_gate = time.perf_counter() - t0
    got = np.array([sum(int(v) << i for i, v in enumerate(tfhe.decrypt(sk, res[m]))) for m in range(M)])
    assert np.array_equal(got, x + y), "gate adder: wrong sums"

    print(f"{M} encrypted 16-bit additions, all correct")
    print(f"  LUT digits (8 calls of {2 * M} rotations): {t_lut * 1e3:8.1f} ms")
    print(f"  LUT digits, digit and carry from one rotation (8 calls of {M} rotations, Z_16): {t_multi * 1e3:8.1f} ms, "
          f"{wrong_multi} wrong sums of {M}")
    print(f"  LUT digits as a device circuit (run_batch, {DIGITS} levels of {2 * M} rotations, Z_8):         {t_circ[False] * 1e3:8.1f} ms")
    print(f"  LUT digits as a device circuit, one rotation per digit (run_batch, Z_16):              {t_circ[True] * 1e3:8.1f} ms, "
          "words identical to the host loops")
    print(f"  ripple-carry gate adder ({len(circ.levels())} levels):   {t_gate * 1e3:8.1f} ms")
    ck.close()


if __name__ == "__main__":
    main()
