#!/usr/bin/env python3
"""A 2-party 8-bit ripple-carry adder under a multi-key cloud key, with the carry as one lookup, against the same adder from gates.

Both adders run as a Circuit on the multi-key wire table (Circuit.run_batch under an MKCloudKey).  Per bit the sum is
XOR(XOR(a, b), c) in both.  The gate adder takes the carry as OR(AND(a, b), AND(c, XOR(a, b))): three more rotations and two more
levels on the carry chain.  The LUT adder takes it as the 3-input majority in ONE rotation: the three gate-encoded bits (+-1/8) add
up to -3/8, -1/8, 1/8 or 3/8, whose sign is the majority, so a programmable bootstrap with the constant table (1/8, ..., 1/8) on the
sum returns the carry as a gate bit (tfhe_mk_lut_level).  Its margin is 1/8, as a gate's, but from a sum of three fresh bootstrap
outputs.  Prints the time of each adder and the fraction of sums that decrypt correctly.

    python examples/multikey_lut.py [--instances M]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe

BITS = 8
P8 = 1 << 29          # encode_message(1, 8): a gate-encoded 1


def adder(lut_carry):
    """Inputs a_0 .. a_7, b_0 .. b_7 (least significant first), a constant-0 carry in; outputs the 8 sum bits and the carry out."""
    c = tfhe.Circuit()
    a, b = c.inputs(BITS), c.inputs(BITS)
    carry = c.constant(False)
    sums = []
    for i in range(BITS):
        t = c.xor(a[i], b[i])
        sums.append(c.xor(t, carry))
        if lut_carry:
            carry = c.lut(np.full(1024, P8, np.int32), [a[i], b[i], carry], 2)      # majority: the sign of the sum
        else:
            carry = c.or_(c.and_(a[i], b[i]), c.and_(carry, t))
    c.set_outputs(sums + [carry])
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=64)
    M = ap.parse_args().instances
    p = tfhe.mktfhe_parameters_2party
    rng = np.random.default_rng(2024)
    sks = [tfhe.SecretKey(rng, p) for _ in range(2)]
    shared = tfhe.SharedKey(rng, p)
    ck = tfhe.MKCloudKey([tfhe.CloudKeyPart(rng, sk, shared) for sk in sks])
    x, y = rng.integers(0, 2**BITS, M), rng.integers(0, 2**BITS, M)
    bits = np.concatenate([(x[:, None] >> np.arange(BITS)) & 1, (y[:, None] >> np.arange(BITS)) & 1], axis=1).astype(bool)   # [M][16]
    inputs = tfhe.mk_encrypt(rng, sks, bits.reshape(-1)).reshape(M, 2 * BITS, -1)
    want = x + y
    for name, lut_carry in (("gates", False), ("LUT carry", True)):
        c = adder(lut_carry)
        c.run_batch(ck, inputs[:1])                                   # warm-up: tables, wire table, kernels
        t0 = time.perf_counter()
        out = c.run_batch(ck, inputs)
        ms = (time.perf_counter() - t0) * 1e3
        dec = tfhe.mk_decrypt(sks, out.reshape(-1, out.shape[2])).reshape(M, BITS + 1)
        got = (dec.astype(np.int64) << np.arange(BITS + 1)).sum(axis=1)
        print(f"{name:>10}: {M} additions of {BITS} bits in {ms:.1f} ms ({len(c.levels())} levels), "
              f"{(got == want).mean() * 100:.1f} % of the sums decrypt correctly")
    ck.close()


if __name__ == "__main__":
    main()
