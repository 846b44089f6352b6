"""The millionaires' problem: party 0 holds x, party 1 holds y, 32 pairs of 16-bit integers, and the server computes x < y on jointly
encrypted data without either party showing its integer, two ways.

Leveled: each party uni-encrypts the 16 bits of its own integer (RGSW.UniEnc) under its own TLWE key; the server expands them against
both public keys on the GPU and evaluates the five-state comparator automaton backwards as a CMUX network on trivial multi-key TLWE
samples (tfhe_jl_amd.leveled.less_than_net: 32 levels of at most 4 nodes, 48 multi-key external products per pair, no blind rotation;
mk_cmux_net_lookup).  What is left is x < y as a multi-key LWE sample, which the parties decrypt together and every mk_gate accepts.
Gates: the same comparison with what the engine had before — the bits as multi-key LWE samples and the bitwise compare of
examples/encrypted_compare.py (XNOR then MUX per bit, a 16-deep ripple: 48 multi-key blind rotations per pair) through Circuit under
the same MKCloudKey.  A multi-key MUX is noise-bound (two rotations summed), so some of ITS answers can come out wrong; the answers of
both ways are counted, not asserted.

    python examples/multikey_compare.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402
from encrypted_compare import BITS, PAIRS, compare_circuit, to_bits  # noqa: E402
from multikey_rom import PARTIES, setup, uni_encrypt_addresses  # noqa: E402

OWNER = np.array([0] * BITS + [1] * BITS, np.int32)                   # variables 0 ... 15: the bits of x, party 0; 16 ... 31: of y, party 1


def main():
    rng, params, sks, shared, parts, ck = setup(2026)
    N = params.tlwe_polynomial_degree
    x = rng.integers(0, 1 << BITS, PAIRS)
    y = rng.integers(0, 1 << BITS, PAIRS)
    y[:4] = [x[0], x[1] ^ 1, x[2] + 1 if x[2] + 1 < 1 << BITS else 0, 65535]       # equal, one bit apart, the successor, the extreme
    x[3] = 0
    bits = np.concatenate([to_bits(x), to_bits(y)], axis=1)                          # [PAIRS][2 BITS]: the network's variable order
    want = x < y

    # leveled: uni-encrypted bits, the five end-state weights as trivial multi-key TLWE samples, one call
    net, table = leveled.less_than_net(BITS)
    data = leveled.table_to_tlwe(table, N, k=PARTIES)
    uni = uni_encrypt_addresses(rng, params, shared, parts, bits, OWNER)
    leveled.mk_cmux_net_lookup(ck, data, net, uni, OWNER)                # warm-up: workspaces, expansion scratch
    t0 = time.perf_counter()
    less = leveled.mk_cmux_net_lookup(ck, data, net, uni, OWNER)
    ms_leveled = (time.perf_counter() - t0) * 1e3
    eng = ck.engine(0)
    ms_kernels, kernel = eng.last_timing_ms(2), eng.last_kernel_name()
    leveled_ok = int(np.sum(tfhe.mk_decrypt(sks, less) == want))

    # the same comparison as a circuit of multi-key gates under the same cloud key
    circuit = compare_circuit()
    inputs = tfhe.mk_encrypt(rng, sks, bits.reshape(-1))
    circuit.run(ck, inputs)                                             # warm-up
    t0 = time.perf_counter()
    compared = circuit.run(ck, inputs)
    ms_gates = (time.perf_counter() - t0) * 1e3
    gates_ok = int(np.sum(tfhe.mk_decrypt(sks, compared) == want))

    print(f"{PAIRS} pairs of jointly encrypted {BITS}-bit integers (x: party 0, y: party 1), x < y")
    print(f"  leveled CMUX network : {ms_leveled:8.2f} ms  ({leveled_ok} of {PAIRS} answers correct; kernels {ms_kernels:.2f} ms; {net.levels} levels, "
          f"{PAIRS * net.products} multi-key external products, expansion of {PAIRS * 2 * BITS} selectors included; {kernel})")
    print(f"  multi-key gate circuit: {ms_gates:8.2f} ms  ({gates_ok} of {PAIRS} answers correct; {PAIRS * 2 * BITS} gates = {PAIRS * 3 * BITS} multi-key blind "
          f"rotations in {len(circuit.levels())} levels through Circuit)")
    ck.close()
    return ms_leveled, ms_gates


if __name__ == "__main__":
    main()
