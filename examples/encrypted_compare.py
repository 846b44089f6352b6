"""Comparing encrypted integers: x < y for 32 pairs of encrypted 16-bit integers, two ways.

Leveled: every bit of x and y is a TGSW sample, and x < y is a five-state automaton over the letters x_15, y_15, ..., x_0, y_0 evaluated
backwards as a CMUX network (tfhe_jl_amd.leveled.less_than_net: 32 levels of at most 4 nodes, 48 external products per pair, no blind
rotation; cmux_net_lookup).  What is left is an LWE sample under the gate key: the results are NANDed with fresh encryptions through
the ordinary gates and decrypted.  A 2^32-entry CMUX tree would compute the same function.
Gates: the same comparison with what the engine had before — the bits as LWE samples and the bitwise compare of examples/tutorial.py
(XNOR then MUX per bit, a 16-deep ripple: 48 blind rotations per pair) through Circuit.

    python examples/encrypted_compare.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe  # noqa: E402

BITS, PAIRS = 16, 32


def compare_circuit(pairs=PAIRS, nb_bits=BITS):
    """One circuit for all pairs: inputs = pairs x (x bits, then y bits), lowest bit first; outputs = pairs x (x < y)."""
    c = tfhe.Circuit()
    ins = [(c.inputs(nb_bits), c.inputs(nb_bits)) for _ in range(pairs)]
    outs = []
    for x, y in ins:
        gt = c.constant(False)                                          # tutorial.py: "y > x so far", decided by the highest differing bit
        for i in range(nb_bits):
            gt = c.mux(c.xnor(y[i], x[i]), gt, y[i])
        outs.append(gt)
    c.set_outputs(outs)
    return c


def to_bits(values, nb_bits=BITS):
    return ((np.asarray(values)[:, None] >> np.arange(nb_bits)[None, :]) & 1).astype(bool)


def main():
    rng = np.random.default_rng(2025)
    params = tfhe.tfhe_parameters_80()
    sk, ck = tfhe.make_key_pair(rng, params)
    N, k = params.tlwe_polynomial_degree, params.tlwe_mask_size
    x = rng.integers(0, 1 << BITS, PAIRS)
    y = rng.integers(0, 1 << BITS, PAIRS)
    y[:4] = [x[0], x[1] ^ 1, x[2] + 1 if x[2] + 1 < 1 << BITS else 0, 65535]       # equal, one bit apart, the successor, the extreme
    x[3] = 0
    bits = np.concatenate([to_bits(x), to_bits(y)], axis=1)                          # [PAIRS][2 BITS]: the network's variable order
    want = x < y

    # leveled: TGSW bits, the five end-state weights as trivial TLWE samples, one call
    net, table = tfhe.less_than_net(BITS)
    data = tfhe.table_to_tlwe(table, N, k)
    tgsw = tfhe.tgsw_encrypt_bits(rng, sk, bits.reshape(-1))
    tgsw = tgsw.reshape((PAIRS, 2 * BITS) + tgsw.shape[1:])
    tfhe.cmux_net_lookup(ck, data, net, tgsw)                            # warm-up: workspaces, selector upload
    t0 = time.perf_counter()
    less = tfhe.cmux_net_lookup(ck, data, net, tgsw)
    ms_leveled = (time.perf_counter() - t0) * 1e3
    eng = ck.engine(0)
    ms_kernels, kernel = eng.last_timing_ms(2), eng.last_kernel_name()
    z = rng.integers(0, 2, PAIRS).astype(bool)
    nand = tfhe.gate_nand(ck, less, tfhe.encrypt(rng, sk, z))
    assert np.array_equal(tfhe.decrypt(sk, less), want), "the network's comparison decrypts wrongly"
    assert np.array_equal(tfhe.decrypt(sk, nand), ~(want & z)), "NAND of the comparisons decrypts wrongly"

    # the same comparison as a gate circuit
    circuit = compare_circuit()
    inputs = tfhe.encrypt(rng, sk, bits.reshape(-1))
    circuit.run(ck, inputs)                                             # warm-up
    t0 = time.perf_counter()
    compared = circuit.run(ck, inputs)
    ms_gates = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(tfhe.decrypt(sk, compared), want), "the gate circuit's comparison decrypts wrongly"

    print(f"{PAIRS} pairs of encrypted {BITS}-bit integers, x < y: all answers correct, NAND of the answers correct")
    print(f"  leveled CMUX network : {ms_leveled:8.2f} ms  (kernels {ms_kernels:.2f} ms; {net.levels} levels, {PAIRS * net.products} external products, "
          f"selector upload included; {kernel})")
    print(f"  gate circuit         : {ms_gates:8.2f} ms  ({PAIRS * 2 * BITS} gates = {PAIRS * 3 * BITS} blind rotations in {len(circuit.levels())} levels through Circuit)")
    ck.close()
    return ms_leveled, ms_gates


if __name__ == "__main__":
    main()
