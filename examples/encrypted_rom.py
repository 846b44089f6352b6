"""An encrypted-index ROM: a 256-entry public table of bits read at 32 encrypted 8-bit addresses, two ways.

Leveled: each address bit is a TGSW sample, the table a row of trivial TLWE samples, and a depth-8 CMUX tree (255 external products per
address, no blind rotation; tfhe_jl_amd.leveled.cmux_lookup) leaves table[address] as an LWE sample under the gate key.  The results
are NANDed with fresh encryptions through the ordinary gates and decrypted.
Gates: the same selection with what the engine had before — the address bits as LWE samples, the table as CONST gates, and a tree of
255 MUX gates per address through Circuit (two blind rotations per MUX).

    python examples/encrypted_rom.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe  # noqa: E402

DEPTH, ADDRESSES = 8, 32


def mux_tree_circuit(bits):
    """One circuit for all addresses: inputs = ADDRESSES x DEPTH address bits, outputs = ADDRESSES selected entries."""
    c = tfhe.Circuit()
    addr = [c.inputs(DEPTH) for _ in range(ADDRESSES)]
    consts = [c.constant(bool(b)) for b in bits]                       # shared by every address
    outs = []
    for a in addr:
        cur = consts
        for v in range(DEPTH):
            cur = [c.mux(a[v], cur[2 * i + 1], cur[2 * i]) for i in range(len(cur) // 2)]
        outs.append(cur[0])
    c.set_outputs(outs)
    return c


def main():
    rng = np.random.default_rng(2024)
    params = tfhe.tfhe_parameters_80()
    sk, ck = tfhe.make_key_pair(rng, params)
    N, k = params.tlwe_polynomial_degree, params.tlwe_mask_size
    bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
    addr = rng.integers(0, 1 << DEPTH, ADDRESSES)
    abits = ((addr[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)

    # leveled: TGSW address bits, trivial TLWE table, one call
    table = tfhe.table_to_tlwe(bits, N, k)
    tgsw = tfhe.tgsw_encrypt_bits(rng, sk, abits.reshape(-1))
    tgsw = tgsw.reshape((ADDRESSES, DEPTH) + tgsw.shape[1:])
    tfhe.cmux_lookup(ck, table, tgsw)                                   # warm-up: workspaces, selector upload
    t0 = time.perf_counter()
    looked_up = tfhe.cmux_lookup(ck, table, tgsw)
    ms_leveled = (time.perf_counter() - t0) * 1e3
    eng = ck.engine(0)
    ms_kernels = eng.last_timing_ms(2)
    y = rng.integers(0, 2, ADDRESSES).astype(bool)
    nand = tfhe.gate_nand(ck, looked_up, tfhe.encrypt(rng, sk, y))
    assert np.array_equal(tfhe.decrypt(sk, looked_up), bits[addr]), "leveled lookup decrypts wrongly"
    assert np.array_equal(tfhe.decrypt(sk, nand), ~(bits[addr] & y)), "NAND of the looked-up bits decrypts wrongly"

    # the same selection as a tree of MUX gates
    circuit = mux_tree_circuit(bits)
    inputs = tfhe.encrypt(rng, sk, abits.reshape(-1))
    circuit.run(ck, inputs)                                             # warm-up
    t0 = time.perf_counter()
    selected = circuit.run(ck, inputs)
    ms_gates = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(tfhe.decrypt(sk, selected), bits[addr]), "MUX-gate tree decrypts wrongly"

    products = ADDRESSES * ((1 << DEPTH) - 1)
    print(f"{ADDRESSES} encrypted {DEPTH}-bit addresses into a {1 << DEPTH}-entry table: all answers correct, NAND of the answers correct")
    print(f"  leveled CMUX tree : {ms_leveled:8.2f} ms  (kernels {ms_kernels:.2f} ms; {products} external products, selector upload included)")
    print(f"  MUX-gate tree     : {ms_gates:8.2f} ms  ({products} MUX gates = {2 * products} blind rotations through Circuit)")
    ck.close()
    return ms_leveled, ms_gates


if __name__ == "__main__":
    main()
