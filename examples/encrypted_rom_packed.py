"""The ROM of examples/encrypted_rom.py read through a packed table: 256 public bits at 32 encrypted 8-bit addresses, two ways, and then
a 2^16-entry table that the CMUX tree cannot hold.

Tree: the table as 256 trivial TLWE samples, one bit on coefficient 0 of each, folded by a depth-8 CMUX tree: 255 external products per
address (tfhe_jl_amd.leveled.cmux_lookup).
Packed: the same 256 bits on the first 256 coefficients of ONE sample (pack_table_to_tlwe); CMUX(C_b; acc, X^(-2^b) acc) for the eight
address bits rotates the wanted coefficient to position 0, where the extraction reads it: 8 external products per address
(packed_lookup; tfhe_rot_net_batch).  Both leave table[address] as an LWE sample under the gate key; the results are NANDed with fresh
encryptions through the ordinary gates and decrypted.
The 2^16-entry table is 64 samples: a depth-6 tree picks the sample by the high address bits (63 products), ten rotation levels pick the
coefficient (10 products).

    python examples/encrypted_rom_packed.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe  # noqa: E402

DEPTH, BIG_DEPTH, ADDRESSES = 8, 16, 32


def encrypt_addresses(rng, sk, addr, depth):
    abits = ((addr[:, None] >> np.arange(depth)[None, :]) & 1).astype(bool)
    tgsw = tfhe.tgsw_encrypt_bits(rng, sk, abits.reshape(-1))
    return tgsw.reshape((len(addr), depth) + tgsw.shape[1:])


def timed(call):
    call()                                                              # warm-up: workspaces, selector upload
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    rng = np.random.default_rng(2025)
    params = tfhe.tfhe_parameters_80()
    sk, ck = tfhe.make_key_pair(rng, params)
    eng = ck.engine(0)
    N, k = params.tlwe_polynomial_degree, params.tlwe_mask_size
    bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
    addr = rng.integers(0, 1 << DEPTH, ADDRESSES)
    tgsw = encrypt_addresses(rng, sk, addr, DEPTH)

    tree_out, ms_tree = timed(lambda: tfhe.cmux_lookup(ck, tfhe.table_to_tlwe(bits, N, k), tgsw))
    ms_tree_kernels = eng.last_timing_ms(2)
    packed_out, ms_packed = timed(lambda: tfhe.packed_lookup(ck, bits, tgsw))
    ms_packed_kernels = eng.last_timing_ms(2)
    y = rng.integers(0, 2, ADDRESSES).astype(bool)
    nand = tfhe.gate_nand(ck, packed_out, tfhe.encrypt(rng, sk, y))
    assert np.array_equal(tfhe.decrypt(sk, tree_out), bits[addr]), "CMUX-tree lookup decrypts wrongly"
    assert np.array_equal(tfhe.decrypt(sk, packed_out), bits[addr]), "packed lookup decrypts wrongly"
    assert np.array_equal(tfhe.decrypt(sk, nand), ~(bits[addr] & y)), "NAND of the looked-up bits decrypts wrongly"

    big = rng.integers(0, 2, 1 << BIG_DEPTH).astype(bool)
    big_addr = rng.integers(0, 1 << BIG_DEPTH, ADDRESSES)
    big_tgsw = encrypt_addresses(rng, sk, big_addr, BIG_DEPTH)
    big_table = tfhe.pack_table_to_tlwe(big, N, k)                      # packed once: [64][k+1][N]
    big_out, ms_big = timed(lambda: tfhe.packed_lookup(ck, big_table, big_tgsw))
    ms_big_kernels = eng.last_timing_ms(2)
    assert np.array_equal(tfhe.decrypt(sk, big_out), big[big_addr]), "2^16-entry packed lookup decrypts wrongly"

    tree_p, packed_p, big_p = (1 << DEPTH) - 1, tfhe.packed_lookup_net(DEPTH, N).products, tfhe.packed_lookup_net(BIG_DEPTH, N).products
    print(f"{ADDRESSES} encrypted addresses, all answers correct, NAND of the answers correct")
    print(f"  {1 << DEPTH}-entry table, CMUX tree     : {ms_tree:8.2f} ms  (kernels {ms_tree_kernels:.2f} ms; {tree_p} external products per address)")
    print(f"  {1 << DEPTH}-entry table, packed        : {ms_packed:8.2f} ms  (kernels {ms_packed_kernels:.2f} ms; {packed_p} external products per address)")
    print(f"  {1 << BIG_DEPTH}-entry table, packed      : {ms_big:8.2f} ms  (kernels {ms_big_kernels:.2f} ms; {big_p} external products per address, "
          f"{big_table.shape[0]} table samples)")
    ck.close()
    return ms_tree, ms_packed, ms_big


if __name__ == "__main__":
    main()
