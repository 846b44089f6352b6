"""A jointly addressed ROM: two parties each hold four bits of an 8-bit address into a 256-entry public table, 32 lookups read jointly.

Leveled: each party uni-encrypts its four address bits (RGSW.UniEnc) under its own TLWE key; the server expands them against both public
keys on the GPU and folds the table — a row of trivial multi-key TLWE samples — with a depth-8 CMUX tree (255 multi-key external products
per address, no blind rotation; tfhe_jl_amd.leveled.mk_cmux_lookup).  What is left is table[address] as a multi-key LWE sample, which
the parties decrypt together and which every mk_gate accepts: the results are NANDed with fresh encryptions.
Gates: the same selection with what the engine had before — the address bits as multi-key LWE samples and a tree of 255 MUX gates per
address through Circuit (two multi-key blind rotations per MUX).  A multi-key MUX is noise-bound (two rotations summed), so some of ITS
answers can come out wrong; they are counted, not asserted.

    python examples/multikey_rom.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402

DEPTH, ADDRESSES, PARTIES = 8, 32, 2
OWNER = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)                 # party 0 holds the low four address bits, party 1 the high four


def setup(seed=2024):
    params = tfhe.mktfhe_parameters_2party
    rng = np.random.default_rng(seed)
    secret_keys = [tfhe.SecretKey(rng, params) for _ in range(PARTIES)]                          # on the two clients
    shared_key = tfhe.SharedKey(rng, params)                                                      # created by the server
    parts = [tfhe.CloudKeyPart(rng, sk, shared_key, keep_tlwe_key=True) for sk in secret_keys]   # on the clients
    return rng, params, secret_keys, shared_key, parts, tfhe.MKCloudKey(parts, expand="device")


def uni_encrypt_addresses(rng, params, shared_key, parts, abits, owner=OWNER):
    """Every party uni-encrypts the address bits it owns: six arrays [addresses][depth][l][N]."""
    A, D = abits.shape
    l, N = params.bs_decomp_length, params.tlwe_polynomial_degree
    uni = [np.zeros((A, D, l, N), np.int32) for _ in range(6)]
    for i, part in enumerate(parts):
        cols = np.nonzero(owner == i)[0]
        arrs = leveled.mk_tgsw_uni_encrypt_bits(rng, part.tlwe_key, shared_key, part.public_b, abits[:, cols].reshape(-1))
        for dst, a in zip(uni, arrs):
            dst[:, cols] = a.reshape(A, cols.size, l, N)
    return uni


def table_to_mk_tlwe(bits, N, parties):
    mu = np.zeros((len(bits), N), np.int32)
    mu[:, 0] = [leveled.encode_gate_bit(b) for b in bits]
    return leveled.mk_tlwe_trivial(mu, parties)


def mux_tree_circuit(bits, addresses=ADDRESSES, depth=DEPTH):
    """One circuit for all addresses: inputs = addresses x depth address bits, outputs = the selected entries."""
    c = tfhe.Circuit()
    addr = [c.inputs(depth) for _ in range(addresses)]
    consts = [c.constant(bool(b)) for b in bits]                       # shared by every address
    outs = []
    for a in addr:
        cur = consts
        for v in range(depth):
            cur = [c.mux(a[v], cur[2 * i + 1], cur[2 * i]) for i in range(len(cur) // 2)]
        outs.append(cur[0])
    c.set_outputs(outs)
    return c


def main():
    rng, params, sks, shared, parts, ck = setup()
    N = params.tlwe_polynomial_degree
    bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
    addr = rng.integers(0, 1 << DEPTH, ADDRESSES)
    abits = ((addr[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)

    # leveled: uni-encrypted address bits, trivial MK TLWE table, one call
    table = table_to_mk_tlwe(bits, N, PARTIES)
    uni = uni_encrypt_addresses(rng, params, shared, parts, abits)
    leveled.mk_cmux_lookup(ck, table, uni, OWNER)                       # warm-up: workspaces, expansion scratch
    t0 = time.perf_counter()
    looked_up = leveled.mk_cmux_lookup(ck, table, uni, OWNER)
    ms_leveled = (time.perf_counter() - t0) * 1e3
    ms_kernels = ck.engine(0).last_timing_ms(2)
    y = rng.integers(0, 2, ADDRESSES).astype(bool)
    nand = tfhe.mk_gate_nand(ck, looked_up, tfhe.mk_encrypt(rng, sks, y))
    assert np.array_equal(tfhe.mk_decrypt(sks, looked_up), bits[addr]), "leveled lookup decrypts wrongly"
    nand_ok = int(np.sum(tfhe.mk_decrypt(sks, nand) == ~(bits[addr] & y)))

    # the same selection as a tree of multi-key MUX gates
    circuit = mux_tree_circuit(bits)
    inputs = tfhe.mk_encrypt(rng, sks, abits.reshape(-1))
    circuit.run(ck, inputs)                                             # warm-up
    t0 = time.perf_counter()
    selected = circuit.run(ck, inputs)
    ms_gates = (time.perf_counter() - t0) * 1e3
    gates_ok = int(np.sum(tfhe.mk_decrypt(sks, selected) == bits[addr]))

    products = ADDRESSES * ((1 << DEPTH) - 1)
    print(f"{ADDRESSES} jointly encrypted {DEPTH}-bit addresses into a {1 << DEPTH}-entry table: all {ADDRESSES} leveled answers correct, "
          f"{nand_ok} of {ADDRESSES} NANDs of the answers correct")
    print(f"  leveled CMUX tree : {ms_leveled:8.2f} ms  (kernels {ms_kernels:.2f} ms; {products} multi-key external products, expansion of "
          f"{ADDRESSES * DEPTH} selectors included)")
    print(f"  MUX-gate tree     : {ms_gates:8.2f} ms  ({products} MUX gates = {2 * products} multi-key blind rotations through Circuit; "
          f"{gates_ok} of {ADDRESSES} answers correct)")
    ck.close()
    return ms_leveled, ms_gates


if __name__ == "__main__":
    main()
