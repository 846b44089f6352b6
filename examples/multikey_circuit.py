#!/usr/bin/env python3
"""A sealed comparison of two parties' numbers: the tutorial's 16-bit encrypted minimum under a 2-party multi-key cloud key.

Two parties each hold a 16-bit number and encrypt it under their joint key; the server runs the encrypted-minimum circuit of
examples/tutorial.py (the reference's ripple and the log-depth form) level by level on the GPU's multi-key wire table
(tfhe_mk_gates_level); the parties decrypt the result together.  For comparison the same computation is then written with
mk_gate_nand only (the one multi-key gate the reference exports): XNOR and MUX become several NANDs over more levels, and
every level is a host round trip.

    python examples/multikey_circuit.py

Keys and encryptions use fixed seeds.  Multi-key decryption is noise-bound (about 0.2 % per gate at the 2-party
set, more for MUX, whose two blind rotations are summed), so with other seeds a result bit can come out wrong."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfhe_jl_amd as tfhe
from tutorial import bits_to_int, encrypted_minimum_circuit, int_to_bits


def setup(seed=2024):
    params = tfhe.mktfhe_parameters_2party
    rng = np.random.default_rng(seed)
    secret_keys = [tfhe.SecretKey(rng, params) for _ in range(2)]              # on the two clients
    shared_key = tfhe.SharedKey(rng, params)                                   # created by the server
    parts = [tfhe.CloudKeyPart(rng, sk, shared_key) for sk in secret_keys]     # on the clients
    return secret_keys, tfhe.MKCloudKey(parts, expand="device")               # on the server, expanded on its GPU


def nand_only(circuit):
    """The circuit's gates rewritten as NANDs: (levels of (a, b, out) wire triples, number of wires, output wires, constant wires)."""
    wires = circuit.num_wires
    gates, level, consts = [], {}, []

    def nand(a, b):
        nonlocal wires
        level[wires] = 1 + max(level.get(a, 0), level.get(b, 0))
        gates.append((a, b, wires))
        wires += 1
        return wires - 1

    alias = {}
    for ops, a, b, c, out in circuit.level_arrays():
        for op, x, y, z, o in zip(ops, a, b, c, out):
            x, y, z = alias.get(x, x), alias.get(y, y), alias.get(z, z)
            name = next(k for k, v in tfhe.OPCODES.items() if v == op)
            if name == "CONST0" or name == "CONST1":
                consts.append((int(o), name == "CONST1"))
                r = int(o)
            elif name == "AND":
                t = nand(x, y)
                r = nand(t, t)
            elif name == "ANDNY":                                              # (not x) and y
                t = nand(nand(x, x), y)
                r = nand(t, t)
            elif name == "XNOR":                                               # (x and y) or (not x and not y)
                r = nand(nand(x, y), nand(nand(x, x), nand(y, y)))
            elif name == "MUX":                                                # x ? y : z
                r = nand(nand(x, y), nand(nand(x, x), z))
            else:
                raise ValueError(f"no NAND form for {name} here")
            alias[int(o)] = r
    depth = max(level.values())
    levels = [[g for g in gates if level[g[2]] == d] for d in range(1, depth + 1)]
    return levels, wires, [alias.get(w, w) for w in circuit.outputs], consts


def run_nand_only(ck, levels, num_wires, outputs, consts, inputs):
    table = np.zeros((num_wires, inputs.shape[1]), np.int32)
    table[:inputs.shape[0]] = inputs
    for w, value in consts:
        table[w] = tfhe.mk_gate_constant(ck, value)
    for lv in levels:                                                          # one mk_gate_nand batch call per level
        a, b, out = (np.array(v) for v in zip(*lv))
        table[out] = tfhe.mk_gate_nand(ck, table[a], table[b])
    return table[outputs]


if __name__ == "__main__":
    secret_keys, cloud_key = setup()
    # party 1's number, then party 2's, encrypted under the joint key
    inputs = tfhe.mk_encrypt(np.random.default_rng(1), secret_keys, int_to_bits(2017) + int_to_bits(42))
    cloud_key.engine(0)                                                        # key expansion and upload, not timed
    for log_depth in (False, True):
        circuit = encrypted_minimum_circuit(16, log_depth=log_depth)
        circuit.run(cloud_key, inputs)                                         # warm-up
        t0 = time.perf_counter()
        answer = circuit.run(cloud_key, inputs)
        ms = 1e3 * (time.perf_counter() - t0)
        trivial = {tfhe.OPCODES[k] for k in ("NOT", "COPY", "CONST0", "CONST1")}
        rotations = sum(2 if op == tfhe.OPCODES["MUX"] else 0 if op in trivial else 1 for ops, *_ in circuit.level_arrays() for op in ops)
        print(f"{'log-depth' if log_depth else 'ripple'} form: {sum(len(l) for l in circuit.levels())} gates, {rotations} blind rotations, "
              f"{len(circuit.levels())} levels: {ms:.1f} ms")
        print(f"Answer: {bits_to_int(tfhe.mk_decrypt(secret_keys, answer))}")
        levels, num_wires, outputs, consts = nand_only(circuit)
        run_nand_only(cloud_key, levels, num_wires, outputs, consts, inputs)
        t0 = time.perf_counter()
        answer = run_nand_only(cloud_key, levels, num_wires, outputs, consts, inputs)
        ms = 1e3 * (time.perf_counter() - t0)
        value = bits_to_int(tfhe.mk_decrypt(secret_keys, answer))
        print(f"  the same with mk_gate_nand only: {sum(len(l) for l in levels)} NANDs, {len(levels)} levels: {ms:.1f} ms, "
              f"answer {value}{'' if value == min(2017, 42) else ' (noise failure)'}")
