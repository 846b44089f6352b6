"""examples/private_lut.py's program as ONE Circuit: gates and lookups compute the low address digit, a CMUX tree over the client's TGSW
address bits picks the private test polynomial, the blind rotation reads the digit from the wires, and gates consume the answer — with
nothing crossing PCIe between the circuit's inputs and its outputs.

The two device-resident tables carry it: the encrypted table goes into the TLWE table as the circuit's TLWE inputs, the tree
(Circuit.rot_net with tree_net, out="tlwe") leaves the picked test polynomial in a slot, Circuit.blind_rotate rotates that slot by the
digit's wire and keyswitches the answer into a wire, and LUT and XOR nodes read it from there (here: its three bits and their parity).
The selector set is loaded once — the bootstrapping key's n selectors, three address-bit selectors behind them — and every request swaps
only its three address selectors (Engine.tgsw_update).

The host path (two_stage_lookup around a digit circuit: three downloads and three uploads per request, the whole key re-uploaded as
selectors) computes the same words; the example checks the circuit's answer against it word for word and both by decryption.

    python examples/private_lut_circuit.py [--tuned]

--tuned: the circuit is also run with its rotation node on the gates' own key and kernels (Circuit.blind_rotate(..., tuned=True):
tfhe_bootstrap_acc_level) and the engine's option acc_dispatch at 1, so that the one row of a request takes the kernel a single gate
takes; the selector set then holds the three address selectors alone.  Equal words, both times printed.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402

P, DEPTH, ADDRESSES = 8, 3, 32


def digit_of(m):
    """The low address digit the server computes from the sum m = a + b of the two encrypted digits."""
    return (5 * m + 3) % P


def digit_circuit():
    """(a, b) in Z_4 x Z_4, each encrypted as a message of Z_8 -> digit_of(a + b) in Z_8 (examples/private_lut.py's)."""
    c = tfhe.Circuit()
    a, b = c.inputs(2)
    s = c.linear([a, b], const=-(1 << 27))                              # (2a+1)/32 + (2b+1)/32 - 1/32 = (2(a+b)+1)/32
    c.set_outputs([c.lut(digit_of, [s], P)])
    return c


def lookup_circuit(n, N, tuned=False):
    """The whole request: outputs (the table entry as a message of Z_8, the parity of its three bits as a gate bit).  `n` is where the
    three address selectors sit in the loaded set; tuned: the rotation on the gates' key, which reads no selector."""
    c = tfhe.Circuit()
    a, b = c.inputs(2)
    table = c.tlwe_inputs(1 << DEPTH)
    s = c.linear([a, b], const=-(1 << 27))
    low = c.lut(digit_of, [s], P)                                       # the digit, computed from the wires
    picked = c.rot_net(leveled.tree_net(DEPTH), table, [n + v for v in range(DEPTH)], out="tlwe")[0]
    answer = c.blind_rotate(picked, [low], tuned=tuned)                 # steps 0 ... n-1 on the key's selectors (sel None), or on the gates' key
    bits = [c.lut(tfhe.make_gate_test_vector(lambda m, t=t: (m >> t) & 1, P, N), [answer], P) for t in range(3)]
    c.set_outputs([answer, c.xor(c.xor(bits[0], bits[1]), bits[2])])
    return c


def request_inputs(rng, sk, table, high, da, db):
    """The client's side: the encrypted table, every request's high bits as TGSW samples, its two digits as LWE samples."""
    params = sk.params
    N = params.tlwe_polynomial_degree
    polys = np.stack([tfhe.make_test_vector(lambda m, h=h: table[P * h + m], P, N) for h in range(1 << DEPTH)])
    enc_table = tfhe.tlwe_encrypt(rng, sk, polys)
    hbits = ((np.asarray(high)[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)
    tgsw = tfhe.tgsw_encrypt_bits(rng, sk, hbits.reshape(-1))
    tgsw = tgsw.reshape((len(high), DEPTH) + tgsw.shape[1:])
    digits = np.stack([tfhe.lut_encrypt(rng, sk, da, P).data, tfhe.lut_encrypt(rng, sk, db, P).data], axis=1)       # [B][2][n+1]
    return enc_table, tgsw, digits


def host_path(ck, enc_table, tgsw, digits):
    """The digit circuit, then two_stage_lookup: the wires come down and go up again between every stage."""
    low = digit_circuit().run_batch(ck, digits)[:, 0]
    return tfhe.two_stage_lookup(ck, enc_table, tgsw, low, P).data


def circuit_path(ck, enc_table, tgsw, digits, tuned=False):
    """One Circuit.run per request; the key's selectors are loaded once, the request's three address selectors swapped behind them.
    tuned: the rotation node on the gates' key (option acc_dispatch 1 while it runs), the selector set the address selectors alone."""
    first = 0 if tuned else ck.params.lwe_size
    eng = ck.engine(0)
    eng.tgsw_load(tgsw[0] if tuned else np.concatenate([leveled.bootstrap_key_selectors(ck), tgsw[0]]))
    circuit = lookup_circuit(first, ck.params.tlwe_polynomial_degree, tuned)
    out = []
    eng.set_option("acc_dispatch", 1 if tuned else 0)
    try:
        for g in range(digits.shape[0]):
            if g:
                eng.tgsw_update(first, tgsw[g])
            out.append(circuit.run(ck, digits[g], tlwe_inputs=enc_table).data)
    finally:
        eng.set_option("acc_dispatch", 0)
    return np.stack(out)                                                 # [B][2][n+1]: the answer, the parity bit


def timed(call):
    call()                                                              # warm-up: workspaces, tables
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def lookup_both_ways(rng, sk, ck, addresses, tuned=False):
    """`addresses` random requests through both paths; returns (circuit ms, host ms) after checking the words and the decryptions —
    and, with tuned, (circuit ms, host ms, tuned circuit ms) after checking the tuned circuit's words against the circuit's."""
    table = [int(v) for v in rng.integers(0, P, P << DEPTH)]
    high = rng.integers(0, 1 << DEPTH, addresses)
    da, db = rng.integers(0, 4, addresses), rng.integers(0, 4, addresses)
    want = np.array([table[P * h + digit_of(a + b)] for h, a, b in zip(high, da, db)])
    enc_table, tgsw, digits = request_inputs(rng, sk, table, high, da, db)
    out_host, ms_host = timed(lambda: host_path(ck, enc_table, tgsw, digits))
    out_circ, ms_circ = timed(lambda: circuit_path(ck, enc_table, tgsw, digits))
    assert np.array_equal(out_circ[:, 0], out_host), "the circuit's answer differs from the host path's words"
    got = tfhe.lut_decrypt(sk, tfhe.LweSampleArray(np.ascontiguousarray(out_circ[:, 0])), P)
    assert np.array_equal(got, want), "the circuit's lookup decrypts wrongly"
    parity = tfhe.decrypt(sk, tfhe.LweSampleArray(np.ascontiguousarray(out_circ[:, 1])))
    assert np.array_equal(parity, [bin(int(v)).count("1") & 1 == 1 for v in want]), "the gates on the answer decrypt wrongly"
    if tuned:
        out_tuned, ms_tuned = timed(lambda: circuit_path(ck, enc_table, tgsw, digits, tuned=True))
        assert np.array_equal(out_tuned, out_circ), "the tuned rotation node's words differ"
        return ms_circ, ms_host, ms_tuned
    return ms_circ, ms_host


def main(tuned=False):
    rng = np.random.default_rng(2026)
    params = tfhe.tfhe_parameters_80()
    sk, ck = tfhe.make_key_pair(rng, params)
    ms_circ, ms_host, *ms_tuned = lookup_both_ways(rng, sk, ck, ADDRESSES, tuned)
    print(f"{ADDRESSES} addresses into a private {P << DEPTH}-entry table, the same words both ways, all answers correct")
    print(f"  one Circuit per request on the device-resident tables : {ms_circ:8.2f} ms")
    if tuned:
        print(f"  the same, its rotation node on the gates' key (tuned)  : {ms_tuned[0]:8.2f} ms  (equal words)")
    print(f"  digit circuit, then two_stage_lookup through the host : {ms_host:8.2f} ms  (all requests in one batch)")
    ck.close()
    return ms_circ, ms_host


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuned", action="store_true", help="also run the circuit with its rotation node on the gates' key (tfhe_bootstrap_acc_level, acc_dispatch 1)")
    main(ap.parse_args().tuned)
