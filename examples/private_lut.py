"""A private table of 64 entries read at an address the server helps to compute: the high three address bits come from the client as TGSW
samples, the low digit (of Z_8) is computed ON THE SERVER from two encrypted digits by Circuit.linear / lut, and the table itself is
encrypted by the client — the server never sees an entry.

New: the table is 2^3 TLWE encryptions of test polynomials of 8 entries each (tlwe_encrypt of make_test_vector).  A CMUX tree over the
TGSW bits picks the row's test polynomial (7 external products, out_form 0), and the blind rotation of THAT accumulator by the computed
LWE digit reads the entry (two_stage_lookup; tfhe_cmux_tree_batch + tfhe_blind_rotate_batch): one rotation for the digit, one for the
lookup.

Today's way, for the timing: nothing turns an LWE digit into an address of the leveled half, and a test polynomial must be public.  So
the table is public, the client sends the high address bits as three gate-encrypted LWE bits, and a Circuit looks every bit of all eight
sub-tables up at the digit (24 rotations, gate-encoded outputs) and folds them by three trees of 7 MUX gates (two rotations each): 67
rotations per address, and the answer comes as three bits.  (Masking the eight looked-up values with a one-hot address by a bivariate
lookup in Z_16 needs 17 rotations, but its +-1/64 window does not hold a bootstrap's output noise at this parameter set: it was tried
and fails to decrypt.)

    python examples/private_lut.py [--tuned [--by-size]]

--tuned: the two-stage lookup is also run with its rotation on the gates' own kernel and key (two_stage_lookup(..., tuned=True);
tfhe_bootstrap_acc_batch: the accumulator stays in LDS, the bootstrapping key is not loaded a second time as selectors), the same program
both ways: equal words, both times.
--by-size (with --tuned): the engine's option acc_dispatch is set to 1 for that run, so the rotation of these 32 rows takes the kernel a
gate batch of 32 rotations takes (every transform split over two waves) instead of one wave per row.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tfhe_jl_amd as tfhe  # noqa: E402

P, DEPTH, ADDRESSES = 8, 3, 32


def digit_of(m):
    """The low address digit the server computes from the sum m = a + b of the two encrypted digits."""
    return (5 * m + 3) % P


def digit_circuit(q):
    """(a, b) in Z_4 x Z_4, each encrypted as a message of Z_8 -> digit_of(a + b) in Z_q: a + b <= 6 stays inside Z_8."""
    c = tfhe.Circuit()
    a, b = c.inputs(2)
    s = c.linear([a, b], const=-(1 << 27))                              # (2a+1)/32 + (2b+1)/32 - 1/32 = (2(a+b)+1)/32
    c.set_outputs([c.lut(digit_of, [s], P, q)])
    return c


def todays_circuit(table, N):
    """The same selection with a public table and the high address as three gate-encrypted bits: per output bit, eight lookups at the
    digit (gate-encoded results) and a tree of MUX gates."""
    c = tfhe.Circuit()
    a, b, *hb = c.inputs(2 + DEPTH)
    s = c.linear([a, b], const=-(1 << 27))
    low = c.lut(digit_of, [s], P)
    outs = []
    for t in range(P.bit_length() - 1):
        cur = [c.lut(tfhe.make_gate_test_vector(lambda m, h=h, t=t: (table[P * h + m] >> t) & 1, P, N), [low], P) for h in range(1 << DEPTH)]
        for v in range(DEPTH):
            cur = [c.mux(hb[v], cur[2 * i + 1], cur[2 * i]) for i in range(len(cur) // 2)]
        outs.append(cur[0])
    c.set_outputs(outs)
    return c


def timed(call):
    call()                                                              # warm-up: workspaces, selector upload
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main(tuned=False, by_size=False):
    rng = np.random.default_rng(2026)
    params = tfhe.tfhe_parameters_80()
    sk, ck = tfhe.make_key_pair(rng, params)
    N = params.tlwe_polynomial_degree
    table = [int(v) for v in rng.integers(0, P, P << DEPTH)]
    high = rng.integers(0, 1 << DEPTH, ADDRESSES)
    da, db = rng.integers(0, 4, ADDRESSES), rng.integers(0, 4, ADDRESSES)
    want = np.array([table[P * h + digit_of(a + b)] for h, a, b in zip(high, da, db)])

    # the client's side: the encrypted table, the high bits as TGSW, the two digits as LWE
    polys = np.stack([tfhe.make_test_vector(lambda m, h=h: table[P * h + m], P, N) for h in range(1 << DEPTH)])
    enc_table = tfhe.tlwe_encrypt(rng, sk, polys)
    hbits = ((high[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)
    tgsw = tfhe.tgsw_encrypt_bits(rng, sk, hbits.reshape(-1))
    tgsw = tgsw.reshape((ADDRESSES, DEPTH) + tgsw.shape[1:])
    digits = np.stack([tfhe.lut_encrypt(rng, sk, da, P).data, tfhe.lut_encrypt(rng, sk, db, P).data], axis=1)       # [B][2][n+1]

    def new_way():
        low = digit_circuit(P).run_batch(ck, digits)[:, 0]
        return tfhe.two_stage_lookup(ck, enc_table, tgsw, low, P)

    out_new, ms_new = timed(new_way)
    got_new = tfhe.lut_decrypt(sk, out_new, P)
    assert np.array_equal(got_new, want), "the two-stage lookup decrypts wrongly"
    ms_tuned = None
    if tuned:
        def tuned_way():
            low = digit_circuit(P).run_batch(ck, digits)[:, 0]
            return tfhe.two_stage_lookup(ck, enc_table, tgsw, low, P, tuned=True)

        eng = ck.engine(0)
        eng.set_option("acc_dispatch", 1 if by_size else 0)
        try:
            out_tuned, ms_tuned = timed(tuned_way)
            tuned_kernel = eng.last_kernel_name()
        finally:
            eng.set_option("acc_dispatch", 0)
        assert np.array_equal(out_tuned.data, out_new.data), "the tuned rotation's words differ"

    hlwe = tfhe.encrypt(rng, sk, hbits.reshape(-1)).data.reshape(ADDRESSES, DEPTH, -1)                                 # [B][3][n+1]
    old_inputs = np.concatenate([digits, hlwe], axis=1)
    old = todays_circuit(table, N)
    out_old, ms_old = timed(lambda: old.run_batch(ck, old_inputs))
    bits_old = np.stack([tfhe.decrypt(sk, np.ascontiguousarray(out_old[:, t])) for t in range(out_old.shape[1])], axis=1)
    got_old = (bits_old.astype(np.int64) << np.arange(bits_old.shape[1])[None, :]).sum(axis=1)
    assert np.array_equal(got_old, want), "today's circuit decrypts wrongly"

    print(f"{ADDRESSES} addresses into a {P << DEPTH}-entry table, all answers correct both ways")
    print(f"  private table, TGSW high bits, computed LWE digit : {ms_new:8.2f} ms  (2 rotations + {(1 << DEPTH) - 1} external products per address)")
    if tuned:
        print(f"  the same with the rotation on the gates' kernel   : {ms_tuned:8.2f} ms  (equal words; {tuned_kernel})")
    print(f"  public table, LWE high bits, lookups and MUX gates: {ms_old:8.2f} ms  ({1 + 3 * ((1 << DEPTH) + 2 * ((1 << DEPTH) - 1))} rotations per address)")
    ck.close()
    return ms_new, ms_old


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuned", action="store_true", help="also run the lookup with its rotation on the gates' kernel (tfhe_bootstrap_acc_batch)")
    ap.add_argument("--by-size", action="store_true", help="with --tuned: option acc_dispatch 1, the rotation's kernel chosen by batch size as a gate batch's is")
    args = ap.parse_args()
    main(args.tuned, args.by_size)
