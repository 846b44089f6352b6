"""One party's private table on jointly encrypted data: two parties, a 64-entry bit table that party 0 owns and the server never
sees, read at an address whose high four bits the two parties hold (two each) and whose low digit (of Z_4) is computed ON THE SERVER.

New: the table is 2^4 multi-key TLWE encryptions of gate-encoded test polynomials of 4 entries each (mk_tlwe_encrypt of
make_gate_test_vector).  The high address bits come uni-encrypted by their owners and are expanded on the device; the low digit is
digit_of(m) of an encrypted digit m, computed by mk_bootstrap_tv.  A multi-key CMUX tree over the address bits picks the row's test
polynomial (15 multi-key external products, out_form 0), and the multi-key blind rotation of THAT accumulator by the computed digit
reads the entry (mk_two_stage_lookup; tfhe_mk_cmux_tree_batch + tfhe_mk_blind_rotate_batch): one rotation for the digit, one for the
lookup.  The answer is a multi-key LWE sample, decrypted by the parties together (mk_decrypt) and an operand of every mk_gate.

The way without it, for comparison: a test polynomial must be public and nothing turns an LWE digit into an address of the leveled
half.  So the table is public, the high address bits come as gate-encrypted multi-key LWE bits, every one of the sixteen sub-tables is
looked up at the digit (16 rotations) and a tree of 15 MUX gates (two rotations each) folds them: 47 rotations per address.

Every multi-key rotation at this parameter set adds noise with a standard deviation near 0.06 of the torus to a +-1/8 window (DESIGN
4.11), so neither way decrypts every answer; the number that does is printed for both.

    python examples/multikey_private_lut.py [--tuned]

--tuned: the two-stage lookup is also run with its rotation on the multi-key gates' own kernel and key (mk_two_stage_lookup(...,
tuned=True); tfhe_mk_bootstrap_acc_batch): the bootstrapping key is not expanded and loaded a second time as P n selectors, the selector
set holds the address bits alone.  The words are the same; the time and the kernel are printed.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import lut  # noqa: E402
import multikey_rom as rom  # noqa: E402

P, DEPTH, ADDRESSES = 4, 4, 32
OWNER = np.array([0, 1, 0, 1], np.int32)                                # high address bit v is held by party v mod 2


def digit_of(m):
    """The low address digit the server computes from the encrypted digit m."""
    return (3 * m + 1) % P


def timed(call):
    call()                                                              # warm-up: workspaces, expansion scratch
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main(tuned=False):
    rng, params, sks, shared, parts, ck = rom.setup(2027)
    eng = ck.engine(0)
    N = params.tlwe_polynomial_degree
    table = rng.integers(0, 2, P << DEPTH).astype(bool)
    high = rng.integers(0, 1 << DEPTH, ADDRESSES)
    m = rng.integers(0, P, ADDRESSES)
    want = np.array([table[P * h + digit_of(v)] for h, v in zip(high, m)])

    # the parties' side: party 0's table under both TLWE keys, the high bits uni-encrypted by their owners, the digit as a multi-key sample
    polys = np.stack([tfhe.make_gate_test_vector(lambda v, h=h: table[P * h + v], P, N) for h in range(1 << DEPTH)])
    enc_table = tfhe.mk_tlwe_encrypt(rng, [part.tlwe_key for part in parts], params.bs_noise_stddev, polys)
    hbits = ((high[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)
    uni = rom.uni_encrypt_addresses(rng, params, shared, parts, hbits, OWNER)
    digits = lut.mk_lut_encrypt(rng, sks, m, P)
    digit_tv = tfhe.make_test_vector(digit_of, P, N)[None]

    def new_way():
        low = eng.mk_bootstrap_tv(digit_tv, digits)
        return tfhe.mk_two_stage_lookup(ck, enc_table, uni, OWNER, low, P)

    out_new, ms_new = timed(new_way)
    right_new = int(np.sum(tfhe.mk_decrypt(sks, out_new) == want))

    ms_tuned = None
    if tuned:
        def tuned_way():
            low = eng.mk_bootstrap_tv(digit_tv, digits)
            return tfhe.mk_two_stage_lookup(ck, enc_table, uni, OWNER, low, P, tuned=True)

        out_tuned, ms_tuned = timed(tuned_way)
        tuned_kernel = eng.last_kernel_name()
        assert np.array_equal(out_tuned, out_new), "the tuned rotation's words differ"

    hlwe = tfhe.mk_encrypt(rng, sks, hbits.reshape(-1)).reshape(ADDRESSES, DEPTH, -1)
    idx = np.tile(np.arange(1 << DEPTH, dtype=np.int32), ADDRESSES)

    def old_way():
        low = eng.mk_bootstrap_tv(digit_tv, digits)
        cur = eng.mk_bootstrap_tv(polys, np.repeat(low, 1 << DEPTH, axis=0), index=idx).reshape(ADDRESSES, 1 << DEPTH, -1)
        for v in range(DEPTH):
            sel = np.repeat(hlwe[:, v], cur.shape[1] // 2, axis=0)
            cur = tfhe.mk_gate_mux(ck, sel, cur[:, 1::2].reshape(len(sel), -1), cur[:, 0::2].reshape(len(sel), -1)).reshape(ADDRESSES, cur.shape[1] // 2, -1)
        return cur[:, 0]

    out_old, ms_old = timed(old_way)
    right_old = int(np.sum(tfhe.mk_decrypt(sks, out_old) == want))
    assert right_new >= ADDRESSES * 3 // 4, f"the two-stage lookup decrypts {right_new} of {ADDRESSES}"

    print(f"{ADDRESSES} jointly encrypted addresses into party 0's {P << DEPTH}-entry table")
    print(f"  private table, uni-encrypted high bits, computed digit : {ms_new:8.2f} ms  {right_new} of {ADDRESSES} decrypt  "
          f"(2 rotations + {(1 << DEPTH) - 1} multi-key external products per address)")
    if tuned:
        print(f"  the same with the rotation on the gates' kernel         : {ms_tuned:8.2f} ms  (equal words; {tuned_kernel})")
    print(f"  public table, LWE high bits, lookups and MUX gates     : {ms_old:8.2f} ms  {right_old} of {ADDRESSES} decrypt  "
          f"({1 + (1 << DEPTH) + 2 * ((1 << DEPTH) - 1)} rotations per address)")
    ck.close()
    return ms_new, ms_old, right_new, right_old


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuned", action="store_true", help="also run the lookup with its rotation on the multi-key gates' kernel (tfhe_mk_bootstrap_acc_batch)")
    main(ap.parse_args().tuned)
