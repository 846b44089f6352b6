"""examples/multikey_private_lut.py's program — gates, a jointly addressed private lookup, gates — without leaving the device: two
parties, a 32-entry bit table that party 0 owns and the server never sees, read at an address whose high three bits the two parties
hold and whose low digit (of Z_4) is computed ON THE SERVER, and the answer consumed by a gate, request after request.

The host path (leveled.mk_two_stage_lookup) goes through the host five times per request — the digit comes down and goes up again as
`rows`, the tree's MK TLWE output comes down and goes up again as `acc`, the answer comes down and goes up into the gate — and
re-expands and re-uploads the whole multi-key bootstrapping key as selectors (P n expanded RGSW samples) because the request's address
bits sit in the same selector set.

The device-resident path (leveled.mk_two_stage_lookup_device; tfhe_mk_tlwe_alloc, tfhe_mk_tgsw_expand_update, tfhe_mk_rot_net_level,
tfhe_mk_blind_rotate_level):
  1. the request's digits go up into multi-key wires;
  2. mk_lut_level computes the low digit, wire to wire;
  3. the request's address bits are swapped in behind the key's selectors, which were loaded once, and a depth-3 jointly addressed tree
     picks each row's private test polynomial from the MK TLWE table into a slot;
  4. the rotation of that slot reads its digit from the wires and writes the answer, keyswitched, into wires;
  5. an mk_gates_level NAND consumes the answer;
  6. one gather brings the request's results down.

Both paths compute the same words.  Every multi-key rotation at this parameter set adds noise with a standard deviation near 0.06 of the
torus to a +-1/8 window, so neither path decrypts every answer; the number that does is printed for both.

    python examples/multikey_private_lut_device.py [--tuned]

--tuned: the device-resident path is also run with its rotation on the multi-key gates' own kernel and key
(mk_two_stage_lookup_device(..., tuned=True); tfhe_mk_bootstrap_acc_level): the key's P n selectors are never loaded, the selector set
holds a request's address bits alone.  The words are the same; the time is printed.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled, lut  # noqa: E402
import multikey_rom as rom  # noqa: E402

P, DEPTH, REQUESTS, ROWS = 4, 3, 4, 8                                   # Z_4 digits, 2^3 sub-tables, 4 requests of 8 addresses
OWNER = np.array([0, 1, 0], np.int32)                                   # high address bit v is held by party v mod 2
NAND = 0
# the wires of one request: digits | computed low digits | answers | the gate's other operand | the gate's results
W_DIGIT, W_LOW, W_ANS, W_MASK, W_OUT, WIRES = 0, ROWS, 2 * ROWS, 3 * ROWS, 4 * ROWS, 5 * ROWS
# the MK TLWE slots: the 2^DEPTH sub-tables, then one work slot per row
S_TABLE, S_WORK, SLOTS = 0, 1 << DEPTH, (1 << DEPTH) + ROWS


def digit_of(m):
    """The low address digit the server computes from the encrypted digit m."""
    return (3 * m + 1) % P


def request_inputs(rng, params, sks, shared, parts, table, high, m, mask):
    """The parties' side of all requests: party 0's table under both TLWE keys, per request the high bits uni-encrypted by their owners,
    the digits and the gate's other operand as multi-key samples."""
    N = params.tlwe_polynomial_degree
    polys = np.stack([tfhe.make_gate_test_vector(lambda v, h=h: table[P * h + v], P, N) for h in range(1 << DEPTH)])
    enc_table = tfhe.mk_tlwe_encrypt(rng, [part.tlwe_key for part in parts], params.bs_noise_stddev, polys)
    hbits = ((high[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)
    uni = rom.uni_encrypt_addresses(rng, params, shared, parts, hbits, OWNER)
    return enc_table, uni, lut.mk_lut_encrypt(rng, sks, m, P), tfhe.mk_encrypt(rng, sks, mask)


def host_path(ck, enc_table, uni, digits, masks, digit_tv):
    """Request by request through the host-buffer calls: [REQUESTS * ROWS][P n + 1]."""
    eng = ck.engine(0)
    out = []
    for r in range(REQUESTS):
        rows = slice(r * ROWS, (r + 1) * ROWS)
        low = eng.mk_bootstrap_tv(digit_tv, digits[rows])
        answer = leveled.mk_two_stage_lookup(ck, enc_table, [a[rows] for a in uni], OWNER, low, P)
        out.append(eng.mk_gates_batch(np.full(ROWS, NAND, np.uint8), answer, masks[rows]))
    return np.concatenate(out)


def device_path(ck, enc_table, uni, digits, masks, digit_tv, tuned=False):
    """The same requests between the device-resident tables: per request one upload of its wires, four level calls and one gather.
    tuned: the rotation by tfhe_mk_bootstrap_acc_level, on the gates' kernel and key."""
    eng = ck.engine(0)
    eng.mk_tlwe_alloc(SLOTS)
    eng.mk_tlwe_upload(S_TABLE, enc_table)
    eng.mk_wires_alloc(WIRES)
    one, every = np.ones(ROWS, np.int32), np.arange(ROWS, dtype=np.int32)
    out = []
    for r in range(REQUESTS):
        rows = slice(r * ROWS, (r + 1) * ROWS)
        eng.wires_upload(W_DIGIT, digits[rows])
        eng.wires_upload(W_MASK, masks[rows])
        eng.mk_lut_level(digit_tv, np.arange(ROWS + 1, dtype=np.int32), W_DIGIT + every, one, None, W_LOW + every)
        leveled.mk_two_stage_lookup_device(ck, S_TABLE, [a[rows] for a in uni], OWNER, W_LOW + every, W_ANS + every, work_slot=S_WORK, tuned=tuned)
        eng.mk_gates_level(np.full(ROWS, NAND, np.uint8), W_ANS + every, W_MASK + every, None, W_OUT + every)
        out.append(eng.wires_gather(W_OUT + every))
    return np.concatenate(out)


def selectors_moved(params, parties=2):
    """Expanded RGSW samples uploaded per request on each path (after the device path's first request)."""
    return {"host": parties * params.lwe_size + ROWS * DEPTH, "device": ROWS * DEPTH}


def timed(call):
    call()                                                              # warm-up: workspaces, expansion scratch, the key's selectors
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main(tuned=False):
    rng, params, sks, shared, parts, ck = rom.setup(2028)
    N = params.tlwe_polynomial_degree
    A = REQUESTS * ROWS
    table = rng.integers(0, 2, P << DEPTH).astype(bool)
    high, m, mask = rng.integers(0, 1 << DEPTH, A), rng.integers(0, P, A), rng.integers(0, 2, A).astype(bool)
    want = ~(np.array([table[P * h + digit_of(v)] for h, v in zip(high, m)]) & mask)
    enc_table, uni, digits, masks = request_inputs(rng, params, sks, shared, parts, table, high, m, mask)
    digit_tv = tfhe.make_test_vector(digit_of, P, N)[None]

    out_host, ms_host = timed(lambda: host_path(ck, enc_table, uni, digits, masks, digit_tv))
    out_dev, ms_dev = timed(lambda: device_path(ck, enc_table, uni, digits, masks, digit_tv))
    equal = bool(np.array_equal(out_host, out_dev))
    ms_tuned = None
    if tuned:
        out_tuned, ms_tuned = timed(lambda: device_path(ck, enc_table, uni, digits, masks, digit_tv, tuned=True))
        assert np.array_equal(out_tuned, out_dev), "the tuned rotation's words differ"
    right_host = int(np.sum(tfhe.mk_decrypt(sks, out_host) == want))
    right_dev = int(np.sum(tfhe.mk_decrypt(sks, out_dev) == want))
    moved = selectors_moved(params)
    assert equal, "the device-resident path differs from the host path"
    assert right_dev >= A // 2, f"the device-resident path decrypts {right_dev} of {A}"

    print(f"{REQUESTS} requests of {ROWS} jointly encrypted addresses into party 0's {P << DEPTH}-entry table, each answer into a NAND gate")
    print(f"  host path   : {ms_host:8.2f} ms  {right_host} of {A} decrypt  ({moved['host']} selectors expanded and uploaded per request, 5 host round trips)")
    print(f"  device path : {ms_dev:8.2f} ms  {right_dev} of {A} decrypt  ({moved['device']} selectors expanded and uploaded per request, 1 upload and 1 gather)")
    if tuned:
        print(f"  device path, rotation on the gates' kernel : {ms_tuned:8.2f} ms  (equal words; no key selectors loaded, {moved['device']} per request)")
    print(f"  the two paths' words are equal: {equal}")
    ck.close()
    return ms_host, ms_dev, right_host, right_dev, equal


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tuned", action="store_true", help="also run the device path with its rotation on the multi-key gates' kernel (tfhe_mk_bootstrap_acc_level)")
    main(ap.parse_args().tuned)
