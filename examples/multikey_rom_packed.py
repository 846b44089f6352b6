"""The jointly addressed ROM of examples/multikey_rom.py read through a packed table, then a 2^16-entry table that the multi-key CMUX
tree cannot hold, then a vote count over bits of both parties.

Tree: 256 public bits as 256 trivial multi-key TLWE samples folded by a depth-8 CMUX tree, 255 multi-key external products per address
(tfhe_jl_amd.leveled.mk_cmux_lookup).
Packed: the same bits on the first 256 coefficients of ONE sample (pack_table_to_tlwe with k = P); CMUX(C_b; acc, X^(-2^b) acc) for the
eight address bits, each under the party that owns the bit, rotates the wanted coefficient to position 0: 8 products per address
(mk_packed_lookup; tfhe_mk_rot_net_batch).  The addresses are the same: party 0 holds the low four bits, party 1 the high four.
The 2^16-entry table is 64 samples: 63 tree products on the high address bits, ten rotation levels on the low ones.
Every answer is a multi-key LWE sample; all are decrypted by the parties together and NANDed with fresh encryptions (mk_gate_nand).
Votes: each party uni-encrypts its own ballot bits; one state looping on itself with X^-1 on a set bit (wfa_net) rotates a gate-encoded
threshold table by minus the count: coefficient 0 is "at least THRESHOLD of the bits are set", one product per ballot.

    python examples/multikey_rom_packed.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402
import multikey_rom as rom  # noqa: E402

DEPTH, BIG_DEPTH, ADDRESSES, PARTIES = rom.DEPTH, 16, rom.ADDRESSES, rom.PARTIES
BIG_OWNER = np.array([0] * 8 + [1] * 8, np.int32)                    # party 0 holds the low byte of a 16-bit address, party 1 the high byte
BALLOTS, COUNTS, THRESHOLD = 15, 8, 8                                # 15 ballot bits per count, bit v cast by party v mod 2


def timed(call):
    call()                                                              # warm-up: workspaces, expansion scratch
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    rng, params, sks, shared, parts, ck = rom.setup()
    eng = ck.engine(0)
    N = params.tlwe_polynomial_degree
    bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
    addr = rng.integers(0, 1 << DEPTH, ADDRESSES)
    abits = ((addr[:, None] >> np.arange(DEPTH)[None, :]) & 1).astype(bool)
    uni = rom.uni_encrypt_addresses(rng, params, shared, parts, abits)

    def check(out, truth, what):
        assert np.array_equal(tfhe.mk_decrypt(sks, out), truth), f"{what} decrypts wrongly"
        y = rng.integers(0, 2, len(truth)).astype(bool)
        nand = tfhe.mk_gate_nand(ck, out, tfhe.mk_encrypt(rng, sks, y))
        assert np.array_equal(tfhe.mk_decrypt(sks, nand), ~(truth & y)), f"NAND of {what} decrypts wrongly"

    tree_out, ms_tree = timed(lambda: leveled.mk_cmux_lookup(ck, rom.table_to_mk_tlwe(bits, N, PARTIES), uni, rom.OWNER))
    ms_tree_kernels = eng.last_timing_ms(2)
    packed_out, ms_packed = timed(lambda: leveled.mk_packed_lookup(ck, bits, uni, rom.OWNER))
    ms_packed_kernels = eng.last_timing_ms(2)
    check(tree_out, bits[addr], "the CMUX-tree lookup")
    check(packed_out, bits[addr], "the packed lookup")

    big = rng.integers(0, 2, 1 << BIG_DEPTH).astype(bool)
    big_addr = rng.integers(0, 1 << BIG_DEPTH, ADDRESSES)
    big_bits = ((big_addr[:, None] >> np.arange(BIG_DEPTH)[None, :]) & 1).astype(bool)
    big_uni = rom.uni_encrypt_addresses(rng, params, shared, parts, big_bits, BIG_OWNER)
    big_table = leveled.pack_table_to_tlwe(big, N, k=PARTIES)           # packed once: [64][P+1][N]
    big_out, ms_big = timed(lambda: leveled.mk_packed_lookup(ck, big_table, big_uni, BIG_OWNER))
    ms_big_kernels = eng.last_timing_ms(2)
    check(big_out, big[big_addr], "the 2^16-entry packed lookup")

    # the vote count: f(popcount) with f = "at least THRESHOLD", one product per ballot bit
    votes = rng.integers(0, 2, (COUNTS, BALLOTS)).astype(bool)
    votes[0], votes[1] = False, True
    voter = np.arange(BALLOTS, dtype=np.int32) % PARTIES
    vote_uni = rom.uni_encrypt_addresses(rng, params, shared, parts, votes, voter)
    count_net = leveled.wfa_net([0], [0], [0], [2 * N - 1], 0, BALLOTS, N)
    threshold = leveled.mk_tlwe_trivial(np.array([[leveled.encode_gate_bit(c >= THRESHOLD) for c in range(N)]], np.int32), PARTIES)
    passed, ms_votes = timed(lambda: leveled.mk_rot_net_lookup(ck, threshold, count_net, vote_uni, voter))
    ms_votes_kernels = eng.last_timing_ms(2)
    check(passed, votes.sum(axis=1) >= THRESHOLD, "the vote count")

    tree_p, packed_p, big_p = (1 << DEPTH) - 1, leveled.packed_lookup_net(DEPTH, N).products, leveled.packed_lookup_net(BIG_DEPTH, N).products
    print(f"{ADDRESSES} jointly encrypted addresses, all answers correct, NAND of every answer correct")
    print(f"  {1 << DEPTH}-entry table, multi-key CMUX tree : {ms_tree:8.2f} ms  (kernels {ms_tree_kernels:.2f} ms; {tree_p} multi-key external products per address)")
    print(f"  {1 << DEPTH}-entry table, packed              : {ms_packed:8.2f} ms  (kernels {ms_packed_kernels:.2f} ms; {packed_p} products per address)")
    print(f"  {1 << BIG_DEPTH}-entry table, packed            : {ms_big:8.2f} ms  (kernels {ms_big_kernels:.2f} ms; {big_p} products per address, "
          f"{big_table.shape[0]} table samples)")
    print(f"  {COUNTS} counts of {BALLOTS} ballots, at least {THRESHOLD}   : {ms_votes:8.2f} ms  (kernels {ms_votes_kernels:.2f} ms; {count_net.products} products per count; "
          f"all {COUNTS} correct)")
    print("  (wall times include the expansion of the uni-encrypted selectors on the device)")
    ck.close()
    return ms_tree, ms_packed, ms_big, ms_votes


if __name__ == "__main__":
    main()
