#!/usr/bin/env python3
"""Times the CMUX networks with monomial edges under a multi-key cloud key (tfhe_mk_rot_net_batch) at B = 1, 32 and 1024 rows under
mktfhe_parameters_2party (party 0 owns the low half of the address bits, party 1 the high half):

  rotated_read   a depth-8 tree_net run as a RotNet with every rotation 0, alternating with tfhe_mk_cmux_net_batch on the same operands —
                 what the rotated read costs per multi-key external product, with the existing kernel as the yardstick;
  packed         a 256-entry table packed into one MK TLWE sample and read through packed_lookup_net(8, N) (the call mk_packed_lookup
                 makes: 8 launches of width 1, 8 products per row), alternating with tfhe_mk_cmux_tree_batch of depth 8 (255 products
                 per row) on the same selectors;
  table_2_16     a 2^16-entry table (64 samples, 63 + 10 products per row) at B = 32, which no multi-key CMUX tree of the library holds.

CMUX levels and keyswitch from HIP events (tfhe_last_timing_ms), wall time around the call; medians of `--calls` calls after a warm-up
call.  Rows share `--selectors` uni-encrypted selectors per party (the time does not depend on the bits), so the expansion is not part
of what is timed.  The kernel's register figures are copied from the build's report when it is there.

    python tools/mk_rot_net_measure.py --out profiles/mk_rot_net_measure.json [--sizes 1 32 1024]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402
import multikey_rom as rom  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="+", default=[1, 32, 1024])
ap.add_argument("--big-rows", type=int, default=32, help="rows of the 2^16-entry lookup")
ap.add_argument("--selectors", type=int, default=32, help="distinct selectors per party (rows share them)")
args = ap.parse_args()

DEPTH, BIG, P = 8, 16, rom.PARTIES
rng, params, sks, shared, parts, ck = rom.setup(79)
eng = ck.engine(0)
N = params.tlwe_polynomial_degree
S = args.selectors
# selector i + S * party encrypts bit i & 1 and belongs to `party`
owners = np.repeat(np.arange(P, dtype=np.int32), S)
sel_bits = np.tile(np.arange(S) & 1, P)
uni = rom.uni_encrypt_addresses(rng, params, shared, parts, sel_bits[None, :].astype(bool), owners)
t0 = time.perf_counter()
eng.mk_tgsw_expand_load(np.stack([part.public_b for part in parts]), owners, *[a[0] for a in uni])
expand_ms = (time.perf_counter() - t0) * 1e3


def pick(want_bits, party):
    """For each wanted bit a random loaded selector of party[...] that encrypts it."""
    half = rng.integers(0, S // 2, want_bits.shape)
    return (2 * half + want_bits + S * party).astype(np.int32)


def row(kernel, lv, ks, wall, products, correct, B):
    lv = np.array(lv)
    return {"kernel": kernel, "rows": B, "correct": correct, "levels_ms": float(np.median(lv)), "levels_min": float(lv.min()), "levels_max": float(lv.max()),
            "keyswitch_ms": float(np.median(ks)), "wall_ms": float(np.median(wall)), "external_products": products,
            "us_per_external_product": float(np.median(lv)) * 1e3 / products}


def alternate(calls, truth, B):
    """calls: {name: (callable, external products per row)}; one warm-up call each, then they alternate so that drift of the clock falls
    on all of them."""
    for call, _ in calls.values():
        call()
    t = {name: ([], [], []) for name in calls}
    seen = {}
    for _ in range(args.calls):
        for name, (call, _) in calls.items():
            t0 = time.perf_counter()
            o = call()
            t[name][2].append((time.perf_counter() - t0) * 1e3)
            t[name][0].append(eng.last_timing_ms(0))
            t[name][1].append(eng.last_timing_ms(1))
            seen[name] = (eng.last_kernel_name(), int(np.sum(tfhe.mk_decrypt(sks, o) == truth)))
    return {name: row(seen[name][0], *t[name], B * calls[name][1], seen[name][1], B) for name in calls}


result = {"note": "the series mk_packed_lookup times Engine.mk_rot_net with packed_lookup_net(depth, N) on selectors loaded once: the engine call that leveled.mk_packed_lookup makes, without its expansion of the uni-encryptions (examples/multikey_rom_packed.py times the whole function)", "selectors": int(P * S), "expand_load_ms": expand_ms, "rotated_read": {}, "packed": {}, "table_2_16": {}}
table_bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
tree_data = leveled.table_to_tlwe(table_bits, N, k=P)
packed_data = leveled.pack_table_to_tlwe(table_bits, N, k=P)
tree = leveled.tree_net(DEPTH)
tree_rot = leveled.RotNet(tree.widths, np.concatenate([tree.nodes, np.zeros((len(tree.nodes), 2), np.int32)], axis=1), N, entries=tree.entries,
                          variables=tree.variables)
packed = leveled.packed_lookup_net(DEPTH, N)
for B in args.sizes:
    addr = rng.integers(0, 1 << DEPTH, B)
    asel = pick((addr[:, None] >> np.arange(DEPTH)) & 1, rom.OWNER[None, :])
    r = alternate({"mk_rot_net_zero": (lambda: eng.mk_rot_net(tree_data, tree_rot, asel)[:, 0], tree.products),
                   "mk_cmux_net": (lambda: eng.mk_cmux_net(tree_data, tree, asel)[:, 0], tree.products)}, table_bits[addr], B)
    r["per_product_vs_mk_cmux_net"] = r["mk_rot_net_zero"]["levels_ms"] / r["mk_cmux_net"]["levels_ms"]
    result["rotated_read"][str(B)] = r
    print("rotated_read", B, r, flush=True)
    r = alternate({"mk_packed_lookup": (lambda: eng.mk_rot_net(packed_data, packed, asel)[:, 0], packed.products),
                   "mk_cmux_tree": (lambda: eng.mk_cmux_tree(tree_data, asel), tree.products)}, table_bits[addr], B)
    r["levels_vs_mk_cmux_tree"] = r["mk_packed_lookup"]["levels_ms"] / r["mk_cmux_tree"]["levels_ms"]
    r["wall_vs_mk_cmux_tree"] = r["mk_packed_lookup"]["wall_ms"] / r["mk_cmux_tree"]["wall_ms"]
    result["packed"][str(B)] = r
    print("packed", B, r, flush=True)

B = args.big_rows
big_bits = rng.integers(0, 2, 1 << BIG).astype(bool)
big_data = leveled.pack_table_to_tlwe(big_bits, N, k=P)
big = leveled.packed_lookup_net(BIG, N)
addr = rng.integers(0, 1 << BIG, B)
big_owner = np.array([0] * (BIG // 2) + [1] * (BIG // 2))
bsel = pick((addr[:, None] >> np.arange(BIG)) & 1, big_owner[None, :])
r = alternate({"mk_packed_lookup": (lambda: eng.mk_rot_net(big_data, big, bsel)[:, 0], big.products)}, big_bits[addr], B)
r["table_samples"] = int(big_data.shape[0])
result["table_2_16"][str(B)] = r
print("table_2_16", B, r, flush=True)

report = os.path.join(ROOT, "tfhe.jl_amd", "build", "resource_usage_mk_rot_net.txt")
if os.path.exists(report):
    txt = open(report).read()
    result["kernel_resources"] = {name: int(m.group(1)) for name, pat in
                                  (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                                   ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                                   ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")) for m in [re.search(pat, txt)] if m}
json.dump(result, open(args.out, "w"), indent=1)
ck.close()
