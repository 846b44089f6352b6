#!/usr/bin/env python3
"""Times the CMUX networks with monomial edges (tfhe_rot_net_batch) at B = 1, 32 and 1024 rows under tfhe_parameters_80:

  rotated_read   a depth-8 tree_net run as a RotNet with every rotation 0, alternating with tfhe_cmux_net_batch on the same operands —
                 what the rotated read costs per external product, with the existing kernel as the yardstick;
  packed         a 256-entry table packed into one sample and read through packed_lookup_net(8, N) (8 launches of width 1, 8 products per
                 row), alternating with tfhe_cmux_tree_batch of depth 8 (255 products per row) on the same selectors;
  table_2_16     a 2^16-entry table (64 samples, 63 + 10 products per row) at B = 32, which no CMUX tree of the library can hold.

CMUX levels and keyswitch from HIP events (tfhe_last_timing_ms), wall time around the call; medians of `--calls` calls after a warm-up
call.  The kernel's register figures are copied from the build's report when it is there.

    python tools/rot_net_measure.py --out profiles/rot_net_measure.json [--sizes 1 32 1024]
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
import tfhe_jl_amd as tfhe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--sizes", type=int, nargs="+", default=[1, 32, 1024])
ap.add_argument("--big-rows", type=int, default=32, help="rows of the 2^16-entry lookup")
ap.add_argument("--selectors", type=int, default=64, help="distinct TGSW samples loaded (rows share them: the time does not depend on the bits)")
args = ap.parse_args()

DEPTH, BIG = 8, 16
rng = np.random.default_rng(78)
params = tfhe.tfhe_parameters_80()
sk, ck = tfhe.make_key_pair(rng, params)
eng = ck.engine(0)
N, k = params.tlwe_polynomial_degree, params.tlwe_mask_size
S = args.selectors
eng.tgsw_load(tfhe.tgsw_encrypt_bits(rng, sk, np.arange(S) & 1))       # selector s encrypts bit s & 1


def pick(want_bits):
    """For each wanted bit a random loaded selector that encrypts it."""
    half = rng.integers(0, S // 2, want_bits.shape)
    return (2 * half + want_bits).astype(np.int32)


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
            seen[name] = (eng.last_kernel_name(), int(np.sum(tfhe.decrypt(sk, o) == truth)))
    return {name: row(seen[name][0], *t[name], B * calls[name][1], seen[name][1], B) for name in calls}


result = {"rotated_read": {}, "packed": {}, "table_2_16": {}}
table_bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
tree_data = tfhe.table_to_tlwe(table_bits, N, k)
packed_data = tfhe.pack_table_to_tlwe(table_bits, N, k)
tree = tfhe.tree_net(DEPTH)
tree_rot = tfhe.RotNet(tree.widths, np.concatenate([tree.nodes, np.zeros((len(tree.nodes), 2), np.int32)], axis=1), N, entries=tree.entries,
                       variables=tree.variables)
packed = tfhe.packed_lookup_net(DEPTH, N)
for B in args.sizes:
    addr = rng.integers(0, 1 << DEPTH, B)
    asel = pick((addr[:, None] >> np.arange(DEPTH)) & 1)
    r = alternate({"rot_net_zero": (lambda: eng.rot_net(tree_data, tree_rot, asel)[:, 0], tree.products),
                   "cmux_net": (lambda: eng.cmux_net(tree_data, tree, asel)[:, 0], tree.products)}, table_bits[addr], B)
    r["per_product_vs_cmux_net"] = r["rot_net_zero"]["levels_ms"] / r["cmux_net"]["levels_ms"]
    result["rotated_read"][str(B)] = r
    print("rotated_read", B, r, flush=True)
    r = alternate({"packed_lookup": (lambda: eng.rot_net(packed_data, packed, asel)[:, 0], packed.products),
                   "cmux_tree": (lambda: eng.cmux_tree(tree_data, asel), tree.products)}, table_bits[addr], B)
    r["levels_vs_cmux_tree"] = r["packed_lookup"]["levels_ms"] / r["cmux_tree"]["levels_ms"]
    r["wall_vs_cmux_tree"] = r["packed_lookup"]["wall_ms"] / r["cmux_tree"]["wall_ms"]
    result["packed"][str(B)] = r
    print("packed", B, r, flush=True)

B = args.big_rows
big_bits = rng.integers(0, 2, 1 << BIG).astype(bool)
big_data = tfhe.pack_table_to_tlwe(big_bits, N, k)
big = tfhe.packed_lookup_net(BIG, N)
addr = rng.integers(0, 1 << BIG, B)
bsel = pick((addr[:, None] >> np.arange(BIG)) & 1)
r = alternate({"packed_lookup": (lambda: eng.rot_net(big_data, big, bsel)[:, 0], big.products)}, big_bits[addr], B)
r["table_samples"] = int(big_data.shape[0])
result["table_2_16"][str(B)] = r
print("table_2_16", B, r, flush=True)

report = os.path.join(ROOT, "tfhe.jl_amd", "build", "resource_usage_rot_net.txt")
if os.path.exists(report):
    txt = open(report).read()
    result["kernel_resources"] = {name: int(m.group(1)) for name, pat in
                                  (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                                   ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                                   ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")) for m in [re.search(pat, txt)] if m}
json.dump(result, open(args.out, "w"), indent=1)
ck.close()
