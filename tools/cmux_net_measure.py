#!/usr/bin/env python3
"""Times the CMUX networks of the leveled mode (tfhe_cmux_net_batch) at B = 1, 32 and 1024 rows under tfhe_parameters_80: the 16-bit
comparator less_than_net(16) (32 levels, 48 external products per row) and a depth-8 tree_net (255 products per row), the latter
alternating with tfhe_cmux_tree_batch on the same operands — the per-product yardstick.  CMUX levels and keyswitch from HIP events
(tfhe_last_timing_ms), wall time around the call; medians of `--calls` calls after a warm-up call.

    python tools/cmux_net_measure.py --out profiles/cmux_net_measure.json [--sizes 1 32 1024]
"""
import argparse
import json
import os
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
ap.add_argument("--selectors", type=int, default=64, help="distinct TGSW samples loaded (rows share them: the time does not depend on the bits)")
args = ap.parse_args()

BITS, DEPTH = 16, 8
rng = np.random.default_rng(77)
params = tfhe.tfhe_parameters_80()
sk, ck = tfhe.make_key_pair(rng, params)
eng = ck.engine(0)
N, k = params.tlwe_polynomial_degree, params.tlwe_mask_size
S = args.selectors
sel_bits = np.arange(S) & 1                                             # selector s encrypts bit s & 1
eng.tgsw_load(tfhe.tgsw_encrypt_bits(rng, sk, sel_bits))


def timed(call):
    call()                                                              # warm-up: workspaces
    lv, ks, wall = [], [], []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        lv.append(eng.last_timing_ms(0))
        ks.append(eng.last_timing_ms(1))
    return out, lv, ks, wall


def pick(want_bits):
    """For each wanted bit a random loaded selector that encrypts it."""
    half = rng.integers(0, S // 2, want_bits.shape)
    return (2 * half + want_bits).astype(np.int32)


def row(kernel, lv, ks, wall, products, correct, B):
    lv = np.array(lv)
    return {"kernel": kernel, "rows": B, "correct": correct, "levels_ms": float(np.median(lv)), "levels_min": float(lv.min()), "levels_max": float(lv.max()),
            "keyswitch_ms": float(np.median(ks)), "wall_ms": float(np.median(wall)), "external_products": products,
            "us_per_external_product": float(np.median(lv)) * 1e3 / products}


result = {"comparator": {}, "tree_net": {}, "cmux_tree": {}}
lt, end_table = tfhe.less_than_net(BITS)
lt_data = tfhe.table_to_tlwe(end_table, N, k)
tree = tfhe.tree_net(DEPTH)
table_bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
tree_data = tfhe.table_to_tlwe(table_bits, N, k)
for B in args.sizes:
    x, y = rng.integers(0, 1 << BITS, B), rng.integers(0, 1 << BITS, B)
    bits = np.concatenate([(x[:, None] >> np.arange(BITS)) & 1, (y[:, None] >> np.arange(BITS)) & 1], axis=1)
    sel = pick(bits)
    out, lv, ks, wall = timed(lambda: eng.cmux_net(lt_data, lt, sel))
    ok = int(np.sum(tfhe.decrypt(sk, out[:, 0]) == (x < y)))
    result["comparator"][str(B)] = row(eng.last_kernel_name(), lv, ks, wall, B * lt.products, ok, B)
    print("comparator", B, result["comparator"][str(B)], flush=True)

    addr = rng.integers(0, 1 << DEPTH, B)
    asel = pick((addr[:, None] >> np.arange(DEPTH)) & 1)
    # the network and the tree call alternate, so that drift of the clock falls on both
    eng.cmux_net(tree_data, tree, asel); eng.cmux_tree(tree_data, asel)
    t = {"tree_net": ([], [], []), "cmux_tree": ([], [], [])}
    names = {}
    for _ in range(args.calls):
        for name, call in (("tree_net", lambda: eng.cmux_net(tree_data, tree, asel)[:, 0]), ("cmux_tree", lambda: eng.cmux_tree(tree_data, asel))):
            t0 = time.perf_counter()
            o = call()
            t[name][2].append((time.perf_counter() - t0) * 1e3)
            t[name][0].append(eng.last_timing_ms(0))
            t[name][1].append(eng.last_timing_ms(1))
            names[name] = (eng.last_kernel_name(), int(np.sum(tfhe.decrypt(sk, o) == table_bits[addr])))
    for name in t:
        result[name][str(B)] = row(names[name][0], *t[name], B * tree.products, names[name][1], B)
        print(name, B, result[name][str(B)], flush=True)
    result["tree_net"][str(B)]["per_product_vs_cmux_tree"] = result["tree_net"][str(B)]["levels_ms"] / result["cmux_tree"][str(B)]["levels_ms"]

json.dump(result, open(args.out, "w"), indent=1)
ck.close()
