#!/usr/bin/env python3
"""Times the CMUX networks under a multi-key cloud key (tfhe_mk_cmux_net_batch) at B = 1, 32 and 1024 rows under
mktfhe_parameters_2party: the 16-bit comparator less_than_net(16) (32 levels, 48 multi-key external products per row; party 0 owns x,
party 1 owns y) and a depth-8 tree_net (255 products per row), the latter alternating with tfhe_mk_cmux_tree_batch on the same operands —
the per-product yardstick.  CMUX levels and keyswitch from HIP events (tfhe_last_timing_ms), wall time around the call; medians of
`--calls` calls after a warm-up call.  Rows share `--selectors` uni-encrypted selectors per party (the time does not depend on the
bits), so the expansion is not part of what is timed.

    python tools/mk_cmux_net_measure.py --out profiles/mk_cmux_net_measure.json [--sizes 1 32 1024]
"""
import argparse
import json
import os
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
ap.add_argument("--selectors", type=int, default=32, help="distinct selectors per party (rows share them)")
args = ap.parse_args()

BITS, DEPTH, P = 16, 8, rom.PARTIES
rng, params, sks, shared, parts, ck = rom.setup(77)
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


def row(kernel, lv, ks, wall, products, correct, B):
    lv = np.array(lv)
    return {"kernel": kernel, "rows": B, "correct": correct, "levels_ms": float(np.median(lv)), "levels_min": float(lv.min()), "levels_max": float(lv.max()),
            "keyswitch_ms": float(np.median(ks)), "wall_ms": float(np.median(wall)), "external_products": products,
            "us_per_external_product": float(np.median(lv)) * 1e3 / products}


result = {"selectors": int(P * S), "expand_load_ms": expand_ms, "comparator": {}, "tree_net": {}, "mk_cmux_tree": {}}
lt, end_table = leveled.less_than_net(BITS)
lt_data = leveled.table_to_tlwe(end_table, N, k=P)
lt_party = np.array([0] * BITS + [1] * BITS)[None, :]
tree = leveled.tree_net(DEPTH)
table_bits = rng.integers(0, 2, 1 << DEPTH).astype(bool)
tree_data = leveled.table_to_tlwe(table_bits, N, k=P)
for B in args.sizes:
    x, y = rng.integers(0, 1 << BITS, B), rng.integers(0, 1 << BITS, B)
    bits = np.concatenate([(x[:, None] >> np.arange(BITS)) & 1, (y[:, None] >> np.arange(BITS)) & 1], axis=1)
    sel = pick(bits, lt_party)
    out, lv, ks, wall = timed(lambda: eng.mk_cmux_net(lt_data, lt, sel))
    ok = int(np.sum(tfhe.mk_decrypt(sks, out[:, 0]) == (x < y)))
    result["comparator"][str(B)] = row(eng.last_kernel_name(), lv, ks, wall, B * lt.products, ok, B)
    print("comparator", B, result["comparator"][str(B)], flush=True)

    addr = rng.integers(0, 1 << DEPTH, B)
    asel = pick((addr[:, None] >> np.arange(DEPTH)) & 1, rom.OWNER[None, :])
    # the network and the tree call alternate, so that drift of the clock falls on both
    eng.mk_cmux_net(tree_data, tree, asel); eng.mk_cmux_tree(tree_data, asel)
    t = {"tree_net": ([], [], []), "mk_cmux_tree": ([], [], [])}
    names = {}
    for _ in range(args.calls):
        for name, call in (("tree_net", lambda: eng.mk_cmux_net(tree_data, tree, asel)[:, 0]), ("mk_cmux_tree", lambda: eng.mk_cmux_tree(tree_data, asel))):
            t0 = time.perf_counter()
            o = call()
            t[name][2].append((time.perf_counter() - t0) * 1e3)
            t[name][0].append(eng.last_timing_ms(0))
            t[name][1].append(eng.last_timing_ms(1))
            names[name] = (eng.last_kernel_name(), int(np.sum(tfhe.mk_decrypt(sks, o) == table_bits[addr])))
    for name in t:
        result[name][str(B)] = row(names[name][0], *t[name], B * tree.products, names[name][1], B)
        print(name, B, result[name][str(B)], flush=True)
    result["tree_net"][str(B)]["per_product_vs_mk_cmux_tree"] = result["tree_net"][str(B)]["levels_ms"] / result["mk_cmux_tree"][str(B)]["levels_ms"]

json.dump(result, open(args.out, "w"), indent=1)
ck.close()
