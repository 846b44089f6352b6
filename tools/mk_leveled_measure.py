#!/usr/bin/env python3
"""Times the multi-key leveled lookup of examples/multikey_rom.py (depth 8, 2-party set) at B = 1, 32 and 1024 addresses:
tfhe_mk_cmux_tree_batch's CMUX levels and keyswitch (HIP events, tfhe_last_timing_ms) and its wall time, against the same selection as a
tree of multi-key MUX gates through Circuit (wall time).  Medians of `--calls` interleaved calls after a warm-up round.

    python tools/mk_leveled_measure.py --out profiles/mk_leveled_measure.json [--gate-calls 3] [--sizes 1 32 1024]
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
import multikey_rom as rom  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--gate-calls", type=int, default=3, help="timed Circuit runs per size (each is 510 B multi-key rotations)")
ap.add_argument("--sizes", type=int, nargs="+", default=[1, 32, 1024])
args = ap.parse_args()

rng, params, sks, shared, parts, ck = rom.setup(321)
eng = ck.engine(0)
N, D = params.tlwe_polynomial_degree, rom.DEPTH
bits = rng.integers(0, 2, 1 << D).astype(bool)
table = rom.table_to_mk_tlwe(bits, N, rom.PARTIES)
pub = np.stack([part.public_b for part in parts])

cases = {}
for B in args.sizes:
    addr = rng.integers(0, 1 << D, B)
    abits = ((addr[:, None] >> np.arange(D)[None, :]) & 1).astype(bool)
    # (every address has its own D selectors, as in a jointly encrypted lookup)
    uni = rom.uni_encrypt_addresses(rng, params, shared, parts, abits)
    who = np.broadcast_to(rom.OWNER, (B, D)).reshape(-1)
    cases[B] = dict(addr=addr, abits=abits, sel=np.arange(B * D, dtype=np.int32).reshape(B, D), uni=uni, who=who, levels=[], ks=[], wall=[])

# the selector set is per size and reloading it costs more than the lookup: the sizes follow each other, each with its own expansion
# and warm-up call, and the timed calls of one size run back to back
result = {}
for B, c in cases.items():
    t0 = time.perf_counter()
    eng.mk_tgsw_expand_load(pub, c["who"], *[a.reshape((B * D,) + a.shape[2:]) for a in c["uni"]])
    c["expand_ms"] = (time.perf_counter() - t0) * 1e3
    out = eng.mk_cmux_tree(table, c["sel"])                                # warm-up
    ok = int(np.sum(tfhe.mk_decrypt(sks, out) == bits[c["addr"]]))
    for _ in range(args.calls):
        t0 = time.perf_counter()
        eng.mk_cmux_tree(table, c["sel"])
        c["wall"].append((time.perf_counter() - t0) * 1e3)
        c["levels"].append(eng.last_timing_ms(0))
        c["ks"].append(eng.last_timing_ms(1))
    lv = np.array(c["levels"])
    result[str(B)] = {
        "kernel": eng.last_kernel_name(), "correct": ok, "rows": B,
        "levels_ms": float(np.median(lv)), "levels_min": float(lv.min()), "levels_max": float(lv.max()),
        "keyswitch_ms": float(np.median(c["ks"])), "wall_ms": float(np.median(c["wall"])),
        "expand_load_ms": c["expand_ms"], "us_per_external_product": float(np.median(lv)) * 1e3 / (((1 << D) - 1) * B),
    }
    print(B, result[str(B)], flush=True)

for B, c in cases.items():
    if args.gate_calls <= 0:
        break
    circuit = rom.mux_tree_circuit(bits, B, D)
    inputs = tfhe.mk_encrypt(rng, sks, c["abits"].reshape(-1))
    got = circuit.run(ck, inputs)                                           # warm-up
    walls = []
    for _ in range(args.gate_calls):
        t0 = time.perf_counter()
        circuit.run(ck, inputs)
        walls.append((time.perf_counter() - t0) * 1e3)
    result[str(B)].update(mux_gates_wall_ms=float(np.median(walls)), mux_gates_calls=args.gate_calls,
                          mux_gates_correct=int(np.sum(tfhe.mk_decrypt(sks, got) == bits[c["addr"]])), mux_gates=((1 << D) - 1) * B)
    print(B, "gates", result[str(B)]["mux_gates_wall_ms"], flush=True)

json.dump(result, open(args.out, "w"), indent=1)
ck.close()
