#!/usr/bin/env python3
"""Host cost of the four TLWE rotation calls and the two level network calls, this tree's library against another build's (the
parent commit's): timing slot 0 and wall time of tfhe_blind_rotate_batch, tfhe_blind_rotate_level, tfhe_rot_net_level at
tfhe_parameters_80 and of their multi-key forms at mktfhe_parameters_2party, at B = 1024 rows (the size tools/*_levels_measure.py use)
and at B = 1, where the host cost is the whole call.

    python tools/rotation_runner_ab.py --parent-lib <the other library> [--runs 4] [--out profiles/rotation_runner_ab.jsonl]

One process per run and side (TFHE_MI355X_LIB), the two sides alternating, one at a time; in a process every call is warmed twice and
the medians of 5 calls are kept.  One JSON line per process.  Keys, selectors, samples and wires are arbitrary words of a seeded
generator: the kernels accept any, and no time depends on a value.  The summary printed at the end compares this tree's median of each
figure with the other side's min - max."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INNER, WARM, T, SIZES = 5, 2, 8, (1024, 1)


def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


def timed(eng, call):
    for _ in range(WARM):
        call()
    wall, slot0 = [], []
    for _ in range(INNER):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        slot0.append(eng.last_timing_ms(0))
    return {"slot0_ms": float(np.median(slot0)), "wall_ms": float(np.median(wall))}


def worker(side):
    import tfhe_jl_amd as tfhe
    from tfhe_jl_amd import leveled
    out = {"side": side, "lib": os.path.basename(tfhe.LIB_PATH)}
    rng = np.random.default_rng(7)
    for mk in (False, True):
        p = tfhe.mktfhe_parameters_2party if mk else tfhe.tfhe_parameters_80()
        n, N, l, P = p.lwe_size, p.tlwe_polynomial_degree, p.bs_decomp_length, (2 if mk else 1)
        k = 1
        eng = tfhe.Engine(p)
        ks_words = P * k * N * p.ks_decomp_length * ((1 << p.ks_log2_base) - 1) * (n + 1)
        if mk:
            bk = _words(rng, P, n, 2 * l * P + 2 * l, N)
            eng.mk_load_bootstrap_key(bk, P)
            eng.mk_load_keyswitch_key(_words(rng, ks_words), P)
            eng.mk_tgsw_load(bk.reshape((P * n,) + bk.shape[2:]), np.repeat(np.arange(P, dtype=np.int32), n))
            pre, polys, steps = "mk_", P + 1, P * n
        else:
            bk = _words(rng, n, l, k + 1, k + 1, N)
            eng.load_bootstrap_key(bk)
            eng.load_keyswitch_key(_words(rng, ks_words))
            eng.tgsw_load(bk)
            pre, polys, steps = "", k + 1, n
        f = lambda name: getattr(eng, pre + name)      # noqa: E731
        net = leveled.RotNet([2, 1], [(0, 1, 0, 0, 1), (2, 3, 1, 5, N + 3), (0, 1, 2, 0, 7)], N, entries=4, variables=3)
        for B in SIZES:
            acc, x = _words(rng, T, polys, N), _words(rng, B, steps + 1)
            idx = (np.arange(B) % T).astype(np.int32)
            f("tlwe_alloc")(T + B)
            f("tlwe_upload")(0, acc)
            (eng.mk_wires_alloc if mk else eng.wires_alloc)(2 * B)
            eng.wires_upload(0, x)
            start, wire, coef, outw = np.arange(B + 1, dtype=np.int32), np.arange(B, dtype=np.int32), np.ones(B, np.int32), (B + np.arange(B)).astype(np.int32)
            sel = rng.integers(0, steps, (B, 3)).astype(np.int32)
            first = (np.arange(B) % (T - 3)).astype(np.int32)
            calls = {"blind_rotate_batch": lambda: f("blind_rotate")(acc, x, acc_index=idx, in_form=0, out_form=2),
                     "blind_rotate_level": lambda: f("blind_rotate_level")(idx, start, wire, coef, out_form=2, out_wires=outw),
                     "rot_net_level": lambda: f("rot_net_level")(net, sel, table_first=first, out_form=0, out_first=T)}
            for name, call in calls.items():
                out[f"{pre}{name},B={B}"] = timed(eng, call)
        eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rotation_runner_ab.jsonl"))
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the library built from the parent commit (make -C tfhe.jl_amd/csrc in a checkout of it)")
    rows = []
    for _ in range(a.runs):
        for side, lib in (("parent", os.path.abspath(a.parent_lib)), ("tree", None)):
            env = dict(os.environ)
            env.pop("TFHE_MI355X_LIB", None)
            if lib:
                env["TFHE_MI355X_LIB"] = lib
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--worker", side], env=env, capture_output=True, text=True,
                               cwd=ROOT)
            if r.returncode != 0:
                sys.exit(f"{side} worker failed ({r.returncode}): {r.stderr[-2000:]}")      # (nothing more is started on the device)
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rows[-1]) + "\n")
    for key in [k for k in rows[0] if k not in ("side", "lib")]:
        for fig in ("slot0_ms", "wall_ms"):
            base = [r[key][fig] for r in rows if r["side"] == "parent"]
            new = float(np.median([r[key][fig] for r in rows if r["side"] == "tree"]))
            where = "inside" if min(base) <= new <= max(base) else "fast side" if new < min(base) else "SLOW SIDE"
            print(f"{key:32s} {fig:9s} parent {np.median(base):9.4f} ({min(base):.4f} - {max(base):.4f})  tree {new:9.4f}  {where}")


if __name__ == "__main__":
    main()
