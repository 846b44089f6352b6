"""Measurements of the level calls on the device-resident tables at tfhe_parameters_80 (profiles/tlwe_levels_measure.json,
profiles/tlwe_levels_ab_parent.jsonl):
(1) tfhe_blind_rotate_level, B = 1024, one term per row, out_form 2, timing slot 0, against tfhe_blind_rotate_batch on the same samples in
    ANOTHER build of the library (the parent commit's);
(2) the wall time of examples/private_lut_circuit.py's 32 requests through one Circuit per request and through the host path;
(3) bench.py --gpus 1 --steps 20 --warmup 5 with the parent's library and with this tree's, alternating.

    python tools/tlwe_levels_measure.py --parent-lib /path/to/parent/libtfhe_mi355x.so [--runs 5] [--bench-runs 6] [--part 1,2,3]

One process per run (2 warm-up calls, then the median of 5 calls), the two sides' processes alternating on one device, one at a time, each
under its own time limit; the first failure ends the session."""
import argparse
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402

INNER, WARM, B, T = 5, 2, 1024, 8


def example():
    spec = importlib.util.spec_from_file_location("private_lut_circuit", os.path.join(ROOT, "examples", "private_lut_circuit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(call, kernel_ms=None):
    for _ in range(WARM):
        call()
    ms, wall = [], []
    for _ in range(INNER):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        if kernel_ms:
            ms.append(kernel_ms())
    out = {"wall_ms_median": float(np.median(wall)), "wall_ms": wall}
    if kernel_ms:
        out.update(kernel_ms_median=float(np.median(ms)), kernel_ms=ms)
    return out


def worker(mode, path):
    """batch: (1)'s baseline, run with TFHE_MI355X_LIB = the parent's library; level: (1); host / circuit: the two paths of (2)."""
    d = np.load(path)
    ck = tfhe.load_cloud_key(os.path.join(os.path.dirname(path), "ck.tfhe"))
    eng = ck.engine(0)
    out = {"mode": mode, "lib": tfhe.LIB_PATH}
    if mode in ("batch", "level"):
        x, acc = d["x"], d["acc"]
        idx = (np.arange(B) % T).astype(np.int32)
        eng.tgsw_load(leveled.bootstrap_key_selectors(ck))
        if mode == "batch":
            out["run"] = timed(lambda: eng.blind_rotate(acc, x, acc_index=idx, in_form=0, out_form=2), lambda: eng.last_timing_ms(0))
        else:
            eng.tlwe_alloc(T)
            eng.tlwe_upload(0, acc)
            eng.wires_alloc(2 * B)
            eng.wires_upload(0, x)
            start, wire, coef, outw = np.arange(B + 1, dtype=np.int32), np.arange(B, dtype=np.int32), np.ones(B, np.int32), (B + np.arange(B)).astype(np.int32)
            out["run"] = timed(lambda: eng.blind_rotate_level(idx, start, wire, coef, out_form=2, out_wires=outw), lambda: eng.last_timing_ms(0))
            out["kernel"] = eng.last_kernel_name()
            got = eng.wires_gather(outw[:8])
            out["equal_words"] = bool(np.array_equal(got, eng.blind_rotate(acc, x[:8], acc_index=idx[:8], in_form=0, out_form=2)[:, 0]))
        out.setdefault("kernel", eng.last_kernel_name())
    else:
        ex = example()
        call = (lambda: ex.host_path(ck, d["enc_table"], d["tgsw"], d["digits"])) if mode == "host" else (lambda: ex.circuit_path(ck, d["enc_table"], d["tgsw"], d["digits"])[:, 0])
        out["run"] = timed(call)
        out["sha"] = hashlib.sha256(np.ascontiguousarray(call()).tobytes()).hexdigest()
    ck.close()
    print(json.dumps(out))


def spawn(argv, env_lib=None, limit=180):
    env = dict(os.environ)
    if env_lib:
        env["TFHE_MI355X_LIB"] = env_lib
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + argv, env=env, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.exit(f"{argv} failed rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=6)
    ap.add_argument("--part", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tlwe_levels_measure.json"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "tlwe_levels_ab_parent.jsonl"))
    ap.add_argument("--worker")
    ap.add_argument("--keys")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.keys)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the library built from the parent commit (make -C tfhe.jl_amd/csrc in a checkout of it)")
    parent = os.path.abspath(a.parent_lib)
    parts = {int(v) for v in a.part.split(",")}
    me = os.path.abspath(__file__)
    rnd = lambda v: [round(t, 3) for t in v]
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = "level calls on the device-resident tables at tfhe_parameters_80 (n = 500, N = 1024, k = 1, l = 2), one MI355X; times in ms"
    out["method"] = (f"one process per run: {WARM} warm-up calls, then the median of {INNER} calls; the two sides' processes alternating, one at a time; the "
                     "baseline processes of 1 and 3 load the library built from the parent commit")
    if parts & {1, 2}:
        ex = example()
        rng = np.random.default_rng(5)
        p = tfhe.tfhe_parameters_80()
        sk, ck = tfhe.make_key_pair(rng, p)
        N = p.tlwe_polynomial_degree
        x = tfhe.lut_encrypt(rng, sk, rng.integers(0, 8, B), 8).data
        acc = leveled.tlwe_encrypt(rng, sk, np.stack([tfhe.make_test_vector(lambda m, h=h: (3 * m + h) % 8, 8, N) for h in range(T)]))
        table = [int(v) for v in rng.integers(0, ex.P, ex.P << ex.DEPTH)]
        high, da, db = rng.integers(0, 1 << ex.DEPTH, ex.ADDRESSES), rng.integers(0, 4, ex.ADDRESSES), rng.integers(0, 4, ex.ADDRESSES)
        enc_table, tgsw, digits = ex.request_inputs(rng, sk, table, high, da, db)
        with tempfile.TemporaryDirectory() as tmp:
            keys = os.path.join(tmp, "keys.npz")
            np.savez(keys, x=x, acc=acc, enc_table=enc_table, tgsw=tgsw, digits=digits)
            tfhe.save_cloud_key(os.path.join(tmp, "ck.tfhe"), ck)
            if 1 in parts:
                rows = []
                for _ in range(a.runs):
                    rows.append(spawn([me, "--worker", "batch", "--keys", keys], parent))
                    rows.append(spawn([me, "--worker", "level", "--keys", keys]))
                base = [r["run"]["kernel_ms_median"] for r in rows if r["mode"] == "batch"]
                new = [r["run"]["kernel_ms_median"] for r in rows if r["mode"] == "level"]
                out["1_blind_rotate_level_B1024_out_form_2_slot_0"] = {
                    "baseline": "tfhe_blind_rotate_batch (tlwe_rotate_kernel), in_form 0, the same 1024 LWE rows and 8 accumulators, parent commit's library",
                    "baseline_runs_ms": rnd(base), "baseline_median_ms": round(float(np.median(base)), 3), "baseline_min_ms": round(min(base), 3),
                    "baseline_max_ms": round(max(base), 3),
                    "level": rows[1]["kernel"] + ", one term per row (coefficient 1), the rows in the wire table, the accumulators in the TLWE table",
                    "level_runs_ms": rnd(new), "level_median_ms": round(float(np.median(new)), 3),
                    "level_minus_baseline_ms": round(float(np.median(new) - np.median(base)), 3),
                    "level_median_within_baseline_min_max": bool(min(base) <= float(np.median(new)) <= max(base)),
                    "first_8_rows_equal_words": all(r["equal_words"] for r in rows if r["mode"] == "level")}
            if 2 in parts:
                rows = []
                for _ in range(a.runs):
                    rows.append(spawn([me, "--worker", "host", "--keys", keys]))
                    rows.append(spawn([me, "--worker", "circuit", "--keys", keys]))
                host = [r["run"]["wall_ms_median"] for r in rows if r["mode"] == "host"]
                circ = [r["run"]["wall_ms_median"] for r in rows if r["mode"] == "circuit"]
                out["2_private_lookup_32_requests_wall"] = {
                    "host_path": "digit circuit (run_batch over the 32 requests), download, two_stage_lookup: the key re-uploaded as selectors, one batch per stage",
                    "host_runs_ms": rnd(host), "host_median_ms": round(float(np.median(host)), 3),
                    "circuit_path": "tgsw_load once per call, then per request tgsw_update of 3 selectors and one Circuit.run (two more outputs per request than the host path: three bit lookups and two XOR gates)",
                    "circuit_runs_ms": rnd(circ), "circuit_median_ms": round(float(np.median(circ)), 3),
                    "circuit_minus_host_ms": round(float(np.median(circ) - np.median(host)), 3),
                    "equal_words": len({r["sha"] for r in rows}) == 1}
        ck.close()
    if 3 in parts:
        lines = []
        for i in range(a.bench_runs):
            for side, lib in (("parent", parent), ("this tree", None)):
                r = spawn([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, limit=600)
                lines.append({"lib": side, "round": i + 1, "value": r["value"], "ms_per_step": r["ms_per_step"]})
        with open(a.bench_out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
        val = {side: [r["value"] for r in lines if r["lib"] == side] for side in ("parent", "this tree")}
        out["3_bench_ab"] = {
            "command": "bench.py --gpus 1 --steps 20 --warmup 5, the parent's library and this tree's alternating", "runs_each": a.bench_runs,
            "parent_gates_per_s": rnd(val["parent"]), "parent_median": round(float(np.median(val["parent"])), 1),
            "parent_spread_pct": round(100 * (max(val["parent"]) - min(val["parent"])) / float(np.median(val["parent"])), 2),
            "tree_gates_per_s": rnd(val["this tree"]), "tree_median": round(float(np.median(val["this tree"])), 1),
            "tree_median_within_parent_min_max": bool(min(val["parent"]) <= float(np.median(val["this tree"])) <= max(val["parent"]))}
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
