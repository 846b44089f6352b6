"""Measurements of the private-table rotation on the multi-wave gate kernels at tfhe_parameters_80 (DESIGN §4.21;
profiles/bootstrap_acc_small_measure.json, profiles/bootstrap_acc_small_ab_parent.jsonl), tools/bootstrap_acc_measure.py's protocol:
(1) tfhe_bootstrap_acc_batch, rows 1, 64, 256, 1024 and 2560, out_form 2, timing slot 0 (the rotation), three sides:
    reference — option acc_dispatch 0, blind_rotate_kernel_v3_acc at every size (the parent's code path);
    new       — the same call with acc_dispatch 1 (h2_acc, w2_acc, v3_acc + w2_acc by size);
    floor     — tfhe_bootstrap_tv_batch on the same rows at default dispatch: the gates' own h2 / w2 / split on public tables;
(2) bench.py --gpus 1 --steps 20 --warmup 5 with the parent's library and with this tree's, alternating;
(3) examples/private_lut_circuit.py's requests, one Circuit.run each, with the rotation node untuned and tuned (acc_dispatch 1).

    python tools/bootstrap_acc_small_measure.py [--parent-lib /path/to/parent/libtfhe_mi355x.so] [--runs 5] [--bench-runs 6] [--part 1,2,3]

One process per run and side (2 warm-up calls, then the median of 5 calls, at every size), the sides' processes alternating on one device,
one at a time, each under its own time limit; the first failure ends the session."""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402

INNER, WARM, SIZES, T = 5, 2, (1, 64, 256, 1024, 2560), 8
SIDES = ("reference", "new", "floor")
GATED = (1, 1024)               # sizes at which the new side's min-max must lie wholly below the reference's
REQUESTS = 8


def timed(call, kernel_ms):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(INNER):
        call()
        ms.append(kernel_ms())
    return {"kernel_ms_median": float(np.median(ms)), "kernel_ms": ms}


def worker(side, path):
    d = np.load(path)
    ck = tfhe.load_cloud_key(os.path.join(os.path.dirname(path), "ck.tfhe"))
    eng = ck.engine(0)
    out = {"side": side, "sizes": {}}
    x, acc, tv = d["x"], d["acc"], d["tv"]
    eng.set_option("acc_dispatch", 1 if side == "new" else 0)
    for B in SIZES:
        rows, idx = np.ascontiguousarray(x[:B]), (np.arange(B) % T).astype(np.int32)
        if side == "floor":
            call = lambda: eng.bootstrap_tv(tv, rows, index=idx, with_keyswitch=True)
        else:
            call = lambda: eng.bootstrap_acc(acc, rows, acc_index=idx, out_form=2)
        run = timed(call, lambda: eng.last_timing_ms(0))
        run["kernel"] = eng.last_kernel_name()
        out["sizes"][str(B)] = run
    if side == "new":      # the two option values return the same words: the first rows of the largest size, across the seam of its split
        B = max(SIZES)
        idx = (np.arange(B) % T).astype(np.int32)
        got = eng.bootstrap_acc(acc, x[:B], acc_index=idx, out_form=2)
        eng.set_option("acc_dispatch", 0)
        out["equal_words"] = bool(np.array_equal(got, eng.bootstrap_acc(acc, x[:B], acc_index=idx, out_form=2)))
    ck.close()
    print(json.dumps(out))


def circuit_worker():
    spec = importlib.util.spec_from_file_location("private_lut_circuit", os.path.join(ROOT, "examples", "private_lut_circuit.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    rng = np.random.default_rng(2026)
    sk, ck = tfhe.make_key_pair(rng, tfhe.tfhe_parameters_80())
    ms_circ, ms_host, ms_tuned = example.lookup_both_ways(rng, sk, ck, REQUESTS, tuned=True)
    ck.close()
    print(json.dumps({"requests": REQUESTS, "untuned_ms_per_request": ms_circ / REQUESTS, "tuned_ms_per_request": ms_tuned / REQUESTS}))


def spawn(argv, env_lib=None, limit=240):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_acc_small_measure.json"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "bootstrap_acc_small_ab_parent.jsonl"))
    ap.add_argument("--worker")
    ap.add_argument("--keys")
    a = ap.parse_args()
    if a.worker == "circuit":
        return circuit_worker()
    if a.worker:
        return worker(a.worker, a.keys)
    parts = {int(v) for v in a.part.split(",")}
    if 2 in parts and (not a.parent_lib or not os.path.exists(a.parent_lib)):
        sys.exit("--parent-lib: the library built from the parent commit (make -C tfhe.jl_amd/csrc in a checkout of it)")
    me = os.path.abspath(__file__)
    rnd = lambda v: [round(t, 3) for t in v]
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = "private-table rotation by batch size (option acc_dispatch) at tfhe_parameters_80 (n = 500, N = 1024, k = 1, l = 2), one MI355X; times in ms"
    out["method"] = (f"one process per run and side: {WARM} warm-up calls, then the median of {INNER} calls at each size; the sides' processes alternating, "
                     "one at a time; timing slot 0 (the rotation alone)")
    if 1 in parts:
        rng = np.random.default_rng(5)
        p = tfhe.tfhe_parameters_80()
        sk, ck = tfhe.make_key_pair(rng, p)
        N = p.tlwe_polynomial_degree
        polys = np.stack([tfhe.make_test_vector(lambda m, h=h: (3 * m + h) % 8, 8, N) for h in range(T)])
        x = tfhe.lut_encrypt(rng, sk, rng.integers(0, 8, max(SIZES)), 8).data
        acc = leveled.tlwe_encrypt(rng, sk, polys)
        with tempfile.TemporaryDirectory() as tmp:
            keys = os.path.join(tmp, "keys.npz")
            np.savez(keys, x=x, acc=acc, tv=polys)
            tfhe.save_cloud_key(os.path.join(tmp, "ck.tfhe"), ck)
            ck.close()
            rows = [spawn([me, "--worker", side, "--keys", keys]) for _ in range(a.runs) for side in SIDES]
        res = {"reference": "tfhe_bootstrap_acc_batch on 8 encrypted accumulators, out_form 2, acc_dispatch 0 (the parent's code path)",
               "new": "the same call with acc_dispatch 1",
               "floor": "tfhe_bootstrap_tv_batch of the same rows with the 8 test polynomials public, default dispatch (the gates' own kernels)",
               "both_option_values_equal_words_at_2560_rows": all(r["equal_words"] for r in rows if r["side"] == "new")}
        for B in SIZES:
            e = {}
            for side in SIDES:
                v = [r["sizes"][str(B)]["kernel_ms_median"] for r in rows if r["side"] == side]
                e[side] = {"kernel": next(r["sizes"][str(B)]["kernel"] for r in rows if r["side"] == side), "runs_ms": rnd(v),
                           "median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            e["new_max_below_reference_min"] = bool(e["new"]["max_ms"] < e["reference"]["min_ms"])
            e["gated"] = B in GATED
            e["reference_over_new"] = round(e["reference"]["median_ms"] / e["new"]["median_ms"], 2)
            e["new_minus_floor_ms"] = round(e["new"]["median_ms"] - e["floor"]["median_ms"], 3)
            res[f"rows_{B}"] = e
        res["accepted"] = all(res[f"rows_{B}"]["new_max_below_reference_min"] for B in GATED)
        out["1_bootstrap_acc_batch_out_form_2_slot_0"] = res
    if 3 in parts:
        v = [spawn([me, "--worker", "circuit"], limit=400) for _ in range(3)]
        out["3_private_lut_circuit_ms_per_request"] = {
            "what": f"examples/private_lut_circuit.py, {REQUESTS} requests, one Circuit.run each (wall clock of the second pass over them, per request), three processes",
            "untuned": rnd([r["untuned_ms_per_request"] for r in v]), "tuned_acc_dispatch_1": rnd([r["tuned_ms_per_request"] for r in v])}
    if 2 in parts:
        parent = os.path.abspath(a.parent_lib)
        lines = []
        for i in range(a.bench_runs):
            for side, lib in (("parent", parent), ("this tree", None)):
                r = spawn([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], lib, limit=600)
                lines.append({"lib": side, "round": i + 1, "value": r["value"], "ms_per_step": r["ms_per_step"]})
        with open(a.bench_out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
        val = {side: [r["value"] for r in lines if r["lib"] == side] for side in ("parent", "this tree")}
        spread = max(val["parent"]) - min(val["parent"])
        out["2_bench_ab"] = {
            "command": "bench.py --gpus 1 --steps 20 --warmup 5, the parent's library and this tree's alternating", "runs_each": a.bench_runs,
            "parent_gates_per_s": rnd(val["parent"]), "parent_median": round(float(np.median(val["parent"])), 1),
            "parent_spread_pct": round(100 * spread / float(np.median(val["parent"])), 2),
            "tree_gates_per_s": rnd(val["this tree"]), "tree_median": round(float(np.median(val["this tree"])), 1),
            "medians_differ_by_less_than_parent_spread": bool(abs(float(np.median(val["this tree"])) - float(np.median(val["parent"]))) < spread)}
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
