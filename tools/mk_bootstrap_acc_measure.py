"""Measurements of the multi-key private-table rotation on the 2-party gates' kernel at mktfhe_parameters_2party (DESIGN §4.22;
profiles/mk_bootstrap_acc_measure.json, profiles/mk_bootstrap_acc_ab_parent.jsonl), tools/bootstrap_acc_measure.py's protocol:
(1) timing slot 0 (the rotation alone) at B = 1 and B = 1024 rows, out_form 2, three sides:
    a — tfhe_mk_bootstrap_acc_batch in this tree (mk_blind_rotate_kernel_w2_acc);
    b — tfhe_mk_blind_rotate_batch (steps = P n, in_form 0, sel NULL, the key loaded as selectors) in the library built from the parent
        commit, on the same rows and accumulators; side a also checks its first 8 rows against that call word for word;
    c — tfhe_mk_bootstrap_tv_batch in this tree on the same rows with the test polynomials public: the gates' own kernel;
(2) bench.py --gpus 1 --steps 20 --warmup 5 with the parent's library and with this tree's, alternating.

    python tools/mk_bootstrap_acc_measure.py --parent-lib /path/to/parent/libtfhe_mi355x.so [--runs 5] [--bench-runs 6] [--part 1,2]

One process per run and side (2 warm-up calls, then the median of 5 calls, at both sizes), the sides' processes alternating on one device,
one at a time, each under its own time limit; the first failure ends the session.  Every process makes the same keys from the same seed."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled, lut  # noqa: E402

INNER, WARM, SIZES, T = 5, 2, (1, 1024), 4
SIDES = ("a", "b", "c")


def timed(call, kernel_ms):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(INNER):
        call()
        ms.append(kernel_ms())
    return {"kernel_ms_median": float(np.median(ms)), "kernel_ms": ms}


def setup():
    """The same keys, accumulators and rows in every process: T private tables Z_4 -> Z_2 under both TLWE keys, 1024 multi-key digits."""
    p = tfhe.mktfhe_parameters_2party
    rng = np.random.default_rng(2029)
    sks = [tfhe.SecretKey(rng, p) for _ in range(2)]
    shared = tfhe.SharedKey(rng, p)
    parts = [tfhe.CloudKeyPart(rng, sk, shared, keep_tlwe_key=True) for sk in sks]
    N = p.tlwe_polynomial_degree
    polys = np.stack([lut.make_test_vector(lambda m, h=h: (m + h) & 1, 4, N, 2) for h in range(T)])
    acc = leveled.mk_tlwe_encrypt(rng, [part.tlwe_key for part in parts], p.bs_noise_stddev, polys)
    x = lut.mk_lut_encrypt(rng, sks, rng.integers(0, 4, max(SIZES)), 4)
    return tfhe.MKCloudKey(parts, expand="device"), acc, polys, x


def worker(side):
    ck, acc, polys, x = setup()
    eng = ck.engine(0)
    out = {"side": side, "sizes": {}}
    if side == "b":
        eng.mk_tgsw_load(*leveled.mk_bootstrap_key_selectors(ck))
    for B in SIZES:
        rows, idx = np.ascontiguousarray(x[:B]), (np.arange(B) % T).astype(np.int32)
        if side == "a":
            call = lambda: eng.mk_bootstrap_acc(acc, rows, acc_index=idx, out_form=2)
        elif side == "b":
            call = lambda: eng.mk_blind_rotate(acc, rows, acc_index=idx, in_form=0, out_form=2)
        else:
            call = lambda: eng.mk_bootstrap_tv(polys, rows, index=idx, with_keyswitch=True)
        run = timed(call, lambda: eng.last_timing_ms(0))
        run["kernel"] = eng.last_kernel_name()
        out["sizes"][str(B)] = run
    if side == "a":      # the first 8 rows against the any-N call on the key's selectors, word for word
        idx = (np.arange(8) % T).astype(np.int32)
        got = eng.mk_bootstrap_acc(acc, x[:8], acc_index=idx, out_form=2)
        eng.mk_tgsw_load(*leveled.mk_bootstrap_key_selectors(ck))
        out["equal_words_first_8_rows"] = bool(np.array_equal(got, eng.mk_blind_rotate(acc, x[:8], acc_index=idx, in_form=0, out_form=2)))
    ck.close()
    print(json.dumps(out))


def spawn(argv, env_lib=None, limit=300):
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
    ap.add_argument("--part", default="1,2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mk_bootstrap_acc_measure.json"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "mk_bootstrap_acc_ab_parent.jsonl"))
    ap.add_argument("--worker")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the library built from the parent commit (make -C tfhe.jl_amd/csrc in a checkout of it)")
    parent = os.path.abspath(a.parent_lib)
    parts = {int(v) for v in a.part.split(",")}
    me = os.path.abspath(__file__)
    rnd = lambda v: [round(t, 3) for t in v]
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out["what"] = "multi-key private-table rotation at mktfhe_parameters_2party (2 parties, n = 500, N = 1024, l = 4), one MI355X; times in ms"
    out["method"] = (f"one process per run and side: {WARM} warm-up calls, then the median of {INNER} calls at each size; the sides' processes alternating, "
                     "one at a time; timing slot 0 (the rotation alone)")
    if 1 in parts:
        rows = [spawn([me, "--worker", side], parent if side == "b" else None) for _ in range(a.runs) for side in SIDES]
        res = {"a": "tfhe_mk_bootstrap_acc_batch on 4 encrypted accumulators, out_form 2, this tree",
               "b": "tfhe_mk_blind_rotate_batch (steps = P n, in_form 0, sel NULL, the key as selectors) on the same rows and accumulators, the parent's library",
               "c": "tfhe_mk_bootstrap_tv_batch of the same rows with the 4 test polynomials public, this tree (the gates' own kernel)",
               "a_equals_the_any_n_call_on_the_first_8_rows": all(r["equal_words_first_8_rows"] for r in rows if r["side"] == "a")}
        for B in SIZES:
            e = {}
            for side in SIDES:
                v = [r["sizes"][str(B)]["kernel_ms_median"] for r in rows if r["side"] == side]
                e[side] = {"kernel": next(r["sizes"][str(B)]["kernel"] for r in rows if r["side"] == side), "runs_ms": rnd(v),
                           "median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            e["a_median_below_b_median"] = bool(e["a"]["median_ms"] < e["b"]["median_ms"])
            e["b_over_a"] = round(e["b"]["median_ms"] / e["a"]["median_ms"], 2)
            e["a_inside_c_min_max"] = bool(e["c"]["min_ms"] <= e["a"]["median_ms"] <= e["c"]["max_ms"])
            e["a_minus_c_ms"] = round(e["a"]["median_ms"] - e["c"]["median_ms"], 3)
            res[f"rows_{B}"] = e
        res["required_a_below_b_at_both_sizes"] = all(res[f"rows_{B}"]["a_median_below_b_median"] for B in SIZES)
        out["1_rotation_out_form_2_slot_0"] = res
    if 2 in parts:
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
    if 1 in parts and not out["1_rotation_out_form_2_slot_0"]["required_a_below_b_at_both_sizes"]:
        sys.exit("side a's median is not below side b's at both sizes")


if __name__ == "__main__":
    main()
