"""Measurements of the multi-key level calls on the device-resident tables at mktfhe_parameters_2party (DESIGN §4.19;
profiles/mk_tlwe_levels_measure.json, profiles/mk_tlwe_levels_ab_parent.jsonl), in the manner of tools/tlwe_levels_measure.py:
(1) tfhe_mk_blind_rotate_level, B = 1024, one term per row, out_form 2, timing slot 0, against tfhe_mk_blind_rotate_batch on the same
    samples in ANOTHER build of the library (the parent commit's);
(2) the wall time of examples/multikey_private_lut_device.py's requests on the device-resident path and on the host path, with the
    selectors moved per request on each;
(3) bench.py --gpus 1 --steps 20 --warmup 5 with the parent's library and with this tree's, alternating.

    python tools/mk_tlwe_levels_measure.py --parent-lib /path/to/parent/libtfhe_mi355x.so [--runs 5] [--bench-runs 6] [--part 1,2,3]

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
sys.path.insert(0, os.path.join(ROOT, "examples"))
import tfhe_jl_amd as tfhe  # noqa: E402
from tfhe_jl_amd import leveled  # noqa: E402

INNER, WARM, B, T, PARTIES, SEED = 5, 2, 1024, 8, 2, 2028


def example():
    spec = importlib.util.spec_from_file_location("multikey_private_lut_device", os.path.join(ROOT, "examples", "multikey_private_lut_device.py"))
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


def example_inputs():
    """The example's keys and requests, the same in every process (seeded)."""
    ex = example()
    rng, params, sks, shared, parts, ck = ex.rom.setup(SEED)
    A = ex.REQUESTS * ex.ROWS
    table = rng.integers(0, 2, ex.P << ex.DEPTH).astype(bool)
    high, m, mask = rng.integers(0, 1 << ex.DEPTH, A), rng.integers(0, ex.P, A), rng.integers(0, 2, A).astype(bool)
    enc_table, uni, digits, masks = ex.request_inputs(rng, params, sks, shared, parts, table, high, m, mask)
    digit_tv = tfhe.make_test_vector(ex.digit_of, ex.P, params.tlwe_polynomial_degree)[None]
    return ex, params, ck, (enc_table, uni, digits, masks, digit_tv)


def worker(mode, path):
    """batch: (1)'s baseline, run with TFHE_MI355X_LIB = the parent's library; level: (1); host / device: the two paths of (2)."""
    out = {"mode": mode, "lib": tfhe.LIB_PATH}
    if mode in ("batch", "level"):
        d = np.load(path)
        bk, ks, x, acc = d["bk"], d["ks"], d["x"], d["acc"]
        p = tfhe.mktfhe_parameters_2party
        n, P = p.lwe_size, PARTIES
        eng = tfhe.Engine(p)
        eng.mk_load_bootstrap_key(bk, P)
        eng.mk_load_keyswitch_key(ks, P)
        eng.mk_tgsw_load(bk.reshape((P * n,) + bk.shape[2:]), np.repeat(np.arange(P, dtype=np.int32), n))
        idx = (np.arange(B) % T).astype(np.int32)
        if mode == "batch":
            out["run"] = timed(lambda: eng.mk_blind_rotate(acc, x, acc_index=idx, in_form=0, out_form=2), lambda: eng.last_timing_ms(0))
        else:
            eng.mk_tlwe_alloc(T)
            eng.mk_tlwe_upload(0, acc)
            eng.mk_wires_alloc(2 * B)
            eng.wires_upload(0, x)
            start, wire, coef, outw = np.arange(B + 1, dtype=np.int32), np.arange(B, dtype=np.int32), np.ones(B, np.int32), (B + np.arange(B)).astype(np.int32)
            out["run"] = timed(lambda: eng.mk_blind_rotate_level(idx, start, wire, coef, out_form=2, out_wires=outw), lambda: eng.last_timing_ms(0))
            out["kernel"] = eng.last_kernel_name()
            got = eng.wires_gather(outw[:8])
            out["equal_words"] = bool(np.array_equal(got, eng.mk_blind_rotate(acc, x[:8], acc_index=idx[:8], in_form=0, out_form=2)[:, 0]))
        out.setdefault("kernel", eng.last_kernel_name())
        eng.close()
    else:
        ex, params, ck, args = example_inputs()
        call = (lambda: ex.host_path(ck, *args)) if mode == "host" else (lambda: ex.device_path(ck, *args))
        out["run"] = timed(call)
        out["sha"] = hashlib.sha256(np.ascontiguousarray(call()).tobytes()).hexdigest()
        out["selectors_per_request"] = ex.selectors_moved(params)[mode]
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
    ap.add_argument("--part", default="1,2,3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mk_tlwe_levels_measure.json"))
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "mk_tlwe_levels_ab_parent.jsonl"))
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
    out["what"] = "multi-key level calls on the device-resident tables at mktfhe_parameters_2party (P = 2, n = 500, N = 1024, l = 4), one MI355X; times in ms"
    out["method"] = (f"one process per run: {WARM} warm-up calls, then the median of {INNER} calls; the two sides' processes alternating, one at a time; the "
                     "baseline processes of 1 and 3 load the library built from the parent commit")
    if 1 in parts:
        rng = np.random.default_rng(5)
        p = tfhe.mktfhe_parameters_2party
        N = p.tlwe_polynomial_degree
        sks = [tfhe.SecretKey(rng, p) for _ in range(PARTIES)]
        shared = tfhe.SharedKey(rng, p)
        cparts = [tfhe.CloudKeyPart(rng, sk, shared, keep_tlwe_key=True) for sk in sks]
        ck = tfhe.MKCloudKey(cparts)
        x = tfhe.lut.mk_lut_encrypt(rng, sks, rng.integers(0, 4, B), 4)
        tvs = np.stack([tfhe.make_test_vector(lambda m, h=h: (3 * m + h) % 4, 4, N) for h in range(T)])
        acc = tfhe.mk_tlwe_encrypt(rng, [part.tlwe_key for part in cparts], p.bs_noise_stddev, tvs)
        with tempfile.TemporaryDirectory() as tmp:
            keys = os.path.join(tmp, "keys.npz")
            np.savez(keys, bk=np.asarray(ck.bootstrap_key, np.int32), ks=np.asarray(ck.keyswitch_key, np.int32), x=x, acc=acc)
            ck.close()
            rows = []
            for _ in range(a.runs):
                rows.append(spawn([me, "--worker", "batch", "--keys", keys], parent))
                rows.append(spawn([me, "--worker", "level", "--keys", keys]))
        base = [r["run"]["kernel_ms_median"] for r in rows if r["mode"] == "batch"]
        new = [r["run"]["kernel_ms_median"] for r in rows if r["mode"] == "level"]
        out["1_mk_blind_rotate_level_B1024_out_form_2_slot_0"] = {
            "baseline": "tfhe_mk_blind_rotate_batch (mk_tlwe_rotate_kernel), in_form 0, the same 1024 multi-key LWE rows and 8 accumulators, parent commit's library",
            "baseline_runs_ms": rnd(base), "baseline_median_ms": round(float(np.median(base)), 3), "baseline_min_ms": round(min(base), 3),
            "baseline_max_ms": round(max(base), 3),
            "level": rows[1]["kernel"] + ", one term per row (coefficient 1), the rows in the multi-key wire table, the accumulators in the MK TLWE table",
            "level_runs_ms": rnd(new), "level_median_ms": round(float(np.median(new)), 3),
            "level_minus_baseline_ms": round(float(np.median(new) - np.median(base)), 3),
            "level_median_within_baseline_min_max": bool(min(base) <= float(np.median(new)) <= max(base)),
            "first_8_rows_equal_words": all(r["equal_words"] for r in rows if r["mode"] == "level")}
    if 2 in parts:
        ex = example()
        rows = []
        for _ in range(a.runs):
            rows.append(spawn([me, "--worker", "host"]))
            rows.append(spawn([me, "--worker", "device"]))
        host = [r["run"]["wall_ms_median"] for r in rows if r["mode"] == "host"]
        dev = [r["run"]["wall_ms_median"] for r in rows if r["mode"] == "device"]
        out[f"2_private_lookup_{ex.REQUESTS}_requests_of_{ex.ROWS}_wall"] = {
            "host_path": "per request: mk_bootstrap_tv of the digits, mk_two_stage_lookup (the key and the address bits expanded and uploaded as selectors, tree and "
                         "rotation through host buffers), mk_gates_batch",
            "host_runs_ms": rnd(host), "host_median_ms": round(float(np.median(host)), 3), "host_selectors_per_request": rows[0]["selectors_per_request"],
            "device_path": "tables allocated and the private table uploaded once per call; per request: two wire uploads, mk_lut_level, mk_tgsw_expand_update of "
                           "the address bits, mk_rot_net_level, mk_blind_rotate_level, mk_gates_level, one gather",
            "device_runs_ms": rnd(dev), "device_median_ms": round(float(np.median(dev)), 3), "device_selectors_per_request": rows[1]["selectors_per_request"],
            "device_minus_host_ms": round(float(np.median(dev) - np.median(host)), 3),
            "equal_words": len({r["sha"] for r in rows}) == 1}
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
