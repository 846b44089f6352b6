"""Measurements of tfhe_mk_blind_rotate_batch at mktfhe_parameters_2party, out_form 1 (profiles/mk_blind_rotate_measure.json),
in the manner of tools/blind_rotate_measure.py: (a) B = 1024 against tfhe_mk_bootstrap_tv_batch without keyswitch under br_anyn = 1 in
ANOTHER build of the library (the parent commit's), and against the default tuned tfhe_mk_bootstrap_tv_batch, (b) B = 1 against the
tfhe_mk_rot_net_batch chain of P n + 1 launches.

    python tools/mk_blind_rotate_measure.py --parent-lib /path/to/parent/libtfhe_mi355x.so [--runs 5] [--out profiles/mk_blind_rotate_measure.json]

One process per run (2 warm-up calls, then the median of 5 calls, HIP events), baseline and new processes alternating on one device,
one at a time, each under its own time limit; the first failure ends the session."""
import argparse
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

INNER, WARM = 5, 2


def timed(eng, call):
    for _ in range(WARM):
        call()
    ms, wall = [], []
    for _ in range(INNER):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(eng.last_timing_ms(0))
    return {"kernel_ms_median": float(np.median(ms)), "kernel_ms": ms, "wall_ms_median": float(np.median(wall)), "kernel": eng.last_kernel_name()}


def worker(mode, path):
    """base: the baseline of (a), run with TFHE_MI355X_LIB = the parent's library; new: (a) and the tuned rotation; chain: (b)."""
    d = np.load(path)
    bk, x, tv = d["bk"], d["x"], d["tv"]
    p = tfhe.mktfhe_parameters_2party
    N, n, P = p.tlwe_polynomial_degree, p.lwe_size, 2
    out = {"mode": mode, "lib": tfhe.LIB_PATH}
    eng = tfhe.Engine(p)
    if mode == "base":
        eng.set_option("br_anyn", 1)
        eng.mk_load_bootstrap_key(bk, P)
        out["base"] = timed(eng, lambda: eng.mk_bootstrap_tv(tv, x, with_keyswitch=False))
    else:
        eng.mk_load_bootstrap_key(bk, P)
        eng.mk_tgsw_load(bk.reshape((P * n,) + bk.shape[2:]), np.repeat(np.arange(P, dtype=np.int32), n))
        acc = leveled.mk_tlwe_trivial(tv, P)
    if mode == "new":
        out["new"] = timed(eng, lambda: eng.mk_blind_rotate(acc, x, in_form=0, out_form=1))
        out["tuned"] = timed(eng, lambda: eng.mk_bootstrap_tv(tv, x, with_keyswitch=False))
        out["equal_words"] = bool(np.array_equal(eng.mk_blind_rotate(acc, x[:8], in_form=0, out_form=1)[:, 0], eng.mk_bootstrap_tv(tv, x[:8], with_keyswitch=False)))
    elif mode == "chain":
        shift = 32 - N.bit_length()                                     # log2(2N) = bit_length(N): decode_message(., 2N) mod 2N
        rows = ((((x[:1].astype(np.int64) + (1 << (shift - 1))) & 0xFFFFFFFF) >> shift) & (2 * N - 1)).astype(np.int32)
        r = (2 * N - int(rows[0, P * n])) % (2 * N)
        net = leveled.RotNet([1] * (P * n + 1), [(0, 0, 0, r, r)] + [(0, 0, i, 0, int(rows[0, i])) for i in range(P * n)], N, entries=1, variables=P * n)
        sel = np.arange(P * n, dtype=np.int32)[None, :]
        out["fused_B1"] = timed(eng, lambda: eng.mk_blind_rotate(acc, rows, in_form=1, out_form=1))
        out["rot_net_chain_B1"] = timed(eng, lambda: eng.mk_rot_net(acc, net, sel, out_form=1))
        out["equal_words"] = bool(np.array_equal(eng.mk_blind_rotate(acc, rows, in_form=1, out_form=1)[:, 0], eng.mk_rot_net(acc, net, sel, out_form=1)[:, 0]))
    eng.close()
    print(json.dumps(out))


def spawn(mode, keys, lib=None):
    env = dict(os.environ)
    if lib:
        env["TFHE_MI355X_LIB"] = lib
    r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--worker", mode, "--keys", keys], env=env, capture_output=True,
                       text=True)
    if r.returncode != 0:
        sys.exit(f"worker {mode} failed rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    line = r.stdout.strip().splitlines()[-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mk_blind_rotate_measure.json"))
    ap.add_argument("--worker")
    ap.add_argument("--keys")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.keys)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent-lib: the library built from the parent commit (make -C tfhe.jl_amd/csrc in a checkout of it)")
    rng = np.random.default_rng(5)
    p = tfhe.mktfhe_parameters_2party
    sks = [tfhe.SecretKey(rng, p) for _ in range(2)]
    shared = tfhe.SharedKey(rng, p)
    bk = tfhe.MKCloudKey([tfhe.CloudKeyPart(rng, sk, shared) for sk in sks]).bootstrap_key
    x = rng.integers(-2**31, 2**31, (1024, 2 * p.lwe_size + 1), dtype=np.int64).astype(np.int32)
    tv = tfhe.make_test_vector(lambda m: (3 * m + 1) % 4, 4, p.tlwe_polynomial_degree).reshape(1, -1)
    with tempfile.TemporaryDirectory() as tmp:
        keys = os.path.join(tmp, "keys.npz")
        np.savez(keys, bk=bk.astype(np.int32), x=x, tv=tv)
        rows = []
        for _ in range(a.runs):
            rows.append(spawn("base", keys, os.path.abspath(a.parent_lib)))
            rows.append(spawn("new", keys))
        ch = spawn("chain", keys)
    base = [r["base"]["kernel_ms_median"] for r in rows if r["mode"] == "base"]
    new = [r["new"]["kernel_ms_median"] for r in rows if r["mode"] == "new"]
    tuned = [r["tuned"]["kernel_ms_median"] for r in rows if r["mode"] == "new"]
    rnd = lambda v: [round(t, 3) for t in v]
    out = {
        "what": "tfhe_mk_blind_rotate_batch at mktfhe_parameters_2party (P = 2, n = 500, N = 1024, l = 4), out_form 1, random multi-key LWE rows, one MI355X, "
                "one session; HIP-event kernel times (tfhe_last_timing_ms slot 0) in ms",
        "method": f"one process per run: 2 warm-up calls, then the median of 5 calls; baseline and new processes alternating, {a.runs} runs each; the "
                  "baseline process loads the library built from the parent commit",
        "a_B1024_vs_anyn_rotation_at_parent": {
            "baseline": "tfhe_mk_bootstrap_tv_batch without keyswitch, br_anyn = 1, parent commit's library: " + rows[0]["base"]["kernel"],
            "baseline_runs_ms": rnd(base), "baseline_median_ms": round(float(np.median(base)), 3), "baseline_spread_ms": round(max(base) - min(base), 3),
            "new": rows[1]["new"]["kernel"], "new_runs_ms": rnd(new), "new_median_ms": round(float(np.median(new)), 3),
            "new_over_baseline": round(float(np.median(new) / np.median(base)), 3), "allowed": 1.10,
            "first_8_rows_equal_words": all(r["equal_words"] for r in rows if r["mode"] == "new")},
        "a_B1024_vs_default_tuned_rotation": {
            "tuned": "tfhe_mk_bootstrap_tv_batch without keyswitch, default dispatch: " + rows[1]["tuned"]["kernel"], "tuned_runs_ms": rnd(tuned),
            "tuned_median_ms": round(float(np.median(tuned)), 3), "new_over_tuned": round(float(np.median(new) / np.median(tuned)), 2)},
        "b_B1_fused_vs_mk_rot_net_chain": {
            "fused_kernel_ms": round(ch["fused_B1"]["kernel_ms_median"], 3), "fused_wall_ms": round(ch["fused_B1"]["wall_ms_median"], 3),
            "mk_rot_net_chain": "1001 launches of mk_rot_net_level_kernel: a rotated copy, then 1000 levels of width 1",
            "chain_kernel_ms": round(ch["rot_net_chain_B1"]["kernel_ms_median"], 3), "chain_wall_ms": round(ch["rot_net_chain_B1"]["wall_ms_median"], 3),
            "chain_over_fused": round(ch["rot_net_chain_B1"]["kernel_ms_median"] / ch["fused_B1"]["kernel_ms_median"], 3), "equal_words": ch["equal_words"]},
    }
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
