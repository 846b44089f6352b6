#!/usr/bin/env python3
"""Parameter-space fuzz of tfhe_mk_rot_net_batch (not collected by pytest — run it as `python tests/fuzz_mk_rot_net.py [cases] [seed]`
on a GPU box): the multi-key parameter sets, shapes and inputs of tests/fuzz_leveled.py (imported, not edited) with rotations added to
the netlist, against the integer schoolbook word for word (np.array_equal, no tolerance anywhere).

Per case: mk_tgsw_load, then Engine.mk_rot_net in out_forms 0, 1 and 2 against test_rot_net.rot_net_ref over the case's MKTree (form 2
against MKTree.keyswitch), once with the spectrum accumulators where the engine puts them and once with anyn_spec = 1 (global memory);
then the known answer of tests/leveled_ref.py: trivial selectors and a table of multiples of h against RotNet.evaluate_clear, no
schoolbook involved, at every exactness class.

The case generator is a function of the rng alone: fuzz_leveled.draw_case(rng, True) draws the set, the shape, the owners and the seed
of the inputs and draws no rotations for a multi-key case; add_rotations then takes them from a second generator seeded by the case's
own seed (itself a draw of the rng): fuzz_leveled._rot for both edges of every node (the planted values 0, 1, N/2, N-1, N, N+1, 2N-1
and a uniform one), a non-zero rotation on both edges of the first copy node (a rotated copy) and, where another node is free, src0 =
src1 with rot0 != rot1 (a true product).  The host budget is fuzz_leveled's, applied once more with the rotated network counted:
fit_host_budget sheds rows, tree depth, then levels and nodes of both netlists alike."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fuzz_leveled as F                                                        # noqa: E402


def add_rotations(c):
    """c["rnodes"]: the case's netlist with (rot0, rot1) on every record, drawn by a generator seeded with c["seed"] alone."""
    rng, N = np.random.default_rng([c["seed"], 0x726F74]), c["N"]
    rnodes = [list(rec) + [F._rot(rng, N), F._rot(rng, N)] for rec in c["nodes"]]
    copies = [i for i, rec in enumerate(rnodes) if rec[0] == rec[1]]
    r = [1, N - 1, N, N + 1, 2 * N - 1][int(rng.integers(0, 5))] % (2 * N)        # never 0: N >= 2
    for i in copies[1:]:                                                          # copies the shape drew by chance keep being copies
        rnodes[i][4] = rnodes[i][3]
    if copies:
        rnodes[copies[0]][3:] = [r, r]                                            # the rotated copy
    free = [i for i, rec in enumerate(rnodes) if rec[0] <= rec[1] and i not in copies]
    if free:                                                                      # src0 = src1 and rot0 != rot1: a true product
        at = free[int(rng.integers(0, len(free)))]
        rnodes[at][1] = rnodes[at][0]
        rnodes[at][4] = int((rnodes[at][3] + 1 + rng.integers(0, 2 * N - 1)) % (2 * N))
    c["rnodes"] = rnodes
    return c


def draw_case(rng):
    """One multi-key case with a rotated netlist, within the host budget: a function of the rng alone."""
    return F.fit_host_budget(add_rotations(F.draw_case(rng, True)))


def pinned_case(P, N, l, beta):
    """fuzz_leveled.pinned_case(True, ...) with rotations; at N >= 2048 at most three products in the rotated network."""
    c = add_rotations(F.pinned_case(True, P, N, l, beta))
    while N >= 2048 and _rot_products(c) > 3 and F._shed(c):
        pass
    return F.fit_host_budget(c)


def _rot_products(c):
    rn = np.asarray(c["rnodes"])
    return int(np.count_nonzero((rn[:, 0] != rn[:, 1]) | (rn[:, 3] != rn[:, 4])))


def describe(c):
    return f"{F.describe(c)} rotations={','.join(c['rot_kinds'])}"


def rot_net_of(c):
    from tfhe_jl_amd import leveled
    return leveled.RotNet(c["widths"], c["rnodes"], c["N"], entries=c["E"], variables=c["V"])


def expected(inp, rnet, ref=None, data=None):
    """The three forms of the schoolbook's rotated network over the case's inputs: int32 [B][F][...] each."""
    import leveled_ref as R
    ref, data = ref or inp.ref, inp.net_data if data is None else data
    rows = [R.rot_net_ref(ref, rnet, data[inp.table_of[g]], inp.net_sel[g]) for g in range(inp.case["B"])]
    return inp.forms(ref, np.stack(rows))


def known(inp, rnet):
    """The known answer: (trivial selectors, table, (samples, extracted)) with what RotNet.evaluate_clear selects on multiples of h."""
    import leveled_ref as R
    tgsw, _, _, net_data, _ = inp.known()
    bits = np.array([int(t.any()) for t in tgsw])
    out = np.stack([R.known_rot_net(rnet, net_data[inp.table_of[g]], bits[inp.net_sel[g]]) for g in range(inp.case["B"])])
    return tgsw, net_data, (out, np.stack([[R.extract0(w) for w in row] for row in out]))


def _run_calls(eng, inp, rnet, data, want, forms, what):
    c = inp.case
    who = f"mk_rot_net_level_kernel(N={c['N']},P={c['P']},l={c['l']}"
    names = []
    try:
        for spec in (-1, 1):
            eng.set_option("anyn_spec", spec)
            for form in forms:
                got = eng.mk_rot_net(data, rnet, inp.net_sel, table_index=inp.index, out_form=form)
                F._same(got, want[form], f"mk_rot_net out_form {form} ({what}, anyn_spec {spec})")
                name = eng.last_kernel_name()
                assert name.startswith(who), name
                assert spec != 1 or name.endswith(",spec=global)"), name
            names.append(name)
    finally:
        eng.set_option("anyn_spec", -1)
    return names                                                                 # [where the engine puts the accumulators, anyn_spec = 1]


def run_case(tfhe, orc, c):
    """The whole per-case body on device 0; returns a short summary.  Closes the keys and the context on every path."""
    inp = F.Inputs(tfhe, orc, c)
    try:
        rnet = rot_net_of(c)
        eng = inp.ck.engine(0)
        assert eng.get_option("exact_domain") == inp.cls, (eng.get_option("exact_domain"), inp.cls)
        if inp.cls >= 1:                                                         # word for word against the schoolbook
            eng.mk_tgsw_load(inp.tgsw, inp.owners)
            _run_calls(eng, inp, rnet, inp.net_data, expected(inp, rnet), (0, 1, 2), "schoolbook")
        tgsw, net_data, want = known(inp, rnet)                                  # the known answer: every class
        eng.mk_tgsw_load(tgsw, inp.owners)
        own, forced = _run_calls(eng, inp, rnet, net_data, want, (0, 1), "known answer")
        return f"class {inp.cls}  {own}" + ("" if own == forced else " and spec=global")
    finally:
        inp.close()


def main(argv):
    import tfhe_jl_amd as tfhe
    import oracle
    cases = int(argv[0]) if len(argv) > 0 else 120
    seed = int(argv[1]) if len(argv) > 1 else 7
    rng = np.random.default_rng(seed)
    t0 = time.time()
    by_class, slowest, kinds = [0, 0, 0], (0.0, None), set()
    for case in range(cases):
        c = draw_case(rng)
        t1 = time.time()
        try:
            summary = run_case(tfhe, oracle, c)
        except BaseException:
            print(f"case {case:4d} FAILED (fuzz seed {seed}): {describe(c)}\n  full case: {c}", flush=True)
            raise
        dt = time.time() - t1
        by_class[int(summary.split()[1])] += 1
        kinds |= set(c["rot_kinds"])
        if dt > slowest[0]:
            slowest = (dt, describe(c))
        print(f"case {case:4d} {describe(c)} {dt:5.2f} s  {summary}", flush=True)
    print(f"mk rot net fuzz ok: {cases} parameter sets (class 2: {by_class[2]}, class 1: {by_class[1]}, class 0, known answer only: {by_class[0]}; none skipped), "
          f"rotations {sorted(kinds)} in {time.time() - t0:.1f} s; slowest case {slowest[0]:.1f} s: {slowest[1]}")


if __name__ == "__main__":
    main(sys.argv[1:])
