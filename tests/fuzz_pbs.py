#!/usr/bin/env python3
"""Parameter-space fuzz of programmable bootstrapping and of the wire-table levels (as tests/fuzz_leveled.py for leveled mode; not
collected by pytest — run it as `python tests/fuzz_pbs.py [cases] [seed] [--mk]` on a GPU box): random parameter sets over everything
tfhe_ctx_create accepts, each with a random shape, against the integer schoolbook of tests/test_independent.py word for word
(np.array_equal on Int32 words, no tolerance anywhere).  The references are imported from the test modules that own them, nothing is
restated: Schoolbook / MKSchoolbook / schoolbook_gate (test_independent.py), expected / combine / edge_rows / edge_tables / edge_level /
closed_form (test_independent_pbs.py).  No expected word comes from the engine, from oracle/ or from a checker of tests/pbs_ref/.

Single key: bootstrap_tv and bootstrap_tv_multi at every n_out of the case, with and without keyswitch, from ONE schoolbook rotation per
row (expected()); a constant table full(mu) against bootstrap(mu); wires_alloc / wires_upload, linear_level with cst and with cst = None
against combine, lut_level at n_out = 1 and at the largest allowed n_out into output wires in a random order, one gates_level with the
opcodes of tfhe.OPCODES (MUX included) against schoolbook_gate; the call just above the n_out limit (n_out = 2 at N = 2 and 4, twice the
largest allowed n_out elsewhere) returns TFHE_ERR_INVALID_ARG naming n_out and the next valid call is still right; last_kernel_name ends
in "+tv" and last_rotation_count is the row count; where the dispatcher took the any-N kernel the TV calls run once more with
anyn_spec = 1 (spectrum accumulators in global memory).
Multi-key (--mk): mk_bootstrap_tv / mk_bootstrap_tv_multi in both forms, mk_linear_level, mk_lut_level, mk_gates_batch with all 15 opcodes
against MKSchoolbook.mk_gate, one mk_gates_level on the same operands, and — one case in three, drawn with the case — the key loaded
through mk_expand_load_bootstrap_key, the device expansion compared with the host expansion.
Every case, every class: the zero-mask closed form (closed_form of test_independent_pbs.py: a delta table on rows whose mask is zero, the
answer is one monomial): all 2N exponents where 2N <= 1024, otherwise 64 of them: -N, 1 - N, -1, 0, 1, N - 1 and a random draw.

The case generator is a function of the rng alone (draw_case).  Single key, the distribution of tests/fuzz_params.py: log2 N 1 .. 13
with its weights, k 1 .. 6 with its weights and k N <= 16384, beta 1 .. 12, l 1 .. min(32 // beta, 8), lwe_size 1 .. 40, any keyswitch
(t, gamma) with t gamma <= 31, one case in three forced to (8, 2) so that the MFMA and tiled keyswitch families see multi-output rows.
Multi-key: P 2 .. 6, log2 N 1 .. 11, k = 1, the same beta and l, lwe_size 1 .. 6, (t, gamma) as tests/fuzz_mk_params.py draws it (gamma
1 .. 4, t 1 .. min(31 // gamma, 10)).  Shape: n_tv 1 .. 8 tables, tv_index mixed or None, the n_out values {1, min(32, N / 4), one power
of two drawn between them}, 1 .. 4 random rows after the edge rows, the output wires of every level a random permutation.

Host budget.  Schoolbook.rotate makes, for each of the n mask words of a row, one extern_mul: (k + 1) decomposed polynomials times l
digits times (k + 1) key columns, each an N x N np.convolve: n (k+1)^2 l N^2 integer multiplications per rotation.  MKSchoolbook.mk_rotate
makes P n steps of mk_extern_mul: l P + l products for the party's mask, l for each of the P - 1 other masks, l P + l for the body:
P n (3P+1) l N^2.  A case makes one rotation per TV row (every n_out, both keyswitch forms and the anyn_spec re-run share it), one per
level row (both n_out share it) and one per bootstrapped gate, MUX counting twice.  A case above HOST_BUDGET = 2.5e9 (the figure of
tests/fuzz_leveled.py, about 2 s of np.convolve) sheds, in this order: the random rows, the edge rows down to a fixed core of six
(CORE_ROWS), the level rows (of the LUT level down to one, then the bootstrapped gates of the gate level down to MUX alone; the four
opcodes without a rotation stay), then lwe_size — never N, k, P, l or beta.  A set whose single rotation is still above the budget keeps
one row per call.  Key generation on the host is held down the way fuzz_params.py / fuzz_leveled.py do it (lwe_size, then the keyswitch
table).

Inputs by exactness class, decided by SchemeParameters.exactness() (the host law; the engine's exact_domain must agree).  Class 1 or 2:
the bootstrapping key comes from keygen (real in both classes), the rows are arbitrary Int32 words (edge_rows plus random rows), the
tables edge_tables, the levels edge_level (its wire indices taken modulo the wire count where there are fewer wires than it names).
Class 0: no rotation is compared; the closed form and linear_level, both exact at every set, still run.  No case is skipped."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HOST_BUDGET = 2.5e9
MU = 2**29
EDGE_ROWS = 29                      # edge_rows plants 28 rows, one more where the sample has more than two mask words
CORE_ROWS = 6                       # what shedding keeps of them: the first six of edge_order
LEVEL_ROWS = 11                     # rows of edge_level
CLOSED_FORM_WORDS = 1 << 24         # the closed form's rows go to the device in slices whose un-keyswitched result has at most this many words
FREE_GATES = ("NOT", "COPY", "CONST0", "CONST1")                                  # no rotation
ROTATING_GATES = ("MUX", "NAND", "OR", "AND", "XOR", "XNOR", "NOR", "ANDNY", "ANDYN", "ORNY", "ORYN")      # shed from the end: MUX stays


def refs():
    """(test_independent, test_independent_pbs): the modules that own the references, looked up at call time so that a test may
    replace one of their functions (tests/test_pbs_fuzz.py: the mutations)."""
    import test_independent as TI
    import test_independent_pbs as TP
    return TI, TP


# ---- the case generator: a function of the rng alone -------------------------------------------------------------------------------
def n_out_max(N):
    """The largest n_out the library takes at degree N: a power of two <= 32, and 1 or <= N / 4."""
    return max(1, min(32, N // 4))


def n_out_refused(N):
    """The call just above the limit: n_out = 2 at N = 2 and 4, twice the largest allowed n_out elsewhere."""
    return 2 * n_out_max(N)


def draw_shape(rng, N):
    top = n_out_max(N)
    mid = 1 << int(rng.integers(0, top.bit_length()))
    return {"n_tv": int(rng.integers(1, 9)), "index": bool(rng.integers(0, 2)), "n_outs": sorted({1, mid, top}), "random_rows": int(rng.integers(1, 5)),
            "edge": EDGE_ROWS, "level_rows": LEVEL_ROWS, "gates": len(ROTATING_GATES)}


def width(c):
    """Mask words of a sample: n, or P n."""
    return c["n"] * (c["P"] if c["mk"] else 1)


def edge_count(c):
    return min(c["edge"], EDGE_ROWS - 1 + (width(c) > 2))


def rows_of(c):
    return edge_count(c) + c["random_rows"]


def rotations(c):
    """Schoolbook rotations of the case: TV rows, LUT level rows, bootstrapped gates (MUX twice)."""
    return rows_of(c) + c["level_rows"] + c["gates"] + 1


def host_cost(c):
    """Integer multiplications of the case's schoolbook (module docstring)."""
    per = c["P"] * c["n"] * (3 * c["P"] + 1) if c["mk"] else c["n"] * (c["k"] + 1) ** 2
    return rotations(c) * per * c["l"] * c["N"] ** 2


def single_row(c):
    """What is left of a set whose single rotation is above the budget: one row per call (the gate level: MUX and the free opcodes)."""
    return c["random_rows"] == 0 and c["edge"] == 1 and c["level_rows"] == 1 and c["gates"] == 1 and c["n"] == 1


def _shed(c):
    """One step of shedding host work, in the order of the module docstring.  False when nothing is left."""
    if c["random_rows"] > 0:
        c["random_rows"] -= 1
    elif edge_count(c) > CORE_ROWS:
        c["edge"] = edge_count(c) - 1
    elif c["level_rows"] > 1:
        c["level_rows"] -= 1
    elif c["gates"] > 1:
        c["gates"] -= 1
    elif c["n"] > 1:
        c["n"] -= 1
    elif c["edge"] > 1:
        c["edge"] = 1
    else:
        return False
    return True


def fit_host_budget(c):
    while host_cost(c) > HOST_BUDGET and _shed(c):
        pass
    return c


def draw_case(rng, mk):
    """One fuzz case as a plain dict (parameters, shape, the seed of its inputs): a function of the rng alone."""
    c = {"mk": bool(mk)}
    if mk:
        P = int(rng.integers(2, 7))
        N = 1 << int(rng.integers(1, 12))
        beta = int(rng.integers(1, 13))
        l = int(rng.integers(1, min(32 // beta, 8) + 1))
        n = int(rng.integers(1, 7))
        gamma = int(rng.integers(1, 5))
        t = int(rng.integers(1, min(31 // gamma, 10) + 1))
        while n > 1 and (P * n * (2 * l * P + 2 * l) * N > 3_000_000 or P * n * (P - 1) * l * l * N > 20_000_000):      # (host keygen and RGSW.Expand time)
            n -= 1
        c.update(P=P, N=N, k=1, l=l, beta=beta, n=n, t=t, gamma=gamma)
    else:
        N = 1 << int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 10, 10, 10, 11, 11, 12, 13]))
        k = int(rng.choice([1, 1, 1, 2, 2, 3, 4, 5, 6]))
        if N * k > 16384:
            k = max(1, 16384 // N)
        beta = int(rng.integers(1, 13))
        l = int(rng.integers(1, min(32 // beta, 8) + 1))
        n = int(rng.integers(1, 41))
        if rng.integers(0, 3) == 0:
            t, gamma = 8, 2
        else:
            t = int(rng.integers(1, 32))
            gamma = int(rng.integers(1, 31 // t + 1))
        while n > 1 and n * l * (k + 1) ** 2 * N > 6_000_000:                  # (host keygen time, not an engine limit)
            n -= 1
        while k * N * t * ((1 << gamma) - 1) * (n + 1) > 12_000_000 and (gamma > 1 or t > 1):
            if gamma > 1 and (t, gamma) != (8, 2):
                gamma -= 1
            elif t > 1:
                t -= 1
            else:
                gamma -= 1
        c.update(N=N, k=k, l=l, beta=beta, n=n, t=t, gamma=gamma)
    c.update(draw_shape(rng, N))
    if mk:
        c["expand"] = bool(rng.integers(0, 3) == 0)
    c["seed"] = int(rng.integers(1, 2**31))
    return fit_host_budget(c)


def pinned_case(mk, *params, expand=False):
    """The case of a pinned set: (N, k, l, beta, n, t, gamma) or, multi-key, (P, N, l, beta, n, t, gamma); the shape drawn from a generator
    seeded by the set, tv_index mixed, eight tables, and every power of two up to the largest allowed n_out where there are at most
    three (so N = 8 runs n_out = 2 and N = 16 runs n_out = 4)."""
    if mk:
        P, N, l, beta, n, t, gamma = params
        c = {"mk": True, "P": P, "N": N, "k": 1, "l": l, "beta": beta, "n": n, "t": t, "gamma": gamma}
    else:
        N, k, l, beta, n, t, gamma = params
        c = {"mk": False, "N": N, "k": k, "l": l, "beta": beta, "n": n, "t": t, "gamma": gamma}
    rng = np.random.default_rng([int(mk)] + [int(v) for v in params])
    c.update(draw_shape(rng, N))
    c.update(n_tv=8, index=True)
    if n_out_max(N) <= 4:
        c["n_outs"] = [1 << i for i in range(n_out_max(N).bit_length())]
    if mk:
        c["expand"] = bool(expand)
    c["seed"] = int(rng.integers(1, 2**31))
    return fit_host_budget(c)


def describe(c):
    keys = ("P", "N", "l", "beta", "n", "t", "gamma") if c["mk"] else ("N", "k", "l", "beta", "n", "t", "gamma")
    head = " ".join(f"{key}={c[key]}" for key in keys)
    tail = " expand=device" if c.get("expand") else ""
    return (f"{head} n_tv={c['n_tv']} index={'mixed' if c['index'] else 'None'} n_outs={c['n_outs']} rows={rows_of(c)} level_rows={c['level_rows']} "
            f"gates={c['gates'] + len(FREE_GATES)} seed={c['seed']}{tail}")


def params_of(tfhe, c):
    if c["mk"]:
        return tfhe.SchemeParameters(c["n"], 0.012467, c["N"], 1, c["l"], c["beta"], 3.29e-10, c["t"], c["gamma"], 2.44e-5, c["P"])
    return tfhe.SchemeParameters(c["n"], 1 / 2**15, c["N"], c["k"], c["l"], c["beta"], 9e-9, c["t"], c["gamma"], 1 / 2**15, 1)


# ---- a case's inputs and expected words: host only -----------------------------------------------------------------------------------
def edge_order(total):
    """The edge rows of edge_rows in the order shedding keeps them: first the core — every mask word -N, one bara = +1, barb = -N, all
    zero, one bara = -1 at the last index, and the last edge row (a mask word that decodes to -1 with body 7) — then the others."""
    core = [3, 1, 2, 0, 5, total - 1]
    return core + [i for i in range(total) if i not in core]


def _index(rng, rows, n_tv, mixed):
    if not mixed:
        return None
    index = rng.integers(0, n_tv, rows).astype(np.int32)
    index[0], index[rows - 1] = 0, n_tv - 1
    return index


class Inputs:
    """Keys, rows, tables, levels, gates and the integer reference of one case.  Nothing here touches a device."""

    def __init__(self, tfhe, c):
        self.ck = None
        try:
            self._build(tfhe, c)
        except BaseException:
            self.close()
            raise

    def _build(self, tfhe, c):
        TI, TP = refs()
        self.case, self.mk = c, c["mk"]
        self.p = params_of(tfhe, c)
        self.cls = self.p.exactness()[0]
        N, n, l, beta, t, gamma = c["N"], c["n"], c["l"], c["beta"], c["t"], c["gamma"]
        rng = self.rng = np.random.default_rng(c["seed"])
        if self.mk:
            P = c["P"]
            self.sks = [tfhe.SecretKey(rng, self.p) for _ in range(P)]
            shared = tfhe.SharedKey(rng, self.p)
            self.ck = tfhe.MKCloudKey([tfhe.CloudKeyPart(rng, sk, shared) for sk in self.sks], expand="host")
            self.sb = TI.MKSchoolbook(n, N, l, beta, t, gamma, P, self.ck.bootstrap_key, self.ck.keyswitch_key) if self.cls >= 1 else None
        else:
            self.sk, self.ck = tfhe.make_key_pair(rng, self.p)
            self.sb = TI.Schoolbook(n, N, c["k"], l, beta, t, gamma, self.ck.bootstrap_key, self.ck.keyswitch_key) if self.cls >= 1 else None
        w = width(c)
        rows = TP.edge_rows(rng, w, N, c["random_rows"])
        total = len(rows) - c["random_rows"]
        assert total == EDGE_ROWS - 1 + (w > 2)
        keep = sorted(edge_order(total)[:edge_count(c)]) + list(range(total, len(rows)))
        self.x = np.ascontiguousarray(rows[keep])
        R = len(self.x)
        assert R == rows_of(c)
        self.tables = np.ascontiguousarray(TP.edge_tables(rng, N)[:c["n_tv"]])
        self.index = _index(rng, R, c["n_tv"], c["index"])
        # the level: edge_level over the rows as wires 0 .. R - 1, cut to the rows the budget left
        start, wire, coef, cst = TP.edge_level(rng, self.x, N)
        L = c["level_rows"]
        T = int(start[L])
        self.level = (np.ascontiguousarray(start[:L + 1]), np.ascontiguousarray(wire[:T] % R).astype(np.int32), np.ascontiguousarray(coef[:T]))
        self.cst = np.ascontiguousarray(cst[:L])
        self.lindex = _index(rng, L, c["n_tv"], c["index"])
        self.level_n_outs = sorted({1, n_out_max(N)})
        # the gate level: every opcode the budget left, in a random order, on random operand wires
        names = list(ROTATING_GATES[:c["gates"]]) + list(FREE_GATES)
        self.gate_names = [names[i] for i in rng.permutation(len(names))]
        G = len(names)
        self.ops = np.array([tfhe.OPCODES[nm] for nm in self.gate_names], np.uint8)
        self.ga, self.gb, self.gc = (rng.integers(0, R, G).astype(np.int32) for _ in range(3))
        # the output wires: a random permutation of what lies behind the rows
        self.out_linear = (R + rng.permutation(L)).astype(np.int32)
        first = R + L
        self.out_lut = {}
        for K in self.level_n_outs:
            self.out_lut[K] = (first + rng.permutation(L * K)).astype(np.int32)
            first += L * K
        self.out_gates = (first + rng.permutation(G)).astype(np.int32)
        self.num_wires = first + G

    def gate(self, name, x, y, z):
        TI, _ = refs()
        return self.sb.mk_gate(name, x, y, z) if self.mk else TI.schoolbook_gate(self.sb, name, x, y, z)

    def linear(self, with_cst=True):
        """The level's combinations (class-independent: integers mod 2^32)."""
        _, TP = refs()
        return TP.combine(self.x, *self.level, self.cst if with_cst else None)

    def expected(self):
        """The integer reference's words of every rotation-dependent call of the case (class >= 1): {"tv": {(n_out, ks): [R][n_out][width]},
        "linear": the level's combinations, "lut": as "tv" over them, "gates": [G][width]}."""
        _, TP = refs()
        x = self.x
        want = {"tv": TP.expected(self.sb, self.tables, self.index, x, self.case["n_outs"], mk=self.mk)}
        want["linear"] = self.linear()
        want["lut"] = TP.expected(self.sb, self.tables, self.lindex, want["linear"], self.level_n_outs, mk=self.mk)
        gates = [self.gate(nm, x[self.ga[g]], x[self.gb[g]], x[self.gc[g]]) for g, nm in enumerate(self.gate_names)]
        want["gates"] = np.stack(gates).astype(np.int32)
        return want

    def closed_exponents(self):
        """None (all 2N) where 2N <= 1024, otherwise 64 exponents: -N, 1 - N, -1, 0, 1, N - 1 and a random draw."""
        N = self.case["N"]
        if 2 * N <= 1024:
            return None
        rng = np.random.default_rng(self.case["seed"] ^ 0xC105ED)
        planted = [-N, 1 - N, -1, 0, 1, N - 1]
        drawn = [int(e) for e in rng.permutation(np.arange(2 - N, N - 1))[:64] if int(e) not in (-1, 0, 1)]
        return tuple(planted + drawn[:64 - len(planted)])

    def close(self):
        if self.ck is not None:
            self.ck.close()


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: {int(np.count_nonzero(got != want)) if got.shape == want.shape else got.shape} words differ"


def _engine(tfhe, inp):
    """The engine of the case on device 0.  A multi-key case drawn with expand = device loads its key through RGSW.Expand on the device
    and compares the expansion with the host's."""
    c = inp.case
    if not (inp.mk and c["expand"]):
        return inp.ck.engine(0), None
    eng = tfhe.Engine(inp.p, 0)
    try:
        expanded = eng.mk_expand_load_bootstrap_key(c["P"], *inp.ck._part_arrays(), want_expanded=True)
        _same(expanded.reshape(inp.ck.bootstrap_key.shape), inp.ck.bootstrap_key, "mk_expand_load_bootstrap_key against the host expansion")
        eng.mk_load_keyswitch_key(inp.ck.keyswitch_key, c["P"])
    except BaseException:
        eng.close()
        raise
    return eng, eng


def _run_closed_form(eng, inp):
    """Delta table, zero masks: the un-keyswitched bodies of every TV entry point, and the levels' wires (the keyswitch of a zero mask
    subtracts nothing, keyswitch.jl:66-68: the wire is (0, body))."""
    _, TP = refs()
    c, mk = inp.case, inp.mk
    N, w = c["N"], width(c)
    exps = inp.closed_exponents()
    one, multi, lut, alloc = ((eng.mk_bootstrap_tv, eng.mk_bootstrap_tv_multi, eng.mk_lut_level, eng.mk_wires_alloc) if mk else
                              (eng.bootstrap_tv, eng.bootstrap_tv_multi, eng.lut_level, eng.wires_alloc))
    for K in c["n_outs"]:
        v, body, want = TP.closed_form(N, K, exps)
        E = len(body)
        assert want.any()
        x = np.zeros((E, w + 1), np.int32)
        x[:, w] = body
        step = max(1, CLOSED_FORM_WORDS // (K * ((c["P"] if mk else c["k"]) * N + 1)))         # rows per call: the un-keyswitched result stays below 64 MB

        def check(got, what, first=0):
            assert got.shape[1] == K and not got[:, :, :-1].any(), f"closed form, {what}, n_out {K}: a mask word is not zero"
            _same(got[:, :, -1], want[first:first + len(got)], f"closed form, {what}, n_out {K}")

        for first in range(0, E, step):
            rows = x[first:first + step]
            if K == 1:
                check(one(v, rows, with_keyswitch=False)[:, None], "bootstrap_tv", first)
            for ks in (False, True):
                check(multi(v, rows, K, with_keyswitch=ks), f"bootstrap_tv_multi keyswitch {ks}", first)
        if K in inp.level_n_outs:
            alloc(E * K)
            lut(v, np.zeros(E + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), body, np.arange(E * K, dtype=np.int32), n_out=K)
            check(eng.wires_download(0, E * K).reshape(E, K, -1), "lut_level")


def _run_tv(eng, inp, want, what):
    """bootstrap_tv and bootstrap_tv_multi at every n_out, with and without keyswitch; returns the kernel names seen."""
    c, mk = inp.case, inp.mk
    one, multi = (eng.mk_bootstrap_tv, eng.mk_bootstrap_tv_multi) if mk else (eng.bootstrap_tv, eng.bootstrap_tv_multi)
    R, names = len(inp.x), set()
    for ks in (False, True):
        got = one(inp.tables, inp.x, index=inp.index, with_keyswitch=ks)
        names.add(eng.last_kernel_name())
        assert eng.last_rotation_count() == R, (eng.last_rotation_count(), R)
        _same(got, want[1, ks][:, 0], f"bootstrap_tv keyswitch {ks} ({what})")
        for K in c["n_outs"]:
            got = multi(inp.tables, inp.x, K, index=inp.index, with_keyswitch=ks)
            names.add(eng.last_kernel_name())
            assert eng.last_rotation_count() == R, (eng.last_rotation_count(), R)
            _same(got, want[K, ks], f"bootstrap_tv_multi n_out {K} keyswitch {ks} ({what})")
    assert all(name.endswith("+tv") for name in names), names
    return names


def _run_linear(eng, inp):
    """wires_alloc, wires_upload, linear_level with cst and with cst = None (every class: integers mod 2^32)."""
    linear = eng.mk_linear_level if inp.mk else eng.linear_level
    (eng.mk_wires_alloc if inp.mk else eng.wires_alloc)(inp.num_wires)
    eng.wires_upload(0, inp.x)
    linear(*inp.level, inp.cst, inp.out_linear)
    _same(eng.wires_gather(inp.out_linear), inp.linear(), "linear_level")
    linear(*inp.level, None, inp.out_linear)
    _same(eng.wires_gather(inp.out_linear), inp.linear(with_cst=False), "linear_level, cst = None")
    _same(eng.wires_download(0, len(inp.x)), inp.x, "the input wires after linear_level")


def _run_levels(tfhe, eng, inp, want):
    """lut_level at n_out 1 and the largest allowed into permuted output wires, the refused n_out, one gates_level (multi-key: the gate
    batch and one level on the same operands)."""
    c, mk = inp.case, inp.mk
    L, R = c["level_rows"], len(inp.x)
    lut = eng.mk_lut_level if mk else eng.lut_level

    def lut_at(K):
        lut(inp.tables, *inp.level, inp.cst, inp.out_lut[K], index=inp.lindex, n_out=K)
        assert eng.last_rotation_count() == L and eng.last_kernel_name().endswith("+tv"), (eng.last_rotation_count(), eng.last_kernel_name())
        _same(eng.wires_gather(inp.out_lut[K]).reshape(L, K, -1), want["lut"][K, True], f"lut_level n_out {K}")

    for K in inp.level_n_outs:
        lut_at(K)
    # just above the limit: refused with a message that names n_out, nothing disturbed
    bad = n_out_refused(c["N"])
    multi = eng.mk_bootstrap_tv_multi if mk else eng.bootstrap_tv_multi
    for call in (lambda: multi(inp.tables, inp.x, bad, index=inp.index), lambda: lut(inp.tables, *inp.level, inp.cst, np.arange(R, R + L * bad, dtype=np.int32), index=inp.lindex, n_out=bad)):
        try:
            call()
        except tfhe.EngineError as e:
            assert e.code == 1 and "n_out" in str(e), str(e)                     # TFHE_ERR_INVALID_ARG
        else:
            raise AssertionError(f"n_out = {bad} at N = {c['N']} was not refused")
    top = inp.level_n_outs[-1]
    _same(multi(inp.tables, inp.x, top, index=inp.index), want["tv"][top, True], f"bootstrap_tv_multi n_out {top} after the refused call")
    lut_at(top)
    _same(eng.wires_download(0, R), inp.x, "the input wires after lut_level")
    # gates
    rot = sum(2 if nm == "MUX" else 0 if nm in FREE_GATES else 1 for nm in inp.gate_names)
    if mk:
        got = eng.mk_gates_batch(inp.ops, inp.x[inp.ga], inp.x[inp.gb], inp.x[inp.gc])
        assert eng.last_rotation_count() == rot, (eng.last_rotation_count(), rot)
        for g, nm in enumerate(inp.gate_names):
            _same(got[g], want["gates"][g], f"mk_gates_batch {nm} (gate {g})")
    (eng.mk_gates_level if mk else eng.gates_level)(inp.ops, inp.ga, inp.gb, inp.gc, inp.out_gates)
    assert eng.last_rotation_count() == rot, (eng.last_rotation_count(), rot)
    got = eng.wires_gather(inp.out_gates)
    for g, nm in enumerate(inp.gate_names):
        _same(got[g], want["gates"][g], f"gates_level {nm} (gate {g})")


def run_case(tfhe, orc, c):
    """The whole per-case body on device 0; returns a short summary.  Closes the keys and the context on every path.  (`orc` is not
    used, every expected word is the schoolbook's: the argument keeps the signature of fuzz_leveled.run_case.)"""
    inp = Inputs(tfhe, c)
    own = None
    try:
        eng, own = _engine(tfhe, inp)
        assert eng.get_option("exact_domain") == inp.cls, (eng.get_option("exact_domain"), inp.cls)
        _run_closed_form(eng, inp)
        _run_linear(eng, inp)
        name = eng.last_kernel_name()
        if inp.cls >= 1:                                                         # word for word against the schoolbook
            want = inp.expected()
            names = _run_tv(eng, inp, want["tv"], "schoolbook")
            name = sorted(names)[0]
            if not inp.mk:                                                       # a constant table is the mu bootstrap
                for ks in (False, True):
                    full = np.full((1, c["N"]), MU, np.int32)
                    _same(eng.bootstrap_tv(full, inp.x, with_keyswitch=ks), eng.bootstrap(MU, inp.x, with_keyswitch=ks), f"full(mu) against bootstrap(mu), keyswitch {ks}")
            _run_levels(tfhe, eng, inp, want)
            if any("anyn" in nm for nm in names):                                # spectrum accumulators in global memory
                eng.set_option("anyn_spec", 1)
                try:
                    again = _run_tv(eng, inp, want["tv"], "schoolbook, anyn_spec 1")
                    assert all("spec=global" in nm for nm in again), again
                finally:
                    eng.set_option("anyn_spec", -1)
        return f"class {inp.cls}  {name}"
    finally:
        if own is not None:
            own.close()
        inp.close()


def main(argv):
    import tfhe_jl_amd as tfhe
    mk = "--mk" in argv
    args = [a for a in argv if a != "--mk"]
    cases = int(args[0]) if len(args) > 0 else 100
    seed = int(args[1]) if len(args) > 1 else 5
    rng = np.random.default_rng(seed)
    t0 = time.time()
    by_class, slowest = [0, 0, 0], []
    for case in range(cases):
        c = draw_case(rng, mk)
        t1 = time.time()
        try:
            summary = run_case(tfhe, None, c)
        except BaseException:
            print(f"case {case:4d} FAILED (fuzz seed {seed}{', --mk' if mk else ''}): {describe(c)}\n  full case: {c}", flush=True)
            raise
        dt = time.time() - t1
        by_class[int(summary.split()[1])] += 1
        slowest = sorted(slowest + [(dt, describe(c))], reverse=True)[:3]
        print(f"case {case:4d} {describe(c)} {dt:5.2f} s  {summary}", flush=True)
    kind = "mk pbs" if mk else "pbs"
    print(f"{kind} fuzz ok: {cases} parameter sets (class 2: {by_class[2]}, class 1: {by_class[1]}, class 0, closed form and linear level only: {by_class[0]}; none skipped) "
          f"in {time.time() - t0:.1f} s; slowest cases: " + "; ".join(f"{dt:.1f} s: {d}" for dt, d in slowest))


if __name__ == "__main__":
    main(sys.argv[1:])
