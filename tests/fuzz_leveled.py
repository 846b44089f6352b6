#!/usr/bin/env python3
"""Parameter-space fuzz of leveled mode (as tests/fuzz_params.py for the blind rotation; not collected by pytest — run it as
`python tests/fuzz_leveled.py [cases] [seed] [--mk]` on a GPU box): random parameter sets over everything tfhe_ctx_create accepts, each
with a random shape, against the integer schoolbook of tests/leveled_ref.py word for word (np.array_equal, no tolerance anywhere).

Single key: tgsw_load, extern_mul against Tree.extern_mul, cmux_tree against Tree.tree, cmux_net against net_ref, rot_net against
rot_net_ref, the three network-shaped calls in out_forms 0 and 1 and in out_form 2 against ks_ref (the integer keyswitch, never
eng.keyswitch), everything once more with anyn_spec = 1 (spectrum accumulators in global memory), then the known answer of
leveled_ref: trivial selectors and a table of multiples of h against evaluate_clear, no schoolbook involved.
Multi-key (--mk): mk_tgsw_load, mk_extern_mul / mk_cmux_tree / mk_cmux_net against MKTree / net_ref in the same forms (form 2 against
MKTree.keyswitch), both accumulator placements, mk_tgsw_expand_load of the uni-encryptions against mk_tgsw_load of the host expansion,
and the known answer.

The case generator is a function of the rng alone (draw_case): log2 N 1 .. 13 (weighted towards <= 10; multi-key 1 .. 11), k 1 .. 6
with k N <= 16384 (multi-key: P 2 .. 6), beta 1 .. 12, l 1 .. min(32 // beta, 16), lwe_size 1 .. 40 (multi-key 1 .. 6), any keyswitch
(t, gamma) with t gamma <= 31, one case in three forced to (8, 2) so that the MFMA and tiled keyswitch families see leveled rows
(multi-key: always (8, 2), the only pair test_mk_leveled.Setup makes keys for); S 1 .. 6 selectors, T 1 .. 3 tables, B in {1, 2, 3, 5, 9}
rows, table_index mixed or None, tree depth 1 .. 3, networks of 1 .. 4 levels of 1 .. 6 nodes over E 1 .. 6 entries and V 1 .. 4
variables with, wherever the widths allow, a copy node, a node with src0 > src1, a selector behind two variables, rows using different
selectors, and for RotNet rotations from {0, 1, N/2, N-1, N, N+1, 2N-1, uniform} mod 2N, a rotated copy and a node with src0 = src1
and rot0 != rot1.

Host budget: the schoolbook of one case makes (products) x (k+1)^2 l N^2 integer multiplications (multi-key: (3P+1) l N^2 per
product: l P + l for the party's mask, l for each other mask, l P + l for the body); a case above HOST_BUDGET = 2.5e9 (about 2 s of
np.convolve) sheds rows, then tree depth, then network levels and nodes — never N, k, l, beta — down to one product per call.  Key
generation on the host is held down the way fuzz_params.py does it, by lowering lwe_size and the keyswitch table (gamma, then t).

Inputs by exactness class, decided by SchemeParameters.exactness() (the host law; the engine's exact_domain must agree): class 2
arbitrary Int32 words with all-(2^31 - 1), all-(-2^31) and all-zero samples planted; class 1 real encryptions; class 0 only the known
answer, which is exact in Float64 at every set (leveled_ref's docstring).  No case is skipped."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HOST_BUDGET = 2.5e9
ROT_KINDS = ("0", "1", "N/2", "N-1", "N", "N+1", "2N-1", "uniform")
B_CHOICES = (1, 2, 3, 5, 9)


# ---- the case generator: a function of the rng alone -------------------------------------------------------------------------------
def _rot(rng, N):
    kind = int(rng.integers(0, len(ROT_KINDS)))
    return int([0, 1, N // 2, N - 1, N, N + 1, 2 * N - 1, int(rng.integers(0, 2 * N))][kind] % (2 * N))


def rot_kinds(rnodes, N):
    """Which of ROT_KINDS the rotations of a netlist hold, by value: a rotation that equals none of the planted values mod 2N counts as
    "uniform" (at N = 2 the planted values are all of 0 .. 3)."""
    named = {"0": 0, "1": 1, "N/2": N // 2, "N-1": N - 1, "N": N, "N+1": (N + 1) % (2 * N), "2N-1": 2 * N - 1}
    kinds = set()
    for rec in rnodes:
        for r in rec[3:]:
            hit = {name for name, v in named.items() if v == r}
            kinds |= hit or {"uniform"}
    return sorted(kinds)


def draw_shape(rng, N, rot):
    """S, T, B, table_index or None, tree depth and the public wiring of one CmuxNet (and one RotNet on the same sources if `rot`)."""
    c = {"S": int(rng.integers(1, 7)), "T": int(rng.integers(1, 4)), "B": int(rng.choice(B_CHOICES)), "index": bool(rng.integers(0, 2)),
         "depth": int(rng.integers(1, 4)), "E": int(rng.integers(1, 7)), "V": int(rng.integers(1, 5))}
    widths = [int(w) for w in rng.integers(1, 7, int(rng.integers(1, 5)))]
    nodes, below_of = [], []
    for v, w in enumerate(widths):
        below = c["E"] if v == 0 else widths[v - 1]
        for _ in range(w):
            nodes.append([int(rng.integers(0, below)), int(rng.integers(0, below)), int(rng.integers(0, c["V"]))])
            below_of.append(below)
    order = [int(i) for i in rng.permutation(len(nodes))]
    copy_at = order[0]
    nodes[copy_at][1] = nodes[copy_at][0]                                       # a copy node
    down_at = next((i for i in order[1:] if below_of[i] >= 2), None)
    if down_at is not None:                                                     # a node with src0 > src1
        nodes[down_at][0] = int(rng.integers(1, below_of[down_at]))
        nodes[down_at][1] = int(rng.integers(0, nodes[down_at][0]))
    c.update(widths=widths, nodes=nodes)
    if rot:
        rnodes = [rec + [_rot(rng, N), _rot(rng, N)] for rec in nodes]
        r = [1, N - 1, N, N + 1, 2 * N - 1][int(rng.integers(0, 5))] % (2 * N)  # never 0: N >= 2
        rnodes[copy_at][3:] = [r, r]                                            # the rotated copy
        twice_at = next((i for i in order[1:] if i != down_at), None)
        if twice_at is not None:                                                # src0 = src1 and rot0 != rot1: a true product
            rnodes[twice_at][1] = rnodes[twice_at][0]
            rnodes[twice_at][4] = int((rnodes[twice_at][3] + 1 + rng.integers(0, 2 * N - 1)) % (2 * N))
        c.update(rnodes=rnodes)
    return c


def _products(c):
    """External products the schoolbook makes for the case: B extern_mul rows, B trees, B networks (and B rotation networks)."""
    per_row = 1 + (1 << c["depth"]) - 1
    nd = np.asarray(c["nodes"])
    per_row += int(np.count_nonzero(nd[:, 0] != nd[:, 1]))
    if "rnodes" in c:
        rn = np.asarray(c["rnodes"])
        per_row += int(np.count_nonzero((rn[:, 0] != rn[:, 1]) | (rn[:, 3] != rn[:, 4])))
    return c["B"] * per_row


def host_cost(c):
    """Integer multiplications of the case's schoolbook (module docstring)."""
    per = (3 * c["P"] + 1) if c["mk"] else (c["k"] + 1) ** 2
    return _products(c) * per * c["l"] * c["N"] ** 2


def _shed(c):
    """One step of shedding host work: rows, then tree depth, then the last network level, then the last node.  False when nothing is left."""
    if c["B"] > 1:
        c["B"] = B_CHOICES[B_CHOICES.index(c["B"]) - 1]
    elif c["depth"] > 1:
        c["depth"] -= 1
    elif len(c["widths"]) > 1 or c["widths"][0] > 1:
        if c["widths"][-1] > 1 and len(c["widths"]) == 1:
            c["widths"][-1] -= 1
        else:
            c["widths"].pop()
        keep = sum(c["widths"])
        c["nodes"] = c["nodes"][:keep]
        if "rnodes" in c:
            c["rnodes"] = c["rnodes"][:keep]
    else:
        return False
    return True


def fit_host_budget(c):
    """Shed down to HOST_BUDGET, then describe the rotations of the netlist that is left (rot_kinds), not of the one first drawn."""
    while host_cost(c) > HOST_BUDGET and _shed(c):
        pass
    if "rnodes" in c:
        c["rot_kinds"] = rot_kinds(c["rnodes"], c["N"])
    return c


def draw_case(rng, mk):
    """One fuzz case as a plain dict (parameters, shape, wiring, the seed of its inputs): a function of the rng alone."""
    c = {"mk": bool(mk)}
    beta = int(rng.integers(1, 13))
    l = int(rng.integers(1, min(32 // beta, 16) + 1))
    if mk:
        P = int(rng.integers(2, 7))
        N = 1 << int(rng.integers(1, 12))
        n = int(rng.integers(1, 7))
        while n > 1 and P * n * (P - 1) * l * l * N > 20_000_000:              # (RGSW.Expand of the cloud key on the host)
            n -= 1
        c.update(P=P, N=N, k=1, l=l, beta=beta, n=n, t=8, gamma=2)
    else:
        N = 1 << int(rng.choice(list(range(1, 11)) * 2 + [11, 12, 13]))
        k = min(int(rng.integers(1, 7)), 16384 // N)
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
    c.update(draw_shape(rng, N, rot=not mk))
    if mk:
        owners = [int(o) for o in rng.integers(0, c["P"], c["S"])]
        owners[:min(c["S"], c["P"])] = [int(o) for o in rng.permutation(c["P"])[:c["S"]]]      # as many different parties as fit
        while c["S"] > 1 and c["S"] * (c["P"] - 1) * l * l * N > 20_000_000:    # (RGSW.Expand of the selectors on the host)
            c["S"] -= 1
        c["owners"] = owners[:c["S"]]
    c["seed"] = int(rng.integers(1, 2**31))
    return fit_host_budget(c)


def pinned_case(mk, *params):
    """The case of a pinned set: (N, k, l, beta) or, multi-key, (P, N, l, beta); lwe_size 6 (multi-key 4), keyswitch (8, 2), the shape drawn
    from a generator seeded by the set; at N >= 2048 one row and one product per call, so that the schoolbook stays within seconds: three
    products under a multi-key key, four under a single key, whose per-case body has four calls (extern_mul, tree, net, rot net)."""
    if mk:
        P, N, l, beta = params
        c = {"mk": True, "P": P, "N": N, "k": 1, "l": l, "beta": beta, "n": 4, "t": 8, "gamma": 2}
    else:
        N, k, l, beta = params
        c = {"mk": False, "N": N, "k": k, "l": l, "beta": beta, "n": 6, "t": 8, "gamma": 2}
    rng = np.random.default_rng([int(mk)] + [int(v) for v in params])
    c.update(draw_shape(rng, N, rot=not mk))
    if mk:
        c["owners"] = [int(o) for o in (list(rng.permutation(c["P"])) + list(rng.integers(0, c["P"], 6)))[:c["S"]]]
    c["seed"] = int(rng.integers(1, 2**31))
    if N >= 2048:
        c["B"] = 1
        while _products(c) > (3 if mk else 4) and _shed(c):
            pass
    return fit_host_budget(c)


def describe(c):
    keys = ("P", "N", "l", "beta", "n") if c["mk"] else ("N", "k", "l", "beta", "n", "t", "gamma")
    head = " ".join(f"{key}={c[key]}" for key in keys)
    return f"{head} S={c['S']} T={c['T']} B={c['B']} index={'mixed' if c['index'] else 'None'} depth={c['depth']} widths={c['widths']} E={c['E']} V={c['V']} seed={c['seed']}"


def params_of(tfhe, c):
    if c["mk"]:
        return tfhe.SchemeParameters(c["n"], 0.012467, c["N"], 1, c["l"], c["beta"], 3.29e-10, 8, 2, 2.44e-5, c["P"])
    return tfhe.SchemeParameters(c["n"], 1 / 2**15, c["N"], c["k"], c["l"], c["beta"], 9e-9, c["t"], c["gamma"], 1 / 2**15, 1)


# ---- a case's inputs and expected words: host only -----------------------------------------------------------------------------------
def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


class Inputs:
    """Keys, selectors, samples, wiring and the integer reference of one case.  Nothing here touches a device."""

    def __init__(self, tfhe, orc, c):
        self.ck = None
        try:
            self._build(tfhe, orc, c)
        except BaseException:
            self.close()                                                         # a key made before the failure is closed too
            raise

    def _build(self, tfhe, orc, c):
        from tfhe_jl_amd import leveled
        import leveled_ref as R
        self.case, self.mk = c, c["mk"]
        self.p = params_of(tfhe, c)
        self.cls = self.p.exactness()[0]
        N, l, beta, S, T, B = c["N"], c["l"], c["beta"], c["S"], c["T"], c["B"]
        self.polys = polys = (c["P"] if self.mk else c["k"]) + 1
        self.net = leveled.CmuxNet(c["widths"], c["nodes"], entries=c["E"], variables=c["V"])
        self.rnet = None if self.mk else leveled.RotNet(c["widths"], c["rnodes"], N, entries=c["E"], variables=c["V"])
        rng = self.rng = np.random.default_rng(c["seed"])
        counts = (B, T << c["depth"], T * c["E"])                                # extern_mul rows | tree tables | network tables
        if self.mk:
            self.setup = s = R.Setup(tfhe, c["P"], N, l, beta, int(rng.integers(1, 2**31)), c["owners"], n=c["n"])
            self.ck, self.tgsw, self.owners = s.ck, s.tgsw, s.owners
            self.ref = s.tree(orc, with_ks=True)
            samples = _words(rng, sum(counts), polys, N) if self.cls == 2 else s.encrypt(_words(rng, sum(counts), N))
        else:
            self.sk, self.ck = tfhe.make_key_pair(rng, self.p)
            if self.cls == 2:                                                    # exact for ANY words (test_leveled._setup)
                self.tgsw = _words(rng, S, l, polys, polys, N)
                self.tgsw[0, 0, 0, 0, :] = 2**31 - 1
                self.tgsw[1 % S, 0, 0, polys - 1, :] = -2**31
                self.tgsw[S - 1, l - 1, polys - 1, polys - 1, :] = 0
                samples = _words(rng, sum(counts), polys, N)
            else:
                self.tgsw = leveled.tgsw_encrypt_bits(rng, self.sk, rng.integers(0, 2, S))
                samples = leveled.tlwe_encrypt(rng, self.sk, _words(rng, sum(counts), N))
            self.ref = R.Tree(N, c["k"], l, beta, self.tgsw)
            self.sb = R.ks_schoolbook(self.p, self.ck.keyswitch_key)
        samples = np.ascontiguousarray(samples, np.int32)
        if self.cls == 2:
            self._plant(samples, counts)
        self.rows, self.tree_data, self.net_data = self._split(samples, counts)
        # selectors: rows differ where they can, one selector sits behind two variables
        self.rows_sel = rng.integers(0, S, B).astype(np.int32)
        self.tree_sel = rng.integers(0, S, (B, c["depth"])).astype(np.int32)
        self.net_sel = rng.integers(0, S, (B, c["V"])).astype(np.int32)
        if c["V"] >= 2:
            self.net_sel[0, 1] = self.net_sel[0, 0]
        if B >= 2 and S >= 2:
            self.net_sel[1, 0] = (self.net_sel[0, 0] + 1) % S
            self.tree_sel[1, 0] = (self.tree_sel[0, 0] + 1) % S
        self.index = None
        if c["index"]:
            self.index = rng.integers(0, T, B).astype(np.int32)
            self.index[B - 1] = T - 1
        self.table_of = [0] * B if self.index is None else [int(t) for t in self.index]

    def _split(self, samples, counts):
        c, N = self.case, self.case["N"]
        a, b = counts[0], counts[0] + counts[1]
        return (samples[:a], samples[a:b].reshape(c["T"], 1 << c["depth"], self.polys, N), samples[b:].reshape(c["T"], c["E"], self.polys, N))

    @staticmethod
    def _plant(samples, counts):
        first = 0
        for count in counts:                                                     # in every group that has room: all-max, all-min, all-zero
            for i, v in enumerate((2**31 - 1, -2**31, 0)):
                if count > i + 1:
                    samples[first + 1 + i] = v
            first += count

    def keyswitch(self, ref, ext):
        """out_form 2 of extracted rows [...][polys' N + 1], in integers."""
        import leveled_ref as R
        if not self.mk:
            return R.ks_ref(self.sb, ext)
        flat = ext.reshape(-1, ext.shape[-1])
        return np.stack([ref.keyswitch(e) for e in flat]).astype(np.int32).reshape(ext.shape[:-1] + (-1,))

    def forms(self, ref, want):
        """(samples, extracted at coefficient 0, keyswitched) of reference outputs int64 [B][F][polys][N], as int32."""
        ext = np.stack([[ref.extract(w) for w in row] for row in want]).astype(np.int32)
        return want.astype(np.int32), ext, self.keyswitch(ref, ext)

    def expected(self, ref=None, net=None, rnet=None, data=None):
        """The integer reference's words of every call of the case: {"extern_mul": [B][polys][N], "tree" / "net" / "rot": the three forms}.
        `ref`, `net`, `rnet` replace the case's own (tests/test_leveled_fuzz.py passes mutated ones), `data` = (rows, tree_data,
        net_data) the case's samples."""
        import leveled_ref as R
        ref, net, rnet = ref or self.ref, net or self.net, rnet or self.rnet
        rows, tree_data, net_data = data or (self.rows, self.tree_data, self.net_data)
        B = self.case["B"]
        want = {"extern_mul": np.stack([ref.extern_mul(rows[g], self.rows_sel[g]) for g in range(B)]).astype(np.int32)}
        tree = np.stack([ref.tree(tree_data[self.table_of[g]], self.tree_sel[g]) for g in range(B)])
        want["tree"] = tuple(w[:, 0] for w in self.forms(ref, tree[:, None]))
        want["net"] = self.forms(ref, np.stack([R.net_ref(ref, net, net_data[self.table_of[g]], self.net_sel[g]) for g in range(B)]))
        if rnet is not None:
            want["rot"] = self.forms(ref, np.stack([R.rot_net_ref(ref, rnet, net_data[self.table_of[g]], self.net_sel[g]) for g in range(B)]))
        return want

    def reference_over(self, orc, tgsw):
        """The case's integer reference over another selector set (the trivial selectors of the known answer)."""
        import leveled_ref as R
        c = self.case
        if self.mk:
            return R.MKTree(orc, c["N"], c["l"], c["beta"], c["P"], tgsw, self.owners, ks=self.ck.keyswitch_key, n=c["n"])
        return R.Tree(c["N"], c["k"], c["l"], c["beta"], tgsw)

    def known(self):
        """The known answer: trivial selectors of random bits, samples that are multiples of h = 2^(32 - l beta) (the extremes among
        them), and what evaluate_clear selects: (tgsw, rows, tree_data, net_data, {"extern_mul", "tree", "net", "rot": (samples, extracted)})."""
        import leveled_ref as R
        c, N, l, beta = self.case, self.case["N"], self.case["l"], self.case["beta"]
        rng = np.random.default_rng(c["seed"] ^ 0x5EED)
        bits = rng.integers(0, 2, c["S"])
        bits[0] = 1
        counts = (c["B"], c["T"] << c["depth"], c["T"] * c["E"])
        samples = _words(rng, sum(counts), self.polys, N)
        self._plant(samples, counts)
        rows, tree_data, net_data = self._split(R.multiples_of_h(samples, l, beta), counts)
        tgsw = R.mk_trivial_selectors(bits, c["owners"], N, l, beta, c["P"]) if self.mk else R.trivial_selectors(bits, N, c["k"], l, beta)
        B = c["B"]

        def both(rows_out):                                                      # [B][F][polys][N] -> samples and extractions
            return rows_out, np.stack([[R.extract0(w) for w in row] for row in rows_out])

        want = {"extern_mul": np.where(bits[self.rows_sel][:, None, None] == 1, rows, 0).astype(np.int32)}
        tree = np.stack([R.known_tree(tree_data[self.table_of[g]], bits[self.tree_sel[g]]) for g in range(B)])
        want["tree"] = tuple(w[:, 0] for w in both(tree[:, None]))
        want["net"] = both(np.stack([R.known_net(self.net, net_data[self.table_of[g]], bits[self.net_sel[g]]) for g in range(B)]))
        if self.rnet is not None:
            want["rot"] = both(np.stack([R.known_rot_net(self.rnet, net_data[self.table_of[g]], bits[self.net_sel[g]]) for g in range(B)]))
        return tgsw, rows, tree_data, net_data, want

    def close(self):
        if self.ck is not None:
            self.ck.close()


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), f"{what}: {int(np.count_nonzero(got != want)) if got.shape == want.shape else got.shape} words differ"


def _run_calls(eng, inp, rows, tree_data, net_data, want, forms, what):
    """Every call of the case on the loaded selector set, in both accumulator placements, against `want`."""
    c, mk = inp.case, inp.mk
    N, l = c["N"], c["l"]
    who = f"N={N},P={c['P']},l={l}" if mk else f"N={N},k={c['k']},l={l}"
    extern_mul, tree, net = (eng.mk_extern_mul, eng.mk_cmux_tree, eng.mk_cmux_net) if mk else (eng.extern_mul, eng.cmux_tree, eng.cmux_net)
    try:
        for spec in (-1, 1):
            eng.set_option("anyn_spec", spec)
            tag = f"{what}, anyn_spec {spec}"
            level = "mk_cmux_level_kernel" if mk else "cmux_level_kernel"

            def level_name():
                name = eng.last_kernel_name()
                assert name.startswith(f"{level}({who}"), name
                assert spec != 1 or name.endswith(",spec=global)"), name

            _same(extern_mul(rows, inp.rows_sel), want["extern_mul"], f"extern_mul ({tag})")
            level_name()
            for form in forms:
                _same(tree(tree_data, inp.tree_sel, table_index=inp.index, out_form=form), want["tree"][form], f"cmux_tree out_form {form} ({tag})")
                level_name()
                _same(net(net_data, inp.net, inp.net_sel, table_index=inp.index, out_form=form), want["net"][form], f"cmux_net out_form {form} ({tag})")
                name = eng.last_kernel_name()
                assert name.startswith(f"{'mk_' if mk else ''}cmux_net_level_kernel({who}"), name
                assert spec != 1 or name.endswith(",spec=global)"), name
                if not mk:
                    _same(eng.rot_net(net_data, inp.rnet, inp.net_sel, table_index=inp.index, out_form=form), want["rot"][form], f"rot_net out_form {form} ({tag})")
                    name = eng.last_kernel_name()
                    assert name.startswith(f"rot_net_level_kernel({who}"), name
                    assert spec != 1 or name.endswith(",spec=global)"), name
    finally:
        eng.set_option("anyn_spec", -1)


def run_case(tfhe, orc, c):
    """The whole per-case body on device 0; returns a short summary.  Closes the keys and the context on every path."""
    inp = Inputs(tfhe, orc, c)
    try:
        eng = inp.ck.engine(0)
        assert eng.get_option("exact_domain") == inp.cls, (eng.get_option("exact_domain"), inp.cls)
        load = (lambda tg: eng.mk_tgsw_load(tg, inp.owners)) if inp.mk else eng.tgsw_load
        if inp.cls >= 1:                                                         # word for word against the schoolbook
            want = inp.expected()
            load(inp.tgsw)
            _run_calls(eng, inp, inp.rows, inp.tree_data, inp.net_data, want, (0, 1, 2), "schoolbook")
            if inp.mk:                                                           # RGSW.Expand on the device gives the same selector set
                s = inp.setup
                got = eng.mk_tgsw_expand_load(s.pub, s.owners, *s.uni, want_expanded=True)
                _same(got, s.tgsw, "mk_tgsw_expand_load")
                _same(eng.mk_cmux_tree(inp.tree_data, inp.tree_sel, table_index=inp.index, out_form=0), want["tree"][0], "mk_cmux_tree after mk_tgsw_expand_load")
                _same(eng.mk_cmux_net(inp.net_data, inp.net, inp.net_sel, table_index=inp.index, out_form=2), want["net"][2], "mk_cmux_net after mk_tgsw_expand_load")
        tgsw, rows, tree_data, net_data, want = inp.known()                      # the known answer: every class
        load(tgsw)
        _run_calls(eng, inp, rows, tree_data, net_data, want, (0, 1), "known answer")
        return f"class {inp.cls}  {eng.last_kernel_name()}"
    finally:
        inp.close()


def main(argv):
    import tfhe_jl_amd as tfhe
    import oracle
    mk = "--mk" in argv
    args = [a for a in argv if a != "--mk"]
    cases = int(args[0]) if len(args) > 0 else 100
    seed = int(args[1]) if len(args) > 1 else 5
    rng = np.random.default_rng(seed)
    t0 = time.time()
    by_class, slowest = [0, 0, 0], (0.0, None)
    for case in range(cases):
        c = draw_case(rng, mk)
        t1 = time.time()
        try:
            summary = run_case(tfhe, oracle, c)
        except BaseException:
            print(f"case {case:4d} FAILED (fuzz seed {seed}{', --mk' if mk else ''}): {describe(c)}\n  full case: {c}", flush=True)
            raise
        dt = time.time() - t1
        by_class[int(summary.split()[1])] += 1
        if dt > slowest[0]:
            slowest = (dt, describe(c))
        print(f"case {case:4d} {describe(c)} {dt:5.2f} s  {summary}", flush=True)
    kind = "mk leveled" if mk else "leveled"
    print(f"{kind} fuzz ok: {cases} parameter sets (class 2: {by_class[2]}, class 1: {by_class[1]}, class 0, known answer only: {by_class[0]}; none skipped) "
          f"in {time.time() - t0:.1f} s; slowest case {slowest[0]:.1f} s: {slowest[1]}")


if __name__ == "__main__":
    main(sys.argv[1:])
