"""The device-resident wire table under random programs: program generator, host model and replica simulator (host only, no GPU).

A program is a seeded list of steps over a table of W wires (W = 24 ... 64, so that wires are rewritten often):

    alloc(W)          tfhe_wires_alloc / tfhe_mk_wires_alloc, also in the middle of a program with another W (always followed by an
                      upload of the whole table: a fresh table holds nothing a program may read)
    upload            tfhe_wires_upload of a partial range
    gates             tfhe_gates_level: outputs are random distinct wires of the WHOLE table, operands any wires the level does not write;
                      shapes: one, two, three gates, trivial gates only (NOT / COPY / CONST), every MUX at the head with trivial gates behind,
                      the mirror image, random mixes of all 15 opcodes
    linear            tfhe_linear_level: rows of 0 ... 4 terms, small and wrapping coefficients, cst or NULL
    lut               tfhe_lut_level: n_out in {1, 2, 4}, three tables, tv_index or NULL, rows of several terms
    download, gather  reads: a range / any indices in any order with duplicates; every read yields the words the engine must return
    option            level_split_min in {1, 2, 8, 4096}, level_exchange in {0, 1, 2}
    refused           a level the engine must refuse and that leaves the table as it was: reads its own output (gates), writes a wire
                      twice (linear), an index out of range (lut), a decreasing term_start (linear); in multi-key programs also the
                      single-key call on the multi-key table and the multi-key call on a table from tfhe_wires_alloc (wrong_call)

`Model` holds ONE numpy table and applies each step with reference arithmetic (`Arith`: Oracle.gates / MKGateRef for gate levels,
`combine` for linear levels, `combine` then the schoolbook's bootstrap_tv (`expected`) for LUT levels).

`Replicas` follows the protocol of csrc/engine_circuits.hip on nk copies of the table: valid[k][w], owner[w]; a level is cut by
`shard_bounds` (the mirror of shard_bounds_by_rotations: a gate weighs 1000 rotations + 1) from level_split_min rotations on, an integer
level into B r / nk from level_split_min rows on; every shard pulls what is not valid on its replica from the owner (all pulls before
any shard), computes from its OWN replica and becomes the owner of what it wrote; uploads reach every replica; download / gather pull to
replica 0.  It counts the events a program reaches (EVENTS) and emulates one protocol fault at a time (FAULTS).

upload_owner: with every replica written by an upload, wire_owner is consulted only for rows that are not valid somewhere, and only a
later rewrite (which sets the owner) makes a row so: leaving the owner alone is invisible under that protocol, on any program.  The fault
is therefore emulated in the form in which the owner matters - the rows reach the first replica only, the others are marked stale and
fetch from the recorded owner, which the upload did not reset: a device that owned the wire keeps serving (and reading) its old value."""
import collections

import numpy as np

from test_mk_gates import OPS

ERR_INVALID, ERR_STATE = 1, 5
NAMES = list(OPS)
TRIVIAL = tuple(OPS[nm] for nm in ("NOT", "COPY", "CONST0", "CONST1"))
MUX = OPS["MUX"]
SPLIT_MINS, EXCHANGES, N_OUTS, N_TV = (1, 2, 8, 4096), (0, 1, 2), (1, 2, 4), 3
SHAPES = ("one", "two", "three", "trivial", "mux_head", "mux_tail", "random", "random")
REFUSALS = ("reads_own", "writes_twice", "out_of_range", "dec_start")
LEVELS = ("gates", "linear", "lut")
READS = ("download", "gather")

EVENTS = ("pull_from_dev0", "pull_from_dev1", "pull_from_dev2", "read_of_shared_then_rewritten", "upload_over_foreign_owner", "dup_in_pull_list",
          "zero_gate_shard", "two_sources_in_one_pull", "five_transfers_one_pair", "split_multi_output_lut", "nine_levels_queued",
          "read_after_refused")
FAULTS = ("stale_valid", "upload_owner", "pull_from_0", "dup_skip", "tv_index_base", "cst_base", "out_stride", "term_start_base",
          "refused_writes_first", "download_no_pull")


class Step(dict):
    __getattr__ = dict.__getitem__


def has_a(op):
    return op not in (OPS["CONST0"], OPS["CONST1"])


def has_b(op):
    return has_a(op) and op not in (OPS["NOT"], OPS["COPY"])


def rotations(ops):
    return int(sum(2 if op == MUX else 1 if has_b(op) else 0 for op in ops))


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
def _words(rng, rows, width):
    return rng.integers(-2**31, 2**31, size=(rows, width), dtype=np.int64).astype(np.int32)


class Generator:
    """The steps of a program, drawn from `rng` for the table of self.W wires; gate shapes and refusals are taken in turn."""

    def __init__(self, rng, width, mk=False, sk_width=None, W=0):
        self.rng, self.width, self.mk, self.sk_width, self.W = rng, width, mk, sk_width, W
        self.shape_at, self.refusal_at = int(rng.integers(0, len(SHAPES))), int(rng.integers(0, len(REFUSALS)))

    def alloc(self, rows=None):
        rng = self.rng
        W = int(rng.integers(24, 65))
        while W == self.W:
            W = int(rng.integers(24, 65))
        self.W = W
        rows = rows or ("mk" if self.mk else "sk")
        width = self.width if rows == "mk" or not self.mk else self.sk_width
        return [Step(kind="alloc", W=W, rows=rows, width=width), Step(kind="upload", first=0, data=_words(rng, W, width))]

    def upload(self):
        first = int(self.rng.integers(0, self.W - 1))
        count = int(self.rng.integers(1, min(12, self.W - first) + 1))
        return Step(kind="upload", first=first, data=_words(self.rng, count, self.width))

    def _outs(self, count):
        out = self.rng.choice(self.W, count, replace=False).astype(np.int32)
        return out, np.setdiff1d(np.arange(self.W, dtype=np.int32), out)

    def gates(self, shape=None, max_gates=12):
        rng = self.rng
        if shape is None:
            shape = SHAPES[self.shape_at % len(SHAPES)]
            self.shape_at += 1
        B = {"one": 1, "two": 2, "three": 3}.get(shape) or int(rng.integers(4, max_gates + 1))
        if shape == "trivial":
            ops = rng.choice(TRIVIAL, B)
        elif shape in ("mux_head", "mux_tail"):
            m = int(rng.integers(1, B - 1))
            ops = np.concatenate([np.full(m, MUX), rng.choice(TRIVIAL, B - m)])
            ops = ops[::-1] if shape == "mux_tail" else ops
        else:
            ops = rng.integers(0, len(NAMES), B)
        out, pool = self._outs(B)
        a, b, c = (rng.choice(pool, B).astype(np.int32) for _ in range(3))
        return Step(kind="gates", shape=shape, B=B, ops=np.ascontiguousarray(ops, np.uint8), a=a, b=b, c=c, out=out)

    def _terms(self, B, pool, several):
        rng = self.rng
        counts = rng.integers(0, 5, B)
        if several:
            counts[int(rng.integers(0, B))] = 4
        else:
            counts[int(rng.integers(0, B))] = 0                                   # a row with no terms: the trivial sample (0, cst)
        start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        T = int(start[-1])
        wire = rng.choice(pool, T).astype(np.int32)
        coef = np.where(rng.random(T) < 0.5, rng.integers(-3, 4, T), rng.integers(-2**31, 2**31, T)).astype(np.int32)      # half of them wrap
        return start, wire, coef

    def linear(self):
        rng = self.rng
        B = int(rng.integers(1, 11))
        out, pool = self._outs(B)
        start, wire, coef = self._terms(B, pool, False)
        cst = None if rng.random() < 0.25 else _words(rng, 1, B)[0]
        return Step(kind="linear", B=B, n_out=1, start=start, wire=wire, coef=coef, cst=cst, out=out, index=None)

    def lut(self, tables):
        rng = self.rng
        K = int(rng.choice(N_OUTS))
        B = int(rng.integers(1, min(8, (self.W - 4) // K) + 1))
        out, pool = self._outs(B * K)
        start, wire, coef = self._terms(B, pool, True)
        cst = None if rng.random() < 0.2 else _words(rng, 1, B)[0]
        index = None if rng.random() < 0.2 else rng.integers(0, N_TV, B).astype(np.int32)
        return Step(kind="lut", B=B, n_out=K, tables=tables, start=start, wire=wire, coef=coef, cst=cst, out=out, index=index)

    def refused(self, tables):
        """The first gate / row of a refused level is itself a valid one (what refused_writes_first writes)."""
        rng = self.rng
        why = REFUSALS[self.refusal_at % len(REFUSALS)]
        self.refusal_at += 1
        if why == "reads_own":
            lv = self.gates("random")
            lv.ops[-1] = OPS["NAND"]
            lv.a[-1] = lv.out[0]
        elif why == "writes_twice":
            lv = self.linear()
            while lv.B < 2:
                lv = self.linear()
            lv.out[-1] = lv.out[0]
        elif why == "out_of_range":
            lv = self.lut(tables)
            while lv.start[-1] == lv.start[1]:                                    # a term after row 0
                lv = self.lut(tables)
            lv.wire[-1] = self.W
        else:
            lv = self.linear()
            while lv.B < 3 or lv.start[2] <= lv.start[1] or lv.start[1] == 0:
                lv = self.linear()
            lv.start[2] = lv.start[1] - 1
        return Step(kind="refused", why=why, level=lv, call=("mk_" if self.mk else "") + lv.kind, code=ERR_INVALID)


def make_program(seed, steps, width, N, mk=False, sk_width=None):
    """`steps` steps (the closing gather of the whole table included); width: words per row; mk: a multi-key program (no options, the two
    wrong_call refusals in the middle, sk_width = n + 1 for the table from tfhe_wires_alloc)."""
    rng = np.random.default_rng(seed)
    g = Generator(rng, width, mk, sk_width)
    tables = _words(rng, N_TV, N)
    prog = g.alloc()
    if not mk:
        prog.append(Step(kind="option", split_min=int(rng.choice(SPLIT_MINS[:3])), exchange=int(rng.choice(EXCHANGES))))
    kinds = ["gates", "linear", "lut", "upload", "download", "gather", "option", "refused", "alloc"]
    weight = np.array([0.30, 0.12, 0.20, 0.07, 0.05, 0.08, 0.0 if mk else 0.07, 0.08, 0.03])
    wrong = {steps // 3: "sk_call", 2 * steps // 3: "sk_table"} if mk else {}
    while len(prog) < steps - 1:
        todo = wrong.pop(min(wrong), None) if wrong and len(prog) >= min(wrong) else None
        if todo == "sk_call":                                                     # tfhe_gates_level on the multi-key table
            prog.append(Step(kind="refused", why="wrong_call", level=g.gates("random"), call="gates", code=ERR_STATE))
            continue
        if todo == "sk_table":                                                    # tfhe_mk_gates_level on a table from tfhe_wires_alloc
            g.width, keep = sk_width, g.width
            prog += g.alloc("sk")
            prog.append(Step(kind="refused", why="wrong_call", level=g.gates("random"), call="mk_gates", code=ERR_STATE))
            prog.append(Step(kind="gather", wires=np.arange(g.W, dtype=np.int32)))
            g.width = keep
            prog += g.alloc("mk")
            continue
        kind = kinds[int(rng.choice(len(kinds), p=weight / weight.sum()))]
        if kind == "alloc":
            prog += g.alloc()
        elif kind == "upload":
            prog.append(g.upload())
        elif kind == "gates":
            prog.append(g.gates())
        elif kind == "linear":
            prog.append(g.linear())
        elif kind == "lut":
            prog.append(g.lut(tables))
        elif kind == "download":
            first = int(rng.integers(0, g.W - 1))
            prog.append(Step(kind="download", first=first, count=int(rng.integers(1, g.W - first + 1))))
        elif kind == "gather":
            prog.append(Step(kind="gather", wires=rng.integers(0, g.W, int(rng.integers(1, 2 * g.W))).astype(np.int32)))      # any order, duplicates
        elif kind == "option":
            prog.append(Step(kind="option", split_min=int(rng.choice(SPLIT_MINS)), exchange=int(rng.choice(EXCHANGES))))
        else:
            prog.append(g.refused(tables))
    prog.append(Step(kind="gather", wires=np.arange(g.W, dtype=np.int32)))
    return prog


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------
class Arith:
    """Reference arithmetic with a memo per gate / LUT row (a function of the operand words alone), so that the replica simulator costs
    nothing where it computes what the model computed.  gates_fn(ops, x, y, z) -> [B][w]; lut_fn(tables, index, x, n_out) -> [B][n_out][w]."""

    def __init__(self, gates_fn, lut_fn):
        self.gates_fn, self.lut_fn, self.memo = gates_fn, lut_fn, {}

    def gates(self, ops, x, y, z):
        x, y, z = x.copy(), y.copy(), z.copy()
        for g, op in enumerate(ops):                                              # operands an opcode does not read do not enter the key
            if not has_a(op):
                x[g] = 0
            if not has_b(op):
                y[g] = 0
            if op != MUX:
                z[g] = 0
        keys = [(int(op), x[g].tobytes(), y[g].tobytes(), z[g].tobytes()) for g, op in enumerate(ops)]
        miss = [g for g, k in enumerate(keys) if k not in self.memo]
        if miss:
            rows = self.gates_fn(np.ascontiguousarray(ops[miss], np.uint8), x[miss], y[miss], z[miss])
            for g, r in zip(miss, rows):
                self.memo[keys[g]] = np.array(r, np.int32)
        return np.stack([self.memo[k] for k in keys])

    def lut(self, tables, index, x, n_out):
        idx = np.zeros(len(x), np.int32) if index is None else index
        keys = [(tables[idx[g]].tobytes(), x[g].tobytes(), n_out) for g in range(len(x))]
        miss = [g for g, k in enumerate(keys) if k not in self.memo]
        if miss:
            rows = self.lut_fn(tables, idx[miss], x[miss], n_out)
            for g, r in zip(miss, rows):
                self.memo[keys[g]] = np.array(r, np.int32)
        return np.stack([self.memo[k] for k in keys])


def single_key_arith(oracle, sb):
    from test_independent_pbs import expected
    return Arith(lambda ops, x, y, z: oracle.gates(ops, x, y, z, nthreads=8),
                 lambda tables, index, x, K: expected(sb, tables, index, x, (K,))[K, True])


def multi_key_arith(gate_ref, msb):
    from test_independent_pbs import expected
    return Arith(gate_ref.batch, lambda tables, index, x, K: expected(msb, tables, index, x, (K,), mk=True)[K, True])


def run_level(arith, table, lv, g0, g1, fault=None):
    """Gates / rows [g0, g1) of the level computed from `table`, as the device that gets this shard computes them (the arrays re-based to
    the shard's first row; `fault` leaves one of them as it was): (output wires, rows)."""
    from test_independent_pbs import combine
    cnt = g1 - g0
    if lv.kind == "gates":
        ops = lv.ops[g0:g1]
        return lv.out[g0:g1], arith.gates(ops, table[lv.a[g0:g1]], table[lv.b[g0:g1]], table[lv.c[g0:g1]])
    K, T = lv.n_out, len(lv.wire)
    base = int(lv.start[g0])
    start = lv.start[g0:g1 + 1].astype(np.int64) - (0 if fault == "term_start_base" else base)
    at = (base + np.arange(int(start[0]), max(int(start[-1]), int(start[0])))) % max(T, 1)      # (past the end only under term_start_base)
    wire, coef = lv.wire[at], lv.coef[at]
    cst = None if lv.cst is None else lv.cst[:cnt] if fault == "cst_base" else lv.cst[g0:g1]
    index = None if lv.index is None else lv.index[:cnt] if fault == "tv_index_base" else lv.index[g0:g1]
    o0 = g0 if fault == "out_stride" else g0 * K
    x = combine(table, start - start[0], wire, coef, cst) if cnt else np.zeros((0, table.shape[1]), np.int32)
    rows = x if lv.kind == "linear" else arith.lut(lv.tables, index, x, K).reshape(cnt * K, -1)
    return lv.out[o0:o0 + cnt * K], rows


def read_of(table, s):
    return table[s.first:s.first + s.count].copy() if s.kind == "download" else table[s.wires].copy()


class Model:
    """One table; run(program) -> per step (the words a read must return or None, the whole table after the step)."""

    def __init__(self, arith):
        self.arith = arith

    def run(self, prog):
        table, res = None, []
        for s in prog:
            read = None
            if s.kind == "alloc":
                table = np.zeros((s.W, s.width), np.int32)
            elif s.kind == "upload":
                table[s.first:s.first + len(s.data)] = s.data
            elif s.kind in LEVELS:
                wires, rows = run_level(self.arith, table, s, 0, s.B)
                table[wires] = rows
            elif s.kind in READS:
                read = read_of(table, s)
            res.append((read, table.copy()))                                      # (option, refused: the table as it was)
        return res


# ---- sharding ---------------------------------------------------------------------------------------------------------------------------
def shard_bounds(ops, nk):
    """shard_bounds_by_rotations of csrc/engine_context.hip: bounds[r] = the smallest g with weight(gates before g) nk >= total r."""
    cost = [1000 * (2 if op == MUX else 1 if has_b(op) else 0) + 1 for op in ops]
    total, bounds, cum, g = sum(cost), [0], 0, 0
    for r in range(1, nk):
        while g < len(cost) and cum * nk < total * r:
            cum += cost[g]
            g += 1
        bounds.append(g)
    return bounds + [len(cost)]


def is_split(lv, nk, split_min):
    size = rotations(lv.ops) if lv.kind == "gates" else lv.B
    return nk > 1 and split_min >= 0 and size >= split_min


def plan(lv, nk, split_min):
    """bounds [nk + 1] of the level's shards on nk devices."""
    if not is_split(lv, nk, split_min):
        return [0] + [lv.B] * nk
    return shard_bounds(lv.ops, nk) if lv.kind == "gates" else [lv.B * r // nk for r in range(nk + 1)]


def device_count(lv, nk, split_min):
    b = plan(lv, nk, split_min)
    return sum(b[r + 1] > b[r] for r in range(nk))


def reads_of(lv, g0, g1):
    """The wires the shard's device pulls before the level (multi_gates_level / multi_int_level)."""
    if lv.kind != "gates":
        return [int(w) for w in lv.wire[lv.start[g0]:lv.start[g1]]]
    r = []
    for g in range(g0, g1):
        op = lv.ops[g]
        r += ([int(lv.a[g])] if has_a(op) else []) + ([int(lv.b[g])] if has_b(op) else []) + ([int(lv.c[g])] if op == MUX else [])
    return r


# ---- the replica simulator ------------------------------------------------------------------------------------------------------------------
class Replicas:
    def __init__(self, arith, nk, fault=None, split_min=4096):
        assert fault is None or fault in FAULTS
        self.arith, self.nk, self.fault, self.split_min = arith, nk, fault, split_min
        self.events = collections.Counter()
        self.counts = {}                                                          # step -> devices the level ran on

    def _pull(self, dst, wires):
        valid, ev = self.valid[dst], self.events
        need = [w for w in wires if not valid[w]]
        if len(set(need)) < len(need):
            ev["dup_in_pull_list"] += 1
        lists, seen, skip = {}, set(), False
        for w in need:
            if skip:                                                              # dup_skip: the wire after a duplicate is taken for fetched
                skip = False
                seen.add(w)
                continue
            if w in seen:
                skip = self.fault == "dup_skip"
                continue
            seen.add(w)
            lists.setdefault(0 if self.fault == "pull_from_0" else int(self.owner[w]), []).append(w)
        for src, ws in lists.items():
            if src == dst:                                                        # (only a fault names the reader itself as the source)
                continue
            self.tables[dst][ws] = self.tables[src][ws]
            ev[f"pull_from_dev{src}"] += 1
            if any(self.shared[w] for w in ws):
                ev["read_of_shared_then_rewritten"] += 1
            self.xfers[src, dst] += 1
            ev["five_transfers_one_pair"] += int(self.xfers[src, dst] == 5)
        ev["two_sources_in_one_pull"] += int(len([s for s in lists if s != dst]) >= 2)
        for w in seen:
            valid[w] = 1

    def _write(self, r, wires, rows):
        self.tables[r][wires] = rows
        for w in wires:
            self.shared[w] = sum(v[w] for v in self.valid) >= 2
            for k in range(self.nk):
                if k == r or self.fault != "stale_valid":
                    self.valid[k][w] = int(k == r)
            self.owner[w] = r

    def _level(self, i, lv):
        nk, ev = self.nk, self.events
        b = plan(lv, nk, self.split_min)
        shards = [(r, b[r], b[r + 1]) for r in range(nk) if b[r + 1] > b[r]]
        self.counts[i] = len(shards)
        if is_split(lv, nk, self.split_min):
            ev["zero_gate_shard"] += int(len(shards) < nk)
            ev["split_multi_output_lut"] += int(lv.kind == "lut" and lv.n_out > 1 and len(shards) > 1)
        for r, g0, g1 in shards:
            self._pull(r, reads_of(lv, g0, g1))
        for r, g0, g1 in shards:
            self._write(r, *run_level(self.arith, self.tables[r], lv, g0, g1, self.fault))

    def _synced(self, everything):
        self.queued = 0
        for pair in list(self.xfers):
            if everything or pair[1] == 0:
                del self.xfers[pair]

    def run(self, prog, want=None):
        """Per step the words of a read (None otherwise).  With `want` (the model's reads) it stops at the first read that differs and
        returns the step's index."""
        reads, refused = [], False
        for i, s in enumerate(prog):
            read = None
            if s.kind == "alloc":
                self.tables = [np.zeros((s.W, s.width), np.int32) for _ in range(self.nk)]
                self.valid = [np.ones(s.W, np.uint8) for _ in range(self.nk)]
                self.owner, self.shared, self.xfers = np.zeros(s.W, np.int64), np.zeros(s.W, bool), collections.Counter()
                self._synced(True)
            elif s.kind == "upload":
                rng = range(s.first, s.first + len(s.data))
                self.events["upload_over_foreign_owner"] += int(any(self.owner[w] != 0 for w in rng))
                for k in range(self.nk):
                    if k == 0 or self.fault != "upload_owner":
                        self.tables[k][s.first:s.first + len(s.data)] = s.data
                    self.valid[k][s.first:s.first + len(s.data)] = int(k == 0 or self.fault != "upload_owner")
                if self.fault != "upload_owner":
                    self.owner[s.first:s.first + len(s.data)] = 0
                self.shared[s.first:s.first + len(s.data)] = False
                self._synced(True)
            elif s.kind == "option":
                self.split_min = s.split_min
            elif s.kind in LEVELS:
                self._level(i, s)
                self.queued += 1
                self.events["nine_levels_queued"] += int(self.queued == 9)
            elif s.kind == "refused":
                if self.fault == "refused_writes_first" and s.why != "wrong_call":
                    self._pull(0, reads_of(s.level, 0, 1))
                    self._write(0, *run_level(self.arith, self.tables[0], s.level, 0, 1))
            else:
                wires = list(range(s.first, s.first + s.count)) if s.kind == "download" else [int(w) for w in s.wires]
                if self.fault != "download_no_pull":
                    self._pull(0, wires)
                read = read_of(self.tables[0], s)
                self.events["read_after_refused"] += int(refused)
                self._synced(False)
                if want is not None and not np.array_equal(read, want[i]):
                    return i
            refused = s.kind == "refused" or (refused and s.kind == "option")
            reads.append(read)
        return None if want is not None else reads
