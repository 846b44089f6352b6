"""Levelised execution of gate circuits on device-resident ciphertexts.

Real workloads are gate DAGs (examples/tutorial.jl:42-62: a 16-deep XNOR->MUX chain, then 16 parallel
MUXes).  A Circuit records gates with the reference's gate names, assigns every gate the level
1 + max(level of its operands), and runs level by level: one tfhe_gates_level call per level over all the
level's independent gates, ciphertexts staying in the engine's wire table on the GPU — only the inputs go
up and only the requested outputs come down.

Integer nodes join the gates in the same levels (programmable bootstrapping, tfhe_jl_amd.lut): `lut(f, terms, p)` is one blind
rotation of the integer combination of `terms` with test polynomial make_test_vector(f, p, N, q), `lut_multi(fs, terms, p)` K results
from one rotation, `linear(terms)` the combination itself.  A term is a wire or (wire, integer coefficient); `const` is a Torus32 word
added to the body.  Linear nodes are folded into the terms of whatever reads them through a LUT or another linear node (coefficients
multiplied, constants summed mod 2^32), so a LUT never waits a level for one; a linear node is computed (tfhe_linear_level) only if
a gate reads it or it is an output.  A level runs as one tfhe_gates_level, one tfhe_lut_level per distinct K and one
tfhe_linear_level, all on the context's stream.  The caller chooses the coefficients: their noise growth is not checked.

TLWE-valued nodes bring the leveled half into the same circuit (single-key, one-device): `tlwe_inputs(count)` are TLWE samples the caller
supplies to run(..., tlwe_inputs=...), `rot_net(net, entries, selectors)` a CMUX network (a leveled.RotNet, or a CmuxNet / tree_net as its
rotation-0 case) over E TLWE nodes, `blind_rotate(acc, terms)` the blind rotation of a TLWE node by the integer combination of wires that
a LUT would rotate its table by.  Either leaves TLWE nodes (out="tlwe") or, extracted and keyswitched, ordinary wires (out="lwe").  The
planner gives TLWE nodes slots of the engine's TLWE table as wires get rows of the wire table and levels them with the gate, LUT and
linear nodes; a level issues one tfhe_blind_rotate_level per (n_out, out, sel), one tfhe_bootstrap_acc_level per (n_out, out) of its
tuned=True rotations (the gates' own key and kernels: no selector set) and one tfhe_rot_net_level per network node.  The
selectors are indices into the engine's loaded set: loading it (Engine.tgsw_load: the bootstrapping key's n selectors for the rotations'
sel=None, address-bit selectors behind them; Engine.tgsw_update swaps those per request) stays the caller's job."""
import numbers

import numpy as np

from ._lib import OPCODES
from types import SimpleNamespace

from .numeric import wrap32
from .lwe import LweSample, LweSampleArray
from .mk_keys import MKCloudKey, MKLweSample

_ARITY = {"NOT": 1, "COPY": 1, "CONST0": 0, "CONST1": 0, "MUX": 3}


class TlweNode:
    """A TLWE-valued node of a Circuit: slot `slot` of the engine's TLWE table while the circuit runs."""
    __slots__ = ("slot",)

    def __init__(self, slot):
        self.slot = slot

    def __repr__(self):
        return f"TlweNode({self.slot})"


class Circuit:
    def __init__(self):
        self._n_inputs = 0
        self._gates = []          # (opcode name, a, b, c) with wire ids
        self._level = []          # level per wire (inputs: 0)
        self._outputs = []
        self._gate_wire = []      # output wire of gate g
        self._linear = {}         # wire -> ({base wire: coefficient mod 2^32}, constant mod 2^32), terms folded to non-linear wires
        self._luts = []           # (table key, K, terms {base wire: coefficient}, constant, [output wires])
        self._tlwe_level = []     # level per TLWE slot (inputs: 0)
        self._n_tlwe_inputs = 0
        self._rot_nets = []       # (level, E, widths, nodes [..][5] with absolute level-0 sources, selectors [V], out_form, first out slot, [output wires])
        self._rotations = []      # (level, acc slot, terms, constant, n_out, out_form, sel tuple or None, out slot, [output wires])
        self._rotation_tuned = []  # per rotation: True = on the gates' own key and kernels (Engine.bootstrap_acc_level)

    # ---- building -----------------------------------------------------------------------------------
    def input(self):
        if self._gates:
            raise ValueError("declare all inputs before the first gate")
        self._n_inputs += 1
        self._level.append(0)
        return self._n_inputs - 1

    def inputs(self, count):
        return [self.input() for _ in range(count)]

    def _check_wire(self, w):
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, numbers.Integral) or not (0 <= int(w) < len(self._level)):
            raise ValueError(f"operand wire {w} does not exist")
        return int(w)

    def _fold(self, terms, const):
        """terms (wire or (wire, coef)) + const -> ({non-linear wire: coef mod 2^32}, const mod 2^32), linear nodes expanded."""
        if isinstance(const, (bool, np.bool_)) or not isinstance(const, numbers.Integral):
            raise ValueError(f"const {const!r} is not an integer (a Torus32 word)")
        acc, cst = {}, int(const) % 2**32
        for t in terms:
            w, coef = (t, 1) if not isinstance(t, (tuple, list)) else tuple(t)
            w = self._check_wire(w)
            if isinstance(coef, (bool, np.bool_)) or not isinstance(coef, numbers.Integral):
                raise ValueError(f"coefficient {coef!r} of wire {w} is not an integer")
            coef = int(coef)
            inner, inner_c = self._linear.get(w, ({w: 1}, 0))
            for b, cb in inner.items():
                acc[b] = (acc.get(b, 0) + coef * cb) % 2**32
            cst = (cst + coef * inner_c) % 2**32
        return {b: v for b, v in acc.items() if v}, cst

    def _new_wire(self, level):
        self._level.append(level)
        return len(self._level) - 1

    def linear(self, terms, const=0):
        """A wire holding sum coef * wire + const (mod 2^32), no bootstrap: LweSampleArray's +, integer scale and add_constant."""
        folded, cst = self._fold(terms, const)
        w = self._new_wire(1 + max((self._level[b] for b in folded), default=0))
        self._linear[w] = (folded, cst)
        return w

    def _add_lut(self, key, K, terms, const):
        folded, cst = self._fold(terms, const)
        level = 1 + max((self._level[b] for b in folded), default=0)
        outs = [self._new_wire(level) for _ in range(K)]
        self._luts.append((key, K, folded, cst, outs))
        return outs

    @staticmethod
    def _spaces(p, q):
        for v, what in ((p, "p"), (q, "q")):
            if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 2 or v & (v - 1)):
                raise ValueError(f"{what} = {v}: a power of two >= 2")
        return int(p), None if q is None else int(q)

    def lut(self, f, terms, p, q=None, const=0):
        """One wire: f(m) in Z_q (q defaults to p) of the message m in Z_p that the combination of `terms` + const encrypts, by one
        blind rotation with make_test_vector(f, p, N, q).  `f` may also be a raw int32 test polynomial [N] (lut.make_gate_test_vector:
        a gate-encoded bit).  Equal (f, p, q) share one table per level."""
        p, q = self._spaces(p, q)
        if callable(f):
            key = ("f", f, p, q)
        else:
            t = np.ascontiguousarray(f, dtype=np.int32)
            if t.ndim != 1:
                raise ValueError(f"a raw test polynomial is int32 [N], got shape {t.shape}")
            key = ("raw", t.tobytes())
        return self._add_lut(key, 1, terms, const)[0]

    def lut_multi(self, fs, terms, p, q=None, const=0):
        """K = len(fs) wires from ONE blind rotation: fs[j](m) in Z_q for the message m of Z_p encrypted in Z_{pK}
        (make_multi_test_vector; K a power of two, p K <= N / 2)."""
        p, q = self._spaces(p, q)
        fs = tuple(fs)
        K = len(fs)
        if K < 1 or K > 32 or K & (K - 1):
            raise ValueError(f"K = {K} functions: a power of two, 1 <= K <= 32")
        if not all(callable(f) for f in fs):
            raise ValueError("lut_multi takes callables")
        return self._add_lut(("multi", fs, p, q), K, terms, const)

    # ---- TLWE-valued nodes --------------------------------------------------------------------------
    def tlwe_inputs(self, count):
        """`count` TLWE samples supplied to run(..., tlwe_inputs=...): the first slots of the TLWE table, in order."""
        if len(self._tlwe_level) != self._n_tlwe_inputs:
            raise ValueError("declare all TLWE inputs before the first TLWE-valued node")
        first = self._n_tlwe_inputs
        self._n_tlwe_inputs += int(count)
        self._tlwe_level += [0] * int(count)
        return [TlweNode(first + i) for i in range(int(count))]

    def _check_tlwe(self, t):
        if not isinstance(t, TlweNode) or not 0 <= t.slot < len(self._tlwe_level):
            raise ValueError(f"{t!r} is not a TLWE node of this circuit")
        return t.slot

    @staticmethod
    def _out_form(out):
        if out not in ("lwe", "tlwe"):
            raise ValueError(f"out = {out!r}: 'lwe' (wires) or 'tlwe' (TLWE nodes)")
        return 2 if out == "lwe" else 0

    def _new_tlwe(self, level, count):
        first = len(self._tlwe_level)
        self._tlwe_level += [level] * count
        return first

    def rot_net(self, net, entries, selectors, out="lwe"):
        """The F outputs of the CMUX network `net` (leveled.RotNet; a CmuxNet or tree_net is its rotation-0 case) over the E TLWE nodes
        `entries`, variable v selected by selector `selectors[v]` of the engine's loaded set: F wires (out="lwe": extracted at
        coefficient 0 and keyswitched) or F TLWE nodes (out="tlwe")."""
        form = self._out_form(out)
        slots = [self._check_tlwe(t) for t in entries]
        if len(slots) != net.entries:
            raise ValueError(f"the network reads {net.entries} entries, got {len(slots)}")
        sel = [int(v) for v in selectors]
        if len(sel) != net.variables or any(v < 0 for v in sel):
            raise ValueError(f"the network has {net.variables} variables, got {len(sel)} selector indices (each >= 0)")
        nodes = np.asarray(net.nodes, np.int32)
        if nodes.shape[1] == 3:
            nodes = np.concatenate([nodes, np.zeros((nodes.shape[0], 2), np.int32)], axis=1)
        nodes = np.ascontiguousarray(nodes).copy()
        w0 = int(net.widths[0])
        nodes[:w0, 0] = np.asarray(slots, np.int32)[nodes[:w0, 0]]          # level 0 reads absolute slots (table_first NULL)
        nodes[:w0, 1] = np.asarray(slots, np.int32)[nodes[:w0, 1]]
        level = 1 + max(self._tlwe_level[s] for s in slots)
        F = int(net.widths[-1])
        first = self._new_tlwe(level, F) if form == 0 else -1
        wires = [self._new_wire(level) for _ in range(F)] if form == 2 else []
        self._rot_nets.append((level, max(slots) + 1, np.asarray(net.widths, np.int32), nodes, sel, form, first, wires, getattr(net, "degree", None)))
        return wires if form == 2 else [TlweNode(first + i) for i in range(F)]

    def blind_rotate(self, acc, terms, const=0, n_out=1, out="lwe", sel=None, tuned=False):
        """The TLWE node `acc` rotated by the combination of `terms` + const (as lut's; the context's n steps, selector sel[i] — None: i
        — of the engine's loaded set for step i): one TLWE node (out="tlwe", n_out 1) or the n_out extractions at the coefficients
        j N / n_out, keyswitched, as wires (out="lwe"; n_out = 1: one wire, else a list).
        tuned=True rotates on the gates' own key and kernels instead (Engine.bootstrap_acc_level: the same words where
        get_option("bootstrap_acc") is 1, that is N = 1024, k = 1; run raises ValueError elsewhere): the steps are the bootstrapping key's,
        so sel must be None, and the node needs no loaded selector set.  With the engine's option acc_dispatch 1 a level's one or few
        tuned rows take the multi-wave kernels a gate batch of that size takes."""
        if tuned and sel is not None:
            raise ValueError("tuned=True rotates by the gates' key, the bootstrapping key in step order: sel must be None")
        form = self._out_form(out)
        slot = self._check_tlwe(acc)
        n_out = int(n_out)
        if n_out < 1 or n_out > 32 or n_out & (n_out - 1) or (form == 0 and n_out != 1):
            raise ValueError(f"n_out = {n_out}: a power of two, 1 ... 32, and 1 with out='tlwe'")
        folded, cst = self._fold(terms, const)
        level = 1 + max([self._level[b] for b in folded] + [self._tlwe_level[slot]])
        key = None if sel is None else tuple(int(v) for v in sel)
        first = self._new_tlwe(level, 1) if form == 0 else -1
        wires = [self._new_wire(level) for _ in range(n_out)] if form == 2 else []
        self._rotations.append((level, slot, folded, cst, n_out, form, key, first, wires))
        self._rotation_tuned.append(bool(tuned))
        if form == 0:
            return TlweNode(first)
        return wires[0] if n_out == 1 else wires

    @property
    def num_tlwe(self):
        return len(self._tlwe_level)

    def gate(self, name, *operands):
        name = name.upper()
        if name not in OPCODES:
            raise ValueError(f"unknown gate {name}")
        arity = _ARITY.get(name, 2)
        if len(operands) != arity:
            raise ValueError(f"gate {name} takes {arity} operand(s)")
        for w in operands:
            if not (0 <= w < len(self._level)):
                raise ValueError(f"operand wire {w} does not exist")
        ops = list(operands) + [-1] * (3 - arity)
        self._gates.append((name, ops[0], ops[1], ops[2]))
        self._gate_wire.append(len(self._level))
        self._level.append(1 + max([self._level[w] for w in operands], default=0))
        return len(self._level) - 1

    # the reference's names (src/gates.jl)
    def nand(self, x, y): return self.gate("NAND", x, y)
    def or_(self, x, y): return self.gate("OR", x, y)
    def and_(self, x, y): return self.gate("AND", x, y)
    def xor(self, x, y): return self.gate("XOR", x, y)
    def xnor(self, x, y): return self.gate("XNOR", x, y)
    def not_(self, x): return self.gate("NOT", x)
    def nor(self, x, y): return self.gate("NOR", x, y)
    def andny(self, x, y): return self.gate("ANDNY", x, y)
    def andyn(self, x, y): return self.gate("ANDYN", x, y)
    def orny(self, x, y): return self.gate("ORNY", x, y)
    def oryn(self, x, y): return self.gate("ORYN", x, y)
    def mux(self, x, y, z): return self.gate("MUX", x, y, z)
    def constant(self, value): return self.gate("CONST1" if value else "CONST0")

    def set_outputs(self, wires):
        self._outputs = list(wires)

    # ---- analysis -----------------------------------------------------------------------------------
    @property
    def num_wires(self):
        return len(self._level)

    @property
    def outputs(self):
        return list(self._outputs)

    def levels(self):
        """List of levels; each level is a list of gate indices (gate g drives wire gate_wire(g): n_inputs + g in a circuit of
        gates only)."""
        depth = max(self._level + self._tlwe_level, default=0)
        out = [[] for _ in range(depth)]
        for g in range(len(self._gates)):
            out[self._level[self._gate_wire[g]] - 1].append(g)
        return out

    def gate_wire(self, g):
        return self._gate_wire[g]

    def level_arrays(self):
        """Per level: (opcodes u8, a, b, c, out) index arrays as tfhe_gates_level takes them."""
        res = []
        for gates in self.levels():
            ops = np.array([OPCODES[self._gates[g][0]] for g in gates], np.uint8)
            a = np.array([max(self._gates[g][1], 0) for g in gates], np.int32)
            b = np.array([max(self._gates[g][2], 0) for g in gates], np.int32)
            c = np.array([max(self._gates[g][3], 0) for g in gates], np.int32)
            out = np.array([self._gate_wire[g] for g in gates], np.int32)
            res.append((ops, a, b, c, out))
        return res

    def level_plan(self, N, M=1):
        """Per level, what run (M = 1) and run_batch (M instances; wire w of instance i is row w M + i) call:
        {"gates": (opcodes, a, b, c, out) or None, "lut": [(K, tables [n_tv][N], index, term_start, term_wire, term_coef, cst, out)]
        in increasing K, "linear": (term_start, term_wire, term_coef, cst, out) or None}; the index arrays are int32 and spread over
        the instances exactly as the gates' operands are.  Tables are built at ring degree N (ValueError for p K > N / 2)."""
        from .lut import make_multi_test_vector, make_test_vector
        inst = np.arange(M, dtype=np.int64)
        spread = lambda w: (np.asarray(w, np.int64)[:, None] * M + inst[None, :]).reshape(-1).astype(np.int32)
        read_by_gate = {w for (_, a, b, c) in self._gates for w in (a, b, c) if w >= 0}
        outputs = set(self._outputs)
        tables = {}

        def table(key):
            if key not in tables:
                if key[0] == "raw":
                    t = np.frombuffer(key[1], np.int32)
                    if t.size != N:
                        raise ValueError(f"raw test polynomial of {t.size} words, the ring has N = {N}")
                elif key[0] == "f":
                    t = make_test_vector(key[1], key[2], N, key[3])
                else:
                    t = make_multi_test_vector(list(key[1]), key[2], N, key[3])
                tables[key] = t
            return tables[key]

        def rows(nodes, per_row):
            """[(terms, const, outs)] -> spread (term_start, term_wire, term_coef, cst, out)."""
            counts = np.array([len(t) for t, _, _ in nodes], np.int64)
            wires = np.array([w for t, _, _ in nodes for w in sorted(t)], np.int64)
            coefs = np.array([t[w] for t, _, _ in nodes for w in sorted(t)], np.int64)
            first = np.concatenate([[0], np.cumsum(counts)])[:-1]
            row_counts = np.repeat(counts, M)
            start = np.concatenate([[0], np.cumsum(row_counts)]).astype(np.int64)
            T = int(start[-1])
            t_node = np.repeat(np.repeat(first, M), row_counts) + (np.arange(T) - np.repeat(start[:-1], row_counts))
            term_wire = (wires[t_node] * M + np.repeat(np.tile(inst, len(nodes)), row_counts)).astype(np.int32)
            term_coef = wrap32(coefs[t_node])
            cst = wrap32(np.repeat(np.array([c for _, c, _ in nodes], np.int64), M))
            outs = np.array([o for _, _, o in nodes], np.int64).reshape(len(nodes), 1, per_row)
            out = (outs * M + inst[None, :, None]).reshape(-1).astype(np.int32)
            return start.astype(np.int32), term_wire, term_coef, cst, out

        gate_arrays = self.level_arrays()
        plan = []
        for li in range(len(gate_arrays)):
            level = li + 1
            ops, a, b, c, out = gate_arrays[li]
            gates = (np.repeat(ops, M), spread(a), spread(b), spread(c), spread(out)) if ops.size else None
            luts = []
            for K in sorted({K for (_, K, _, _, outs) in self._luts if self._level[outs[0]] == level}):
                nodes = [n for n in self._luts if n[1] == K and self._level[n[4][0]] == level]
                keys = list(dict.fromkeys(n[0] for n in nodes))
                tv = np.stack([table(k) for k in keys]).astype(np.int32)
                index = np.repeat(np.array([keys.index(n[0]) for n in nodes], np.int32), M)
                luts.append((K, tv, index) + rows([(n[2], n[3], n[4]) for n in nodes], K))
            lin = [(t, cst, [w]) for w, (t, cst) in self._linear.items()
                   if self._level[w] == level and (w in read_by_gate or w in outputs)]
            plan.append({"gates": gates, "lut": luts, "linear": rows(lin, 1) if lin else None})
            if self._tlwe_level:
                if M != 1:
                    raise ValueError("a circuit with TLWE nodes runs one instance at a time (run, not run_batch)")
                # one call per (n_out, out, sel), the tuned rotations (sel None) grouped apart from the others: "bootstrap_acc"
                groups = {}
                for r, tuned in zip(self._rotations, self._rotation_tuned):
                    if r[0] == level:
                        groups.setdefault((tuned, r[4], r[5], r[6]), []).append(r)
                rot, rot_tuned = [], []
                for (tuned, n_out, form, sel), rs in groups.items():
                    start, wire, coef, cst, _ = rows([(r[2], r[3], [0]) for r in rs], 1)
                    (rot_tuned if tuned else rot).append(
                        (np.array([r[1] for r in rs], np.int32), start, wire, coef, cst, None if sel is None else np.array(sel, np.int32), n_out, form,
                         np.array([r[7] for r in rs], np.int32) if form == 0 else None,
                         np.array([w for r in rs for w in r[8]], np.int32) if form == 2 else None))
                nets = [(SimpleNamespace(entries=E, widths=widths, levels=int(widths.size), nodes=nodes, variables=len(sel), degree=N if degree is None else degree),
                         np.array([sel], np.int32), form, max(first, 0), np.array(wires, np.int32) if form == 2 else None)
                        for (lv, E, widths, nodes, sel, form, first, wires, degree) in self._rot_nets if lv == level]
                plan[-1]["blind_rotate"], plan[-1]["rot_net"] = rot, nets
                if rot_tuned:
                    plan[-1]["bootstrap_acc"] = rot_tuned
        return plan

    def _run_plan(self, eng, plan, mk):
        level = eng.mk_gates_level if mk else eng.gates_level
        lut_level = eng.mk_lut_level if mk else eng.lut_level
        linear_level = eng.mk_linear_level if mk else eng.linear_level
        for lv in plan:
            if lv["gates"] is not None:
                level(*lv["gates"])
            for K, tv, index, start, wire, coef, cst, out in lv["lut"]:
                lut_level(tv, start, wire, coef, cst, out, index=index, n_out=K)
            if lv["linear"] is not None:
                linear_level(*lv["linear"])
            for acc, start, wire, coef, cst, sel, n_out, form, out_slot, out_wires in lv.get("blind_rotate", ()):
                eng.blind_rotate_level(acc, start, wire, coef, cst=cst, sel=sel, n_out=n_out, out_form=form, out_slot=out_slot, out_wires=out_wires)
            for acc, start, wire, coef, cst, _, n_out, form, out_slot, out_wires in lv.get("bootstrap_acc", ()):
                eng.bootstrap_acc_level(acc, start, wire, coef, cst=cst, n_out=n_out, out_form=form, out_slot=out_slot, out_wires=out_wires)
            for net, sel, form, out_first, out_wires in lv.get("rot_net", ()):
                eng.rot_net_level(net, sel, out_form=form, out_first=out_first, out_wires=out_wires)

    # ---- execution ----------------------------------------------------------------------------------
    def run(self, ck, inputs, device=0, tlwe_inputs=None):
        """inputs: LweSampleArray / list of LweSample / int32 [n_inputs][n+1].  Returns an LweSampleArray
        of the output wires.  Everything between upload and download runs on the GPU.
        Under an MKCloudKey: inputs int32 [n_inputs][P*n+1] (or a list of flat samples / MKLweSample), result int32
        [n_outputs][P*n+1]; the levels run on a multi-key wire table (tfhe_mk_wires_alloc, tfhe_mk_gates_level, tfhe_mk_lut_level,
        tfhe_mk_linear_level).
        A circuit with TLWE nodes (single-key only) also takes tlwe_inputs, int32 [tlwe input count][k+1][N], into the first slots of a
        TLWE table of num_tlwe slots; the engine's selector set must be loaded (see the module's text)."""
        mk = isinstance(ck, MKCloudKey)
        if self._tlwe_level and mk:
            raise ValueError("a circuit with TLWE nodes runs under a single-key CloudKey (the TLWE table is single-key)")
        eng = ck.engine(device)
        if self._tlwe_level:
            t = np.zeros((0, eng.k + 1, eng.N), np.int32) if tlwe_inputs is None else np.asarray(tlwe_inputs, np.int32)
            if t.ndim != 3 or t.shape[0] != self._n_tlwe_inputs:
                raise ValueError(f"circuit has {self._n_tlwe_inputs} TLWE inputs [k+1][N], got shape {t.shape}")
        elif tlwe_inputs is not None:
            raise ValueError("the circuit has no TLWE nodes")
        if isinstance(inputs, LweSampleArray):
            m = inputs.data
        elif isinstance(inputs, (list, tuple)):
            m = np.stack([s.flat() if isinstance(s, (LweSample, MKLweSample)) else np.asarray(s, np.int32) for s in inputs])
        else:
            m = np.asarray(inputs, np.int32)
        if m.shape[0] != self._n_inputs:
            raise ValueError(f"circuit has {self._n_inputs} inputs, got {m.shape[0]}")
        (eng.mk_wires_alloc if mk else eng.wires_alloc)(self.num_wires)
        if self._n_inputs:
            eng.wires_upload(0, m)
        plan = self.level_plan(eng.N)
        if any(self._rotation_tuned) and eng.get_option("bootstrap_acc") != 1:
            raise ValueError(f"tuned=True: Engine.bootstrap_acc serves N = 1024, k = 1 in the gates' key layout; this context has "
                             f"N = {eng.N}, k = {eng.k} (option bootstrap_acc is 0): use tuned=False")
        if self._tlwe_level:
            eng.tlwe_alloc(self.num_tlwe)
            if self._n_tlwe_inputs:
                eng.tlwe_upload(0, t)
        # no per-phase timing events while the levels run: each record keeps the stream's next kernel waiting ~5 us, and a level
        # of a narrow circuit is six short operations around one single-rotation kernel (tutorial circuit: 30.5 -> 30.1 ms)
        timing_before = eng.get_option("timing_events")              # (the engine is shared through ck.engine(): put the caller's setting back)
        eng.set_option("timing_events", 0)
        try:
            self._run_plan(eng, plan, mk)
            rows = eng.wires_gather(self._outputs)                    # one device gather + one copy for all outputs
            return rows if mk else LweSampleArray(rows)
        finally:
            eng.set_option("timing_events", timing_before)

    def run_batch(self, ck, inputs, device=0):
        """The same circuit on M independent input sets at once: inputs int32 [M][n_inputs][n+1] (or a list of M LweSampleArrays),
        result int32 [M][n_outputs][n+1].  Every level becomes ONE tfhe_gates_level call over the M instances' gates — a level of
        a narrow circuit costs one single-rotation latency whether it holds 1 gate or 256 (one blind rotation per CU), so M <= 256 /
        (rotations of the widest level) instances cost what one does; beyond that the levels run at batch throughput.
        Wire w of instance i is row w * M + i of the wire table: the inputs go up as one block, the outputs come down as one gather.
        Under an MKCloudKey the rows are multi-key samples: inputs [M][n_inputs][P*n+1], result [M][n_outputs][P*n+1]."""
        if self._tlwe_level:
            raise ValueError("a circuit with TLWE nodes runs one instance at a time (run, not run_batch)")
        eng = ck.engine(device)
        mk = isinstance(ck, MKCloudKey)
        if isinstance(inputs, (list, tuple)):
            inputs = np.stack([x.data if isinstance(x, LweSampleArray) else np.asarray(x, np.int32) for x in inputs])
        m = np.ascontiguousarray(inputs, dtype=np.int32)
        if m.ndim != 3 or m.shape[1] != self._n_inputs:
            raise ValueError(f"inputs must be [M][{self._n_inputs}][{'P*n+1' if mk else 'n+1'}], got {m.shape}")
        M = m.shape[0]
        if M == 0:
            return np.zeros((0, len(self._outputs), m.shape[2]), np.int32)
        plan = self.level_plan(eng.N, M)
        (eng.mk_wires_alloc if mk else eng.wires_alloc)(self.num_wires * M)
        if self._n_inputs:
            eng.wires_upload(0, np.ascontiguousarray(m.transpose(1, 0, 2)).reshape(self._n_inputs * M, -1))
        spread = lambda w: (w[:, None] * M + np.arange(M, dtype=np.int32)[None, :]).reshape(-1).astype(np.int32)      # wire ids -> rows, instance fastest
        timing_before = eng.get_option("timing_events")
        eng.set_option("timing_events", 0)
        try:
            self._run_plan(eng, plan, mk)
            rows = eng.wires_gather(spread(np.asarray(self._outputs, np.int32)))
        finally:
            eng.set_option("timing_events", timing_before)
        return np.ascontiguousarray(rows.reshape(len(self._outputs), M, -1).transpose(1, 0, 2))

