"""The device-resident TLWE table, the wire table beside it and the loaded selector set under random programs: program generator and
host model (host only, no GPU; not collected).  The wire-side steps, `Step`, `Generator` and `Arith` are tests/wire_table_model.py's.

A program is a seeded list of steps over a TLWE table of 12 ... 24 slots and a wire table of 24 ... 48 wires (rewrites are frequent):

    tlwe_alloc(slots), wires_alloc(W)   also in the middle of a program, always followed by an upload of the whole new table
    tlwe_upload, wires_upload           partial ranges
    tgsw_load                           a whole new selector set, n + 2 ... n + 4 selectors
    tgsw_update(first, count)           in turn: first = 0, the last selector, a range that straddles n, the whole set
    rotate                              tfhe_blind_rotate_level, B = 1 ... 4: out_form 0 into slots or 2 into wires (n_out 1, 2, 4), sel None or n
                                        distinct selectors, cst or None, rows of 0 ... 4 terms (small, wrapping and +-2^31 coefficients),
                                        repeated acc_slots; in turn a copy row (no terms, no constant), a row whose mask exponents are all 0
                                        (no terms, a constant) and a row whose last exponent is 0 while the one before is not (a planted
                                        wire, uploaded by the step before)
    net                                 tfhe_rot_net_level, B = 1 ... 3: tree_net(1), tree_net(2), test_tlwe_levels._two_level_net,
                                        packed_lookup_net(log2 N + 1, N); table_first None or per-row ranges that overlap; out_form 0 with
                                        out_first anywhere legal (below every read range, ending at the last slot) or 2 into permuted wires
    gates, linear, lut                  wire_table_model.Generator's levels
    tlwe_download, wires_download, wires_gather   reads: every read yields the words the engine must return
    option                              anyn_spec in {-1, 1}
    refused                             a call the library must refuse (REFUSALS), both tables as they were

With acc=True (N = 1024, k = 1, where blind_rotate_kernel_v3_acc exists; acc=False draws exactly what it drew before: steps_digest) also:

    acc_rotate                          tfhe_bootstrap_acc_level: `rotate` without sel, B = 1 ... 9, n_out 1, 2, 8 with B n_out at most half the
                                        wires and the outputs apart from every read; the special rows take turns on their own
    acc_batch                           Engine.bootstrap_acc on host buffers between the levels, a read: T = 1 ... 3 arbitrary accumulators,
                                        B = 1 ... 6 rows of arbitrary words, acc_index or None, out_form 0, 1 or 2 (n_out 1, 4, 32)
    option                              also v3_rw in turn 1, 4, 0, 4 (the model ignores it: no word depends on it)
    refused                             REFUSALS and ACC_REFUSALS in turn

Both rotate with a second Rotation over leveled.bootstrap_key_selectors(ck), selector i at step i, whatever set is loaded (ACC_EVENTS,
ACC_FAULTS).

`Model` holds one wire table [W][n+1], one TLWE table [slots][k+1][N] and the selector set [S][l][k+1][k+1][N] and applies each step in
exact integer arithmetic: test_tlwe_levels.form_rows then test_blind_rotate.Rotation.rotate_lwe for a rotation row, Rotation.extract_at
for the extractions, leveled_ref.rot_net_ref over a Tree for the networks, leveled_ref.ks_ref for the keyswitch, wire_table_model's
single_key_arith for the wire-side levels.  No engine call and no batch call takes part.  It counts the events a program reaches (EVENTS)
and emulates one fault at a time (FAULTS)."""
import collections
import hashlib

import numpy as np

import wire_table_model as M
from wire_table_model import Step
from test_tlwe_levels import INVALID, OK, form_rows, model_blind_rotate_level, model_rot_net_level

SLOT_RANGE, WIRE_RANGE, N_OUTS, SPECS = (12, 24), (24, 48), (1, 2, 4), (-1, 1)
NETS = ("tree1", "tree2", "two_level", "packed")
REFUSALS = ("out_is_acc", "slot_twice", "out_meets_read", "term_is_out", "out_form_1", "sel_beyond")
UPDATES = ("first_0", "last", "straddles_n", "whole")
SPECIALS = (None, "copy", "mask_zero", "skip_last")
TLWE_LEVELS = ("rotate", "net")
ACC_LEVELS = ("acc_rotate",)
LEVELS = TLWE_LEVELS + M.LEVELS + ACC_LEVELS
READS = ("tlwe_download", "wires_download", "wires_gather", "acc_batch")
# with acc=True (the programs of tests/test_bootstrap_acc_programs.py at N = 1024, k = 1; never in a program made with acc=False):
ACC_B = (1, 4, 5, 8, 9)                                                            # half of the acc_rotate steps draw B here, the others 1 ... 9
ACC_N_OUTS, BATCH_N_OUTS, V3_RWS = (1, 2, 8), (1, 4, 32), (4, 1, 4, 0)
ACC_REFUSALS = ("acc_out_is_acc", "acc_slot_twice", "acc_term_is_out", "acc_out_form_1")

EVENTS = ("slot_rewritten_then_read", "upload_over_level_written_slot", "net_reads_slot_written_by_rotate", "rotate_reads_slot_written_by_net",
          "rotate_term_wire_written_by_net", "rotate_term_is_gate_output", "gate_reads_wire_written_by_tlwe_level",
          "selector_used_before_and_after_update", "sel_beyond_smaller_load_refused", "wires_realloc_with_live_tlwe",
          "tlwe_realloc_with_live_wires", "copy_row", "last_step_skipped", "shared_acc_slot", "overlapping_read_ranges",
          "outputs_below_read_ranges", "level_under_spec_global", "read_after_refused")
FAULTS = ("stale_selectors", "update_offset", "first_ignored", "net_out_stride", "out_slot_order", "dst_order", "sel_ignored", "cst_dropped",
          "other_sample", "extract_stride", "realloc_clobbers", "refused_writes_first", "stale_slot")
ACC_EVENTS = ("acc_rotate_reads_slot_written_by_rotate", "acc_rotate_reads_slot_written_by_net", "rotate_or_net_reads_slot_written_by_acc_rotate",
              "acc_rotate_term_is_gate_output", "gate_reads_wire_written_by_acc_rotate", "acc_rotate_directly_after_wire_level",
              "wire_level_directly_after_acc_rotate", "acc_batch_between_two_levels", "acc_rotate_after_selector_change",
              "acc_rotate_rw4_with_padding", "acc_rotate_rw4_out_form_0", "acc_rotate_shared_acc_slot", "acc_rotate_copy_row",
              "acc_rotate_last_step_skipped", "acc_rotate_larger_than_every_level_before")
ACC_FAULTS = ("acc_uses_loaded_selectors", "acc_out_index_ignored", "acc_first_rows_slot", "acc_mask_from_zero", "acc_barb_dropped",
              "acc_extract_stride", "acc_batch_stale_rows", "acc_clobbers_wire_level")


def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


def make_nets(N):
    """The four networks of a `net` step: name -> (network, E, F, V)."""
    from tfhe_jl_amd import leveled
    from test_tlwe_levels import _two_level_net
    nets = {"tree1": leveled.tree_net(1), "tree2": leveled.tree_net(2), "two_level": _two_level_net(leveled, N),
            "packed": leveled.packed_lookup_net(N.bit_length(), N)}
    return {name: (net, int(net.entries), int(net.widths[-1]), int(net.variables)) for name, net in nets.items()}


def make_selectors(rng, p, sk, arbitrary, count, plant=False):
    """`count` TGSW samples int32 [count][l][k+1][k+1][N]: encryptions of random bits under sk; with `arbitrary` each is, by a coin,
    arbitrary words instead, and `plant` puts test_tlwe_levels._setup's extreme rows into selectors 0 and 1."""
    from tfhe_jl_amd import leveled
    t = leveled.tgsw_encrypt_bits(rng, sk, rng.integers(0, 2, count))
    if arbitrary:
        for s in np.nonzero(rng.random(count) < 0.4)[0]:
            t[s] = _words(rng, p.l, p.k + 1, p.k + 1, p.N)
        if plant:
            t[0] = _words(rng, p.l, p.k + 1, p.k + 1, p.N)
            t[1] = _words(rng, p.l, p.k + 1, p.k + 1, p.N)
            t[0, 0, 0, 0, :] = 2**31 - 1
            t[1, 0, 0, p.k, :] = -2**31
    return np.ascontiguousarray(t, np.int32)


# ---- the generator ----------------------------------------------------------------------------------------------------------------------
class Generator:
    """The steps of a program for parameters p = (n, N, k, l), drawn from `rng`.  `sk` encrypts the real selectors; with `arbitrary` (the
    set is exact for any key words) a selector is, by a coin, arbitrary words instead.  The wire-side levels come from
    wire_table_model.Generator (self.g), which shares the generator's rng and table size.  What was written by a level lately is
    preferred as an operand (hot_slots, hot_wires), so that levels read what levels wrote."""

    def __init__(self, rng, p, sk, arbitrary, acc=False):
        self.rng, self.p, self.sk, self.arbitrary, self.acc = rng, p, sk, arbitrary, acc
        self.g = M.Generator(rng, p.n + 1)
        self.nets = make_nets(p.N)
        self.slots = self.S = self.S_seen = 0
        self.spec = -1
        self.refusal_at, self.update_at, self.special_at = (int(rng.integers(0, m)) for m in (len(REFUSALS), len(UPDATES), len(SPECIALS)))
        self.hot_slots, self.hot_wires = [], []
        self.tables = _words(rng, M.N_TV, p.N)
        self.refusals = REFUSALS
        if acc:                                                                   # (nothing is drawn for it otherwise: acc=False draws what it drew)
            self.refusals = tuple(w for pair in zip(ACC_REFUSALS + ACC_REFUSALS[:2], REFUSALS[::-1]) for w in pair)      # in turn: one of each
            self.acc_special_at, self.rw_at = int(rng.integers(0, len(SPECIALS))), int(rng.integers(0, len(V3_RWS)))

    W = property(lambda self: self.g.W)

    # -- tables and selectors
    def wires_alloc(self):
        rng, n, N = self.rng, self.p.n, self.p.N
        W = int(rng.integers(WIRE_RANGE[0], WIRE_RANGE[1] + 1))
        while W == self.g.W:
            W = int(rng.integers(WIRE_RANGE[0], WIRE_RANGE[1] + 1))
        self.g.W, self.hot_wires = W, []
        data = _words(rng, W, n + 1)
        half = 2**32 // (2 * N) // 2                                              # (test_tlwe_levels._setup's planted words)
        data[1, :6] = [2**31 - 1, -2**31, half - 1, half, -half - 1, -half]
        data[4, n - 1], data[4, n - 2], data[4, n] = 0, 2**30, 3 * half - 1
        return [Step(kind="wires_alloc", W=W), Step(kind="wires_upload", first=0, data=data)]

    def tlwe_alloc(self):
        rng, p = self.rng, self.p
        slots = int(rng.integers(SLOT_RANGE[0], SLOT_RANGE[1] + 1))
        while slots == self.slots:
            slots = int(rng.integers(SLOT_RANGE[0], SLOT_RANGE[1] + 1))
        self.slots, self.hot_slots = slots, []
        data = _words(rng, slots, p.k + 1, p.N)
        data[0], data[1] = 2**31 - 1, -2**31
        return [Step(kind="tlwe_alloc", slots=slots), Step(kind="tlwe_upload", first=0, data=data)]

    def tlwe_upload(self):
        rng = self.rng
        count = int(rng.integers(1, 7))
        first = int(rng.integers(0, self.slots - count + 1))
        if self.hot_slots and rng.random() < 0.6:                                 # over a slot a level wrote
            first = min(max(int(self.hot_slots[-1]) - int(rng.integers(0, count)), 0), self.slots - count)
        return Step(kind="tlwe_upload", first=first, data=_words(rng, count, self.p.k + 1, self.p.N))

    def wires_upload(self):
        s = self.g.upload()
        s["kind"] = "wires_upload"
        return s

    def _selectors(self, count, plant=False):
        return make_selectors(self.rng, self.p, self.sk, self.arbitrary, count, plant)

    def tgsw_load(self, count=None, plant=False):
        n = self.p.n
        while count is None or count == self.S:
            count = int(self.rng.integers(n + 2, n + 5))
        self.S, self.S_seen = count, max(self.S_seen, count)
        return Step(kind="tgsw_load", data=self._selectors(count, plant))

    def tgsw_update(self):
        n, S = self.p.n, self.S
        how = UPDATES[self.update_at % len(UPDATES)]
        self.update_at += 1
        first, count = {"first_0": (0, int(self.rng.integers(1, 3))), "last": (S - 1, 1), "straddles_n": (n - 1, int(self.rng.integers(2, 4))),
                        "whole": (0, S)}[how]
        return Step(kind="tgsw_update", how=how, first=first, data=self._selectors(count))

    # -- the two TLWE levels
    def _prefer(self, pool, hot, count, p=0.5):
        """`count` draws from pool, each by a coin from the hot ones that are in the pool."""
        hot = [h for h in hot[-6:] if h in set(pool.tolist())]
        return np.array([int(self.rng.choice(hot)) if hot and self.rng.random() < p else int(self.rng.choice(pool)) for _ in range(count)], np.int32)

    def rotate(self, form=None, min_B=1, special="turn"):
        """[steps]: the rotation, behind an upload of the planted wire when the row `skip_last` is due."""
        if special == "turn":
            special = SPECIALS[self.special_at % len(SPECIALS)]
            self.special_at += 1
        B = int(self.rng.integers(min_B, 5))
        return self._rotation("rotate", B, form, N_OUTS, special)

    def acc_rotate(self, form=None, min_B=1, special="turn"):
        """[steps]: `rotate` without sel, B up to 9, n_out 1, 2 or 8 with B n_out at most half the wires."""
        rng = self.rng
        if special == "turn":
            special = SPECIALS[self.acc_special_at % len(SPECIALS)]
            self.acc_special_at += 1
        B = max(int(rng.choice(ACC_B)) if rng.random() < 0.5 else int(rng.integers(1, 10)), min_B)
        return self._rotation("acc_rotate", B, form, [v for v in ACC_N_OUTS if B * v <= self.W // 2], special)

    def _rotation(self, kind, B, form, n_outs, special):
        """A rotation level of B rows; only `rotate` has a sel."""
        rng, n, N = self.rng, self.p.n, self.p.N
        form = int(rng.choice((0, 2))) if form is None else form
        every_slot, every_wire = np.arange(self.slots, dtype=np.int32), np.arange(self.W, dtype=np.int32)
        n_out, out_slot, out_wires = 1, None, None
        if form == 0:
            out_slot = rng.choice(self.slots, B, replace=False).astype(np.int32)
            acc = self._prefer(np.setdiff1d(every_slot, out_slot), self.hot_slots, B)
            pool = every_wire
        else:
            n_out = int(rng.choice(n_outs))
            out_wires = rng.choice(self.W, B * n_out, replace=False).astype(np.int32)
            acc = self._prefer(every_slot, self.hot_slots, B)
            pool = np.setdiff1d(every_wire, out_wires)
        if B >= 2 and rng.random() < 0.5:
            acc[1] = acc[0]                                                       # one accumulator, two rows
        counts = rng.integers(0, 5, B)
        cst = None if rng.random() < 0.25 else _words(rng, B)
        row = int(rng.integers(0, B))
        if special in ("copy", "mask_zero"):
            counts[row] = 0
            if cst is not None:
                cst[row] = 0 if special == "copy" else 3 * (2**32 // (2 * N)) + 5
            elif special == "mask_zero":
                cst = _words(rng, B)
                cst[row] = 3 * (2**32 // (2 * N)) + 5
        elif special == "skip_last":
            counts[row] = 1
        start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        T = int(start[-1])
        wire = self._prefer(pool, self.hot_wires, T)
        u = rng.random(T)
        coef = np.where(u < 0.4, rng.integers(-3, 4, T), np.where(u < 0.8, rng.integers(-2**31, 2**31, T), np.where(u < 0.9, -2**31, 2**31 - 1))).astype(np.int32)
        before = []
        if special == "skip_last":
            planted = _words(rng, 1, n + 1)
            planted[0, n - 1] = int(rng.choice((0, 2**32 // (2 * N) // 2 - 1, -(2**32 // (2 * N) // 2))))      # every one switches to exponent 0
            planted[0, n - 2] = 2**30
            w = int(rng.choice(pool))
            wire[start[row]], coef[start[row]] = w, 1
            before = [Step(kind="wires_upload", first=w, data=planted)]
        sel = None if kind != "rotate" or rng.random() < 0.4 else rng.permutation(self.S)[:n].astype(np.int32)
        s = Step(kind=kind, B=B, special=special, acc_slot=acc, start=start, wire=wire, coef=coef, cst=cst, sel=sel, n_out=n_out, out_form=form,
                 out_slot=out_slot, out_wires=out_wires)
        return before + [s]

    def acc_batch(self):
        """Engine.bootstrap_acc on host buffers: arbitrary accumulators and LWE words; a read."""
        rng, p = self.rng, self.p
        T, B, form = int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(0, 3))
        index = None if rng.random() < 0.3 else rng.integers(0, T, B).astype(np.int32)
        return Step(kind="acc_batch", B=B, acc=_words(rng, T, p.k + 1, p.N), rows=_words(rng, B, p.n + 1), acc_index=index, out_form=form,
                    n_out=int(rng.choice(BATCH_N_OUTS)) if form else 1)

    def option(self):
        if self.acc and self.rng.random() < 0.7:
            self.rw_at += 1
            return Step(kind="option", v3_rw=V3_RWS[self.rw_at % len(V3_RWS)])
        self.spec = -self.spec
        return Step(kind="option", anyn_spec=self.spec)

    def net(self, form=None, name=None):
        rng, slots = self.rng, self.slots
        name = name or str(rng.choice(NETS))
        net, E, F, V = self.nets[name]
        B = int(rng.integers(1, 4))
        G = B * F
        form = int(rng.choice((0, 2))) if form is None else form
        sel = rng.integers(0, self.S, (B, V)).astype(np.int32)
        out_first, out_wires, how = 0, None, "wires"
        legal = list(range(slots - E + 1))
        if form == 2:
            out_wires = rng.choice(self.W, G, replace=False).astype(np.int32)
            ranges = rng.random() < 0.7
        else:
            ranges = rng.random() < 0.75
            if not ranges:
                out_first, how = int(rng.integers(E, slots - G + 1)), "absolute"
            else:
                how = str(rng.choice(("below", "end", "any")))
                out_first = {"below": 0, "end": slots - G, "any": int(rng.integers(0, slots - G + 1))}[how]
                legal = [f for f in legal if f + E <= out_first or f >= out_first + G]
                if not legal:
                    how, out_first = "below", 0
                    legal = list(range(G, slots - E + 1))
        first = None
        if ranges:
            hot = [f for f in legal if any(f <= h < f + E for h in self.hot_slots[-4:])]
            f0 = int(rng.choice(hot if hot and rng.random() < 0.6 else legal))
            near = [f for f in legal if f != f0 and abs(f - f0) < E]
            first = np.array([f0] + [int(rng.choice(near if near and rng.random() < 0.7 else legal)) for _ in range(B - 1)], np.int32)
        return Step(kind="net", name=name, net=net, E=E, F=F, B=B, sel=sel, table_first=first, out_form=form, out_first=out_first, out_wires=out_wires, how=how)

    def level_code(self, lv):
        return level_code(lv, self.slots, self.W, self.p.N, self.S)

    def refused(self):
        """[steps]: the refused call (otherwise a valid one), behind a smaller tgsw_load where `sel_beyond` needs one."""
        rng = self.rng
        why = self.refusals[self.refusal_at % len(self.refusals)]
        self.refusal_at += 1
        before = []
        if why == "out_is_acc":
            lv = self.rotate(0, special=None)[0]
            lv.out_slot[-1] = lv.acc_slot[0]
        elif why == "acc_out_is_acc":
            lv = self.acc_rotate(0, special=None)[0]
            lv.out_slot[-1] = lv.acc_slot[0]
        elif why == "acc_slot_twice":
            lv = self.acc_rotate(0, min_B=2, special=None)[0]
            lv.out_slot[-1] = lv.out_slot[0]
        elif why == "acc_term_is_out":
            lv = self.acc_rotate(2, special=None)[0]
            while len(lv.wire) == 0:
                lv = self.acc_rotate(2, special=None)[0]
            lv.wire[-1] = lv.out_wires[0]
        elif why == "acc_out_form_1":
            lv = self.acc_rotate(special=None)[0]
            lv["out_form"] = 1
        elif why == "slot_twice":
            lv = self.rotate(0, min_B=2, special=None)[0]
            lv.out_slot[-1] = lv.out_slot[0]
        elif why == "out_meets_read":
            lv = self.net(0)
            lo = 0 if lv.table_first is None else int(lv.table_first[-1])
            lv["out_first"] = min(lo + lv.E - 1, self.slots - lv.B * lv.F)        # the last row's range holds the first output slot
        elif why == "term_is_out":
            lv = self.rotate(2, special=None)[0]
            while len(lv.wire) == 0:
                lv = self.rotate(2, special=None)[0]
            lv.wire[-1] = lv.out_wires[0]
        elif why == "out_form_1":
            lv = self.rotate(special=None)[0] if rng.random() < 0.5 else self.net()
            lv["out_form"] = 1
        else:
            if self.S_seen <= self.S:                                             # (the first set has n + 3 selectors at least)
                before = [self.tgsw_load(int(rng.integers(self.p.n + 2, self.S)))]
            if rng.random() < 0.5:
                lv = self.rotate(special=None)[0]
                lv["sel"] = rng.permutation(self.S)[:self.p.n].astype(np.int32)
                lv.sel[int(rng.integers(0, self.p.n))] = self.S
            else:
                lv = self.net()
                lv.sel[-1, -1] = self.S
        return before + [Step(kind="refused", why=why, level=lv, code=self.level_code(lv))]

    def note(self, s):
        """What the step wrote, for the preferences of later steps."""
        if s.kind in ("rotate", "acc_rotate"):
            if s.out_form == 0:
                self.hot_slots += s.out_slot.tolist()
            else:
                self.hot_wires += s.out_wires.tolist()
        elif s.kind == "net":
            if s.out_form == 0:
                self.hot_slots += list(range(s.out_first, s.out_first + s.B * s.F))
            else:
                self.hot_wires += s.out_wires.tolist()
        elif s.kind == "gates":
            self.hot_wires += s.out.tolist()[:3]


def level_code(lv, slots, W, N, S):
    """The code of a TLWE level call on tables of `slots` slots and W wires with S selectors loaded: model_blind_rotate_level /
    model_rot_net_level of tests/test_tlwe_levels.py; those take the state and the keys as in order, so a selector index beyond the
    loaded count is refused here, behind them, as the library does."""
    if lv.kind in ("rotate", "acc_rotate"):
        code, sel = model_blind_rotate_level(slots, W, N, lv.acc_slot, lv.start, lv.wire, lv.n_out, lv.out_form, lv.out_slot, lv.out_wires), lv.sel
    else:
        code, sel = model_rot_net_level(slots, W, lv.E, lv.F, lv.B, lv.table_first, lv.out_form, lv.out_first, lv.out_wires), lv.sel
    if code == OK and sel is not None and ((np.asarray(sel) < 0) | (np.asarray(sel) >= S)).any():
        code = INVALID
    return code


def level_size(s):
    """The rows a level's (or an acc_batch's) workspaces are sized for: rotations of a gate level, B F of a network, B n_out otherwise."""
    if s.kind == "gates":
        return M.rotations(s.ops)
    return s.B * (s.F if s.kind == "net" else s.get("n_out", 1))


def steps_digest(progs):
    """SHA-1 over the steps of the programs in order: each step's kind, then every field in order (an array's dtype, shape and bytes, a
    nested level likewise, numbers, strings and None by value)."""
    h = hashlib.sha1()

    def feed(s):
        h.update(b"<" + str(s["kind"]).encode())
        for key, v in s.items():
            if isinstance(v, np.ndarray):
                h.update(f"|{key}:{v.dtype.str}{v.shape}".encode())
                h.update(np.ascontiguousarray(v).tobytes())
            elif isinstance(v, dict):
                h.update(f"|{key}:".encode())
                feed(v)
            elif v is None or isinstance(v, (bool, int, str, np.integer)):
                h.update(f"|{key}={v}".encode())
        h.update(b">")

    for prog in progs:
        h.update(b"[")
        for s in prog:
            feed(s)
        h.update(b"]")
    return h.hexdigest()


def make_program(seed, steps, p, sk, arbitrary, acc=False):
    """`steps` steps; the last two download both whole tables.  acc: acc_rotate and acc_batch steps, v3_rw options and the acc_ refusals
    as well (without it the draws are those of the programs committed before these existed: steps_digest)."""
    rng = np.random.default_rng(seed)
    g = Generator(rng, p, sk, arbitrary, acc)
    prog = g.wires_alloc() + g.tlwe_alloc() + [g.tgsw_load(int(rng.integers(p.n + 3, p.n + 5)), plant=True)]
    kinds = ["rotate", "net", "gates", "linear", "lut", "tlwe_upload", "wires_upload", "tgsw_load", "tgsw_update", "tlwe_download", "wires_download",
             "wires_gather", "option", "refused", "tlwe_alloc", "wires_alloc"]
    weight = np.array([0.21, 0.19, 0.09, 0.03, 0.05, 0.06, 0.03, 0.03, 0.07, 0.05, 0.02, 0.03, 0.04, 0.07, 0.015, 0.015])
    if acc:
        kinds, weight = kinds + ["acc_rotate", "acc_batch"], np.array([0.10, 0.10, 0.10, 0.02, 0.04, 0.04, 0.02, 0.02, 0.05, 0.03, 0.01, 0.02, 0.09, 0.10, 0.015, 0.015, 0.26, 0.08])
    while len(prog) < steps - 2:
        kind = kinds[int(rng.choice(len(kinds), p=weight / weight.sum()))]
        if len(prog) == steps - 3 and kind in ("rotate", "acc_rotate", "refused", "tlwe_alloc", "wires_alloc"):      # room for one step: these may take two
            continue
        if kind == "rotate":
            new = g.rotate()
        elif kind == "net":
            new = [g.net()]
        elif kind == "gates":
            new = [g.g.gates(max_gates=8)]
        elif kind == "linear":
            new = [g.g.linear()]
        elif kind == "lut":
            new = [g.g.lut(g.tables)]
        elif kind == "tlwe_upload":
            new = [g.tlwe_upload()]
        elif kind == "wires_upload":
            new = [g.wires_upload()]
        elif kind == "tgsw_load":
            new = [g.tgsw_load()]
        elif kind == "tgsw_update":
            new = [g.tgsw_update()]
        elif kind == "tlwe_download":
            first = int(rng.integers(0, g.slots - 1))
            new = [Step(kind="tlwe_download", first=first, count=int(rng.integers(1, g.slots - first + 1)))]
        elif kind == "wires_download":
            first = int(rng.integers(0, g.W - 1))
            new = [Step(kind="wires_download", first=first, count=int(rng.integers(1, g.W - first + 1)))]
        elif kind == "wires_gather":
            new = [Step(kind="wires_gather", wires=rng.integers(0, g.W, int(rng.integers(1, 2 * g.W))).astype(np.int32))]
        elif kind == "option":
            new = [g.option()]
        elif kind == "acc_rotate":
            new = g.acc_rotate()
        elif kind == "acc_batch":
            new = [g.acc_batch()]
        elif kind == "refused":
            new = g.refused()
        elif kind == "tlwe_alloc":
            new = g.tlwe_alloc()
        else:
            new = g.wires_alloc()
        for s in new:
            g.note(s)
        prog += new
    prog += [Step(kind="tlwe_download", first=0, count=g.slots), Step(kind="wires_download", first=0, count=g.W)]
    return prog


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def read_of(tlwe, wires, s):
    if s.kind == "tlwe_download":
        return tlwe[s.first:s.first + s.count].copy()
    return wires[s.first:s.first + s.count].copy() if s.kind == "wires_download" else wires[s.wires].copy()


class Model:
    """p: (n, N, k, l, beta); arith: wire_table_model.single_key_arith (the wire-side levels); ks_sb: leveled_ref.ks_schoolbook of the
    cloud key.  run(program) -> per step (the words a read must return or None, the TLWE table after the step, the wire table after it).
    Rotations, network rows and keyswitches are memoised by their operand words and the selector set's digest: a run under an emulated
    fault computes only what the fault changed."""

    def __init__(self, p, arith, ks_sb, key_selectors=None):
        """key_selectors: leveled.bootstrap_key_selectors(ck), for programs with acc_rotate / acc_batch steps: those rotate with a second
        Rotation over it, built once, selector i at step i whatever set is loaded."""
        self.p, self.arith, self.ks_sb = p, arith, ks_sb
        self.memo, self.refs = {}, {}
        self.ref = self.set_id = self.tgsw = self.acc_ref = None
        self.events = collections.Counter()
        if key_selectors is not None:
            from test_blind_rotate import Rotation
            self.acc_ref = Rotation(p.N, p.k, p.l, p.beta, np.ascontiguousarray(key_selectors, np.int32))

    # -- arithmetic
    def load(self, tgsw):
        """The selector set: the Rotation (a Tree) over it is rebuilt whenever its words change."""
        from test_blind_rotate import Rotation
        p = self.p
        self.tgsw = np.ascontiguousarray(tgsw, np.int32)
        self.set_id = hashlib.sha1(self.tgsw.tobytes()).digest()
        if self.set_id not in self.refs:
            self.refs[self.set_id] = Rotation(p.N, p.k, p.l, p.beta, self.tgsw)
        self.ref = self.refs[self.set_id]

    def exponents(self, x):
        return [int(e) % (2 * self.p.N) for e in self.ref.sb.modswitch(x)]

    def rotation(self, acc, x, sel, before_last=False):
        """Rotation.rotate_lwe(acc, x, sel): int32 [k+1][N].  before_last (a fault): without the last step whose exponent is not 0."""
        key = ("rot", self.set_id, acc.tobytes(), x.tobytes(), None if sel is None else tuple(int(v) for v in sel), before_last)
        if key not in self.memo:
            if before_last:
                w = self.ref.sb.modswitch(x)
                exps = list(w[:-1])
                live = [i for i, e in enumerate(exps) if int(e) % (2 * self.p.N)]
                if live:
                    exps[live[-1]] = 0
                out = self.ref.rotate(acc, exps, w[-1], sel)
            else:
                out = self.ref.rotate_lwe(acc, x, sel)
            self.memo[key] = out.astype(np.int32)
        return self.memo[key]

    def acc_rotation(self, acc, x, fault=None):
        """The same with the bootstrapping key's entries as the selectors, entry i at step i (memo keys tagged "acc": never `rotation`'s)."""
        how = fault if fault in ("acc_uses_loaded_selectors", "acc_mask_from_zero", "acc_barb_dropped") else None
        if how == "acc_uses_loaded_selectors":
            return self.rotation(acc, x, None)
        key = ("acc", acc.tobytes(), x.tobytes(), how)
        if key not in self.memo:
            w = self.acc_ref.sb.modswitch(x)
            if how == "acc_mask_from_zero":
                acc = acc.copy()
                acc[:self.p.k] = 0
            self.memo[key] = self.acc_ref.rotate(acc, w[:-1], 0 if how == "acc_barb_dropped" else w[-1]).astype(np.int32)
        return self.memo[key]

    def net_row(self, name, net, table, sels):
        """leveled_ref.rot_net_ref over the Tree (a CmuxNet as its rotation-0 case): int32 [F][k+1][N]."""
        import leveled_ref
        key = ("net", self.set_id, name, np.ascontiguousarray(table).tobytes(), tuple(int(v) for v in sels))
        if key not in self.memo:
            fn = leveled_ref.rot_net_ref if hasattr(net, "degree") else leveled_ref.net_ref
            self.memo[key] = fn(self.ref, net, table, [int(v) for v in sels]).astype(np.int32)
        return self.memo[key]

    def extract(self, tlwe, c):
        return self.ref.extract_at(tlwe, c).astype(np.int32)

    def keyswitch(self, ext):
        """leveled_ref.ks_ref row by row: int32 [...][n+1]."""
        import leveled_ref
        ext = np.ascontiguousarray(ext, np.int32)
        flat = ext.reshape(-1, ext.shape[-1])
        for row in flat:
            if ("ks", row.tobytes()) not in self.memo:
                self.memo["ks", row.tobytes()] = leveled_ref.ks_ref(self.ks_sb, row[None])[0]
        return np.stack([self.memo["ks", row.tobytes()] for row in flat]).reshape(ext.shape[:-1] + (self.p.n + 1,))

    # -- the two TLWE levels: ("tlwe" or "wires", destinations, rows), written in that order
    def rotate_level(self, s, tlwe, wires, fault=None, count=False):
        p, ev = self.p, self.events
        x = form_rows(wires, s.start, s.wire, s.coef, None if fault == "cst_dropped" else s.cst)
        sel = None if fault == "sel_ignored" else s.sel
        if count:
            for g in range(s.B):
                e = self.exponents(x[g])
                ev["copy_row"] += int(not any(e))
                ev["last_step_skipped"] += int(e[p.n - 1] == 0 and e[p.n - 2] != 0)
        res = np.stack([self.rotation(tlwe[a], x[g], sel, fault == "other_sample") for g, a in enumerate(s.acc_slot)])
        if s.out_form == 0:
            return "tlwe", (np.sort(s.out_slot) if fault == "out_slot_order" else s.out_slot), res
        stride = 1 if fault == "extract_stride" else p.N // s.n_out
        ext = np.stack([[self.extract(r, j * stride) for j in range(s.n_out)] for r in res])
        rows = self.keyswitch(ext).reshape(s.B * s.n_out, p.n + 1)
        return "wires", (np.sort(s.out_wires) if fault == "dst_order" else s.out_wires), rows

    def acc_rotate_level(self, s, tlwe, wires, fault=None, count=False):
        """tfhe_bootstrap_acc_level: rotate_level with sel None over the key's own selectors."""
        p, ev = self.p, self.events
        x = form_rows(wires, s.start, s.wire, s.coef, s.cst)
        if count:
            for g in range(s.B):
                e = self.exponents(x[g])
                ev["acc_rotate_copy_row"] += int(not any(e))
                ev["acc_rotate_last_step_skipped"] += int(e[p.n - 1] == 0 and e[p.n - 2] != 0)
        slots = [s.acc_slot[0]] * s.B if fault == "acc_first_rows_slot" else s.acc_slot
        res = np.stack([self.acc_rotation(tlwe[a], x[g], fault) for g, a in enumerate(slots)])
        if s.out_form == 0:
            return "tlwe", (np.arange(s.B) if fault == "acc_out_index_ignored" else s.out_slot), res
        rows = self.keyswitch(self.extractions(res, s.n_out, fault)).reshape(s.B * s.n_out, p.n + 1)
        return "wires", s.out_wires, rows

    def extractions(self, res, n_out, fault=None):
        stride = 1 if fault == "acc_extract_stride" else self.p.N // n_out
        return np.stack([[self.extract(r, j * stride) for j in range(n_out)] for r in res])

    def acc_batch(self, s, fault=None, stale_rows=None):
        """Engine.bootstrap_acc: the words it must return, by out_form [B][k+1][N], [B][n_out][kN+1] or [B][n_out][n+1]."""
        x = s.rows
        if fault == "acc_batch_stale_rows" and stale_rows is not None:
            x = stale_rows[np.arange(s.B) % len(stale_rows)]
        index = np.zeros(s.B, np.int32) if s.acc_index is None else s.acc_index
        if fault == "acc_first_rows_slot":
            index = np.full(s.B, index[0])
        res = np.stack([self.acc_rotation(s.acc[a], x[g], fault) for g, a in enumerate(index)])
        if s.out_form == 0:
            return res
        ext = self.extractions(res, s.n_out, fault)
        return ext if s.out_form == 1 else self.keyswitch(ext)

    def net_level(self, s, tlwe, fault=None):
        p = self.p
        B, E, F = s.B, s.E, s.F
        first = [0] * B if s.table_first is None else [int(f) for f in s.table_first]
        if fault == "first_ignored":
            first = [first[0]] * B
        res = np.stack([self.net_row(s.name, s.net, tlwe[first[g]:first[g] + E], s.sel[g]) for g in range(B)])          # [B][F][k+1][N]
        at = np.array([g * (1 if fault == "net_out_stride" else F) + i for g in range(B) for i in range(F)])
        if s.out_form == 0:
            return "tlwe", s.out_first + at, res.reshape(B * F, p.k + 1, p.N)
        ext = np.stack([self.extract(r, 0) for r in res.reshape(B * F, p.k + 1, p.N)])
        return "wires", (np.sort(s.out_wires) if fault == "dst_order" else s.out_wires)[at], self.keyswitch(ext)

    # -- events
    def _uses(self, s):
        """The selectors a TLWE level multiplies by."""
        if s.kind == "net":
            nd = np.asarray(s.net.nodes)
            copies = (nd[:, 0] == nd[:, 1]) & ((nd[:, 3] == nd[:, 4]) if nd.shape[1] == 5 else True)
            return {int(s.sel[g, var]) for g in range(s.B) for var in nd[~copies, 2]}
        return set(range(self.p.n)) if s.sel is None else {int(v) for v in s.sel}

    def _count(self, s, st):
        """The events of a fault-free step, before it is applied.  st: slot_by / wire_by (who wrote it last), slot_writes (level writes in
        a row), used / renewed (selectors)."""
        ev = self.events
        if s.kind in TLWE_LEVELS:
            if s.kind == "rotate":
                slots_read = [int(a) for a in s.acc_slot]
                terms = [int(w) for w in s.wire[:s.start[-1]]]
                ev["rotate_reads_slot_written_by_net"] += int(any(st.slot_by[a] == "net" for a in slots_read))
                ev["rotate_term_wire_written_by_net"] += int(any(st.wire_by[w] == "net" for w in terms))
                ev["rotate_term_is_gate_output"] += int(any(st.wire_by[w] == "gates" for w in terms))
                ev["shared_acc_slot"] += int(len(set(slots_read)) < len(slots_read))
                ev["level_under_spec_global"] += int(st.spec == 1)
            else:
                first = [0] * s.B if s.table_first is None else [int(f) for f in s.table_first]
                slots_read = [f + e for f in first for e in range(s.E)]
                ev["net_reads_slot_written_by_rotate"] += int(any(st.slot_by[a] == "rotate" for a in slots_read))
                ev["overlapping_read_ranges"] += int(any(a != b and abs(a - b) < s.E for a in first for b in first))
                ev["outputs_below_read_ranges"] += int(s.out_form == 0 and s.table_first is not None and s.out_first + s.B * s.F <= min(first))
            ev["slot_rewritten_then_read"] += int(any(st.slot_writes[a] >= 2 for a in slots_read))
            uses = self._uses(s)
            ev["selector_used_before_and_after_update"] += int(bool(uses & st.renewed))
            st.renewed -= uses
            st.used |= uses
        elif s.kind == "gates":
            ev["gate_reads_wire_written_by_tlwe_level"] += int(any(st.wire_by[w] in TLWE_LEVELS for w in M.reads_of(s, 0, s.B)))
        elif s.kind == "tlwe_upload" and st.slot_by is not None and len(s.data) < len(st.slot_by):
            ev["upload_over_level_written_slot"] += int(any(st.slot_by[a] in TLWE_LEVELS for a in range(s.first, s.first + len(s.data))))
        elif s.kind == "tgsw_update":
            st.renewed |= st.used & set(range(s.first, s.first + len(s.data)))
        elif s.kind == "tgsw_load":
            st.used, st.renewed = set(), set()
            st.S_seen = max(st.S_seen, len(s.data))
        elif s.kind == "refused" and s.why == "sel_beyond":
            ev["sel_beyond_smaller_load_refused"] += int(len(self.tgsw) <= int(np.max(s.level.sel)) < st.S_seen)

    def _count_acc(self, s, st):
        """ACC_EVENTS, likewise.  st: rw (option v3_rw), before / before2 (the kinds of the two steps in front), selectors_changed (since the
        last acc_rotate), largest (level_size over the levels so far)."""
        ev = self.events
        if s.kind == "acc_rotate":
            slots_read = [int(a) for a in s.acc_slot]
            terms = [int(w) for w in s.wire[:s.start[-1]]]
            ev["acc_rotate_reads_slot_written_by_rotate"] += int(any(st.slot_by[a] == "rotate" for a in slots_read))
            ev["acc_rotate_reads_slot_written_by_net"] += int(any(st.slot_by[a] == "net" for a in slots_read))
            ev["acc_rotate_term_is_gate_output"] += int(any(st.wire_by[w] == "gates" for w in terms))
            ev["acc_rotate_directly_after_wire_level"] += int(st.before in M.LEVELS)
            ev["acc_rotate_after_selector_change"] += int(st.selectors_changed is True)
            ev["acc_rotate_rw4_with_padding"] += int(st.rw == 4 and s.B % 4 != 0)
            ev["acc_rotate_rw4_out_form_0"] += int(st.rw == 4 and s.out_form == 0)
            ev["acc_rotate_shared_acc_slot"] += int(len(set(slots_read)) < len(slots_read))
            ev["acc_rotate_larger_than_every_level_before"] += int(0 < st.largest < level_size(s))
            st.selectors_changed = False
        elif s.kind == "rotate":
            ev["rotate_or_net_reads_slot_written_by_acc_rotate"] += int(any(st.slot_by[int(a)] == "acc_rotate" for a in s.acc_slot))
        elif s.kind == "net":
            first = [0] * s.B if s.table_first is None else [int(f) for f in s.table_first]
            ev["rotate_or_net_reads_slot_written_by_acc_rotate"] += int(any(st.slot_by[f + e] == "acc_rotate" for f in first for e in range(s.E)))
        elif s.kind == "gates":
            ev["gate_reads_wire_written_by_acc_rotate"] += int(any(st.wire_by[w] == "acc_rotate" for w in M.reads_of(s, 0, s.B)))
        elif s.kind in ("tgsw_load", "tgsw_update") and st.selectors_changed is False:
            st.selectors_changed = True
        elif s.kind == "option" and "v3_rw" in s:
            st.rw = s.v3_rw
        if s.kind in M.LEVELS:
            ev["wire_level_directly_after_acc_rotate"] += int(st.before == "acc_rotate")
        if s.kind in LEVELS:
            ev["acc_batch_between_two_levels"] += int(st.before == "acc_batch" and st.before2 in LEVELS)
        if s.kind in LEVELS + ("acc_batch",):
            st.largest = max(st.largest, level_size(s))
        st.before2, st.before = st.before, s.kind

    def _wrote(self, s, st, what, dst):
        if what == "tlwe":
            for a in dst:
                st.slot_by[a] = s.kind
                st.slot_writes[a] += 1
        else:
            for w in dst:
                st.wire_by[w] = s.kind

    # -- a program
    def run(self, prog, fault=None, want=None):
        """Fault-free: the list of (read, TLWE table, wire table) per step, the events counted.  With `fault` and `want` (the fault-free
        reads): the index of the first read that differs, or None."""
        assert fault is None or (fault in FAULTS + ACC_FAULTS and want is not None)
        tlwe = wires = prev_tlwe = stale_rows = wire_level = None
        st = Step(slot_by=None, wire_by=None, slot_writes=None, used=set(), renewed=set(), S_seen=0, spec=-1,
                  rw=0, before=None, before2=None, selectors_changed=None, largest=0)
        res, refused = [], False
        for i, s in enumerate(prog):
            read, before = None, tlwe
            in_front, wire_level = wire_level, None                               # (what a gates, linear or lut step directly in front wrote over)
            if fault is None:
                self._count(s, st)
                self._count_acc(s, st)
            if s.kind == "tlwe_alloc":
                self.events["tlwe_realloc_with_live_wires"] += int(fault is None and tlwe is not None and wires is not None)
                tlwe = np.zeros((s.slots, self.p.k + 1, self.p.N), np.int32)
                st.slot_by, st.slot_writes = [None] * s.slots, [0] * s.slots
                if fault == "realloc_clobbers" and wires is not None:
                    wires = np.zeros_like(wires)
            elif s.kind == "wires_alloc":
                self.events["wires_realloc_with_live_tlwe"] += int(fault is None and tlwe is not None and wires is not None)
                wires = np.zeros((s.W, self.p.n + 1), np.int32)
                st.wire_by = [None] * s.W
                if fault == "realloc_clobbers" and tlwe is not None:
                    tlwe = np.zeros_like(tlwe)
            elif s.kind == "tlwe_upload":
                tlwe = tlwe.copy()
                tlwe[s.first:s.first + len(s.data)] = s.data
                for a in range(s.first, s.first + len(s.data)):
                    st.slot_by[a], st.slot_writes[a] = "upload", 0
            elif s.kind == "wires_upload":
                wires = wires.copy()
                wires[s.first:s.first + len(s.data)] = s.data
                for w in range(s.first, s.first + len(s.data)):
                    st.wire_by[w] = "upload"
            elif s.kind == "tgsw_load":
                self.load(s.data)
            elif s.kind == "tgsw_update":
                if fault != "stale_selectors":
                    t = self.tgsw.copy()
                    first = 0 if fault == "update_offset" else s.first
                    t[first:first + len(s.data)] = s.data
                    self.load(t)
            elif s.kind == "option":
                if "anyn_spec" in s:                                              # (v3_rw changes no word: the model ignores it)
                    st.spec = s.anyn_spec
            elif s.kind == "acc_batch":
                read = self.acc_batch(s, fault, stale_rows)
                stale_rows = s.rows
                if fault is not None and not np.array_equal(read, want[i]):
                    return i
            elif s.kind in LEVELS or (s.kind == "refused" and fault == "refused_writes_first" and s.why in REFUSALS[:4] + ACC_REFUSALS[:3]):
                lv = s.level if s.kind == "refused" else s
                stale = fault == "stale_slot" and prev_tlwe is not None and prev_tlwe.shape == tlwe.shape
                if lv.kind == "rotate":
                    what, dst, rows = self.rotate_level(lv, prev_tlwe if stale else tlwe, wires, fault, count=fault is None)
                elif lv.kind == "acc_rotate":
                    if fault == "acc_clobbers_wire_level" and s is lv and in_front is not None:      # that level's rows as they were before it
                        wires = wires.copy()
                        wires[in_front[0]] = in_front[1]
                    what, dst, rows = self.acc_rotate_level(lv, tlwe, wires, fault, count=fault is None)
                elif lv.kind == "net":
                    what, dst, rows = self.net_level(lv, prev_tlwe if stale else tlwe, fault)
                else:
                    what = "wires"
                    dst, rows = M.run_level(self.arith, wires, lv, 0, lv.B)
                    wire_level = (dst, wires[dst].copy()) if s is lv else None
                if what == "tlwe":
                    tlwe = tlwe.copy()
                    tlwe[dst] = rows
                else:
                    wires = wires.copy()
                    wires[dst] = rows
                if fault is None:
                    self._wrote(lv, st, what, [int(a) for a in dst])
            elif s.kind in READS:
                read = read_of(tlwe, wires, s)
                self.events["read_after_refused"] += int(fault is None and refused)
                if fault is not None and not np.array_equal(read, want[i]):
                    return i
            refused = s.kind == "refused" or (refused and s.kind == "option")
            prev_tlwe = before
            res.append((read, tlwe, wires))                                       # (tables are copied before they are written: these stay)
        return None if fault is not None else res
