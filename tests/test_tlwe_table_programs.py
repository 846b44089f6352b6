"""The device-resident TLWE table, the wire table and the loaded selector set driven by random programs against a host model
(tests/tlwe_table_model.py), and random circuits with TLWE nodes against the same arithmetic.

tests/test_tlwe_levels.py pins each level call to the host-buffer batch call on pristine tables; here the state on top is pinned: slots and
wires rewritten and read again, uploads over what a level wrote, tfhe_tgsw_update and tfhe_tgsw_load between levels that use the same
selector, re-allocation of one table while the other is live, anyn_spec toggled between levels, refused calls in the middle.  Every word
an engine returns is compared (np.array_equal, no row sampled) with exact integer arithmetic: form_rows, Rotation.rotate_lwe / extract_at,
rot_net_ref over a Tree, ks_ref, and the wire model's Oracle.gates / schoolbook LUT rows.  No engine call is a reference.

Two sets, (n, N, k, l, beta) = A (6, 128, 1, 3, 6), the wire programs' set, with an even step count, and B (7, 64, 2, 2, 10), k = 2 and an
odd one: each ping-pong sample ends up final in one of them.  Both are exact for any key words (SchemeParameters.exactness, asserted
against the engine's exact_domain), so selectors are a mix of real encryptions and arbitrary words with the planted extremes.

CPU: the committed programs hold the promised steps, reach every event of tlwe_table_model.EVENTS, and each of the thirteen emulated faults
(FAULTS) changes a word of some read; refusal codes are the model_*_level functions'; the planner of six random circuits issues every node
once, in order, with calls the model_*_level functions accept.  GPU (one device): every program free-running and checked (both whole tables
after every step, the first wrong step named), kernel names, refusal codes; every circuit word for word, twice."""
import collections
import time
from types import SimpleNamespace

import numpy as np
import pytest

import tlwe_table_model as T
import wire_table_model as M
from test_tlwe_levels import INVALID, OK, form_rows, model_blind_rotate_level, model_rot_net_level
from test_wire_table_programs import _call

SETS = {"A": (6, 128, 1, 3, 6), "B": (7, 64, 2, 2, 10)}                          # n, N, k, l, beta (t = 8, gamma = 2)
PROGRAMS = {"A": [(13, 31), (15, 25), (29, 39), (36, 35)],                        # (seed, steps): chosen until the CPU conditions below held
            "B": [(11, 31), (19, 40), (25, 31), (31, 38)]}
CIRCUITS = [1, 2, 3, 4, 5, 6]
CASES = [pytest.param(name, i, id=f"{name}-seed{seed}") for name in SETS for i, (seed, _) in enumerate(PROGRAMS[name])]
GATES2 = ("NAND", "OR", "AND", "XOR", "XNOR", "NOR", "ANDNY", "ANDYN", "ORNY", "ORYN")


AB_STEPS_SHA1 = "4a3638943731efac19672a05bb27bc83f35a80ce"        # tlwe_table_model.steps_digest of the eight programs, taken before the generator learnt acc=True


def build_set(tfhe, orc, name, programs=None, shape=None, acc=False):
    """Keys, reference arithmetic, the programs and the model's result of each (one Model: its memo and event counters span them).
    shape: (n, N, k, l, beta) of a set that is not in SETS; acc: programs with acc_rotate / acc_batch steps (tests/test_bootstrap_acc_programs.py)."""
    import leveled_ref
    from test_any_params import _setup
    from test_independent import Schoolbook
    from tfhe_jl_amd import leveled
    n, N, k, l, beta = shape or SETS[name]
    S = SimpleNamespace(name=name, p=SimpleNamespace(n=n, N=N, k=k, l=l, beta=beta), acc=acc)
    S.K = _setup(tfhe, orc, n, N, k, l, beta)
    S.arbitrary = S.K.params.exactness()[0] == 2
    sb = Schoolbook(n, N, k, l, beta, 8, 2, S.K.ck.bootstrap_key, S.K.ck.keyswitch_key)
    S.arith = M.single_key_arith(S.K.oracle, sb)
    S.model = T.Model(S.p, S.arith, leveled_ref.ks_schoolbook(S.K.params, S.K.ck.keyswitch_key), leveled.bootstrap_key_selectors(S.K.ck) if acc else None)
    S.seeds = PROGRAMS[name] if programs is None else programs
    S.progs = [T.make_program(seed, steps, S.p, S.K.sk, S.arbitrary, acc) for seed, steps in S.seeds]
    S.results = [S.model.run(p) for p in S.progs]
    return S


@pytest.fixture(scope="module")
def sets(tfhe, orc):
    """Both sets, computed once and left unchanged; the time is printed (profiles/tlwe_table_programs.txt)."""
    t0 = time.perf_counter()
    both = {name: build_set(tfhe, orc, name) for name in SETS}
    print(f"models of {sum(len(v) for v in PROGRAMS.values())} programs on two sets: {time.perf_counter() - t0:.1f} s")
    yield both
    for S in both.values():
        S.K.ck.close()


# ---- CPU: the programs ---------------------------------------------------------------------------------------------------------------------
def test_committed_programs_are_the_steps_they_were(sets):
    """The generator's acc=True steps changed no draw of acc=False: the eight programs, every kind and every array's bytes, in order."""
    assert T.steps_digest([p for name in SETS for p in sets[name].progs]) == AB_STEPS_SHA1
    assert not any(s.kind in ("acc_rotate", "acc_batch") or "v3_rw" in s or (s.kind == "refused" and s.why in T.ACC_REFUSALS)
                   for name in SETS for p in sets[name].progs for s in p)


def test_committed_programs_have_the_promised_steps(sets):
    for name, S in sets.items():
        n, N = S.p.n, S.p.N
        assert len(S.seeds) == 4 and all(25 <= steps <= 40 for _, steps in S.seeds) and [len(p) for p in S.progs] == [steps for _, steps in S.seeds]
        steps = [s for p in S.progs for s in p]
        kinds = collections.Counter(s.kind for s in steps)
        print(name, dict(kinds))
        assert set(kinds) == {"tlwe_alloc", "wires_alloc", "tlwe_upload", "wires_upload", "tgsw_load", "tgsw_update", "rotate", "net", "gates", "linear", "lut",
                              "tlwe_download", "wires_download", "wires_gather", "option", "refused"}, kinds
        assert kinds["tlwe_alloc"] > 4 and kinds["wires_alloc"] > 4                                   # re-allocation in the middle of a program
        for p in S.progs:
            for i, s in enumerate(p):
                if s.kind == "tlwe_alloc":
                    assert 12 <= s.slots <= 24 and p[i + 1].kind == "tlwe_upload" and p[i + 1].first == 0 and len(p[i + 1].data) == s.slots
                if s.kind == "wires_alloc":
                    assert 24 <= s.W <= 48 and p[i + 1].kind == "wires_upload" and p[i + 1].first == 0 and len(p[i + 1].data) == s.W
            assert [s.kind for s in p[-2:]] == ["tlwe_download", "wires_download"] and p[-2].first == p[-1].first == 0
            assert p[-2].count == len(S.results[S.progs.index(p)][-1][1]) and p[-1].count == len(S.results[S.progs.index(p)][-1][2])
        assert any(s.kind == "tlwe_upload" and s.first > 0 for s in steps) and any(s.kind == "wires_upload" and s.first > 0 for s in steps)
        loads = [len(s.data) for s in steps if s.kind == "tgsw_load"]
        assert set(loads) <= {n + 2, n + 3, n + 4} and len(set(loads)) >= 2
        assert {s.how for s in steps if s.kind == "tgsw_update"} == set(T.UPDATES)
        for s in steps:
            if s.kind == "tgsw_update":
                assert (s.how == "first_0") <= (s.first == 0) and (s.how == "straddles_n") <= (s.first < n < s.first + len(s.data))
        rot = [s for s in steps if s.kind == "rotate"]
        assert {s.B for s in rot} == {1, 2, 3, 4} and {s.out_form for s in rot} == {0, 2} and {s.n_out for s in rot if s.out_form == 2} == {1, 2, 4}
        assert any(s.sel is None for s in rot) and any(s.sel is not None and len(set(s.sel.tolist())) == n for s in rot)
        assert any(s.cst is None for s in rot) and any(s.cst is not None for s in rot)
        assert {int(c) for s in rot for c in np.diff(s.start)} == {0, 1, 2, 3, 4}
        coef = np.concatenate([s.coef.astype(np.int64) for s in rot])
        assert (np.abs(coef) <= 3).any() and (np.abs(coef) > 2**20).any() and (coef == -2**31).any() and (coef == 2**31 - 1).any()
        assert any(len(set(s.acc_slot.tolist())) < s.B for s in rot)                                  # repeated acc_slots
        rows = [(s, g) for s in rot for g in range(s.B) if s.start[g + 1] == s.start[g]]
        assert any(s.cst is None or s.cst[g] == 0 for s, g in rows)                                   # no terms, no constant: a copy
        assert any(s.cst is not None and s.cst[g] != 0 for s, g in rows)                              # no terms, a constant: every mask exponent 0
        assert any(s.special == "skip_last" for s in rot)                                             # (that it is skipped: the event last_step_skipped)
        for s in rot:                                                                                 # outputs anywhere the call does not read
            outs = s.out_slot if s.out_form == 0 else s.out_wires
            assert len(set(outs.tolist())) == len(outs) == s.B * s.n_out
            assert not set(outs.tolist()) & set((s.acc_slot if s.out_form == 0 else s.wire).tolist())
        nets = [s for s in steps if s.kind == "net"]
        assert {s.name for s in nets} == set(T.NETS) and {s.B for s in nets} == {1, 2, 3} and {s.out_form for s in nets} == {0, 2}
        assert any(s.table_first is None for s in nets) and {s.how for s in nets} >= {"wires", "absolute", "below", "end"}
        for p, res in zip(S.progs, S.results):
            for i, s in enumerate(p):
                if s.kind == "net" and s.how == "end":
                    assert s.out_form == 0 and s.out_first + s.B * s.F == len(res[i][1])              # ending at the last slot
                if s.kind == "net" and s.how == "below":
                    assert s.out_form == 0 and s.out_first == 0 and s.B * s.F <= min(s.table_first)   # below every read range
                if s.kind == "net" and s.table_first is not None:
                    assert 0 <= min(s.table_first) and max(s.table_first) + s.E <= len(res[i][1])
        assert any(s.out_form == 2 and (np.diff(s.out_wires) < 0).any() for s in nets)                # permuted wires
        assert {s.why for s in steps if s.kind == "refused"} == set(T.REFUSALS)
        assert {s.anyn_spec for s in steps if s.kind == "option"} == set(T.SPECS) == {-1, 1}
        assert any(s.kind == "wires_gather" and len(set(s.wires.tolist())) < len(s.wires) for s in steps)


def test_only_levels_change_the_model_and_each_changes_one_table(sets):
    same = lambda a, b: a is b or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))      # noqa: E731
    for S in sets.values():
        for p, res in zip(S.progs, S.results):
            for i, s in enumerate(p):
                tl, w, tl0, w0 = res[i][1], res[i][2], res[i - 1][1] if i else None, res[i - 1][2] if i else None
                if s.kind in ("refused", "option") + T.READS:
                    assert same(tl, tl0) and same(w, w0), (i, s.kind)
                    assert (res[i][0] is not None) == (s.kind in T.READS)
                if s.kind in T.LEVELS:
                    assert same(tl, tl0) != same(w, w0), (i, s.kind)                                  # exactly one of the two
                    assert same(w, w0) == (s.kind in T.TLWE_LEVELS and s.out_form == 0), (i, s.kind)
                if s.kind in ("tgsw_load", "tgsw_update"):
                    assert same(tl, tl0) and same(w, w0)


def test_committed_programs_reach_every_event(sets):
    """A condition on the seeds (they were chosen until it held)."""
    for name, S in sets.items():
        ev = S.model.events
        print(f"set {name}, events over the committed programs:", {k: ev[k] for k in T.EVENTS})
        assert all(ev[k] >= 1 for k in T.EVENTS), (name, {k: ev[k] for k in T.EVENTS if ev[k] < 1})


@pytest.mark.parametrize("fault", T.FAULTS)
def test_every_emulated_fault_changes_a_read(sets, fault):
    hits = []
    for name, S in sets.items():
        for (seed, _), p, res in zip(S.seeds, S.progs, S.results):
            at = S.model.run(p, fault, [r for r, _, _ in res])
            if at is not None:
                hits.append((name, seed, at))
    print(f"{fault}: a read differs in (set, seed, step) {hits}")
    assert {name for name, _, _ in hits} == set(SETS), (fault, hits)


def test_refusal_codes_are_the_level_models(sets):
    """Every refused step's code is model_blind_rotate_level / model_rot_net_level on the tables of that moment; a selector index beyond
    the loaded count — the one refusal those two leave to the state — is an otherwise valid call."""
    seen = collections.Counter()
    for S in sets.values():
        for p, res in zip(S.progs, S.results):
            count = 0
            for i, s in enumerate(p):
                if s.kind == "tgsw_load":
                    count = len(s.data)
                if s.kind != "refused":
                    continue
                lv, slots, W = s.level, len(res[i][1]), len(res[i][2])
                if lv.kind == "rotate":
                    code = model_blind_rotate_level(slots, W, S.p.N, lv.acc_slot, lv.start, lv.wire, lv.n_out, lv.out_form, lv.out_slot, lv.out_wires)
                else:
                    code = model_rot_net_level(slots, W, lv.E, lv.F, lv.B, lv.table_first, lv.out_form, lv.out_first, lv.out_wires)
                if s.why == "sel_beyond":
                    assert code == OK and int(np.max(lv.sel)) == count
                    code = INVALID
                assert s.code == code == INVALID == T.level_code(lv, slots, W, S.p.N, count), (i, s.why)
                seen[s.why, lv.kind] += 1
    print("refused steps:", dict(seen))
    assert {why for why, _ in seen} == set(T.REFUSALS)


def test_every_level_the_programs_run_is_a_valid_call(sets):
    ran = collections.Counter()
    for S in sets.values():
        for p, res in zip(S.progs, S.results):
            count = 0
            for i, s in enumerate(p):
                if s.kind == "tgsw_load":
                    count = len(s.data)
                if s.kind in T.TLWE_LEVELS:
                    assert T.level_code(s, len(res[i][1]), len(res[i][2]), S.p.N, count) == OK, (S.name, i, s.kind)
                    ran[s.kind] += 1
                if s.kind == "tgsw_update":
                    assert 0 <= s.first and s.first + len(s.data) <= count
    assert ran["rotate"] >= 30 and ran["net"] >= 30, ran


# ---- GPU: the programs ---------------------------------------------------------------------------------------------------------------------
def _level_call(eng, lv):
    if lv.kind == "rotate":
        return eng.blind_rotate_level(lv.acc_slot, lv.start, lv.wire, lv.coef, cst=lv.cst, sel=lv.sel, n_out=lv.n_out, out_form=lv.out_form,
                                      out_slot=lv.out_slot, out_wires=lv.out_wires)
    if lv.kind == "acc_rotate":
        return eng.bootstrap_acc_level(lv.acc_slot, lv.start, lv.wire, lv.coef, cst=lv.cst, n_out=lv.n_out, out_form=lv.out_form, out_slot=lv.out_slot,
                                       out_wires=lv.out_wires)
    if lv.kind == "net":
        return eng.rot_net_level(lv.net, lv.sel, table_first=lv.table_first, out_form=lv.out_form, out_first=lv.out_first, out_wires=lv.out_wires)
    return _call(eng, lv, lv.kind)


def _assert_rows(got, want, first, unit, what, index=None):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        g, w = got.reshape(len(got), -1), want.reshape(len(want), -1)
        bad = np.nonzero((g != w).any(axis=1))[0]
        at = int(bad[0]) + first if index is None else int(index[bad[0]])
        raise AssertionError(f"{what}: {len(bad)} {unit}s differ, the first is {unit} {at}: got {g[bad[0]][:4]} ..., want {w[bad[0]][:4]} ...")


def _replay(tfhe, eng, S, which, checked):
    """Runs the program on the engine; every read against the model; checked: both whole tables after every step as well."""
    p = S.p
    tag = f"set {S.name}, seed {S.seeds[which][0]}, {'checked' if checked else 'free-running'},"
    slots = W = rw = 0
    spec = -1
    eng.set_option("anyn_spec", -1)
    eng.set_option("v3_rw", 0)
    try:
        for i, (s, (want, tlwe, wires)) in enumerate(zip(S.progs[which], S.results[which])):
            what = f"{tag} step {i} ({s.kind})"
            if s.kind == "tlwe_alloc":
                eng.tlwe_alloc(s.slots)
                slots = s.slots
            elif s.kind == "wires_alloc":
                eng.wires_alloc(s.W)
                W = s.W
            elif s.kind == "tlwe_upload":
                eng.tlwe_upload(s.first, s.data)
            elif s.kind == "wires_upload":
                eng.wires_upload(s.first, s.data)
            elif s.kind == "tgsw_load":
                eng.tgsw_load(s.data)
            elif s.kind == "tgsw_update":
                eng.tgsw_update(s.first, s.data)
            elif s.kind == "option" and "v3_rw" in s:
                eng.set_option("v3_rw", s.v3_rw)
                rw = s.v3_rw
            elif s.kind == "option":
                eng.set_option("anyn_spec", s.anyn_spec)
                spec = s.anyn_spec
            elif s.kind == "acc_batch":
                got = eng.bootstrap_acc(s.acc, s.rows, acc_index=s.acc_index, n_out=s.n_out, out_form=s.out_form)
                assert eng.last_kernel_name() == _acc_name(p.l, rw == 4), (what, eng.last_kernel_name())
                _assert_rows(got, want, 0, "row", what)
            elif s.kind in T.LEVELS:
                _level_call(eng, s)
                if s.kind == "rotate":
                    assert eng.last_kernel_name() == f"tlwe_rotate_level_kernel(N={p.N},k={p.k},l={p.l},steps={p.n}{',spec=global' if spec == 1 else ''})", what
                elif s.kind == "acc_rotate":
                    assert eng.last_kernel_name() == _acc_name(p.l, rw == 4), (what, eng.last_kernel_name())
                elif s.kind == "net":
                    assert eng.last_kernel_name().startswith("rot_net_level_kernel("), (what, eng.last_kernel_name())
            elif s.kind == "refused":
                what += f", {s.why} ({s.level.kind})"
                with pytest.raises(tfhe.EngineError) as e:
                    _level_call(eng, s.level)
                assert e.value.code == s.code, (what, str(e.value))
            elif s.kind == "tlwe_download":
                _assert_rows(eng.tlwe_download(s.first, s.count), want, s.first, "slot", what)
            elif s.kind == "wires_download":
                _assert_rows(eng.wires_download(s.first, s.count), want, s.first, "wire", what)
            else:
                _assert_rows(eng.wires_gather(s.wires), want, 0, "wire", what, s.wires)
            if checked:                                                           # (a fresh table holds nothing to compare before its upload)
                if slots and s.kind != "tlwe_alloc":
                    _assert_rows(eng.tlwe_download(0, slots), tlwe, 0, "slot", what + ", the TLWE table after it")
                if W and s.kind != "wires_alloc":
                    _assert_rows(eng.wires_download(0, W), wires, 0, "wire", what + ", the wire table after it")
    finally:
        eng.set_option("anyn_spec", -1)
        eng.set_option("v3_rw", 0)


def _acc_name(l, rw4):
    from test_bootstrap_acc import _name
    return _name(l, rw4)


def _engine(S):
    eng = S.K.ck.engine(0)
    assert eng.exact_domain >= 1 and eng.exact_domain == S.K.params.exactness()[0]                    # (what chose the selectors' words)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", CASES)
def test_programs_free_running(tfhe, sets, name, which):
    """Only the program's own reads (the last two download both whole tables): levels queue up behind one another."""
    _replay(tfhe, _engine(sets[name]), sets[name], which, False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", CASES)
def test_programs_checked(tfhe, sets, name, which):
    """Both whole tables after every step: the first wrong step is named (kind, index, slot or wire, four words got / want), and the tables
    right after every refused call are the model's."""
    _replay(tfhe, _engine(sets[name]), sets[name], which, True)


# ---- random circuits with TLWE nodes -------------------------------------------------------------------------------------------------------
def make_circuit(seed, n, N, S=None):
    """A Circuit of 3 ... 5 wire inputs, 3 ... 6 TLWE inputs and 10 ... 16 nodes (two-input gates, rot_net, blind_rotate) over S loaded
    selectors (default n + 3), every sink wire an output; and the nodes in creation order:
    ("gate", name, a, b, wire) / ("rot_net", net name, [slots], [selectors], form, [outputs]) /
    ("blind_rotate", slot, [(wire, coef)], const, n_out, sel or None, form, [outputs])."""
    import tfhe_jl_amd as tfhe
    rng = np.random.default_rng(seed)
    S = S or n + 3
    nets = T.make_nets(N)
    c = tfhe.Circuit()
    wires = list(c.inputs(int(rng.integers(3, 6))))
    tl = list(c.tlwe_inputs(int(rng.integers(3, 7))))
    nodes, read = [], set()
    for _ in range(int(rng.integers(10, 17))):
        kind = str(rng.choice(("gate", "rot_net", "blind_rotate"), p=(0.3, 0.3, 0.4)))
        form = int(rng.choice((0, 2)))
        out = "tlwe" if form == 0 else "lwe"
        if kind == "gate":
            name, (a, b) = str(rng.choice(GATES2)), (int(w) for w in rng.choice(wires, 2))
            w = c.gate(name, a, b)
            nodes.append(("gate", name, a, b, w))
            read |= {a, b}
            wires.append(w)
        elif kind == "rot_net":
            name = str(rng.choice(T.NETS))
            net, E, F, V = nets[name]
            entries = [tl[int(i)] for i in rng.integers(max(0, len(tl) - 6), len(tl), E)]             # any earlier TLWE nodes, repeats allowed
            sel = [int(v) for v in rng.integers(0, S, V)]
            outs = c.rot_net(net, entries, sel, out=out)
            nodes.append(("rot_net", name, [t.slot for t in entries], sel, form, [o.slot if form == 0 else o for o in outs]))
            (tl if form == 0 else wires).extend(outs)
        else:
            T_ = int(rng.integers(0, 4))
            u = rng.random(T_)
            coef = np.where(u < 0.5, rng.integers(-3, 4, T_), np.where(u < 0.8, rng.integers(-2**31, 2**31, T_), np.where(u < 0.9, -2**31, 2**31 - 1)))
            terms = [(int(w), int(cf)) for w, cf in zip(rng.choice(wires, T_), coef)]
            const = int(rng.integers(-2**31, 2**31)) if rng.random() < 0.7 else 0
            n_out = int(rng.choice(T.N_OUTS)) if form == 2 else 1
            sel = None if rng.random() < 0.5 else [int(v) for v in rng.permutation(S)[:n]]
            acc = tl[int(rng.integers(0, len(tl)))]
            outs = c.blind_rotate(acc, terms, const=const, n_out=n_out, out=out, sel=sel)
            outs = outs if isinstance(outs, list) else [outs]
            nodes.append(("blind_rotate", acc.slot, terms, const, n_out, sel, form, [o.slot if form == 0 else o for o in outs]))
            read |= {w for w, _ in terms}
            (tl if form == 0 else wires).extend(outs)
    c.set_outputs([w for w in wires if w not in read])
    return c, nodes


def eval_circuit(model, nets, nodes, ins, tlwe_in, outputs):
    """The circuit node by node in creation order with the model's arithmetic (its selector set loaded): int32 [outputs][n+1]."""
    p = model.p
    wires, slots = {i: r for i, r in enumerate(ins)}, {i: t for i, t in enumerate(tlwe_in)}
    for nd in nodes:
        if nd[0] == "gate":
            _, name, a, b, w = nd
            wires[w] = model.arith.gates(np.array([M.OPS[name]], np.uint8), wires[a][None], wires[b][None], wires[a][None])[0]
            continue
        if nd[0] == "rot_net":
            _, name, entries, sel, form, outs = nd
            res = model.net_row(name, nets[name][0], np.stack([slots[e] for e in entries]), sel)
            ext_at = [0] * len(res)
        else:
            _, acc, terms, const, n_out, sel, form, outs = nd
            table = np.stack([wires[w] for w, _ in terms]) if terms else np.zeros((1, p.n + 1), np.int32)
            coef = np.array([cf for _, cf in terms], np.int64).astype(np.int32)
            cst = np.array([const], np.int64).astype(np.int32)
            x = form_rows(table, [0, len(terms)], np.arange(len(terms)), coef, cst)[0]
            res = [model.rotation(slots[acc], x, sel)] * n_out
            ext_at = [j * (p.N // n_out) for j in range(n_out)]
        for r, c_at, o in zip(res, ext_at, outs):
            if form == 0:
                slots[o] = r
            else:
                wires[o] = model.keyswitch(model.extract(r, c_at))
    return np.stack([wires[w] for w in outputs])


def test_circuit_generator_covers_the_node_kinds(tfhe):
    n, N = SETS["A"][:2]
    made = [make_circuit(seed, n, N) for seed in CIRCUITS]
    nodes = [nd for _, nds in made for nd in nds]
    assert all(10 <= len(nds) <= 16 and 3 <= c._n_inputs <= 5 and 3 <= c._n_tlwe_inputs <= 6 and c.outputs for c, nds in made)
    assert {nd[0] for nd in nodes} == {"gate", "rot_net", "blind_rotate"}
    nets = [nd for nd in nodes if nd[0] == "rot_net"]
    assert {nd[1] for nd in nets} == set(T.NETS) and {nd[4] for nd in nets} == {0, 2} and any(len(set(nd[2])) < len(nd[2]) for nd in nets)
    rots = [nd for nd in nodes if nd[0] == "blind_rotate"]
    assert {nd[6] for nd in rots} == {0, 2} and {nd[4] for nd in rots if nd[6] == 2} == {1, 2, 4}
    assert any(nd[5] is None for nd in rots) and any(nd[5] is not None for nd in rots) and any(nd[3] for nd in rots) and any(len(nd[2]) >= 2 for nd in rots)
    assert any(abs(cf) > 2**20 for nd in rots for _, cf in nd[2])
    inputs = [set(range(c._n_inputs)) for c, _ in made]
    assert any(w not in ins for (_, nds), ins in zip(made, inputs) for nd in nds if nd[0] == "blind_rotate" for w, _ in nd[2])      # a computed wire rotates
    assert any(s >= c._n_tlwe_inputs for c, nds in made for nd in nds if nd[0] == "rot_net" for s in nd[2])                         # a computed TLWE node is an entry


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("seed", CIRCUITS)
def test_planner_issues_every_node_once_in_order_with_valid_calls(tfhe, name, seed):
    n, N = SETS[name][:2]
    c, nodes = make_circuit(seed, n, N)
    slots, W = c.num_tlwe, c.num_wires
    have_w, have_t = set(range(c._n_inputs)), set(range(c._n_tlwe_inputs))
    issued = collections.Counter()
    for lv in c.level_plan(N):
        new_w, new_t = [], []
        assert not lv["lut"] and lv["linear"] is None
        if lv["gates"] is not None:
            ops, a, b, _, out = lv["gates"]
            assert set(a.tolist()) | set(b.tolist()) <= have_w
            new_w += out.tolist()
            issued.update(("gate", int(o)) for o in out)
        for acc, start, wire, coef, cst, sel, n_out, form, out_slot, out_wires in lv["blind_rotate"]:
            assert model_blind_rotate_level(slots, W, N, acc, start, wire, n_out, form, out_slot, out_wires) == OK
            assert len(cst) == len(acc) and (sel is None or len(sel) == n)
            assert set(acc.tolist()) <= have_t and set(wire.tolist()) <= have_w
            outs = (out_slot if form == 0 else out_wires).reshape(len(acc), n_out)
            (new_t if form == 0 else new_w).extend(outs.reshape(-1).tolist())
            issued.update(("blind_rotate", form, int(o[0])) for o in outs)
        for net, sel, form, out_first, out_wires in lv["rot_net"]:
            E, F = int(net.entries), int(net.widths[-1])
            assert model_rot_net_level(slots, W, E, F, 1, None, form, out_first, out_wires) == OK
            level0 = net.nodes[:int(net.widths[0])]
            assert E == int(level0[:, :2].max()) + 1 and set(level0[:, :2].reshape(-1).tolist()) <= have_t and sel.shape == (1, net.variables)
            outs = list(range(out_first, out_first + F)) if form == 0 else out_wires.tolist()
            (new_t if form == 0 else new_w).extend(outs)
            issued[("rot_net", form, int(outs[0]))] += 1
        assert not set(new_w) & have_w and not set(new_t) & have_t and len(set(new_w)) == len(new_w) and len(set(new_t)) == len(new_t)
        have_w |= set(new_w)                                                      # (what a level writes is read from the next level on)
        have_t |= set(new_t)
    want = collections.Counter(("gate", nd[4]) if nd[0] == "gate" else (nd[0], nd[-2], nd[-1][0]) for nd in nodes)
    assert issued == want and set(issued.values()) == {1}
    assert have_w == set(range(W)) and have_t == set(range(slots))


def _circuit_case(tfhe, S, seed):
    p = S.p
    count = p.n + 3
    rng = np.random.default_rng(1000 + seed)
    c, nodes = make_circuit(seed, p.n, p.N, count)
    tgsw = T.make_selectors(rng, p, S.K.sk, S.arbitrary, count, plant=True)
    ins, tl = T._words(rng, c._n_inputs, p.n + 1), T._words(rng, c._n_tlwe_inputs, p.k + 1, p.N)
    S.model.load(tgsw)
    return c, tgsw, ins, tl, eval_circuit(S.model, T.make_nets(p.N), nodes, ins, tl, c.outputs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("seed", CIRCUITS)
def test_gpu_random_circuit_equals_the_model_node_by_node(tfhe, sets, name, seed):
    S = sets[name]
    c, tgsw, ins, tl, want = _circuit_case(tfhe, S, seed)
    eng = _engine(S)
    eng.set_option("anyn_spec", -1)
    eng.tgsw_load(tgsw)
    got = c.run(S.K.ck, ins, tlwe_inputs=tl).data
    _assert_rows(got, want, 0, "output", f"set {name}, circuit {seed}", c.outputs)
    again = c.run(S.K.ck, ins, tlwe_inputs=tl).data
    assert np.array_equal(again, want), "the second run on the same cloud key"
