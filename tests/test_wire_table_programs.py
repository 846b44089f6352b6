"""The device-resident wire table driven by random programs against a host model (tests/wire_table_model.py).

The arithmetic under a level is pinned elsewhere; here the state on top of it is: rewrites of wires, uploads over them, reads in the middle
of a program, refused levels, re-allocation, and on multi-device contexts the replicas' validity and ownership, the pulls between them and
the per-shard re-basing of a level's arrays.  Every word an engine returns is compared with the model's (Oracle.gates / MKGateRef, combine,
the integer schoolbook's bootstrap_tv), no row sampled (but at the 80-bit set, where the sampling is stated).

CPU: the fault-free replica simulator (1, 2 and 3 replicas) equals the model on every read of every committed program; the committed
programs reach every event of wire_table_model.EVENTS; each of the ten emulated protocol faults (FAULTS) changes a word of some read; the
generator emits the shapes it promises; the shard mirror's device count on the closed cases.

GPU: every committed program free-running (its own reads, ending in a gather of the whole table) and checked (the whole table after every
step, the first wrong step named with its shard bounds and wire) on one device, on DEVICE_PAIRS and on three contexts on device 0; the
device count of every level against the mirror; every refusal's code and the table after it; one program at the 80-bit set; multi-key
programs (one device) with the cross-kind refusals."""
import collections

import numpy as np
import pytest

import wire_table_model as M
from conftest import DEVICE_PAIRS

PROGRAMS = [(28, 37), (3, 28), (14, 39), (4, 29), (11, 36), (37, 30)]             # (seed, steps): chosen until every event counter is >= 1
MK_PROGRAMS = [(2, 24), (7, 20)]
ENGINES = [pytest.param(0, id="one_device")] + DEVICE_PAIRS + [pytest.param([0, 0, 0], id="devices000")]
IDS = [f"seed{s}" for s, _ in PROGRAMS]
N, WIDTH, MK_WIDTH, MK_SK_WIDTH = 128, 7, 9, 5


class _Set:
    pass


@pytest.fixture(scope="module")
def sk(tfhe, orc):
    """N = 128, k = 1, n = 6, l = 3, beta = 6 (the gate_set of tests/test_keyswitch_edges.py): keys, reference arithmetic, the committed
    programs and the model's result of each, computed once and left unchanged."""
    from test_any_params import _setup
    from test_independent import Schoolbook
    S = _Set()
    S.K = _setup(tfhe, orc, 6, N, 1, 3, 6)
    sb = Schoolbook(6, N, 1, 3, 6, 8, 2, S.K.ck.bootstrap_key, S.K.ck.keyswitch_key)
    S.arith = M.single_key_arith(S.K.oracle, sb)
    S.progs = [M.make_program(seed, steps, WIDTH, N) for seed, steps in PROGRAMS]
    S.models = [M.Model(S.arith).run(p) for p in S.progs]
    yield S
    S.K.ck.close()


@pytest.fixture(scope="module")
def mk(tfhe, orc):
    """The 2-party N = 128 set of tests/test_keyswitch_edges.py (n = 4, l = 4, beta = 5): MKGateRef on the oracle's multi-key pieces for the
    gates, the multi-key schoolbook for the LUT rows."""
    from test_any_params import _mk_oracle
    from test_keyswitch_edges import _mk_set
    from test_mk_gates import MKGateRef
    S = _Set()
    S.p, S.ck, _, _, msb = _mk_set(tfhe, orc, 2)
    S.arith = M.multi_key_arith(MKGateRef(orc, _mk_oracle(orc, S.p, 2, S.ck)), msb)
    S.progs = [M.make_program(seed, steps, MK_WIDTH, N, mk=True, sk_width=MK_SK_WIDTH) for seed, steps in MK_PROGRAMS]
    S.models = [M.Model(S.arith).run(p) for p in S.progs]
    return S


def _same(a, b):
    return (a is None and b is None) or np.array_equal(a, b)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_committed_programs_have_the_promised_steps(sk):
    assert all(25 <= steps <= 40 for _, steps in PROGRAMS) and [len(p) for p in sk.progs] == [steps for _, steps in PROGRAMS]
    steps = [s for p in sk.progs for s in p]
    kinds = collections.Counter(s.kind for s in steps)
    assert set(kinds) == {"alloc", "upload", "gates", "linear", "lut", "download", "gather", "option", "refused"}, kinds
    assert kinds["alloc"] > len(PROGRAMS)                                          # re-allocation in the middle of a program
    assert all(24 <= s.W <= 64 for s in steps if s.kind == "alloc")
    gates = [s for s in steps if s.kind == "gates"]
    assert {s.shape for s in gates} == set(M.SHAPES) and {1, 2, 3} <= {s.B for s in gates}
    assert {int(op) for s in gates for op in s.ops} == set(range(15))
    for s in gates:
        if s.shape == "trivial":
            assert all(op in M.TRIVIAL for op in s.ops)
        if s.shape in ("mux_head", "mux_tail"):
            ops = list(s.ops if s.shape == "mux_head" else s.ops[::-1])
            m = ops.count(M.MUX)
            assert 0 < m < len(ops) and all(op == M.MUX for op in ops[:m]) and all(op in M.TRIVIAL for op in ops[m:])
    ints = [s for s in steps if s.kind in ("linear", "lut")]
    for s in gates + ints:                                                         # outputs distinct, anywhere in the table; operands never an output
        assert len(set(s.out.tolist())) == len(s.out)
        reads = set(M.reads_of(s, 0, s.B))
        assert not reads & set(s.out.tolist())
    assert any((np.diff(s.start) == 0).any() for s in ints if s.kind == "linear")                   # linear rows with no terms
    luts = [s for s in ints if s.kind == "lut"]
    assert {s.n_out for s in luts} == {1, 2, 4} and any(s.index is not None and len(set(s.index.tolist())) > 1 for s in luts)
    assert all((np.diff(s.start) >= 3).any() for s in luts)                                         # several terms
    assert any((np.abs(s.coef.astype(np.int64)) > 2**20).any() for s in luts)                       # wrapping coefficients
    assert {s.why for s in steps if s.kind == "refused"} == set(M.REFUSALS)
    opts = [s for s in steps if s.kind == "option"]
    assert {s.split_min for s in opts} == set(M.SPLIT_MINS) and {s.exchange for s in opts} == set(M.EXCHANGES)
    assert any(s.kind == "gather" and len(set(s.wires.tolist())) < len(s.wires) for s in steps)     # duplicates in a gather
    assert any(s.kind == "upload" and 0 < len(s.data) < 13 and s.first > 0 for s in steps)          # partial uploads
    assert all(p[-1].kind == "gather" and np.array_equal(p[-1].wires, np.arange(len(m[-1][1]))) for p, m in zip(sk.progs, sk.models))


def test_refused_levels_leave_the_model_as_it_was(sk):
    for p, m in zip(sk.progs, sk.models):
        for i, s in enumerate(p):
            if s.kind in ("refused", "option", "download", "gather"):
                assert np.array_equal(m[i][1], m[i - 1][1])
            if s.kind in M.LEVELS:
                assert not np.array_equal(m[i][1], m[i - 1][1])


@pytest.mark.parametrize("nk", [1, 2, 3])
def test_fault_free_simulator_equals_the_model(sk, nk):
    for (seed, _), p, m in zip(PROGRAMS, sk.progs, sk.models):
        got = M.Replicas(sk.arith, nk).run(p)
        for i, (g, (want, _)) in enumerate(zip(got, m)):
            assert _same(g, want), (seed, nk, i, p[i].kind)


def test_committed_programs_reach_every_event(sk):
    """A condition on the seeds (they were chosen until it held)."""
    ev = collections.Counter()
    for p in sk.progs:
        for nk in (2, 3):
            R = M.Replicas(sk.arith, nk)
            R.run(p)
            ev.update(R.events)
    print("events over the committed programs, 2 and 3 replicas:", {k: ev[k] for k in M.EVENTS})
    assert all(ev[k] >= 1 for k in M.EVENTS), {k: ev[k] for k in M.EVENTS}


@pytest.mark.parametrize("fault", M.FAULTS)
def test_every_emulated_fault_changes_a_read(sk, fault):
    hits = [(seed, nk) for (seed, _), p, m in zip(PROGRAMS, sk.progs, sk.models) for nk in (2, 3)
            if M.Replicas(sk.arith, nk, fault).run(p, [r for r, _ in m]) is not None]
    print(f"{fault}: a read differs in (seed, replicas) {hits}")
    assert hits, fault


def test_shard_mirror_on_the_closed_cases():
    ops = lambda *names: np.array([M.OPS[nm] for nm in names], np.uint8)          # noqa: E731
    lv = lambda *names: M.Step(kind="gates", B=len(names), ops=ops(*names))       # noqa: E731
    for nk in (2, 3):
        for split in M.SPLIT_MINS:
            assert M.device_count(lv("MUX"), nk, split) == 1                       # one gate: one device, whatever the threshold
            assert M.device_count(lv("NAND"), nk, split) == 1
            assert M.device_count(lv("NOT", "COPY", "CONST0", "CONST1"), nk, split) == 1          # no rotation: below every threshold
        assert M.device_count(lv(*["NAND"] * 7), nk, 8) == 1 and M.device_count(lv(*["NAND"] * 8), nk, 8) == nk
        assert M.device_count(lv(*["MUX"] * 3, "NAND"), nk, 8) == 1 and M.device_count(lv(*["MUX"] * 4), nk, 8) == nk
        assert M.device_count(lv(*["XOR"] * 64), nk, 4096) == 1
        assert M.device_count(lv(*["XOR"] * 64), nk, -1) == 1
        for B in (1, 7, 8, 9):
            row = M.Step(kind="lut", B=B)
            assert M.device_count(row, nk, 8) == (nk if B >= 8 else 1)
            assert M.plan(row, nk, 8) == ([B * r // nk for r in range(nk + 1)] if B >= 8 else [0] + [B] * nk)
    assert M.shard_bounds(ops("MUX", "MUX", "MUX", "COPY"), 2) == [0, 2, 4]
    assert M.shard_bounds(ops("COPY", "NOT", "MUX"), 2) == [0, 3, 3]               # every MUX at the tail: the second shard is empty
    assert M.shard_bounds(ops("MUX", "COPY"), 3) == [0, 1, 1, 2]                   # an empty shard in the middle
    assert M.device_count(lv("COPY", "NOT", "MUX"), 2, 2) == 1 and M.device_count(lv("MUX", "COPY"), 3, 1) == 2


def test_shard_mirror_is_the_library_rule(tfhe):
    """tfhe_shard_bounds (host code of the built library) on the gate levels of the committed programs and on random opcode strings."""
    rng = np.random.default_rng(9)
    cases = [rng.integers(0, 15, int(rng.integers(1, 40))).astype(np.uint8) for _ in range(200)]
    cases += [s.ops for seed, steps in PROGRAMS for s in M.make_program(seed, steps, WIDTH, N) if s.kind == "gates"]
    for ops in cases:
        for nk in (2, 3, 5):
            lib = tfhe._lib.shard_bounds(ops, nk)
            assert M.shard_bounds(ops, nk) == [0] + [e for _, e in lib], (ops, nk)


def test_multi_key_programs_hold_the_cross_kind_refusals(mk):
    for p, m in zip(mk.progs, mk.models):
        kinds = [s.kind for s in p]
        assert "option" not in kinds and {"gates", "linear", "lut", "upload", "gather", "refused"} <= set(kinds)
        wrong = [(i, s) for i, s in enumerate(p) if s.kind == "refused" and s.why == "wrong_call"]
        assert [(s.call, s.code) for _, s in wrong] == [("gates", M.ERR_STATE), ("mk_gates", M.ERR_STATE)]
        i = wrong[1][0]
        assert p[i - 2].kind == "alloc" and p[i - 2].rows == "sk" and p[i - 2].width == MK_SK_WIDTH and p[i + 1].kind == "gather"
        assert p[i + 2].kind == "alloc" and p[i + 2].rows == "mk" and m[-1][1].shape[1] == MK_WIDTH
        got = M.Replicas(mk.arith, 1).run(p)
        assert all(_same(g, want) for g, (want, _) in zip(got, m))
    assert any(s.kind == "refused" and s.why != "wrong_call" for p in mk.progs for s in p)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _call(eng, lv, call):
    if call.endswith("gates"):
        return getattr(eng, call + "_level")(lv.ops, lv.a, lv.b, lv.c, lv.out)
    if call.endswith("linear"):
        return getattr(eng, call + "_level")(lv.start, lv.wire, lv.coef, lv.cst, lv.out)
    return getattr(eng, call + "_level")(lv.tables, lv.start, lv.wire, lv.coef, lv.cst, lv.out, index=lv.index, n_out=lv.n_out)


def _assert_rows(got, want, wires, what):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} rows differ, the first is wire {int(wires[bad[0]])} (row {int(bad[0])} of the read): "
                             f"got {got[bad[0]][:4]} ..., want {want[bad[0]][:4]} ...")


def _replay(tfhe, eng, prog, model, nk, checked, mk=False, tag=""):
    """Runs the program on the engine; every read against the model; checked: the whole table after every step as well."""
    split_min, W = None, 0
    for i, (s, (want, table)) in enumerate(zip(prog, model)):
        what = f"{tag} step {i} ({s.kind})"
        if s.kind == "alloc":
            (eng.mk_wires_alloc if s.rows == "mk" else eng.wires_alloc)(s.W)
            W = s.W
            continue                                                              # (nothing to read before the upload that follows)
        if s.kind == "upload":
            eng.wires_upload(s.first, s.data)
        elif s.kind == "option":
            eng.set_option("level_split_min", s.split_min)
            eng.set_option("level_exchange", s.exchange)
            split_min = s.split_min
        elif s.kind in M.LEVELS:
            _call(eng, s, ("mk_" if mk else "") + s.kind)
            if nk > 1:
                bounds = M.plan(s, nk, split_min)
                what += f", shard bounds {bounds} at level_split_min {split_min}"
                assert eng.last_device_count() == M.device_count(s, nk, split_min), what
        elif s.kind == "refused":
            with pytest.raises(tfhe.EngineError) as e:
                _call(eng, s.level, s.call)
            assert e.value.code == s.code, (what, s.why, str(e.value))
            what += f", {s.why}"
        elif s.kind == "download":
            _assert_rows(eng.wires_download(s.first, s.count), want, np.arange(s.first, s.first + s.count), what)
        else:
            _assert_rows(eng.wires_gather(s.wires), want, s.wires, what)
        if checked:
            _assert_rows(eng.wires_gather(np.arange(W, dtype=np.int32)), table, np.arange(W), what + ", the table after it")


def _engine(sk, devices):
    eng = sk.K.ck.engine(devices)
    assert eng.exact_domain >= 1
    return eng, (1 if np.ndim(devices) == 0 else len(devices))


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ENGINES)
@pytest.mark.parametrize("which", range(len(PROGRAMS)), ids=IDS)
def test_programs_free_running(tfhe, sk, which, devices):
    """Only the reads the program itself holds (the last one gathers the whole table): levels queue up behind one another."""
    eng, nk = _engine(sk, devices)
    _replay(tfhe, eng, sk.progs[which], sk.models[which], nk, False, tag=f"seed {PROGRAMS[which][0]}, free-running,")


@pytest.mark.gpu
@pytest.mark.parametrize("devices", ENGINES)
@pytest.mark.parametrize("which", range(len(PROGRAMS)), ids=IDS)
def test_programs_checked(tfhe, sk, which, devices):
    """The whole table after every step: the first wrong step is named (kind, shard bounds from the mirror, wire), and the table right
    after every refused level is the model's."""
    eng, nk = _engine(sk, devices)
    _replay(tfhe, eng, sk.progs[which], sk.models[which], nk, True, tag=f"seed {PROGRAMS[which][0]}, checked,")


@pytest.mark.gpu
def test_80bit_program_on_two_contexts(tfhe, keys80):
    """tfhe_parameters_80: 6 gate levels of at most 40 gates over 64 wires, outputs anywhere in the table (rewrites), one partial upload in
    the middle; {0, 0} at level_split_min 2 against one device on the whole table after every step, and per level 16 output rows (fixed:
    drawn from seed 80; all rows of a narrower level) against Oracle.gates of the one-device table before the level.  The sampling bounds
    the oracle's time at n = 500 and is used here only."""
    n1 = keys80.params.lwe_size + 1
    rng = np.random.default_rng(80)
    g = M.Generator(rng, n1, W=64)
    steps = [g.gates("random", 40) for _ in range(3)] + [g.upload()] + [g.gates(sh, 40) for sh in ("mux_head", "random", "mux_tail")]
    assert max(s.B for s in steps if s.kind == "gates") <= 40 and sum(s.kind == "gates" for s in steps) == 6
    one, two = keys80.ck.engine(0), keys80.ck.engine([0, 0])
    assert one.exact_domain >= 1
    base = tfhe.encrypt(keys80.rng, keys80.sk, rng.integers(0, 2, 64).astype(bool)).data
    everything = np.arange(64, dtype=np.int32)
    two.set_option("level_split_min", 2)
    try:
        for eng in (one, two):
            eng.wires_alloc(64)
            eng.wires_upload(0, base)
        before = base
        for i, s in enumerate(steps):
            if s.kind == "upload":
                one.wires_upload(s.first, s.data)
                two.wires_upload(s.first, s.data)
            else:
                for eng in (one, two):
                    eng.gates_level(s.ops, s.a, s.b, s.c, s.out)
                assert two.last_device_count() == M.device_count(s, 2, 2), (i, M.plan(s, 2, 2))
            after = one.wires_gather(everything)
            _assert_rows(two.wires_gather(everything), after, everything, f"step {i} ({s.kind}), two contexts against one")
            if s.kind == "gates":
                rows = np.sort(rng.choice(s.B, min(16, s.B), replace=False))
                want = keys80.oracle.gates(s.ops[rows], before[s.a[rows]], before[s.b[rows]], before[s.c[rows]], nthreads=16)
                _assert_rows(after[s.out[rows]], want, s.out[rows], f"step {i}, gates {rows.tolist()} against the oracle")
                untouched = np.setdiff1d(everything, s.out)
                assert np.array_equal(after[untouched], before[untouched]), i
            before = after
    finally:
        two.set_option("level_split_min", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("checked", [False, True], ids=["free_running", "checked"])
@pytest.mark.parametrize("which", range(len(MK_PROGRAMS)), ids=[f"seed{s}" for s, _ in MK_PROGRAMS])
def test_multi_key_programs(tfhe, mk, which, checked):
    """mk_wires_alloc / mk_gates_level / mk_linear_level / mk_lut_level programs on a one-device context against MKGateRef and the multi-key
    schoolbook, with tfhe_gates_level refused on the multi-key table and tfhe_mk_gates_level refused on a table from tfhe_wires_alloc (the
    table read back intact after either)."""
    eng = mk.ck.engine(0)
    assert eng.exact_domain >= 1
    _replay(tfhe, eng, mk.progs[which], mk.models[which], 1, checked, mk=True, tag=f"multi-key seed {MK_PROGRAMS[which][0]},")


@pytest.mark.gpu
def test_multi_key_table_is_refused_on_a_multi_device_context(tfhe, mk):
    eng = tfhe.Engine(mk.p, devices=[0, 0])
    try:
        with pytest.raises(tfhe.EngineError) as e:
            eng.mk_wires_alloc(8)
        assert e.value.code == M.ERR_STATE
    finally:
        eng.close()
