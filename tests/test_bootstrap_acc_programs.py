"""tfhe_bootstrap_acc_level and tfhe_bootstrap_acc_batch (blind_rotate_kernel_v3_acc) driven by random programs at the kernel's own size,
N = 1024, k = 1: tests/test_tlwe_table_programs.py's generator, model and replay with acc=True (tests/tlwe_table_model.py).

tests/test_bootstrap_acc.py pins the two calls on pristine tables; here the state on top is pinned.  acc_rotate steps (B = 1 ... 9, out_form
0 into slots, out_form 2 with n_out 1, 2, 8 into wires) interleave on the same slots and wires with tlwe_rotate_level_kernel and
rot_net_level_kernel, which run at N = 1024 here for the first time, with gate, linear and LUT levels that are still queued when the
rotation sizes the workspaces they share, with acc_batch calls on host buffers in between, with tgsw_load / tgsw_update of a selector set
the call must not read, and with option v3_rw 0, 1 and 4 (one wave per workgroup, or four with padding waves).  Every word is compared
(np.array_equal) with exact integer arithmetic: form_rows, Rotation.rotate over leveled.bootstrap_key_selectors(ck), extract_at, ks_ref.
No engine call is a reference.

Two sets, (n, N, k, l, beta) = C (8, 1024, 1, 2, 10): the L = 2 instantiation, n two whole lockstep periods; exact for real keys only
(SchemeParameters.exactness class 1), so every selector is a real encryption; and D (7, 1024, 1, 4, 6): the run-time-l instantiation, odd
n; exact for any key words, so selectors are arbitrary words by a coin, with the planted extremes.

CPU: the committed programs hold the promised steps, reach every event of EVENTS + ACC_EVENTS, every fault of FAULTS + ACC_FAULTS changes
a word of some read in each set, every level is a valid call and every refusal's code is the model's.  GPU (one device): every program
free-running and checked (both whole tables after every step, the first wrong step named), kernel names, refusal codes."""
import collections
import time

import numpy as np
import pytest

import tlwe_table_model as T
from test_tlwe_levels import INVALID, OK, model_blind_rotate_level, model_rot_net_level
from test_tlwe_table_programs import _engine, _replay, build_set

SETS = {"C": (8, 1024, 1, 2, 10), "D": (7, 1024, 1, 4, 6)}                        # n, N, k, l, beta (t = 8, gamma = 2)
PROGRAMS = {"C": [(202, 40), (242, 40), (354, 40)],                                    # (seed, steps): chosen until the CPU conditions below held
            "D": [(2, 40), (3, 40), (58, 40)]}
CASES = [pytest.param(name, i, id=f"{name}-seed{seed}") for name in SETS for i, (seed, _) in enumerate(PROGRAMS[name])]
ALL_EVENTS, ALL_FAULTS, ALL_REFUSALS = T.EVENTS + T.ACC_EVENTS, T.FAULTS + T.ACC_FAULTS, T.REFUSALS + T.ACC_REFUSALS


@pytest.fixture(scope="module")
def sets(tfhe, orc):
    """Both sets, computed once and left unchanged; the time is printed (profiles/tlwe_table_programs.txt)."""
    t0 = time.perf_counter()
    both = {name: build_set(tfhe, orc, name, PROGRAMS[name], SETS[name], acc=True) for name in SETS}
    print(f"models of {sum(len(v) for v in PROGRAMS.values())} programs on sets C and D: {time.perf_counter() - t0:.1f} s")
    yield both
    for S in both.values():
        S.K.ck.close()


# ---- CPU: the programs ---------------------------------------------------------------------------------------------------------------------
def test_sets_are_the_two_exactness_classes(sets):
    assert sets["C"].K.params.exactness()[0] == 1 and sets["C"].arbitrary is False
    assert sets["D"].K.params.exactness()[0] == 2 and sets["D"].arbitrary is True
    bits_or_words = {name: [s for p in S.progs for s in p if s.kind in ("tgsw_load", "tgsw_update")] for name, S in sets.items()}
    assert all(bits_or_words.values())
    planted = [s.data for s in bits_or_words["D"] if s.kind == "tgsw_load" and (s.data[0, 0, 0, 0] == 2**31 - 1).all() and (s.data[1, 0, 0, 1] == -2**31).all()]
    assert len(planted) >= len(PROGRAMS["D"])                                     # (every program's first load)
    assert not any((s.data[0, 0, 0, 0] == 2**31 - 1).all() for s in bits_or_words["C"])


def test_committed_programs_have_the_promised_steps(sets):
    for name, S in sets.items():
        n, N = S.p.n, S.p.N
        assert len(S.seeds) == 3 and all(25 <= steps <= 40 for _, steps in S.seeds) and [len(p) for p in S.progs] == [steps for _, steps in S.seeds]
        steps = [s for p in S.progs for s in p]
        kinds = collections.Counter(s.kind for s in steps)
        print(name, dict(kinds))
        assert kinds["acc_rotate"] >= 12 and kinds["acc_batch"] >= 4, kinds
        assert set(kinds) >= {"tlwe_alloc", "wires_alloc", "tlwe_upload", "wires_upload", "tgsw_load", "tgsw_update", "rotate", "net", "gates", "lut",
                              "acc_rotate", "acc_batch", "tlwe_download", "wires_download", "option", "refused"}, kinds
        for p, res in zip(S.progs, S.results):
            assert [s.kind for s in p[-2:]] == ["tlwe_download", "wires_download"] and p[-2].first == p[-1].first == 0
            assert p[-2].count == len(res[-1][1]) and p[-1].count == len(res[-1][2])
        rot = [s for s in steps if s.kind == "acc_rotate"]
        assert {s.B for s in rot} >= {1, 4, 5, 8, 9} and {s.B for s in rot} <= set(range(1, 10)), sorted({s.B for s in rot})
        assert {s.out_form for s in rot} == {0, 2} and {s.n_out for s in rot if s.out_form == 2} == set(T.ACC_N_OUTS) == {1, 2, 8}
        assert all(s.sel is None for s in rot)
        assert any(s.cst is None for s in rot) and any(s.cst is not None for s in rot)
        assert {int(c) for s in rot for c in np.diff(s.start)} == {0, 1, 2, 3, 4}
        coef = np.concatenate([s.coef.astype(np.int64) for s in rot])
        assert (np.abs(coef) <= 3).any() and (np.abs(coef) > 2**20).any() and (coef == -2**31).any() and (coef == 2**31 - 1).any()
        assert any(len(set(s.acc_slot.tolist())) < s.B for s in rot)                                  # repeated acc_slots
        assert {s.special for s in rot} == set(T.SPECIALS)
        for p, res in zip(S.progs, S.results):
            for i, s in enumerate(p):
                if s.kind != "acc_rotate":
                    continue
                outs = s.out_slot if s.out_form == 0 else s.out_wires
                assert len(set(outs.tolist())) == len(outs) == s.B * s.n_out
                assert not set(outs.tolist()) & set((s.acc_slot if s.out_form == 0 else s.wire).tolist())     # apart from every read
                assert s.out_form == 0 or 2 * s.B * s.n_out <= len(res[i][2])                             # at most half the wires
        assert any(s.out_form == 2 and (np.diff(s.out_wires) < 0).any() for s in rot)                 # permuted wires
        bat = [s for s in steps if s.kind == "acc_batch"]
        assert all(1 <= len(s.acc) <= 3 and 1 <= s.B <= 6 and s.rows.shape == (s.B, n + 1) and s.acc.shape[1:] == (2, N) for s in bat)
        assert {s.out_form for s in bat} == {0, 1, 2} and {s.n_out for s in bat if s.out_form} == set(T.BATCH_N_OUTS) == {1, 4, 32}
        assert all(s.n_out == 1 for s in bat if s.out_form == 0)
        assert any(s.acc_index is None for s in bat) and any(s.acc_index is not None and len(set(s.acc_index.tolist())) > 1 for s in bat)
        assert {s.v3_rw for s in steps if s.kind == "option" and "v3_rw" in s} == {0, 1, 4}
        assert {s.anyn_spec for s in steps if s.kind == "option" and "anyn_spec" in s} <= {-1, 1}
        assert {s.why for s in steps if s.kind == "refused"} >= set(T.ACC_REFUSALS)
        assert {s.kind for s in steps if s.kind in ("rotate", "net")} == {"rotate", "net"}            # the any-N level kernels at N = 1024


def test_only_levels_change_the_model_and_each_changes_one_table(sets):
    same = lambda a, b: a is b or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))      # noqa: E731
    for S in sets.values():
        for p, res in zip(S.progs, S.results):
            for i, s in enumerate(p):
                tl, w, tl0, w0 = res[i][1], res[i][2], res[i - 1][1] if i else None, res[i - 1][2] if i else None
                if s.kind in ("refused", "option") + T.READS:
                    assert same(tl, tl0) and same(w, w0), (i, s.kind)                                 # (acc_batch is a read: both tables alone)
                    assert (res[i][0] is not None) == (s.kind in T.READS)
                if s.kind == "acc_batch":
                    shape = {0: (s.B, 2, S.p.N), 1: (s.B, s.n_out, S.p.N + 1), 2: (s.B, s.n_out, S.p.n + 1)}[s.out_form]
                    assert res[i][0].shape == shape and res[i][0].dtype == np.int32
                if s.kind in T.LEVELS:
                    assert same(tl, tl0) != same(w, w0), (i, s.kind)                                  # exactly one of the two
                    assert same(w, w0) == (s.kind in T.TLWE_LEVELS + T.ACC_LEVELS and s.out_form == 0), (i, s.kind)


def test_committed_programs_reach_every_event(sets):
    """A condition on the seeds (they were chosen until it held)."""
    for name, S in sets.items():
        ev = S.model.events
        print(f"set {name}, events over the committed programs:", {k: ev[k] for k in ALL_EVENTS})
        assert all(ev[k] >= 1 for k in ALL_EVENTS), (name, {k: ev[k] for k in ALL_EVENTS if ev[k] < 1})


@pytest.mark.parametrize("fault", ALL_FAULTS)
def test_every_emulated_fault_changes_a_read(sets, fault):
    hits = []
    for name, S in sets.items():
        for (seed, _), p, res in zip(S.seeds, S.progs, S.results):
            at = S.model.run(p, fault, [r for r, _, _ in res])
            if at is not None:
                hits.append((name, seed, at))
    print(f"{fault}: a read differs in (set, seed, step) {hits}")
    assert {name for name, _, _ in hits} == set(SETS), (fault, hits)


def _loaded_counts(p):
    count = 0
    for s in p:
        count = len(s.data) if s.kind == "tgsw_load" else count
        yield count


def test_refusal_codes_are_the_level_models(sets):
    """Every refused step's code is model_blind_rotate_level / model_rot_net_level on the tables of that moment (sel_beyond: the one
    refusal those two leave to the state)."""
    seen = collections.Counter()
    for S in sets.values():
        for p, res in zip(S.progs, S.results):
            for i, (s, count) in enumerate(zip(p, _loaded_counts(p))):
                if s.kind != "refused":
                    continue
                lv, slots, W = s.level, len(res[i][1]), len(res[i][2])
                if lv.kind == "net":
                    code = model_rot_net_level(slots, W, lv.E, lv.F, lv.B, lv.table_first, lv.out_form, lv.out_first, lv.out_wires)
                else:
                    code = model_blind_rotate_level(slots, W, S.p.N, lv.acc_slot, lv.start, lv.wire, lv.n_out, lv.out_form, lv.out_slot, lv.out_wires)
                if s.why == "sel_beyond":
                    assert code == OK and int(np.max(lv.sel)) == count
                    code = INVALID
                assert (lv.kind == "acc_rotate") == (s.why in T.ACC_REFUSALS)
                assert s.code == code == INVALID == T.level_code(lv, slots, W, S.p.N, count), (i, s.why)
                seen[s.why] += 1
    print("refused steps:", dict(seen))
    assert set(seen) >= set(T.ACC_REFUSALS) and set(seen) <= set(ALL_REFUSALS)


def test_every_level_the_programs_run_is_a_valid_call(sets):
    ran = collections.Counter()
    for S in sets.values():
        for p, res in zip(S.progs, S.results):
            for i, (s, count) in enumerate(zip(p, _loaded_counts(p))):
                if s.kind in T.TLWE_LEVELS + T.ACC_LEVELS:
                    assert T.level_code(s, len(res[i][1]), len(res[i][2]), S.p.N, count) == OK, (S.name, i, s.kind)
                    ran[s.kind] += 1
                if s.kind == "tgsw_update":
                    assert 0 <= s.first and s.first + len(s.data) <= count
    assert ran["acc_rotate"] >= 24 and ran["rotate"] >= 4 and ran["net"] >= 4, ran


# ---- GPU: the programs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,which", CASES)
def test_programs_free_running(tfhe, sets, name, which):
    """Only the program's own reads (the last two download both whole tables): levels queue up behind one another."""
    _replay(tfhe, _engine(sets[name]), sets[name], which, False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", CASES)
def test_programs_checked(tfhe, sets, name, which):
    """Both whole tables after every step: the first wrong step is named, and the tables right after every refused call are the model's."""
    _replay(tfhe, _engine(sets[name]), sets[name], which, True)
