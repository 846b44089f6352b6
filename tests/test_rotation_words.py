"""The four TLWE rotation calls, the two level network calls and the (MK) TLWE table against tests/golden/rotation_words.json
(tests/golden/gen_rotation_words.py wrote it with the library as it was before the rotation calls were put on one runner,
rotate_run.hpp, the two tables on one record and the level calls' checks into leveled_checks.hpp).  The other tests compare the level
calls with the batch calls, and both changed together; here every output keeps its SHA-256, its first words and its kernel name, every
table its hash after every level call, and every refusal its return code and its message, byte for byte.  No tolerance: the recorded
build and this one make the same floating-point operations in the same order.  Cases: gen_rotation_words.py's docstring."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_rotation_words", os.path.join(GOLDEN, "gen_rotation_words.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def test_golden_file_lists_every_case():
    golden = json.load(open(gen.OUT))
    assert sorted(golden) == sorted(gen.key(*a[:5]) for a in gen.ALL)
    for a in gen.ALL:
        cases = golden[gen.key(*a[:5])]
        words = {c: r for c, r in cases.items() if isinstance(r, dict)}
        # per placement: 20 batch calls, 10 level rotations (multi-key: 2 more without a wire table), 4 level networks; 4 table downloads
        assert len(words) == 2 * (34 + (2 if a[0] == "multi_key" else 0)) + 4, (a, len(words))
        for case, rec in words.items():
            assert len(rec["sha256"]) == 64 and len(rec["first"]) <= 8, (a, case)
            if not case.startswith("table,"):
                assert rec["kernel"].endswith(",spec=global)") == case.endswith(",spec=1"), (a, case, rec["kernel"])
            if case.startswith(("level,", "net,")):
                assert len(rec["table"]) == 64 and ("wires" in rec) == ("no wire table" not in case), (a, case)
        refused = [c for c, r in cases.items() if isinstance(r, list) and r[0] != 0]
        assert all(c.startswith(("refuse,", "table,")) for c in refused)
        assert len(refused) >= (100 if a[5] else 14), (a, len(refused))         # the refusal sequences run at the first set of each kind


@pytest.mark.gpu
@pytest.mark.parametrize("family,N,kp,l,beta,refusals", gen.ALL)
def test_gpu_rotation_words_are_the_recorded_ones(tfhe, family, N, kp, l, beta, refusals):
    """kp: k of a single-key set, the party count of a multi-key one."""
    want = json.load(open(gen.OUT))[gen.key(family, N, kp, l, beta)]
    got = json.loads(json.dumps(gen.cases(tfhe, family, N, kp, l, beta, refusals)))      # (as the file holds them: lists, not tuples)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        print(case, got[case])
        assert got[case] == want[case], case
