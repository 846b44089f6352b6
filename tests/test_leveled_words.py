"""The words of the seven leveled calls against tests/golden/leveled_words.json (tests/golden/gen_leveled_words.py wrote it with the
library as it was before the level kernels were put on one shared body, kernels_leveled_core.hpp, and the entry points on one
runner, leveled_run.hpp).  The other leveled tests compare the five level kernels with integer schoolbooks where a parameter set is exact
and with each other where rounding is inexact; here every output array must keep its SHA-256, its first words and its kernel name, so
the kernels cannot drift together.  No tolerance: the recorded build and this one make the same floating-point operations in the same
order.  Cases: gen_leveled_words.py's docstring."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("gen_leveled_words", os.path.join(GOLDEN, "gen_leveled_words.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def test_golden_file_lists_every_case():
    golden = json.load(open(gen.OUT))
    assert sorted(golden) == sorted(gen.key(f, *s) for f in gen.FAMILIES for s in gen.SETS[f])
    for name, cases in golden.items():
        assert len(cases) == (20 if name.startswith("single_key") else 14), name      # (1 + 3 x 3) and (1 + 2 x 3) calls, two placements
        for case, rec in cases.items():
            assert len(rec["sha256"]) == 64 and len(rec["first"]) == 8, (name, case)
            assert rec["kernel"].endswith(",spec=global)") == case.endswith(",spec=1"), (name, case, rec["kernel"])


@pytest.mark.gpu
@pytest.mark.parametrize("family,N,kp,l,beta", [(f,) + s for f in sorted(gen.FAMILIES) for s in gen.SETS[f]])
def test_gpu_leveled_words_are_the_recorded_ones(tfhe, family, N, kp, l, beta):
    """kp: k of a single-key set, the party count of a multi-key one."""
    want = json.load(open(gen.OUT))[gen.key(family, N, kp, l, beta)]
    got = gen.FAMILIES[family](tfhe, N, kp, l, beta)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        print(case, got[case]["kernel"], got[case]["first"][:2])
        assert got[case]["kernel"] == want[case]["kernel"], case
        assert got[case]["first"] == want[case]["first"], case
        assert got[case]["sha256"] == want[case]["sha256"], case
