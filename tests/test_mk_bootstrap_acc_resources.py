"""The unit of the multi-key private-table rotation on the 2-party gates' kernel (csrc/engine_mk_bootstrap_acc.hip) in the compiler's
report of its own, tfhe.jl_amd/build/resource_usage_mk_bootstrap_acc.txt, in the manner of tests/test_bootstrap_acc_small_resources.py: the
report holds exactly the two ACC instantiations that launch_mk_blind_rotate's `special` branch names without DIAG —
mk_blind_rotate_kernel_w2_acc<4, false, 1 | 2> on WithAcc<MkBrArgs> —, neither is in any other report, and each is no worse than the kernel
it was compiled from, mk_blind_rotate_kernel_w2<4, false, RW> in resource_usage.txt: no more scratch (that kernel has 12 bytes per lane),
no more spilled VGPRs, no lower occupancy, the same static LDS.  CPU-only: hipcc cross-compiles here."""
import re

from test_blind_rotate_resources import _blocks, _demangled
from test_bootstrap_acc_resources import OTHERS, REPORT as V3_REPORT
from test_bootstrap_acc_small_resources import REPORT as SMALL_REPORT, _figure

REPORT = "resource_usage_mk_bootstrap_acc.txt"
WANT = sorted(f"void mk_blind_rotate_kernel_w2_acc<4, false, {rw}>(WithAcc<MkBrArgs>)" for rw in (1, 2))
FIGURES = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def test_report_holds_exactly_the_two_acc_instantiations():
    rep = _blocks(REPORT)
    assert sorted(_demangled(rep)) == WANT and len(rep) == 2


def test_the_mk_acc_kernels_are_in_no_other_report():
    new = set(_blocks(REPORT))
    assert len(new) == 2
    for name in OTHERS + [V3_REPORT, SMALL_REPORT]:
        rep = _blocks(name)
        assert rep and not new & set(rep), name
        assert not any("mk_blind_rotate_kernel_w2_acc" in k for k in rep), name


def test_no_worse_than_the_kernel_they_were_compiled_from():
    acc = {n: b for n, b in zip(_demangled(_blocks(REPORT)), _blocks(REPORT).values())}
    base_rep = _blocks("resource_usage.txt")
    base = {n: b for n, b in zip(_demangled(base_rep), base_rep.values())}
    for rw in (1, 2):
        a = acc[f"void mk_blind_rotate_kernel_w2_acc<4, false, {rw}>(WithAcc<MkBrArgs>)"]
        b = base[f"void mk_blind_rotate_kernel_w2<4, false, {rw}>(MkBrArgs)"]
        fa, fb = {f: _figure(a, f) for f in FIGURES}, {f: _figure(b, f) for f in FIGURES}
        print(f"rw {rw}: acc {fa}, parent {fb}")
        assert fb["ScratchSize [bytes/lane]"] == 12                                       # (what the comparison below is against)
        assert fa["ScratchSize [bytes/lane]"] <= fb["ScratchSize [bytes/lane]"], (rw, fa, fb)
        assert fa["VGPRs Spill"] <= fb["VGPRs Spill"] and fa["SGPRs Spill"] <= fb["SGPRs Spill"], (rw, fa, fb)
        assert fa["Occupancy [waves/SIMD]"] >= fb["Occupancy [waves/SIMD]"] >= 2, (rw, fa, fb)
        assert fa["LDS Size [bytes/block]"] == fb["LDS Size [bytes/block]"], (rw, fa, fb)
