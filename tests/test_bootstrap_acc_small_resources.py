"""The unit of the private-table rotation on the multi-wave gate kernels (csrc/engine_bootstrap_acc_small.hip) in the compiler's report of
its own, tfhe.jl_amd/build/resource_usage_bootstrap_acc_small.txt, in the manner of tests/test_bootstrap_acc_resources.py: the report holds
exactly the eight ACC instantiations that br_launch_w2 and br_launch_h2 name without DIAG — blind_rotate_kernel_w2_acc<2 | 3 | 0, false,
1 | 2> on WithAcc<BrArgs> and blind_rotate_kernel_h2_acc<2 | 3, false> on WithAcc<BrArgs> and H2Tables —, each has no scratch and no VGPR
spill, the occupancy is at least the launch bound (two waves per SIMD for the two-wave kernel, one for the 4 l-wave kernel), none of them
is in any other report, and the report of the one-wave form still holds exactly its six.  CPU-only: hipcc cross-compiles here."""
import re

from test_blind_rotate_resources import _blocks, _demangled
from test_bootstrap_acc_resources import OTHERS, REPORT as V3_REPORT, WANT as V3_WANT

REPORT = "resource_usage_bootstrap_acc_small.txt"
W2 = sorted(f"void blind_rotate_kernel_w2_acc<{L}, false, {rw}>(WithAcc<BrArgs>)" for L in (0, 2, 3) for rw in (1, 2))
H2 = sorted(f"void blind_rotate_kernel_h2_acc<{L}, false>(WithAcc<BrArgs>, H2Tables)" for L in (2, 3))


def _figure(block, what):
    m = re.search(re.escape(what) + r": (\d+)", block)
    assert m, (what, block)
    return int(m.group(1))


def test_report_holds_exactly_the_eight_acc_instantiations_without_scratch_or_spill():
    rep = _blocks(REPORT)
    names = _demangled(rep)
    assert sorted(names) == sorted(W2 + H2)
    assert len(rep) == 8
    for mangled, block in rep.items():
        assert _figure(block, "ScratchSize [bytes/lane]") == 0 and _figure(block, "VGPRs Spill") == 0, (mangled, block)
        bound = 2 if "kernel_w2_acc" in mangled else 1
        assert "kernel_w2_acc" in mangled or "kernel_h2_acc" in mangled, mangled
        assert _figure(block, "Occupancy [waves/SIMD]") >= bound, (mangled, block)


def test_the_small_acc_kernels_are_in_no_other_report():
    new = set(_blocks(REPORT))
    assert len(new) == 8
    for name in OTHERS + [V3_REPORT]:
        rep = _blocks(name)
        assert rep and not new & set(rep), name
        assert not any("w2_acc" in k or "h2_acc" in k for k in rep), name


def test_the_v3_report_still_holds_exactly_its_six():
    rep = _blocks(V3_REPORT)
    assert sorted(_demangled(rep)) == V3_WANT and len(rep) == 6
    assert not set(rep) & set(_blocks(REPORT))
