"""The unit of the private-table rotation on the gates' kernel (csrc/engine_bootstrap_acc.hip) in the compiler's report of its own,
tfhe.jl_amd/build/resource_usage_bootstrap_acc.txt, in the manner of tests/test_blind_rotate_resources.py: the report holds exactly the six
ACC instantiations of blind_rotate_kernel_v3 that br_launch_v3 names without DIAG, each has no scratch, no VGPR spill and two waves per SIMD
(the kernel's launch bound: its second wave hides the first one's key latency), none of them is in any other report, and the main report
still holds the kernels of tests/golden/resource_usage_kernels.txt.  CPU-only: hipcc cross-compiles here."""
import os
import re

from test_blind_rotate_resources import ROOT, _blocks, _demangled

REPORT = "resource_usage_bootstrap_acc.txt"
OTHERS = ["resource_usage.txt", "resource_usage_tv.txt", "resource_usage_mk_tv.txt", "resource_usage_leveled.txt", "resource_usage_mk_leveled.txt",
          "resource_usage_cmux_net.txt", "resource_usage_mk_cmux_net.txt", "resource_usage_rot_net.txt", "resource_usage_mk_rot_net.txt",
          "resource_usage_blind_rotate.txt", "resource_usage_mk_blind_rotate.txt", "resource_usage_tlwe_levels.txt", "resource_usage_mk_tlwe_levels.txt"]
WANT = sorted(f"void blind_rotate_kernel_v3_acc<{L}, 8, true, false, {rw}>(WithAcc<BrArgs>)" for L in (0, 2, 3) for rw in (1, 4))


def test_report_holds_exactly_the_six_acc_instantiations_without_scratch_or_spill():
    rep = _blocks(REPORT)
    assert sorted(_demangled(rep)) == WANT
    for name, block in rep.items():
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
        spill = re.search(r"VGPRs Spill: (\d+)", block)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
        assert scratch and int(scratch.group(1)) == 0 and spill and int(spill.group(1)) == 0, (name, block)
        assert occ and int(occ.group(1)) >= 2, (name, block)


def test_the_acc_kernels_are_in_no_other_report():
    new = set(_blocks(REPORT))
    assert len(new) == 6
    for name in OTHERS:
        rep = _blocks(name)
        assert rep and not new & set(rep), name
        assert not any("_acc" in k for k in rep), name
    want = open(os.path.join(ROOT, "tests", "golden", "resource_usage_kernels.txt")).read().split()
    assert sorted(_blocks("resource_usage.txt")) == want
