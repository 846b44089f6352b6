"""The unit of the MK TLWE table and the multi-key rotation between the device-resident tables (csrc/engine_mk_tlwe_levels.hip) in the
compiler's report of its own, tfhe.jl_amd/build/resource_usage_mk_tlwe_levels.txt, in the manner of tests/test_tlwe_levels_resources.py:
the multi-key level rotation kernel is the one kernel there, has no scratch, no VGPR spill and a stated occupancy; it appears in none of
the twelve other reports, which keep their kernels (tests/golden/resource_usage_reports.json and resource_usage_kernels.txt; the level
and rotation reports keep their one kernel each — tfhe_mk_rot_net_level adds none to engine_mk_rot_net.hip).  CPU-only: hipcc
cross-compiles here."""
import json
import os
import re

from test_tlwe_levels_resources import OTHERS as ELEVEN, ROOT, _blocks, _demangled

OTHERS = ELEVEN + ["resource_usage_tlwe_levels.txt"]
NEW = "leveled::mk_tlwe_rotate_level_kernel(leveled::MkRotateLevelArgs)"


def test_mk_tlwe_levels_report_one_kernel_no_scratch_occupancy_stated():
    rep = _blocks("resource_usage_mk_tlwe_levels.txt")
    assert _demangled(rep) == [NEW]
    for name, block in rep.items():
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
        spill = re.search(r"VGPRs Spill: (\d+)", block)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
        assert scratch and int(scratch.group(1)) == 0 and spill and int(spill.group(1)) == 0, (name, block)
        # 512 threads = 2 waves per SIMD of one workgroup: anything below could not even start a row at N >= 2048
        assert occ and int(occ.group(1)) >= 2, (name, block)


def test_the_new_kernel_is_in_no_other_report_and_they_keep_their_kernels():
    new = set(_blocks("resource_usage_mk_tlwe_levels.txt"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "resource_usage_reports.json")))
    assert len(OTHERS) == 12 and set(golden) <= set(OTHERS)
    for name in OTHERS:
        rep = _blocks(name)
        assert rep and not new & set(rep), name
        assert not any("mk_tlwe_rotate_level" in k for k in rep), name
        if name in golden:
            assert sorted(rep) == golden[name], name
    want = open(os.path.join(ROOT, "tests", "golden", "resource_usage_kernels.txt")).read().split()
    assert sorted(_blocks("resource_usage.txt")) == want
    one_kernel = {"resource_usage_rot_net.txt": "leveled::rot_net_level_kernel(leveled::RotNetArgs)",
                  "resource_usage_mk_rot_net.txt": "leveled::mk_rot_net_level_kernel(leveled::MkRotNetArgs)",
                  "resource_usage_blind_rotate.txt": "leveled::tlwe_rotate_kernel(leveled::RotateArgs)",
                  "resource_usage_mk_blind_rotate.txt": "leveled::mk_tlwe_rotate_kernel(leveled::MkRotateArgs)",
                  "resource_usage_tlwe_levels.txt": "leveled::tlwe_rotate_level_kernel(leveled::RotateLevelArgs)"}
    for name, kernel in one_kernel.items():
        assert _demangled(_blocks(name)) == [kernel], name


def test_the_unit_is_in_every_list_of_the_makefile():
    mk = open(os.path.join(ROOT, "tfhe.jl_amd", "csrc", "Makefile")).read()
    assert "../build/engine_mk_tlwe_levels.o" in mk and "kernels_mk_tlwe_levels.hpp" in mk
    assert "../build/engine_mk_tlwe_levels.remarks > ../build/resource_usage_mk_tlwe_levels.txt" in mk
    stamp = [line for line in mk.split("\n") if line.startswith("stamp:") or "-DTFHE_STAMP" in line]
    assert len(stamp) == 2 and all("engine_mk_tlwe_levels.hip" in line for line in stamp)
    asmu = [line for line in mk.split("\n") if line.startswith("ASMU")]
    assert len(asmu) == 1 and "engine_mk_tlwe_levels" in asmu[0].split()
