"""The unit of the TLWE table and the rotation between the device-resident tables (csrc/engine_tlwe_levels.hip) in the compiler's report of
its own, tfhe.jl_amd/build/resource_usage_tlwe_levels.txt, in the manner of tests/test_mk_blind_rotate_resources.py: the level rotation
kernel is the one kernel there, has no scratch, no VGPR spill and a stated occupancy; it appears in none of the eleven other reports,
which keep their kernels (tests/golden/resource_usage_reports.json and resource_usage_kernels.txt; the two rotation reports keep their
one kernel each).  CPU-only: hipcc cross-compiles here."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe.jl_amd", "csrc")
BUILD = os.path.join(ROOT, "tfhe.jl_amd", "build")
OTHERS = ["resource_usage.txt", "resource_usage_tv.txt", "resource_usage_mk_tv.txt", "resource_usage_leveled.txt", "resource_usage_mk_leveled.txt",
          "resource_usage_cmux_net.txt", "resource_usage_mk_cmux_net.txt", "resource_usage_rot_net.txt", "resource_usage_mk_rot_net.txt",
          "resource_usage_blind_rotate.txt", "resource_usage_mk_blind_rotate.txt"]


def _blocks(name):
    subprocess.check_call(["make", "-s", "-C", CSRC])          # no-op when the library is newer than its sources
    path = os.path.join(BUILD, name)
    assert os.path.exists(path), f"{name} is not written by the build"
    return {b.split()[0]: b for b in re.split(r"remark: Function Name: ", open(path).read())[1:]}


def _demangled(rep):
    dem = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return [d for d in dem if d]


def test_tlwe_levels_report_one_kernel_no_scratch_occupancy_stated():
    rep = _blocks("resource_usage_tlwe_levels.txt")
    assert _demangled(rep) == ["leveled::tlwe_rotate_level_kernel(leveled::RotateLevelArgs)"]
    for name, block in rep.items():
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
        spill = re.search(r"VGPRs Spill: (\d+)", block)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
        assert scratch and int(scratch.group(1)) == 0 and spill and int(spill.group(1)) == 0, (name, block)
        # 512 threads = 2 waves per SIMD of one workgroup: anything below could not even start a row at N >= 2048
        assert occ and int(occ.group(1)) >= 2, (name, block)


def test_the_new_kernel_is_in_no_other_report_and_they_keep_their_kernels():
    new = set(_blocks("resource_usage_tlwe_levels.txt"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "resource_usage_reports.json")))
    assert len(OTHERS) == 11 and set(golden) <= set(OTHERS)
    for name in OTHERS:
        rep = _blocks(name)
        assert rep and not new & set(rep), name
        assert not any("tlwe_rotate_level" in k for k in rep), name
        if name in golden:
            assert sorted(rep) == golden[name], name
    want = open(os.path.join(ROOT, "tests", "golden", "resource_usage_kernels.txt")).read().split()
    assert sorted(_blocks("resource_usage.txt")) == want
    assert _demangled(_blocks("resource_usage_rot_net.txt")) == ["leveled::rot_net_level_kernel(leveled::RotNetArgs)"]
    assert _demangled(_blocks("resource_usage_mk_rot_net.txt")) == ["leveled::mk_rot_net_level_kernel(leveled::MkRotNetArgs)"]
    assert _demangled(_blocks("resource_usage_blind_rotate.txt")) == ["leveled::tlwe_rotate_kernel(leveled::RotateArgs)"]
    assert _demangled(_blocks("resource_usage_mk_blind_rotate.txt")) == ["leveled::mk_tlwe_rotate_kernel(leveled::MkRotateArgs)"]
