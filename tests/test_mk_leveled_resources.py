"""The multi-key leveled unit (csrc/engine_mk_leveled.hip) in the compiler's report of its own,
tfhe.jl_amd/build/resource_usage_mk_leveled.txt: the multi-key CMUX level kernel is the one kernel there, has no scratch and a stated
occupancy; the main report (resource_usage.txt) and the single-key leveled report still list exactly the kernels they listed before the
unit existed.  CPU-only: hipcc cross-compiles here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe.jl_amd", "csrc")
BUILD = os.path.join(ROOT, "tfhe.jl_amd", "build")


def _blocks(name):
    subprocess.check_call(["make", "-s", "-C", CSRC])          # no-op when the library is newer than its sources
    path = os.path.join(BUILD, name)
    assert os.path.exists(path), f"{name} is not written by the build"
    return {b.split()[0]: b for b in re.split(r"remark: Function Name: ", open(path).read())[1:]}


def test_mk_leveled_report_one_kernel_no_scratch_occupancy_stated():
    rep = _blocks("resource_usage_mk_leveled.txt")
    dem = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    assert [d for d in dem if d] == ["leveled::mk_cmux_level_kernel(leveled::MkArgs)"], dem
    for name, block in rep.items():
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
        spill = re.search(r"VGPRs Spill: (\d+)", block)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
        assert scratch and int(scratch.group(1)) == 0 and spill and int(spill.group(1)) == 0, (name, block)
        # 512 threads = 2 waves per SIMD of one workgroup: anything below could not even start the widest launch
        assert occ and int(occ.group(1)) >= 2, (name, block)


def test_existing_reports_list_the_kernels_they_listed_before():
    want = open(os.path.join(ROOT, "tests", "golden", "resource_usage_kernels.txt")).read().split()
    assert sorted(_blocks("resource_usage.txt")) == want
    new = set(_blocks("resource_usage_mk_leveled.txt"))
    assert not new & set(want)                                  # the new kernel is in its own report only
    single = _blocks("resource_usage_leveled.txt")
    assert len(single) == 1 and not new & set(single)
