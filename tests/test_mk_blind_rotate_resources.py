"""The unit of the multi-key blind rotation of the caller's accumulators (csrc/engine_mk_blind_rotate.hip) in the compiler's report of its
own, tfhe.jl_amd/build/resource_usage_mk_blind_rotate.txt, in the manner of tests/test_blind_rotate_resources.py: the rotation kernel is
the one kernel there, has no scratch, no VGPR spill and a stated occupancy, and it appears in none of the ten other reports, which keep
their kernels.  CPU-only: hipcc cross-compiles here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe.jl_amd", "csrc")
BUILD = os.path.join(ROOT, "tfhe.jl_amd", "build")
OTHERS = ["resource_usage.txt", "resource_usage_tv.txt", "resource_usage_mk_tv.txt", "resource_usage_leveled.txt", "resource_usage_mk_leveled.txt",
          "resource_usage_cmux_net.txt", "resource_usage_mk_cmux_net.txt", "resource_usage_rot_net.txt", "resource_usage_mk_rot_net.txt",
          "resource_usage_blind_rotate.txt"]


def _blocks(name):
    subprocess.check_call(["make", "-s", "-C", CSRC])          # no-op when the library is newer than its sources
    path = os.path.join(BUILD, name)
    assert os.path.exists(path), f"{name} is not written by the build"
    return {b.split()[0]: b for b in re.split(r"remark: Function Name: ", open(path).read())[1:]}


def _demangled(rep):
    dem = subprocess.run(["c++filt"], input="\n".join(rep), capture_output=True, text=True, check=True).stdout.split("\n")
    return [d for d in dem if d]


def test_mk_blind_rotate_report_one_kernel_no_scratch_occupancy_stated():
    rep = _blocks("resource_usage_mk_blind_rotate.txt")
    assert _demangled(rep) == ["leveled::mk_tlwe_rotate_kernel(leveled::MkRotateArgs)"]
    for name, block in rep.items():
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
        spill = re.search(r"VGPRs Spill: (\d+)", block)
        occ = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block)
        assert scratch and int(scratch.group(1)) == 0 and spill and int(spill.group(1)) == 0, (name, block)
        # 512 threads = 2 waves per SIMD of one workgroup: anything below could not even start a row at N >= 2048
        assert occ and int(occ.group(1)) >= 2, (name, block)


def test_the_new_kernel_is_in_no_other_report():
    new = set(_blocks("resource_usage_mk_blind_rotate.txt"))
    assert len(OTHERS) == 10
    for name in OTHERS:
        rep = _blocks(name)
        assert rep and not new & set(rep), name
        assert not any("mk_tlwe_rotate" in k for k in rep), name
    want = open(os.path.join(ROOT, "tests", "golden", "resource_usage_kernels.txt")).read().split()
    assert sorted(_blocks("resource_usage.txt")) == want
    assert _demangled(_blocks("resource_usage_blind_rotate.txt")) == ["leveled::tlwe_rotate_kernel(leveled::RotateArgs)"]
    assert _demangled(_blocks("resource_usage_mk_rot_net.txt")) == ["leveled::mk_rot_net_level_kernel(leveled::MkRotNetArgs)"]
