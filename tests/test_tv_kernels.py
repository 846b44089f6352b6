"""The TV kernels (programmable bootstrapping, csrc/engine_tv.hip) in the compiler's report of their unit,
tfhe.jl_amd/build/resource_usage_tv.txt: one per non-DIAG instantiation the dispatcher can select, none spills, each keeps the
occupancy of the kernel it was compiled from (tests/test_resource_usage.py's rules).  CPU-only: hipcc cross-compiles here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tfhe.jl_amd", "csrc")
BUILD = os.path.join(ROOT, "tfhe.jl_amd", "build")


def _report(name):
    subprocess.check_call(["make", "-s", "-C", CSRC])
    rows = {}
    for block in re.split(r"remark: Function Name: ", open(os.path.join(BUILD, name)).read())[1:]:
        vals = {}
        for key, pat in (("vgpr", r"VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, block)
            vals[key] = int(m.group(1)) if m else None
        rows[block.split()[0]] = vals
    names = list(rows)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {d: rows[n] for n, d in zip(names, dem)}


def test_every_family_has_its_tv_kernels_and_none_spills():
    tv = _report("resource_usage_tv.txt")
    counts = {}
    for k in tv:
        m = re.match(r"void (?:anyn::)?(blind_rotate_kernel\w*)_tv<", k)
        assert m, k
        counts[m.group(1)] = counts.get(m.group(1), 0) + 1
    assert counts == {"blind_rotate_kernel_v3": 6, "blind_rotate_kernel_w2": 6, "blind_rotate_kernel_h2": 2, "blind_rotate_kernel_k2": 4,
                      "blind_rotate_kernel_k2w3": 2, "blind_rotate_kernel_n512": 6, "blind_rotate_kernel_n512w2": 3,
                      "blind_rotate_kernel_n2048x": 2, "blind_rotate_kernel_general": 2, "blind_rotate_kernel": 1}, counts
    bad = {k: v for k, v in tv.items() if v["scratch"] or v["vgpr_spill"]}
    assert not bad, bad


def test_tv_kernels_keep_the_occupancy_of_their_mu_kernels():
    tv, mu = _report("resource_usage_tv.txt"), _report("resource_usage.txt")
    for k, v in tv.items():
        base = re.sub(r"_tv<", "<", k).replace("WithTv<", "").replace(">)", ")").replace(">, H2Tables)", ", H2Tables)")
        assert base in mu, (k, base)
        assert v["occ"] >= mu[base]["occ"] and v["vgpr"] + v["agpr"] <= 256, (k, v, mu[base])
