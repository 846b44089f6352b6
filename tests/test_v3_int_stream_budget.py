"""blind_rotate_kernel_v3 adds a step's rounded words into its LDS image by ds_add_u32 (csrc/kernels_common.hpp: accumulate_poly_v3).
What that is worth stands or falls with the code the compiler makes of it, so this reads the shipped code objects (no GPU): the
atomic adds are there, without return value, fed straight from the rounding FMA's result register; no scratch, two waves per SIMD,
no more LDS-queue drains than before; and the committed profile of these sources shows the vector instructions gone."""
import glob
import json
import os
import re
import sys

from test_resource_usage import ROOT, _disassemble, _report

HEADLINE = "blind_rotate_kernel_v3<2, 8, true, false, 4>"
WRITES_FP64 = ("v_fma_f64", "v_fmac_f64", "v_add_f64")      # the rounding FMA (an addition where the cosine is 1)


def _v3_kernels():
    _report()                                   # (builds the library if it is stale)
    build = os.path.join(ROOT, "tfhe.jl_amd", "build")
    ks = {}
    for unit in ("engine_dispatch.o", "engine_tv.o"):
        ks.update({k: [l.split("//")[0].strip() for l in v] for k, v in _disassemble(os.path.join(build, unit)).items() if "blind_rotate_kernel_v3" in k})
    return ks


def _last_writer(body, at, reg):
    """The instruction before body[at] that wrote vector register `reg` last: (mnemonic, first register of its destination)."""
    for line in reversed(body[:at]):
        m = re.match(r"(\S+)\s+v(?:(\d+)|\[(\d+):(\d+)\])", line)
        if not m or m.group(1).startswith(("ds_write", "ds_add", "ds_sub", "global_store", "s_")):
            continue
        lo = int(m.group(2) if m.group(2) is not None else m.group(3))
        hi = int(m.group(2) if m.group(2) is not None else m.group(4))
        if lo <= reg <= hi:
            return m.group(1), lo
    return None, None


def test_the_accumulator_is_updated_by_lds_atomic_adds_fed_from_the_rounding_fma():
    ks = _v3_kernels()
    assert len(ks) == 18, sorted(ks)            # l = 2, 3, run-time x one / four rotations per workgroup x timed / DIAG, and the six TV forms
    for k, body in ks.items():
        adds = [i for i, l in enumerate(body) if l.startswith("ds_add_u32")]
        subs = [i for i, l in enumerate(body) if l.startswith("ds_sub_u32")]
        # two polynomials per step: 16 words each, and the last one once more into the mirror; the DIAG forms do the same
        assert len(adds) == 32 and len(subs) == 2 and not [l for l in body if re.match(r"ds_(add|sub)_rtn", l)], (k, len(adds), len(subs))
        for i in adds + subs:
            data = int(re.match(r"ds_\w+ v\d+, v(\d+)", body[i]).group(1))
            op, lo = _last_writer(body, i, data)
            assert op in WRITES_FP64 and lo == data, (k, body[i], op, lo)     # the low word of an FP64 result: no v_mov, no v_add between
        if "ELb0ELi" in k:                      # the timed forms (DIAG = false): no more drains than before this change, 60 in the headline
            assert sum("lgkmcnt(0)" in l for l in body) <= (63 if "_tv" in k else 60), k      # kernel (63 in its TV form, which reads its table first)
        assert not [l for l in body if l.startswith("scratch_")] or "ILi0ELi8ELb1ELb1ELi4EE" in k, k      # (tests/test_resource_usage.py: the one DIAG form that may spill)
    rep = _report()
    v3 = [k for k in rep if "blind_rotate_kernel_v3" in k]
    assert len(v3) >= 12
    for k in v3:
        assert rep[k]["vgpr"] + rep[k]["agpr"] <= 256 and rep[k]["occ"] >= 2, (k, rep[k])
        assert rep[k]["scratch"] == 0 or k == "void blind_rotate_kernel_v3<0, 8, true, true, 4>(BrArgs)", (k, rep[k])


def test_committed_profile_shows_the_vector_adds_gone():
    """SQ_INSTS_VALU per launch of the headline kernel in the profile of the committed sources: 3.9657 G (profiles/tan2_cfg2/) before;
    the accumulator's 2 x (16 adds + the mirror's negation) per wave-step x 4096 x 500 are gone.  Of the two changes this one was
    proposed with, one ships: the bound for one, 3.90 G."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from source_hash import kernel_source_sha16
    want = kernel_source_sha16(ROOT)
    hits = []
    for f in glob.glob(os.path.join(ROOT, "profiles", "*_cfg2", "counters.json")):
        d = json.load(open(f))
        if d.get("_meta", {}).get("kernel_source_sha16") == want:
            hits.append((f, d))
    assert hits, f"no profiles/*_cfg2/counters.json for kernel sources {want}"
    for f, d in hits:
        v3 = [v for k, v in d.items() if HEADLINE in k]
        assert v3, f
        assert v3[0]["valu_insts_per_launch"] <= 3.90e9, (f, v3[0]["valu_insts_per_launch"])
