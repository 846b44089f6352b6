"""Static checks of the leveled wrappers of julia/TFHEMI355X (tgsw_load!, extern_mul, cmux_tree), in the manner of tests/test_julia_shim.py
(no Julia runtime in the build image): each exists as a method on GpuCloudKey, is exported, makes its ccall under the context's lock with
the C prototype's parameter kinds, and turns Julia's 1-based selector / table indices into the library's 0-based ones."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists

WRAPPERS = {"tgsw_load!": "tfhe_tgsw_load", "extern_mul": "tfhe_extern_mul_batch", "cmux_tree": "tfhe_cmux_tree_batch"}


def _body(src, name):
    m = re.search(r"function " + re.escape(name) + r"\(gck::GpuCloudKey.*?\n(.*?)\nend\n", src, flags=re.S)
    assert m, f"no {name}(gck::GpuCloudKey, ...) method"
    return m.group(1)


def test_leveled_wrappers_bind_the_declared_entry_points():
    protos = c_prototypes()
    src = strip_julia(open(JULIA[0]).read())
    exported = _name_lists(src, "export")
    for fn, sym in WRAPPERS.items():
        assert fn in exported, f"{fn} is not exported"
        body = _body(src, fn)
        calls = ccalls(body)
        assert [c[0] for c in calls] == [sym], (fn, calls)
        _, types, nargs = calls[0]
        assert types is not None and len(types) == nargs == len(protos[sym])
        assert [julia_kind(t) for t in types] == protos[sym], (fn, types, protos[sym])
        assert types[0].strip() == "Ptr{Cvoid}"
        line = body[body.rfind("\n", 0, body.index("ccall")):body.index("ccall")]
        assert "@locked gck.ctx" in line and "GC.@preserve" in line and "check(gck.ctx" in line, line
    assert protos["tfhe_cmux_tree_batch"] == ["ptr", "ptr", "int", "ptr", "int", "ptr", "ptr", "int", "int"]


def test_leveled_wrappers_pass_zero_based_indices_and_widths():
    src = strip_julia(open(JULIA[0]).read())
    assert re.search(r"idx = Int32\.\(collect\(sel\) \.- 1\)", _body(src, "extern_mul"))
    tree = _body(src, "cmux_tree")
    assert re.search(r"Matrix\{Int32\}\(sel \.- 1\)", tree) and re.search(r"collect\(table_index\) \.- 1", tree)
    assert re.search(r"idx === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(idx\)", tree)          # NULL = table 0 for every row
    assert re.search(r"depth, B = size\(sel\)", tree) and re.search(r"1 <= depth <= 12", tree)
    assert re.search(r"width = out_form == 2 \? p\.lwe_size : k \* N", tree)
    # the sizes on the C side are Int64 (S, T, B), depth and out_form Int32
    types = ccalls(tree)[0][1]
    assert [t.strip() for t in types] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int64", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int64", "Int32"]
