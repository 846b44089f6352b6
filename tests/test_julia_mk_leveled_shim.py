"""Static checks of the multi-key leveled wrappers of julia/TFHEMI355X (mk_tgsw_load!, mk_extern_mul, mk_cmux_tree), in the manner of
tests/test_julia_leveled_shim.py (no Julia runtime in the build image): each exists as a method on GpuMKCloudKey, is exported, makes its
ccall under the context's lock with the C prototype's parameter kinds, and turns Julia's 1-based party / selector / table indices into
the library's 0-based ones."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists

WRAPPERS = {"mk_tgsw_load!": "tfhe_mk_tgsw_load", "mk_extern_mul": "tfhe_mk_extern_mul_batch", "mk_cmux_tree": "tfhe_mk_cmux_tree_batch"}


def _body(src, name):
    m = re.search(r"function " + re.escape(name) + r"\(mck::GpuMKCloudKey.*?\n(.*?)\nend\n", src, flags=re.S)
    assert m, f"no {name}(mck::GpuMKCloudKey, ...) method"
    return m.group(1)


def test_mk_leveled_wrappers_bind_the_declared_entry_points():
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
        assert "@locked mck.ctx" in line and "GC.@preserve" in line and "check(mck.ctx" in line, line
    assert protos["tfhe_mk_tgsw_load"] == ["ptr", "ptr", "ptr", "int", "int"]
    assert protos["tfhe_mk_cmux_tree_batch"] == protos["tfhe_cmux_tree_batch"]
    assert protos["tfhe_mk_tgsw_expand_load"] == ["ptr", "int"] + ["ptr"] * 8 + ["int", "ptr"]


def test_mk_leveled_wrappers_pass_zero_based_indices_and_widths():
    src = strip_julia(open(JULIA[0]).read())
    load = _body(src, "mk_tgsw_load!")
    assert re.search(r"who = Int32\.\(collect\(party_of\) \.- 1\)", load) and re.search(r"Int64\(length\(who\)\), Int32\(P\)\)\)", load)
    assert re.search(r"idx = Int32\.\(collect\(sel\) \.- 1\)", _body(src, "mk_extern_mul"))
    tree = _body(src, "mk_cmux_tree")
    assert re.search(r"Matrix\{Int32\}\(sel \.- 1\)", tree) and re.search(r"collect\(table_index\) \.- 1", tree)
    assert re.search(r"idx === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(idx\)", tree)          # NULL = table 0 for every row
    assert re.search(r"depth, B = size\(sel\)", tree) and re.search(r"1 <= depth <= 12", tree)
    assert re.search(r"width = out_form == 2 \? P \* n : P \* N", tree)
    types = ccalls(tree)[0][1]
    assert [t.strip() for t in types] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int64", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int64", "Int32"]
    types = ccalls(load)[0][1]
    assert [t.strip() for t in types] == ["Ptr{Cvoid}", "Ptr{Int32}", "Ptr{Int32}", "Int64", "Int32"]
