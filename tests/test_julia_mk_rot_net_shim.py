"""Static checks of the wrapper of the multi-key CMUX networks with monomial edges of julia/TFHEMI355X (mk_rot_net), in the manner of
tests/test_julia_rot_net_shim.py (no Julia runtime in the build image): it exists as a method on GpuMKCloudKey under a name of its own,
is exported, makes its one ccall under the context's lock with the C prototype's parameter kinds, turns Julia's 1-based sources,
variables, selectors and table indices into the library's 0-based ones and passes the rotations, which are exponents, unchanged."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists
from test_julia_mk_leveled_shim import _body


def test_mk_rot_net_wrapper_binds_the_declared_entry_point():
    protos = c_prototypes()
    src = strip_julia(open(JULIA[0]).read())
    assert "mk_rot_net" in _name_lists(src, "export")
    assert not re.search(r"function rot_net\(mck::GpuMKCloudKey", src)               # a name of its own, not a method of rot_net
    body = _body(src, "mk_rot_net")
    calls = ccalls(body)
    assert [c[0] for c in calls] == ["tfhe_mk_rot_net_batch"], calls
    _, types, nargs = calls[0]
    assert types is not None and len(types) == nargs == len(protos["tfhe_mk_rot_net_batch"]) == 13
    assert [julia_kind(t) for t in types] == protos["tfhe_mk_rot_net_batch"], (types, protos["tfhe_mk_rot_net_batch"])
    assert protos["tfhe_mk_rot_net_batch"] == protos["tfhe_mk_cmux_net_batch"]        # the contract differs in the record alone
    line = body[body.rfind("\n", 0, body.index("ccall")):body.index("ccall")]
    assert "@locked mck.ctx" in line and "GC.@preserve" in line and "check(mck.ctx" in line, line
    # the sizes on the C side: T and B Int64; E, levels, V and out_form Int32
    assert [t.strip() for t in types] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int64", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Ptr{Int32}",
                                          "Int32", "Ptr{Int32}", "Int64", "Int32"]


def test_mk_rot_net_wrapper_checks_its_arguments_and_keeps_the_rotations():
    body = _body(strip_julia(open(JULIA[0]).read()), "mk_rot_net")
    # rows 1 ... 3 of a record (src0, src1, var) become 0-based, rows 4 ... 5 (rot0, rot1) pass as they are
    assert re.search(r"Matrix\{Int32\}\(vcat\(nodes\[1:3, :\] \.- 1, nodes\[4:5, :\]\)\)", body) and re.search(r"Matrix\{Int32\}\(sel \.- 1\)", body)
    assert not re.search(r"nodes \.- 1", body)
    assert re.search(r"0 <= r < 2N, view\(nodes, 4:5, :\)", body)
    assert re.search(r"collect\(table_index\) \.- 1", body)
    assert re.search(r"idx === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(idx\)", body)          # NULL = table 0 for every row
    assert re.search(r"1 <= levels <= 1024", body) and re.search(r"1 <= x <= 4096", body)
    assert re.search(r"size\(nodes\) == \(5, sum\(w\)\)", body) and re.search(r"V, B = size\(sel\)", body)
    assert re.search(r"0 <= out_form <= 2", body)
    assert re.search(r"size\(data\)\[1:2\] == \(N, P \+ 1\)", body)
    assert re.search(r"width = out_form == 2 \? P \* n : P \* N", body)
    assert re.search(r"Array\{Int32\}\(undef, N, P \+ 1, F, B\)", body) and re.search(r"Array\{Int32\}\(undef, width \+ 1, F \* B\)", body)
