"""Static checks of the wrapper of the multi-key blind rotation of the caller's accumulators of julia/TFHEMI355X (mk_blind_rotate), in
the manner of tests/test_julia_blind_rotate_shim.py (no Julia runtime in the build image): it exists as a method on GpuMKCloudKey under a
name of its own, is exported, makes its one ccall under the context's lock with the C prototype's parameter kinds, turns Julia's 1-based
selectors and accumulator indices into the library's 0-based ones and passes the rows, which are LWE words or exponents, unchanged."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists
from test_julia_mk_leveled_shim import _body


def test_mk_blind_rotate_wrapper_binds_the_declared_entry_point():
    protos = c_prototypes()
    src = strip_julia(open(JULIA[0]).read())
    assert "mk_blind_rotate" in _name_lists(src, "export")
    assert not re.search(r"function blind_rotate\(mck::GpuMKCloudKey", src)          # a name of its own, not a method of blind_rotate
    body = _body(src, "mk_blind_rotate")
    calls = ccalls(body)
    assert [c[0] for c in calls] == ["tfhe_mk_blind_rotate_batch"], calls
    _, types, nargs = calls[0]
    assert types is not None and len(types) == nargs == len(protos["tfhe_mk_blind_rotate_batch"]) == 12
    assert [julia_kind(t) for t in types] == protos["tfhe_mk_blind_rotate_batch"], (types, protos["tfhe_mk_blind_rotate_batch"])
    assert protos["tfhe_mk_blind_rotate_batch"] == protos["tfhe_blind_rotate_batch"]           # the single-key call, argument for argument
    assert protos["tfhe_mk_blind_rotate_batch"] == ["ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "int", "ptr", "int", "int"]
    line = body[body.rfind("\n", 0, body.index("ccall")):body.index("ccall")]
    assert "@locked mck.ctx" in line and "GC.@preserve" in line and "check(mck.ctx" in line, line
    # the sizes on the C side: T and B Int64; steps, in_form, n_out and out_form Int32
    assert [t.strip() for t in types] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int64", "Ptr{Int32}", "Ptr{Int32}", "Int32", "Int32", "Ptr{Int32}", "Int32",
                                          "Ptr{Int32}", "Int64", "Int32"]


def test_mk_blind_rotate_wrapper_checks_its_arguments_and_keeps_the_rows():
    body = _body(strip_julia(open(JULIA[0]).read()), "mk_blind_rotate")
    # selectors and accumulator indices become 0-based; the rows pass as they are
    assert re.search(r"Int32\.\(collect\(sel\) \.- 1\)", body) and re.search(r"Int32\.\(collect\(acc_index\) \.- 1\)", body)
    assert re.search(r"r = Matrix\{Int32\}\(rows\)", body) and not re.search(r"rows \.- 1", body)
    assert re.search(r"idx === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(idx\)", body)          # NULL = accumulator 0 for every row
    assert re.search(r"s === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(s\)", body)              # NULL = selector i for step i
    assert re.search(r"words, B = size\(rows\)", body) and re.search(r"steps = words - 1", body) and re.search(r"1 <= steps <= 65536", body)
    assert re.search(r"0 <= in_form <= 1", body) and re.search(r"0 <= out_form <= 2", body)
    assert re.search(r"ispow2\(n_out\) && n_out <= 32", body) and re.search(r"out_form != 0 \|\| n_out == 1", body)
    assert re.search(r"in_form == 0 \|\| all\(e -> 0 <= e < 2N, rows\)", body)
    assert re.search(r"size\(acc\)\[1:2\] == \(N, P \+ 1\)", body)
    assert re.search(r"width = out_form == 2 \? P \* n : P \* N", body)
    assert re.search(r"Array\{Int32\}\(undef, N, P \+ 1, B\)", body) and re.search(r"Array\{Int32\}\(undef, width \+ 1, n_out \* B\)", body)
