"""Static checks of the wrappers of the multi-key private-table rotation on the gates' kernel of julia/TFHEMI355X (mk_bootstrap_acc,
mk_bootstrap_acc_level!), in the manner of tests/test_julia_bootstrap_acc_shim.py (no Julia runtime in the build image): each exists as a
method on GpuMKCloudKey, is exported, makes its one ccall under the context's lock with the C prototype's parameter kinds, turns Julia's
1-based accumulator indices, slots and wires into the library's 0-based ones and passes rows, term_start, coefficients and constants
unchanged; neither takes selectors, and both have the single-key calls' prototypes, argument for argument."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists
from test_julia_mk_leveled_shim import _body

WRAPPERS = {"mk_bootstrap_acc": "tfhe_mk_bootstrap_acc_batch", "mk_bootstrap_acc_level!": "tfhe_mk_bootstrap_acc_level"}


def test_wrappers_bind_the_declared_entry_points():
    protos = c_prototypes()
    src = strip_julia(open(JULIA[0]).read())
    exported = _name_lists(src, "export")
    for fn, sym in WRAPPERS.items():
        assert fn in exported, f"{fn} is not exported"
        body = _body(src, fn)                                                             # (asserts the method on GpuMKCloudKey)
        calls = ccalls(body)
        assert [c[0] for c in calls] == [sym], (fn, calls)
        _, types, nargs = calls[0]
        assert types is not None and len(types) == nargs == len(protos[sym]), (fn, types, nargs)
        assert [julia_kind(t) for t in types] == protos[sym], (fn, types, protos[sym])
        line = body[body.rfind("\n", 0, body.index("ccall")):body.index("ccall")]
        assert "@locked mck.ctx" in line and "GC.@preserve" in line and "check(mck.ctx" in line, line
    assert protos["tfhe_mk_bootstrap_acc_batch"] == protos["tfhe_bootstrap_acc_batch"] == ["ptr", "ptr", "int", "ptr", "ptr", "int", "int", "ptr", "int"]
    assert protos["tfhe_mk_bootstrap_acc_level"] == protos["tfhe_bootstrap_acc_level"] == ["ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "int", "int", "ptr", "ptr", "int"]


def test_sizes_on_the_c_side():
    src = strip_julia(open(JULIA[0]).read())
    types = {fn: [t.strip() for t in ccalls(_body(src, fn))[0][1]] for fn in WRAPPERS}
    # T and B Int64; n_out and out_form Int32
    assert types["mk_bootstrap_acc"] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int64", "Ptr{Int32}", "Ptr{Int32}", "Int32", "Int32", "Ptr{Int32}", "Int64"]
    assert types["mk_bootstrap_acc_level!"] == ["Ptr{Cvoid}"] + ["Ptr{Int32}"] * 5 + ["Int32", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int64"]


def test_wrappers_check_their_arguments_and_keep_the_rows():
    src = strip_julia(open(JULIA[0]).read())
    body = _body(src, "mk_bootstrap_acc")
    assert re.search(r"Int32\.\(collect\(acc_index\) \.- 1\)", body) and "sel" not in body
    assert re.search(r"r = Matrix\{Int32\}\(rows\)", body) and not re.search(r"rows \.- 1", body)
    assert re.search(r"idx === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(idx\)", body)          # NULL = accumulator 0 for every row
    assert re.search(r"words == P \* n \+ 1", body)                                                # multi-key LWE samples: the steps are the key's P n
    assert re.search(r"size\(acc\)\[1:2\] == \(N, P \+ 1\)", body)
    assert re.search(r"0 <= out_form <= 2", body) and re.search(r"ispow2\(n_out\) && n_out <= 32", body) and re.search(r"out_form != 0 \|\| n_out == 1", body)
    assert re.search(r"width = out_form == 2 \? P \* n : P \* N", body)
    assert re.search(r"Array\{Int32\}\(undef, N, P \+ 1, B\)", body) and re.search(r"Array\{Int32\}\(undef, width \+ 1, n_out \* B\)", body)
    body = _body(src, "mk_bootstrap_acc_level!")
    for name in ("acc_slot", "term_wire", "out_slot", "out_wires"):
        assert re.search(r"Int32\.\(collect\(" + name + r"\) \.- 1\)", body), name
    for name in ("term_start", "term_coef", "cst"):
        assert re.search(r"Int32\.\(collect\(" + name + r"\)\)", body) and not re.search(name + r"\) \.- 1", body), name
    assert "sel" not in body
    assert re.search(r"out_form == 0 \|\| out_form == 2", body)                                       # extracted rows have no table
    assert re.search(r"c === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(c\)", body)
