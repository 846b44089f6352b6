"""Static checks of the wrappers of the device-resident TLWE table and its level calls of julia/TFHEMI355X (tlwe_alloc!, tlwe_upload!,
tlwe_download, tgsw_update!, rot_net_level!, blind_rotate_level!), in the manner of tests/test_julia_blind_rotate_shim.py (no Julia
runtime in the build image): each exists as a method on GpuCloudKey, is exported, makes its one ccall under the context's lock with the C
prototype's parameter kinds, and turns Julia's 1-based slots, wires and selectors into the library's 0-based ones while term_start,
coefficients, constants and rotations pass unchanged."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists
from test_julia_leveled_shim import _body

WRAPPERS = {"tlwe_alloc!": "tfhe_tlwe_alloc", "tlwe_upload!": "tfhe_tlwe_upload", "tlwe_download": "tfhe_tlwe_download", "tgsw_update!": "tfhe_tgsw_update",
            "rot_net_level!": "tfhe_rot_net_level", "blind_rotate_level!": "tfhe_blind_rotate_level"}


def test_wrappers_bind_the_declared_entry_points():
    protos = c_prototypes()
    src = strip_julia(open(JULIA[0]).read())
    exported = _name_lists(src, "export")
    for fn, sym in WRAPPERS.items():
        assert fn in exported, f"{fn} is not exported"
        body = _body(src, fn)                                                             # (asserts the method on GpuCloudKey)
        calls = ccalls(body)
        assert [c[0] for c in calls] == [sym], (fn, calls)
        _, types, nargs = calls[0]
        assert types is not None and len(types) == nargs == len(protos[sym]), (fn, types, nargs)
        assert [julia_kind(t) for t in types] == protos[sym], (fn, types, protos[sym])
        assert types[0].strip() == "Ptr{Cvoid}"
        line = body[body.rfind("\n", 0, body.index("ccall")):body.index("ccall")]
        assert "@locked gck.ctx" in line and "check(gck.ctx" in line, line
        assert fn == "tlwe_alloc!" or "GC.@preserve" in line, line                        # (tlwe_alloc! passes no array)
    assert protos["tfhe_tlwe_alloc"] == ["ptr", "int"] and protos["tfhe_tgsw_update"] == ["ptr", "ptr", "int", "int"]
    assert protos["tfhe_tlwe_upload"] == protos["tfhe_tlwe_download"] == ["ptr", "int", "int", "ptr"]
    assert protos["tfhe_rot_net_level"] == ["ptr", "ptr", "int", "ptr", "int", "ptr", "ptr", "int", "int", "int", "ptr", "int"]
    assert protos["tfhe_blind_rotate_level"] == ["ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "int", "int", "ptr", "ptr", "int"]


def test_sizes_on_the_c_side():
    src = strip_julia(open(JULIA[0]).read())
    types = {fn: [t.strip() for t in ccalls(_body(src, fn))[0][1]] for fn in WRAPPERS}
    assert types["tlwe_alloc!"] == ["Ptr{Cvoid}", "Int64"]
    assert types["tlwe_upload!"] == types["tlwe_download"] == ["Ptr{Cvoid}", "Int64", "Int64", "Ptr{Int32}"]
    assert types["tgsw_update!"] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int64", "Int64"]
    # E, levels, V and out_form Int32; out_first and B Int64
    assert types["rot_net_level!"] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int32", "Int32", "Int64",
                                       "Ptr{Int32}", "Int64"]
    # n_out and out_form Int32; B Int64
    assert types["blind_rotate_level!"] == ["Ptr{Cvoid}"] + ["Ptr{Int32}"] * 6 + ["Int32", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int64"]


def test_wrappers_turn_one_based_indices_into_zero_based_ones():
    src = strip_julia(open(JULIA[0]).read())
    for fn in ("tlwe_upload!", "tlwe_download", "tgsw_update!"):
        assert re.search(r"Int64\(first - 1\)", _body(src, fn)), fn
    body = _body(src, "rot_net_level!")
    assert re.search(r"vcat\(nodes\[1:3, :\] \.- 1, nodes\[4:5, :\]\)", body) and re.search(r"Matrix\{Int32\}\(sel \.- 1\)", body)
    assert re.search(r"Int32\.\(collect\(table_first\) \.- 1\)", body) and re.search(r"Int32\.\(collect\(out_wires\) \.- 1\)", body)
    assert re.search(r"Int64\(out_first - 1\)", body)
    assert re.search(r"tf === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(tf\)", body)              # NULL = absolute slots
    assert re.search(r"out_form == 0 \|\| out_form == 2", body)                                       # extracted rows have no table
    body = _body(src, "blind_rotate_level!")
    for name in ("acc_slot", "term_wire", "sel", "out_slot", "out_wires"):
        assert re.search(r"Int32\.\(collect\(" + name + r"\) \.- 1\)", body), name
    for name in ("term_start", "term_coef", "cst"):                                                   # pass unchanged
        assert re.search(r"Int32\.\(collect\(" + name + r"\)\)", body) and not re.search(name + r"\) \.- 1", body), name
    assert re.search(r"s === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(s\)", body)                 # NULL = selector i for step i
    assert re.search(r"c === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(c\)", body)
    assert re.search(r"length\(s\) == p\.lwe_size", body)                                             # steps = the context's n
    assert re.search(r"out_form == 0 \|\| out_form == 2", body) and re.search(r"out_form != 0 \|\| n_out == 1", body)
    assert re.search(r"ispow2\(n_out\) && n_out <= 32", body)
