"""Static checks of the wrappers of the device-resident MK TLWE table, the in-place selector updates and the multi-key level calls of
julia/TFHEMI355X (mk_tlwe_alloc!, mk_tlwe_upload!, mk_tlwe_download, mk_tgsw_update!, mk_tgsw_expand_update!, mk_rot_net_level!,
mk_blind_rotate_level!), in the manner of tests/test_julia_tlwe_levels_shim.py (no Julia runtime in the build image): each exists as a
method on GpuMKCloudKey (the key type that holds a multi-key context), is exported, makes its one ccall under the context's lock with the
C prototype's parameter kinds, and turns Julia's 1-based slots, wires, selectors and parties into the library's 0-based ones while
term_start, coefficients, constants and rotations pass unchanged."""
import re

from test_julia_shim import JULIA, c_prototypes, ccalls, julia_kind, strip_julia, _name_lists
from test_julia_mk_leveled_shim import _body

WRAPPERS = {"mk_tlwe_alloc!": "tfhe_mk_tlwe_alloc", "mk_tlwe_upload!": "tfhe_mk_tlwe_upload", "mk_tlwe_download": "tfhe_mk_tlwe_download",
            "mk_tgsw_update!": "tfhe_mk_tgsw_update", "mk_tgsw_expand_update!": "tfhe_mk_tgsw_expand_update", "mk_rot_net_level!": "tfhe_mk_rot_net_level",
            "mk_blind_rotate_level!": "tfhe_mk_blind_rotate_level"}


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
        assert types[0].strip() == "Ptr{Cvoid}"
        line = body[body.rfind("\n", 0, body.index("ccall")):body.index("ccall")]
        assert "@locked mck.ctx" in line and "check(mck.ctx" in line, line
        assert fn == "mk_tlwe_alloc!" or "GC.@preserve" in line, line                     # (mk_tlwe_alloc! passes no array)
    # the single-key calls, argument for argument
    for mk, sk in (("tfhe_mk_tlwe_alloc", "tfhe_tlwe_alloc"), ("tfhe_mk_tlwe_upload", "tfhe_tlwe_upload"), ("tfhe_mk_tlwe_download", "tfhe_tlwe_download"),
                   ("tfhe_mk_rot_net_level", "tfhe_rot_net_level"), ("tfhe_mk_blind_rotate_level", "tfhe_blind_rotate_level")):
        assert protos[mk] == protos[sk], mk
    assert protos["tfhe_mk_tgsw_update"] == ["ptr", "ptr", "ptr", "int", "int", "int"]
    assert protos["tfhe_mk_tgsw_expand_update"] == ["ptr", "int"] + ["ptr"] * 8 + ["int", "int", "ptr"]


def test_sizes_on_the_c_side():
    src = strip_julia(open(JULIA[0]).read())
    types = {fn: [t.strip() for t in ccalls(_body(src, fn))[0][1]] for fn in WRAPPERS}
    assert types["mk_tlwe_alloc!"] == ["Ptr{Cvoid}", "Int64"]
    assert types["mk_tlwe_upload!"] == types["mk_tlwe_download"] == ["Ptr{Cvoid}", "Int64", "Int64", "Ptr{Int32}"]
    # first and count Int64, parties Int32
    assert types["mk_tgsw_update!"] == ["Ptr{Cvoid}", "Ptr{Int32}", "Ptr{Int32}", "Int64", "Int64", "Int32"]
    assert types["mk_tgsw_expand_update!"] == ["Ptr{Cvoid}", "Int32"] + ["Ptr{Int32}"] * 8 + ["Int64", "Int64", "Ptr{Int32}"]
    # E, levels, V and out_form Int32; out_first and B Int64
    assert types["mk_rot_net_level!"] == ["Ptr{Cvoid}", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int32", "Int32", "Int64",
                                          "Ptr{Int32}", "Int64"]
    # n_out and out_form Int32; B Int64
    assert types["mk_blind_rotate_level!"] == ["Ptr{Cvoid}"] + ["Ptr{Int32}"] * 6 + ["Int32", "Int32", "Ptr{Int32}", "Ptr{Int32}", "Int64"]


def test_wrappers_turn_one_based_indices_into_zero_based_ones():
    src = strip_julia(open(JULIA[0]).read())
    for fn in ("mk_tlwe_upload!", "mk_tlwe_download", "mk_tgsw_update!", "mk_tgsw_expand_update!"):
        assert re.search(r"Int64\(first - 1\)", _body(src, fn)), fn
    for fn in ("mk_tgsw_update!", "mk_tgsw_expand_update!"):
        body = _body(src, fn)
        assert re.search(r"Int32\.\(collect\(party_of\) \.- 1\)", body) and re.search(r"Int32\(P\)", body), fn
    assert re.search(r"size\(samples\)\[1:2\] == \(p\.tlwe_polynomial_degree, P \+ 1\)", _body(src, "mk_tlwe_upload!"))
    assert re.search(r"Array\{Int32\}\(undef, p\.tlwe_polynomial_degree, P \+ 1, count\)", _body(src, "mk_tlwe_download"))
    body = _body(src, "mk_rot_net_level!")
    assert re.search(r"vcat\(nodes\[1:3, :\] \.- 1, nodes\[4:5, :\]\)", body) and re.search(r"Matrix\{Int32\}\(sel \.- 1\)", body)
    assert re.search(r"Int32\.\(collect\(table_first\) \.- 1\)", body) and re.search(r"Int32\.\(collect\(out_wires\) \.- 1\)", body)
    assert re.search(r"Int64\(out_first - 1\)", body)
    assert re.search(r"tf === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(tf\)", body)              # NULL = absolute slots
    assert re.search(r"out_form == 0 \|\| out_form == 2", body)                                       # extracted rows have no table
    body = _body(src, "mk_blind_rotate_level!")
    for name in ("acc_slot", "term_wire", "sel", "out_slot", "out_wires"):
        assert re.search(r"Int32\.\(collect\(" + name + r"\) \.- 1\)", body), name
    for name in ("term_start", "term_coef", "cst"):                                                   # pass unchanged
        assert re.search(r"Int32\.\(collect\(" + name + r"\)\)", body) and not re.search(name + r"\) \.- 1", body), name
    assert re.search(r"s === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(s\)", body)                 # NULL = selector i for step i
    assert re.search(r"c === nothing \? Ptr\{Int32\}\(C_NULL\) : pointer\(c\)", body)
    assert re.search(r"length\(s\) == P \* p\.lwe_size", body)                                        # steps = P n
    assert re.search(r"out_form == 0 \|\| out_form == 2", body) and re.search(r"out_form != 0 \|\| n_out == 1", body)
    assert re.search(r"ispow2\(n_out\) && n_out <= 32", body)
