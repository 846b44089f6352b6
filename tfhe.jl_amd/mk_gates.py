"""Multi-key homomorphic gates — the gate set of src/gates.jl over multi-key samples (mk_gates.jl:7-12 is the NAND case).

Each call is one batch call into the HIP engine (tfhe_mk_gates_batch): every bootstrapped gate is one multi-key blind
rotation and one multi-key keyswitch, MUX two rotations and one keyswitch, NOT / constant none.  A flat sample
[P*n+1] in gives a flat sample out; a [B][P*n+1] matrix in gives a matrix out (as mk_gate_nand).  There is no host
fallback.
"""
import numpy as np

from ._lib import OPCODES


def _as_matrix(x):
    a = np.asarray(x, np.int32)
    return (a[None, :], True) if a.ndim == 1 else (a, False)


def _run(ck, op, *operands, device=0):
    eng = ck.engine(device)
    mats, scalar = [], True
    for x in operands:
        m, s = _as_matrix(x)
        mats.append(m)
        scalar = scalar and s
    B = max(m.shape[0] for m in mats)
    mats = [np.broadcast_to(m, (B, m.shape[1])) if m.shape[0] != B else m for m in mats]
    out = eng.mk_gates_batch(np.full(B, OPCODES[op], np.uint8), *mats)
    return out[0] if scalar else out


def mk_gate_or(ck, x, y, device=0):
    """gates.jl:27-30 over multi-key samples"""
    return _run(ck, "OR", x, y, device=device)


def mk_gate_and(ck, x, y, device=0):
    """gates.jl:39-42 over multi-key samples"""
    return _run(ck, "AND", x, y, device=device)


def mk_gate_xor(ck, x, y, device=0):
    """gates.jl:51-54 over multi-key samples"""
    return _run(ck, "XOR", x, y, device=device)


def mk_gate_xnor(ck, x, y, device=0):
    """gates.jl:63-66 over multi-key samples"""
    return _run(ck, "XNOR", x, y, device=device)


def mk_gate_not(ck, x, device=0):
    """gates.jl:76-79 over multi-key samples (no bootstrap)"""
    return _run(ck, "NOT", x, device=device)


def mk_gate_constant(ck, value, device=0):
    """gates.jl:91-93: a trivial multi-key sample of `value` (all-zero masks, b = +-1/8)."""
    out = ck.engine(device).mk_gates_batch(np.array([OPCODES["CONST1" if value else "CONST0"]], np.uint8), None)
    return out[0]


def mk_gate_nor(ck, x, y, device=0):
    """gates.jl:102-105 over multi-key samples"""
    return _run(ck, "NOR", x, y, device=device)


def mk_gate_andny(ck, x, y, device=0):
    """gates.jl:114-117 over multi-key samples"""
    return _run(ck, "ANDNY", x, y, device=device)


def mk_gate_andyn(ck, x, y, device=0):
    """gates.jl:126-129 over multi-key samples"""
    return _run(ck, "ANDYN", x, y, device=device)


def mk_gate_orny(ck, x, y, device=0):
    """gates.jl:138-141 over multi-key samples"""
    return _run(ck, "ORNY", x, y, device=device)


def mk_gate_oryn(ck, x, y, device=0):
    """gates.jl:150-153 over multi-key samples"""
    return _run(ck, "ORYN", x, y, device=device)


def mk_gate_mux(ck, x, y, z, device=0):
    """gates.jl:163-177 over multi-key samples: two rotations, one keyswitch"""
    return _run(ck, "MUX", x, y, z, device=device)


def mk_gates_batch(ck, opcodes, in0, in1=None, in2=None, device=0):
    """Mixed batch of independent multi-key gates: opcodes are names or numbers, operands int32 [B][P*n+1] (None where no
    opcode reads them); returns int32 [B][P*n+1]."""
    ops = np.array([OPCODES[o] if isinstance(o, str) else int(o) for o in opcodes], np.uint8)
    mats = [None if x is None else np.atleast_2d(np.asarray(x, np.int32)) for x in (in0, in1, in2)]
    return ck.engine(device).mk_gates_batch(ops, *mats)
