"""TLWE-valued nodes of Circuit (tlwe_inputs, rot_net, blind_rotate) on the device-resident TLWE table: the planner on the CPU, a mixed
circuit at N = 64 word for word against the same composition through the host-buffer calls, and examples/private_lut_circuit.py's
two-stage private lookup (p = q = 8, inside the noise window by tests/test_blind_rotate.py's schoolbook run) at tfhe_parameters_80."""
import importlib.util
import os

import numpy as np
import pytest

from test_tlwe_levels import SETS, _setup, form_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mixed(tfhe, n, N):
    """Gates, then a tree that picks a TLWE node, a rotation of it by computed wires into a wire and one of an input into a TLWE node, a
    network with monomial edges over both TLWE results into a wire, then a gate on the two wires."""
    from tfhe_jl_amd import leveled
    c = tfhe.Circuit()
    a, b, d = c.inputs(3)
    tl = c.tlwe_inputs(4)
    g = c.nand(a, b)
    picked = c.rot_net(leveled.tree_net(2), tl, [n, n + 1], out="tlwe")[0]
    r = c.blind_rotate(picked, [g, (d, -2)], const=123)
    r2 = c.blind_rotate(tl[1], [g], out="tlwe")
    edge = leveled.RotNet([1], [(0, 1, 0, 1, 2 * N - 5)], N)
    lw = c.rot_net(edge, [r2, picked], [n + 1], out="lwe")[0]
    both = c.blind_rotate(tl[3], [(a, 3)], n_out=2, sel=list(range(1, n + 1)))
    c.set_outputs([c.xor(r, lw), r, lw] + both)
    return c, edge


def test_planner_levels_tlwe_nodes_with_the_gates(tfhe):
    n, N = 7, 64
    c, _ = _mixed(tfhe, n, N)
    assert c.num_tlwe == 6 and c.num_wires == 3 + 1 + 1 + 1 + 2 + 1
    plan = c.level_plan(N)
    assert len(plan) == 4
    assert [len(lv["blind_rotate"]) for lv in plan] == [1, 2, 0, 0] and [len(lv["rot_net"]) for lv in plan] == [1, 0, 1, 0]
    net, sel, form, out_first, out_wires = plan[0]["rot_net"][0]
    assert net.entries == 4 and sel.tolist() == [[n, n + 1]] and form == 0 and out_first == 4 and out_wires is None
    assert net.nodes.tolist() == [[0, 1, 0, 0, 0], [2, 3, 0, 0, 0], [0, 1, 1, 0, 0]]
    acc, start, wire, coef, cst, rsel, n_out, form, out_slot, out_w = plan[0]["blind_rotate"][0]          # the rotation by an input alone
    assert acc.tolist() == [3] and start.tolist() == [0, 1] and wire.tolist() == [0] and coef.tolist() == [3] and rsel.tolist() == list(range(1, n + 1))
    assert n_out == 2 and form == 2 and out_slot is None and len(out_w) == 2
    by_form = {r[7]: r for r in plan[1]["blind_rotate"]}                  # one call per (n_out, out, sel)
    assert by_form[2][0].tolist() == [4] and by_form[2][2].tolist() == [2, 3] and by_form[2][3].tolist() == [-2, 1] and by_form[2][4].tolist() == [123]
    assert by_form[0][0].tolist() == [1] and by_form[0][8].tolist() == [5] and by_form[0][5] is None
    net, sel, form, out_first, out_wires = plan[2]["rot_net"][0]          # absolute sources: slot 5 (r2), slot 4 (picked)
    assert net.entries == 6 and net.nodes.tolist() == [[5, 4, 0, 1, 2 * N - 5]] and form == 2 and len(out_wires) == 1
    assert plan[3]["gates"] is not None and plan[3]["gates"][0].tolist() == [3]
    # a circuit without TLWE nodes plans as before
    plain = tfhe.Circuit()
    x, y = plain.inputs(2)
    plain.set_outputs([plain.nand(x, y)])
    assert sorted(plain.level_plan(N)[0]) == ["gates", "linear", "lut"]


def test_run_batch_and_multikey_raise(tfhe):
    from tfhe_jl_amd import leveled
    c, _ = _mixed(tfhe, 7, 64)
    with pytest.raises(ValueError, match="run_batch"):
        c.run_batch(None, np.zeros((2, 3, 8), np.int32))
    mk = object.__new__(tfhe.MKCloudKey)                                 # (refused before any engine is made)
    with pytest.raises(ValueError, match="single-key"):
        c.run(mk, np.zeros((3, 8), np.int32), tlwe_inputs=np.zeros((4, 2, 64), np.int32))
    with pytest.raises(ValueError):
        c.rot_net(leveled.tree_net(1), [0, 1], [0])                      # wires are not TLWE nodes
    with pytest.raises(ValueError):
        c.blind_rotate(5, [0])
    with pytest.raises(ValueError, match="TLWE inputs"):
        c.tlwe_inputs(1)                                                 # after the first TLWE-valued node


@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta,n", SETS)
def test_gpu_mixed_circuit_equals_the_host_composition(tfhe, N, k, l, beta, n):
    from tfhe_jl_amd import leveled
    rng, sk, ck, eng, tgsw, tlwe, wires = _setup(tfhe, N, k, l, beta, n, 9800 + N, table=False)
    c, edge = _mixed(tfhe, n, N)
    ins, tl = wires[:3], tlwe[2:6]
    got = c.run(ck, ins, tlwe_inputs=tl).data
    # the same composition through the host-buffer calls
    g = eng.gates(np.zeros(1, np.uint8), ins[0:1], ins[1:2])
    picked = eng.cmux_tree(tl, np.array([[n, n + 1]], np.int32), out_form=0)
    w = np.concatenate([ins, g])                                          # wires 0, 1, 2 and g = 3
    x = form_rows(w, [0, 2, 3, 4], [3, 2, 3, 0], [1, -2, 1, 3], [123, 0, 0])
    r = eng.blind_rotate(picked, x[0:1], in_form=0, out_form=2)[:, 0]
    r2 = eng.blind_rotate(tl[1:2], x[1:2], in_form=0, out_form=0)
    lw = eng.rot_net(np.concatenate([r2, picked]), edge, np.array([[n + 1]], np.int32), out_form=2)[:, 0]
    both = eng.blind_rotate(tl[3:4], x[2:3], sel=np.arange(1, n + 1, dtype=np.int32), in_form=0, n_out=2, out_form=2)[0]
    want = np.concatenate([eng.gates(np.array([3], np.uint8), r, lw), r, lw, both])
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(c.run(ck, ins, tlwe_inputs=tl).data, want)     # a second run on the reallocated tables
    ck.close()


@pytest.mark.gpu
def test_gpu_private_lookup_circuit_decrypts_at_full_size(tfhe, keys80):
    """The example's lookup over 16 requests at tfhe_parameters_80: the circuit's words are the host path's, and every answer and every
    parity bit decrypts (asserted inside lookup_both_ways)."""
    spec = importlib.util.spec_from_file_location("private_lut_circuit", os.path.join(ROOT, "examples", "private_lut_circuit.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    K = keys80
    ms_circ, ms_host = example.lookup_both_ways(np.random.default_rng(8181), K.sk, K.ck, 16)
    assert ms_circ > 0 and ms_host > 0
