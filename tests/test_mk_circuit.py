"""Circuits under a multi-key cloud key (tfhe_mk_wires_alloc, tfhe_mk_gates_level): the tutorial's 16-bit encrypted minimum
(examples/tutorial.py, both forms) with two parties' inputs, level by level on the device-resident multi-key wire table,
checked word for word against a level-by-level replay through the multi-key gate helper of test_mk_gates."""
import os
import sys

import numpy as np
import pytest

from test_mk_gates import MKGateRef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tutorial():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import tutorial
    return tutorial


class MKCircuitKeys:
    """2-party mktfhe_parameters_2party at full size, fixed seed, and an oracle with the same keys."""

    def __init__(self, tfhe, orc, seed=2024):
        p = tfhe.mktfhe_parameters_2party
        self.rng = np.random.default_rng(seed)
        self.sks = [tfhe.SecretKey(self.rng, p) for _ in range(2)]
        shared = tfhe.SharedKey(self.rng, p)
        self.ck = tfhe.MKCloudKey([tfhe.CloudKeyPart(self.rng, sk, shared) for sk in self.sks])
        self.oracle = orc.Oracle(p.lwe_size, 1024, 1, p.bs_decomp_length, p.bs_log2_base, p.ks_decomp_length, p.ks_log2_base,
                                 parties=2)
        self.oracle.load_bootstrap_key(self.ck.bootstrap_key)
        self.oracle.load_keyswitch_key(self.ck.keyswitch_key)

    def inputs(self, tfhe, x, y, nbits=16, seed=0):
        """[2 nbits][P n + 1]: party 1's number, then party 2's, encrypted under the joint key with their own seed."""
        bits = lambda v: [(v >> i) & 1 == 1 for i in range(nbits)]
        return tfhe.mk_encrypt(np.random.default_rng(seed), self.sks, bits(x) + bits(y))


def replay(orc, o, circuit, inputs):
    """The circuit level by level through the helper: the words the engine must produce."""
    ref = MKGateRef(orc, o, threads=16)
    wires = np.zeros((circuit.num_wires, inputs.shape[1]), np.int32)
    wires[:inputs.shape[0]] = inputs
    for ops, a, b, c, out in circuit.level_arrays():
        wires[out] = ref.batch(ops, wires[a], wires[b], wires[c])
    return wires[circuit._outputs]


def _value(tfhe, sks, rows):
    return sum(int(bit) << i for i, bit in enumerate(tfhe.mk_decrypt(sks, rows)))


@pytest.fixture(scope="module")
def mkc(tfhe, orc):
    return MKCircuitKeys(tfhe, orc)


@pytest.mark.gpu
@pytest.mark.parametrize("log_depth", [False, True], ids=["ripple", "log_depth"])
def test_mk_tutorial_minimum(tfhe, orc, mkc, log_depth):
    circ = _tutorial().encrypted_minimum_circuit(16, log_depth=log_depth)
    inputs = mkc.inputs(tfhe, 2017, 42, seed=1)
    got = circ.run(mkc.ck, inputs)
    assert got.shape == (16, 2 * 500 + 1)
    assert np.array_equal(got, replay(orc, mkc.oracle, circ, inputs))
    # (decryption is noise-bound, ~0.2 %/gate and more for MUX; these keys and inputs are fixed, and the words above
    #  are the helper's, so the value is too)
    assert _value(tfhe, mkc.sks, got) == 42


@pytest.mark.gpu
def test_mk_tutorial_minimum_run_batch(tfhe, mkc):
    circ = _tutorial().encrypted_minimum_circuit(16)
    pairs = [(2017, 42), (5, 9), (65535, 0), (300, 300)]
    sets = np.stack([mkc.inputs(tfhe, x, y, seed=1 + i) for i, (x, y) in enumerate(pairs)])
    got = circ.run_batch(mkc.ck, sets)
    assert got.shape == (4, 16, 1001)
    for i in range(4):
        assert np.array_equal(got[i], circ.run(mkc.ck, sets[i]))
    assert _value(tfhe, mkc.sks, got[0]) == 42


@pytest.mark.gpu
def test_same_circuit_single_and_multi_key(tfhe, orc, mkc, keys80):
    """One Circuit object under a single-key and a multi-key cloud key, in turn."""
    circ = _tutorial().encrypted_minimum_circuit(4)
    K = keys80
    bits = lambda v: [(v >> i) & 1 == 1 for i in range(4)]
    single = circ.run(K.ck, tfhe.encrypt(K.rng, K.sk, bits(11) + bits(6)))
    assert sum(int(b) << i for i, b in enumerate(tfhe.decrypt(K.sk, single))) == 6
    mk_in = mkc.inputs(tfhe, 11, 6, nbits=4)
    got = circ.run(mkc.ck, mk_in)
    assert np.array_equal(got, replay(orc, mkc.oracle, circ, mk_in))
    again = circ.run(K.ck, tfhe.encrypt(K.rng, K.sk, bits(11) + bits(6)))
    assert sum(int(b) << i for i, b in enumerate(tfhe.decrypt(K.sk, again))) == 6
