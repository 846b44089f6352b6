"""blind_rotate_kernel_v3 with its integer stream trimmed (csrc/kernels_common.hpp: accumulate_poly_v3, a step's rounded words added
into the LDS image and its mirror by ds_add_u32 / ds_sub_u32 instead of read, added and stored), on the GPU.  What the rotation
of the next step reads of that image depends on its exponent (block, sign, offset inside the block, and through the offset the
lanes that read the mirror): a batch of 256 rows with lwe_size = 8 whose mask words mod-switch to 0 ... 2047, each once, walks all
of them in one launch.  Words against the oracle; the batches are forced onto the one-wave kernel and the kernel's name is asserted,
so a dispatcher that sends these sizes elsewhere fails the test instead of quietly testing another kernel."""
import numpy as np
import pytest

from test_pbs import pbs_ref  # noqa: F401  (fixture: the programmable-bootstrap checker)
from test_v3_tan2 import MU, ONE_WAVE, forced

pytestmark = pytest.mark.gpu

N = 1024
ROWS = 256          # x 8 mask words = the 2048 exponents


@pytest.fixture(scope="module", params=[(2, 10), (3, 7), (4, 7)], ids=["l2_80bit", "l3_128bit", "l4_run_time"])
def exponent_case(request, tfhe, orc):
    """lwe_size = 8 with the decomposition of the 80-bit set, of the 128-bit set, and l = 4 (the run-time-l instantiation); 257 rows
    (the first 256 carry every exponent once) and the oracle's words for them, computed once."""
    from conftest import KeySet
    l, beta = request.param
    K = KeySet(tfhe, orc, tfhe.SchemeParameters(8, 1 / 2**15, N, 1, l, beta, 9e-9, 8, 2, 1 / 2**15, 1), seed=1024 + l)
    rng = np.random.default_rng(100 + l)
    x = rng.integers(-2**31, 2**31, size=(ROWS + 1, 9), dtype=np.int64)
    x[:ROWS, :8] = (8 * np.arange(ROWS)[:, None] + np.arange(8)[None, :]) << 21
    x = (x & 0xFFFFFFFF).astype(np.uint32).view(np.int32)      # (the words from 2^31 up wrap to negative Int32)
    # the oracle's own mod-switch sends the mask words of the first 256 rows to 0 ... 2047, each once
    bara = [orc.decode_message(int(w), 2 * N) % (2 * N) for w in x[:ROWS, :8].ravel()]
    assert bara == list(range(2 * N))
    want = K.oracle.bootstrap(MU, x, with_keyswitch=False, nthreads=orc.max_threads())
    want.setflags(write=False)
    yield K, l, x, want
    K.ck.close()


@pytest.mark.parametrize("rw", [1, 4])
def test_every_exponent_equals_the_oracle(exponent_case, rw):
    """256 rows, and 257: at four rotations per workgroup a lockstep group with three padding waves."""
    K, l, x, want = exponent_case
    eng = K.ck.engine(0)
    tail = (",rw4" if rw == 4 else "") + ">"
    name = f"blind_rotate_kernel_v3<0,8,tw2reg{tail}(l={l})" if l == 4 else f"blind_rotate_kernel_v3<{l},8,tw2reg{tail}"
    with forced(eng, {**ONE_WAVE, "v3_rw": rw}):
        for R in (ROWS, ROWS + 1):
            got = eng.bootstrap(MU, x[:R], with_keyswitch=False)
            assert eng.last_kernel_name() == name, eng.last_kernel_name()
            assert eng.last_rotation_count() == R
            bad = np.flatnonzero((got != want[:R]).any(axis=1))
            assert bad.size == 0, (R, bad[:8])


def test_caller_supplied_test_polynomial(pbs_ref, keys80):  # noqa: F811
    """The TV form of the kernel, five rotations, against the checker."""
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(56)
    x = rng.integers(-2**31, 2**31, size=(5, K.params.lwe_size + 1), dtype=np.int64).astype(np.int32)
    tables = rng.integers(-2**31, 2**31, size=(3, N), dtype=np.int64).astype(np.int32)
    index = np.array([1, 2, 0, 2, 1], np.int32)
    with forced(eng, ONE_WAVE):
        got = eng.bootstrap_tv(tables, x, index=index, with_keyswitch=False)
        assert eng.last_kernel_name() == "blind_rotate_kernel_v3<2,8,tw2reg>+tv", eng.last_kernel_name()
    assert np.array_equal(got, pbs_ref(K, tables, index, x, False))


@pytest.fixture(scope="module")
def gates64(tfhe, orc, keys80):
    K = keys80
    rng = np.random.default_rng(64)
    bx, by = rng.integers(0, 2, 64).astype(bool), rng.integers(0, 2, 64).astype(bool)
    x, y = tfhe.encrypt(K.rng, K.sk, bx).data, tfhe.encrypt(K.rng, K.sk, by).data
    ops = np.zeros(64, np.uint8)
    want = K.oracle.gates(ops, x, y, nthreads=orc.max_threads())
    want.setflags(write=False)
    return K, ops, x, y, want


@pytest.mark.parametrize("rw", [1, 4])
def test_diag_form_computes_the_timed_kernels_words(gates64, rw):
    """The DIAG instantiations on 64 gates: the words of the timed kernel and of the oracle, a margin in (0, 0.25)."""
    K, ops, x, y, want = gates64
    eng = K.ck.engine(0)
    name = f"blind_rotate_kernel_v3<2,8,tw2reg{',rw4' if rw == 4 else ''}>"
    with forced(eng, {**ONE_WAVE, "v3_rw": rw}):
        timed = eng.gates(ops, x, y)
        assert eng.last_kernel_name() == name, eng.last_kernel_name()
    with forced(eng, {**ONE_WAVE, "v3_rw": rw, "measure_margin": 1}):
        diag = eng.gates(ops, x, y)
        assert eng.last_kernel_name() == name, eng.last_kernel_name()
        margin = eng.last_rounding_margin()
    print(f"rounding margin rw={rw}: {margin:.4f}")
    assert np.array_equal(timed, want)
    assert np.array_equal(diag, timed)
    assert 0.0 < margin < 0.25, margin
