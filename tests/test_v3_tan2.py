"""blind_rotate_kernel_v3 with its pass-B twiddles in tan form at the receiving lane (csrc/br_core.hpp: LaneTan2), on the GPU: every
instantiation the change touches — l = 2, l = 3 and run-time l, one and four rotations per workgroup, the TV form, DIAG — at the batch
sizes where this kernel can go wrong rather than at the workload's: one rotation, five (single-rotation workgroups), and 1537, the
first size above the 1536-rotation threshold that leaves a lockstep group of four with three padding waves.  Words against the
oracle; the small sizes are forced onto the one-wave kernel with the dispatcher's options and the kernel's name is asserted, so a
dispatcher that sends these sizes elsewhere fails the test instead of quietly testing another kernel."""
import ctypes as C

import numpy as np
import pytest

from test_pbs import pbs_ref  # noqa: F401  (fixture: the programmable-bootstrap checker)

pytestmark = pytest.mark.gpu

MU = 2**29
R_BIG = 1537
ONE_WAVE = {"br_tiny": -1, "br_small": -1}           # no 4 l-wave kernel, no two-wave kernel: blind_rotate_kernel_v3 at every size
DEFAULTS = {"br_tiny": -2, "br_small": 1024}


class forced:
    """`with forced(eng, options):` sets the options and puts the defaults back (the engines are shared by the session)."""

    def __init__(self, eng, opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.eng.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.eng.set_option(k, {**DEFAULTS, "v3_rw": 0, "measure_margin": 0}[k])


def _name(l, R, run_time_l=False):
    rw = ",rw4" if R >= 1536 else ""
    return f"blind_rotate_kernel_v3<0,8,tw2reg{rw}>(l={l})" if run_time_l else f"blind_rotate_kernel_v3<{l},8,tw2reg{rw}>"


@pytest.fixture(scope="module", params=["80", "128"])
def gate_case(request, tfhe, orc, keys80, keys128):
    """1537 NAND gates on a shipped set and the oracle's words for them, computed once; the smaller batches are its first rows."""
    K = keys80 if request.param == "80" else keys128
    rng = np.random.default_rng(int(request.param))
    bx, by = rng.integers(0, 2, R_BIG).astype(bool), rng.integers(0, 2, R_BIG).astype(bool)
    x, y = tfhe.encrypt(K.rng, K.sk, bx).data, tfhe.encrypt(K.rng, K.sk, by).data
    ops = np.zeros(R_BIG, np.uint8)
    want = K.oracle.gates(ops, x, y, nthreads=orc.max_threads())
    want.setflags(write=False)
    return K, K.ck.engine(0), ops, x, y, want


@pytest.mark.parametrize("R", [1, 5, R_BIG])
def test_gate_batches_on_device_pointers_equal_the_oracle(gate_case, R):
    K, eng, ops, x, y, want = gate_case
    hip = C.CDLL("libamdhip64.so")
    x, y = np.ascontiguousarray(x[:R]), np.ascontiguousarray(y[:R])
    bufs = []

    def dev(host):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(host.nbytes)) == 0
        bufs.append(p)
        assert hip.hipMemcpy(p, host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return p

    try:
        dx, dy, dout = dev(x), dev(y), dev(np.zeros_like(x))
        with forced(eng, ONE_WAVE):
            eng.gates_dev(ops[:R], dx.value, dy.value, 0, dout.value, R)
            eng.synchronize()
            assert eng.last_kernel_name() == _name(K.params.bs_decomp_length, R), eng.last_kernel_name()
            assert eng.last_rotation_count() == R
        got = np.empty_like(x)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), dout, C.c_size_t(got.nbytes), 2) == 0          # hipMemcpyDeviceToHost
    finally:
        for p in bufs:
            hip.hipFree(p)
    assert np.array_equal(got, want[:R])


def test_run_time_decomposition_length(tfhe, orc):
    """l = 4 belongs to no shipped set: blind_rotate_kernel_v3<0, ...> reads it at run time.  Five rotations and 1537."""
    from conftest import KeySet
    K = KeySet(tfhe, orc, tfhe.SchemeParameters(8, 1 / 2**15, 1024, 1, 4, 7, 9e-9, 8, 2, 1 / 2**15, 1), seed=1024 + 4)
    eng = K.ck.engine(0)
    rng = np.random.default_rng(4)
    x = rng.integers(-2**31, 2**31, size=(R_BIG, K.params.lwe_size + 1), dtype=np.int64).astype(np.int32)
    x[0, :] = 0
    want = K.oracle.bootstrap(MU, x, with_keyswitch=False, nthreads=orc.max_threads())
    try:
        with forced(eng, ONE_WAVE):
            for R in (5, R_BIG):
                got = eng.bootstrap(MU, x[:R], with_keyswitch=False)
                assert eng.last_kernel_name() == _name(4, R, run_time_l=True), eng.last_kernel_name()
                assert np.array_equal(got, want[:R]), R
    finally:
        K.ck.close()


def test_caller_supplied_test_polynomial(pbs_ref, keys80):  # noqa: F811
    """The TV form of the kernel (programmable bootstrapping), five rotations, against the checker, with and without keyswitch."""
    K = keys80
    eng = K.ck.engine(0)
    rng = np.random.default_rng(55)
    x = rng.integers(-2**31, 2**31, size=(5, K.params.lwe_size + 1), dtype=np.int64).astype(np.int32)
    tables = rng.integers(-2**31, 2**31, size=(3, 1024), dtype=np.int64).astype(np.int32)
    index = np.array([2, 0, 1, 1, 2], np.int32)
    with forced(eng, ONE_WAVE):
        for ks in (True, False):
            got = eng.bootstrap_tv(tables, x, index=index, with_keyswitch=ks)
            assert eng.last_kernel_name() == _name(2, 5) + "+tv", eng.last_kernel_name()
            assert np.array_equal(got, pbs_ref(K, tables, index, x, ks)), ks


@pytest.mark.parametrize("rw", [1, 4])
def test_rounding_margin_of_the_one_wave_kernel(gate_case, rw):
    """The DIAG instantiations run the timed kernel's arithmetic and report the largest distance of a pre-rounding value from an
    integer over 256 gates: the same words, and a margin below the 0.25 tests/test_gpu_parity.py asks of the engine."""
    K, eng, ops, x, y, want = gate_case
    B = 256
    with forced(eng, {**ONE_WAVE, "v3_rw": rw, "measure_margin": 1}):
        got = eng.gates(ops[:B], x[:B], y[:B])
        l = K.params.bs_decomp_length
        assert eng.last_kernel_name() == f"blind_rotate_kernel_v3<{l},8,tw2reg{',rw4' if rw == 4 else ''}>", eng.last_kernel_name()
        margin = eng.last_rounding_margin()
    print(f"rounding margin l={l} rw={rw}: {margin:.4f}")
    assert np.array_equal(got, want[:B])
    assert 0.0 < margin < 0.25, margin
