"""ctypes binding of lib/libtfhe_mi355x.so (C ABI: include/tfhe_mi355x.h).

There is no CPU fallback: if the HIP library is missing or no device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFHE_MI355X_LIB", os.path.join(_PKG, "lib", "libtfhe_mi355x.so"))   # override: A/B builds

# symbols include/tfhe_mi355x.h declares (tests check that the .so exports every one of them)
ABI_SYMBOLS = [
    "tfhe_abi_version", "tfhe_device_count", "tfhe_ctx_create", "tfhe_ctx_destroy", "tfhe_last_error",
    "tfhe_ctx_params", "tfhe_load_bootstrap_key_i32", "tfhe_load_bootstrap_key_c128",
    "tfhe_load_keyswitch_key", "tfhe_gates_batch", "tfhe_gates_batch_dev", "tfhe_bootstrap_batch",
    "tfhe_keyswitch_batch", "tfhe_mk_load_bootstrap_key_i32", "tfhe_mk_load_keyswitch_key",
    "tfhe_mk_gate_nand_batch", "tfhe_last_timing_ms", "tfhe_last_rotation_count", "tfhe_set_option",
    "tfhe_last_rounding_margin", "tfhe_wires_alloc", "tfhe_wires_upload", "tfhe_wires_download", "tfhe_gates_level",
    "tfhe_ctx_create_multi", "tfhe_ctx_device_count", "tfhe_shard_bounds", "tfhe_wires_gather",
    "tfhe_last_kernel_name", "tfhe_last_kernel_clock_mhz", "tfhe_mk_load_bootstrap_key_c128",
    "tfhe_mk_expand_load_bootstrap_key", "tfhe_keygen_cloud_key", "tfhe_host_alloc", "tfhe_host_free",
    "tfhe_timing_history_ms", "tfhe_gates_batch_submit", "tfhe_gates_batch_wait", "tfhe_last_device_count",
    "tfhe_get_option", "tfhe_ctx_synchronize", "tfhe_mk_gates_batch", "tfhe_mk_wires_alloc", "tfhe_mk_gates_level",
    "tfhe_bootstrap_tv_batch", "tfhe_bootstrap_tv_multi_batch", "tfhe_lut_level", "tfhe_linear_level",
    "tfhe_mk_bootstrap_tv_batch", "tfhe_mk_bootstrap_tv_multi_batch", "tfhe_mk_lut_level", "tfhe_mk_linear_level",
    "tfhe_tgsw_load", "tfhe_extern_mul_batch", "tfhe_cmux_tree_batch", "tfhe_cmux_net_batch",
    "tfhe_mk_tgsw_load", "tfhe_mk_tgsw_expand_load", "tfhe_mk_extern_mul_batch", "tfhe_mk_cmux_tree_batch",
    "tfhe_mk_cmux_net_batch", "tfhe_rot_net_batch", "tfhe_mk_rot_net_batch", "tfhe_blind_rotate_batch",
    "tfhe_mk_blind_rotate_batch", "tfhe_tlwe_alloc", "tfhe_tlwe_upload", "tfhe_tlwe_download", "tfhe_tgsw_update",
    "tfhe_rot_net_level", "tfhe_blind_rotate_level", "tfhe_mk_tlwe_alloc", "tfhe_mk_tlwe_upload", "tfhe_mk_tlwe_download",
    "tfhe_mk_tgsw_update", "tfhe_mk_tgsw_expand_update", "tfhe_mk_rot_net_level", "tfhe_mk_blind_rotate_level",
    "tfhe_bootstrap_acc_batch", "tfhe_bootstrap_acc_level", "tfhe_mk_bootstrap_acc_batch", "tfhe_mk_bootstrap_acc_level",
]
ABI_VERSION = 7
ERR_NOMEM = 6

OPCODES = dict(NAND=0, OR=1, AND=2, XOR=3, XNOR=4, NOT=5, NOR=6, ANDNY=7, ANDYN=8, ORNY=9, ORYN=10,
               MUX=11, CONST0=12, CONST1=13, COPY=14)


class TfheParams(C.Structure):
    _fields_ = [(f, C.c_int32) for f in
                ("n", "N", "k", "bs_l", "bs_log2_base", "ks_t", "ks_log2_base", "parties")]


def pinned_empty(shape, dtype=np.int32):
    """A numpy array in page-locked host memory (tfhe_host_alloc): operands / results of the host-buffer batch calls held
    in such arrays cross PCIe as single DMA transfers instead of being staged through the runtime's bounce buffers.  The
    block is returned (tfhe_host_free) when the last view of the array is gone."""
    import weakref
    lib = load()
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dtype.itemsize, 1)
    p = C.c_void_p()
    rc = lib.tfhe_host_alloc(nbytes, C.byref(p))
    if rc:
        raise MemoryError(f"tfhe_host_alloc({nbytes}) failed: {lib.tfhe_last_error(None).decode()}")
    buf = (C.c_char * nbytes).from_address(p.value)
    weakref.finalize(buf, lib.tfhe_host_free, p.value)          # numpy holds `buf` for as long as any view lives
    return np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)


class EngineError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"tfhe_mi355x error {code}: {message}")
        self.code = code


_lib = None
_warned_inexact = set()


def _warn_inexact_once(params, margin, bound_log2):
    key = params.engine_tuple()
    if key in _warned_inexact:
        return
    _warned_inexact.add(key)
    import warnings
    warnings.warn(f"TFHE parameter set {key} (lwe_size, N, k, l, log2 Bg, t, log2 ks_base, parties) is outside the Float64 exactness "
                  f"domain: predicted rounding margin {margin:.2f} (a flipped rounding needs 0.5), worst-case magnitude 2^{bound_log2:.1f}. "
                  "The engine computes as the reference does, but result words may differ from the exact negacyclic product; "
                  "tfhe_last_rounding_margin measures the actual margin.", RuntimeWarning, stacklevel=3)


def load():
    """Loads the HIP library; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C tfhe.jl_amd/csrc` (hipcc, gfx950). The engine has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    lib.tfhe_abi_version.restype = i32
    lib.tfhe_device_count.restype = i32
    lib.tfhe_ctx_create.argtypes = [C.POINTER(TfheParams), i32, C.POINTER(vp)]
    lib.tfhe_ctx_destroy.argtypes = [vp]
    lib.tfhe_ctx_destroy.restype = None
    lib.tfhe_last_error.argtypes = [vp]
    lib.tfhe_last_error.restype = C.c_char_p
    lib.tfhe_ctx_params.argtypes = [vp, C.POINTER(TfheParams)]
    lib.tfhe_load_bootstrap_key_i32.argtypes = [vp, vp]
    lib.tfhe_load_bootstrap_key_c128.argtypes = [vp, vp]
    lib.tfhe_load_keyswitch_key.argtypes = [vp, vp]
    lib.tfhe_keygen_cloud_key.argtypes = [vp, vp, vp, C.c_double, C.c_double, vp, vp, vp]
    if hasattr(lib, "tfhe_host_alloc"):
        lib.tfhe_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
        lib.tfhe_host_free.argtypes = [vp]
        lib.tfhe_host_free.restype = None
    lib.tfhe_gates_batch.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    lib.tfhe_gates_batch_dev.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp]
    if hasattr(lib, "tfhe_gates_batch_submit"):
        lib.tfhe_gates_batch_submit.argtypes = [vp, vp, vp, vp, vp, vp, i64, C.POINTER(i32)]
        lib.tfhe_gates_batch_wait.argtypes = [vp, i32]
    lib.tfhe_bootstrap_batch.argtypes = [vp, i32, vp, vp, i64, i32]
    lib.tfhe_bootstrap_tv_batch.argtypes = [vp, vp, i32, vp, vp, vp, i64, i32]
    lib.tfhe_bootstrap_tv_multi_batch.argtypes = [vp, vp, i32, vp, i32, vp, vp, i64, i32]
    lib.tfhe_keyswitch_batch.argtypes = [vp, vp, vp, i64]
    lib.tfhe_mk_load_bootstrap_key_i32.argtypes = [vp, vp, i32]
    lib.tfhe_mk_load_keyswitch_key.argtypes = [vp, vp, i32]
    lib.tfhe_mk_load_bootstrap_key_c128.argtypes = [vp, vp, i32]
    lib.tfhe_mk_expand_load_bootstrap_key.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.tfhe_mk_gate_nand_batch.argtypes = [vp, vp, vp, vp, i64]
    if hasattr(lib, "tfhe_mk_gates_batch"):
        lib.tfhe_mk_gates_batch.argtypes = [vp, vp, vp, vp, vp, vp, i64]
        lib.tfhe_mk_wires_alloc.argtypes = [vp, i64]
        lib.tfhe_mk_gates_level.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    lib.tfhe_last_timing_ms.argtypes = [vp, i32, C.POINTER(C.c_float)]
    if hasattr(lib, "tfhe_timing_history_ms"):
        lib.tfhe_timing_history_ms.argtypes = [vp, i32, C.POINTER(C.c_float), i32, C.POINTER(i32)]
    lib.tfhe_last_rotation_count.argtypes = [vp]
    lib.tfhe_last_rotation_count.restype = i64
    lib.tfhe_last_device_count.argtypes = [vp]
    lib.tfhe_last_device_count.restype = i32
    lib.tfhe_set_option.argtypes = [vp, C.c_char_p, i64]
    lib.tfhe_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    lib.tfhe_last_rounding_margin.argtypes = [vp, C.POINTER(C.c_double)]
    lib.tfhe_wires_alloc.argtypes = [vp, i64]
    lib.tfhe_wires_upload.argtypes = [vp, i64, i64, vp]
    lib.tfhe_wires_download.argtypes = [vp, i64, i64, vp]
    lib.tfhe_gates_level.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    if hasattr(lib, "tfhe_lut_level"):
        lib.tfhe_lut_level.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i64]
        lib.tfhe_linear_level.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    if hasattr(lib, "tfhe_mk_bootstrap_tv_batch"):
        lib.tfhe_mk_bootstrap_tv_batch.argtypes = [vp, vp, i32, vp, vp, vp, i64, i32]
        lib.tfhe_mk_bootstrap_tv_multi_batch.argtypes = [vp, vp, i32, vp, i32, vp, vp, i64, i32]
        lib.tfhe_mk_lut_level.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i64]
        lib.tfhe_mk_linear_level.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    if hasattr(lib, "tfhe_tgsw_load"):
        lib.tfhe_tgsw_load.argtypes = [vp, vp, i64]
        lib.tfhe_extern_mul_batch.argtypes = [vp, vp, vp, vp, i64]
        lib.tfhe_cmux_tree_batch.argtypes = [vp, vp, i64, vp, i32, vp, vp, i64, i32]
    if hasattr(lib, "tfhe_cmux_net_batch"):
        lib.tfhe_cmux_net_batch.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, i32, vp, i64, i32]
    if hasattr(lib, "tfhe_mk_tgsw_load"):
        lib.tfhe_mk_tgsw_load.argtypes = [vp, vp, vp, i64, i32]
        lib.tfhe_mk_tgsw_expand_load.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]
        lib.tfhe_mk_extern_mul_batch.argtypes = [vp, vp, vp, vp, i64]
        lib.tfhe_mk_cmux_tree_batch.argtypes = [vp, vp, i64, vp, i32, vp, vp, i64, i32]
    if hasattr(lib, "tfhe_mk_cmux_net_batch"):
        lib.tfhe_mk_cmux_net_batch.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, i32, vp, i64, i32]
    if hasattr(lib, "tfhe_rot_net_batch"):
        lib.tfhe_rot_net_batch.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, i32, vp, i64, i32]
    if hasattr(lib, "tfhe_mk_rot_net_batch"):
        lib.tfhe_mk_rot_net_batch.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, vp, i32, vp, i64, i32]
    if hasattr(lib, "tfhe_blind_rotate_batch"):
        lib.tfhe_blind_rotate_batch.argtypes = [vp, vp, i64, vp, vp, i32, i32, vp, i32, vp, i64, i32]
    if hasattr(lib, "tfhe_mk_blind_rotate_batch"):
        lib.tfhe_mk_blind_rotate_batch.argtypes = [vp, vp, i64, vp, vp, i32, i32, vp, i32, vp, i64, i32]
    if hasattr(lib, "tfhe_tlwe_alloc"):
        lib.tfhe_tlwe_alloc.argtypes = [vp, i64]
        lib.tfhe_tlwe_upload.argtypes = [vp, i64, i64, vp]
        lib.tfhe_tlwe_download.argtypes = [vp, i64, i64, vp]
        lib.tfhe_tgsw_update.argtypes = [vp, vp, i64, i64]
        lib.tfhe_rot_net_level.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, i32, i64, vp, i64]
        lib.tfhe_blind_rotate_level.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i64]
    if hasattr(lib, "tfhe_mk_tlwe_alloc"):
        lib.tfhe_mk_tlwe_alloc.argtypes = [vp, i64]
        lib.tfhe_mk_tlwe_upload.argtypes = [vp, i64, i64, vp]
        lib.tfhe_mk_tlwe_download.argtypes = [vp, i64, i64, vp]
        lib.tfhe_mk_tgsw_update.argtypes = [vp, vp, vp, i64, i64, i32]
        lib.tfhe_mk_tgsw_expand_update.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp]
        lib.tfhe_mk_rot_net_level.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, i32, i64, vp, i64]
        lib.tfhe_mk_blind_rotate_level.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i64]
    if hasattr(lib, "tfhe_bootstrap_acc_batch"):
        lib.tfhe_bootstrap_acc_batch.argtypes = [vp, vp, i64, vp, vp, i32, i32, vp, i64]
        lib.tfhe_bootstrap_acc_level.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i64]
    if hasattr(lib, "tfhe_mk_bootstrap_acc_batch"):
        lib.tfhe_mk_bootstrap_acc_batch.argtypes = [vp, vp, i64, vp, vp, i32, i32, vp, i64]
        lib.tfhe_mk_bootstrap_acc_level.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, i64]
    lib.tfhe_ctx_create_multi.argtypes = [C.POINTER(TfheParams), vp, i32, C.POINTER(vp)]
    lib.tfhe_ctx_device_count.argtypes = [vp]
    lib.tfhe_ctx_device_count.restype = i32
    lib.tfhe_shard_bounds.argtypes = [vp, i64, i32, vp]
    lib.tfhe_wires_gather.argtypes = [vp, vp, i64, vp]
    lib.tfhe_last_kernel_name.argtypes = [vp]
    lib.tfhe_last_kernel_name.restype = C.c_char_p
    lib.tfhe_last_kernel_clock_mhz.argtypes = [vp, C.POINTER(C.c_double)]
    if hasattr(lib, "tfhe_ctx_synchronize"):
        lib.tfhe_ctx_synchronize.argtypes = [vp]
    ver = lib.tfhe_abi_version()
    if ver < 0 and not os.environ.get("TFHE_MI355X_ALLOW_EXPERIMENT"):
        # a development build (-DTFHE_EXPERIMENT: in-kernel stamps, environment-variable overrides; csrc/experiment.hpp)
        raise ImportError(f"{LIB_PATH} is a development build (ABI version {ver}): set TFHE_MI355X_ALLOW_EXPERIMENT=1 to load it knowingly")
    if abs(ver) != ABI_VERSION and not os.environ.get("TFHE_MI355X_ALLOW_ABI_MISMATCH"):     # (the override is for A/B runs against an older build)
        raise ImportError(f"{LIB_PATH} has ABI version {ver}, this package needs {ABI_VERSION}: rebuild it")
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i32c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def shard_bounds(opcodes, shards):
    """The library's own sharding rule (tfhe_shard_bounds): list of (start, end) per shard."""
    ops = None if opcodes is None else np.ascontiguousarray(opcodes, dtype=np.uint8)
    B = 0 if ops is None else ops.size
    out = np.zeros(int(shards) + 1, np.int64)
    rc = load().tfhe_shard_bounds(_ptr(ops), B, int(shards), _ptr(out))
    if rc != 0:
        raise EngineError(rc, "tfhe_shard_bounds: invalid argument")
    return [(int(out[r]), int(out[r + 1])) for r in range(int(shards))]


class Engine:
    """One context (tfhe_ctx): keys resident on one GPU — or, with `devices=[...]`, replicated on several, every
    host-buffer batch call fanned out over them inside the library (tfhe_ctx_create_multi)."""

    def __init__(self, params, device=0, devices=None):
        self._lib = load()
        self.params = params
        n, N, k, l, b, t, g, parties = params.engine_tuple()
        self.n, self.N, self.k, self.parties = n, N, k, parties
        p = TfheParams(n, N, k, l, b, t, g, parties)
        h = C.c_void_p()
        if devices is None:
            rc = self._lib.tfhe_ctx_create(C.byref(p), int(device), C.byref(h))
            self.devices = [int(device)]
        else:
            ids = np.ascontiguousarray(devices, dtype=np.int32)
            rc = self._lib.tfhe_ctx_create_multi(C.byref(p), _ptr(ids), ids.size, C.byref(h))
            self.devices = [int(v) for v in ids]
        if rc != 0:
            raise EngineError(rc, self._lib.tfhe_last_error(None).decode())
        self._h = h
        self._in_flight = {}
        self._wire_width = n + 1          # row width of the wire table (multi-key table: P n + 1, mk_wires_alloc)
        self.device = self.devices[0]
        # is this parameter set inside what a Float64 transform computes exactly?  (decided by tfhe_ctx_create from the parameters
        # alone; the reference warns about the same thing, polynomials.jl:135-144)
        self.exact_domain = self.get_option("exact_domain")
        if self.exact_domain == 0:
            _warn_inexact_once(params, self.get_option("exact_margin_x1e6") / 1e6, self.get_option("exact_bound_log2_x1000") / 1e3)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tfhe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(rc, self._lib.tfhe_last_error(self._h).decode())

    # ---- keys ----
    def load_bootstrap_key(self, bk_i32):
        bk = _i32c(bk_i32)
        l = self.params.bs_decomp_length
        want = self.n * l * (self.k + 1) ** 2 * self.N
        if bk.size != want:
            raise ValueError(f"bootstrap key has {bk.size} words, expected {want}")
        self._check(self._lib.tfhe_load_bootstrap_key_i32(self._h, _ptr(bk)))

    def load_bootstrap_key_spectra(self, spectra):
        s = np.ascontiguousarray(spectra, dtype=np.complex128)
        l = self.params.bs_decomp_length
        want = self.n * l * (self.k + 1) ** 2 * (self.N // 2)
        if s.size != want:
            raise ValueError(f"bootstrap key spectra have {s.size} values, expected {want}")
        self._check(self._lib.tfhe_load_bootstrap_key_c128(self._h, _ptr(s)))

    def load_keyswitch_key(self, ks):
        ks = _i32c(ks)
        p = self.params
        want = self.k * self.N * p.ks_decomp_length * ((1 << p.ks_log2_base) - 1) * (self.n + 1)
        if ks.size != want:
            raise ValueError(f"keyswitch key has {ks.size} words, expected {want}")
        self._check(self._lib.tfhe_load_keyswitch_key(self._h, _ptr(ks)))

    def keygen_cloud_key(self, lwe_key, tlwe_key, bs_noise_stddev, ks_noise_stddev, seed, want_arrays=True):
        """Generates bootstrap + keyswitch key on the device and loads them (tfhe_keygen_cloud_key).  `seed`: six 32-bit
        words; words 0-1 key the (public) mask streams, words 2-5 are the 128-bit noise key and AS SECRET AS THE SECRET KEY.
        Returns the canonical Int32 arrays (bk [n][l][k+1][k+1][N], ks [kN][t][base-1][n+1]) unless want_arrays is False."""
        lwe_key, tlwe_key = _i32c(lwe_key), _i32c(tlwe_key)
        seed = np.ascontiguousarray(seed, dtype=np.uint32).reshape(-1)
        if seed.size != 6:
            raise ValueError("keygen_cloud_key: seed must be six 32-bit words (2 for the masks, 4 secret ones for the noise)")
        p = self.params
        if lwe_key.size != self.n or tlwe_key.size != self.k * self.N:
            raise ValueError(f"secret keys have {lwe_key.size} / {tlwe_key.size} words, expected {self.n} / {self.k * self.N}")
        bk = ks = None
        if want_arrays:
            bk = np.empty((self.n, p.bs_decomp_length, self.k + 1, self.k + 1, self.N), np.int32)
            ks = np.empty((self.k * self.N, p.ks_decomp_length, (1 << p.ks_log2_base) - 1, self.n + 1), np.int32)
        self._check(self._lib.tfhe_keygen_cloud_key(self._h, _ptr(lwe_key), _ptr(tlwe_key), float(bs_noise_stddev),
                                                    float(ks_noise_stddev), _ptr(seed), _ptr(bk), _ptr(ks)))
        return bk, ks

    # ---- hot path, host buffers ----
    def gates(self, opcodes, in0, in1=None, in2=None, out=None):
        """`out`: an int32 [B][n+1] array to receive the result (e.g. one from pinned_empty, reused across calls);
        a fresh array otherwise."""
        ops = np.ascontiguousarray(opcodes, dtype=np.uint8)
        B = ops.size
        in0, in1, in2 = _i32c(in0), _i32c(in1), _i32c(in2)
        for a in (in0, in1, in2):
            if a is not None and a.shape != (B, self.n + 1):
                raise ValueError(f"operand shape {a.shape}, expected {(B, self.n + 1)}")
        if out is None:
            out = np.empty((B, self.n + 1), np.int32)
        elif out.dtype != np.int32 or out.shape != (B, self.n + 1) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous int32 array of shape {(B, self.n + 1)}")
        self._check(self._lib.tfhe_gates_batch(self._h, _ptr(ops), _ptr(in0), _ptr(in1), _ptr(in2), _ptr(out), B))
        return out

    def gates_submit(self, opcodes, in0, in1=None, in2=None, out=None):
        """Streaming form of gates(): enqueues the batch and returns (ticket, out) at once; `out` is complete after
        gates_wait(ticket).  Two batches may be in flight (the upload of one under the kernels of the other); operands
        and `out` should come from pinned_empty and must not be touched until the wait.  Arrays passed here are kept
        alive until then; an operand that is not already a C-contiguous int32 array is copied first."""
        ops = np.ascontiguousarray(opcodes, dtype=np.uint8)
        B = ops.size
        in0, in1, in2 = _i32c(in0), _i32c(in1), _i32c(in2)
        for a in (in0, in1, in2):
            if a is not None and a.shape != (B, self.n + 1):
                raise ValueError(f"operand shape {a.shape}, expected {(B, self.n + 1)}")
        if out is None:
            out = pinned_empty((B, self.n + 1))
        elif out.dtype != np.int32 or out.shape != (B, self.n + 1) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous int32 array of shape {(B, self.n + 1)}")
        ticket = C.c_int32(-1)
        self._check(self._lib.tfhe_gates_batch_submit(self._h, _ptr(ops), _ptr(in0), _ptr(in1), _ptr(in2), _ptr(out), B, C.byref(ticket)))
        if ticket.value in (0, 1):
            self._in_flight[ticket.value] = (in0, in1, in2, out)      # a displaced batch has been waited for by the library
        return ticket.value, out

    def gates_wait(self, ticket):
        self._check(self._lib.tfhe_gates_batch_wait(self._h, int(ticket)))
        self._in_flight.pop(int(ticket), None)

    def synchronize(self):
        """Blocks until everything queued on the context has completed (tfhe_ctx_synchronize): callable from any thread, also
        while another thread is inside a call on this engine."""
        rc = self._lib.tfhe_ctx_synchronize(self._h)
        if rc != 0:
            raise EngineError(rc, "tfhe_ctx_synchronize failed")

    def gates_dev(self, opcodes, d_in0, d_in1, d_in2, d_out, B, stream=0):
        """Device-pointer variant: operands are integer device addresses (e.g. torch tensor .data_ptr())."""
        ops = np.ascontiguousarray(opcodes, dtype=np.uint8)
        assert ops.size == B
        self._check(self._lib.tfhe_gates_batch_dev(self._h, _ptr(ops), d_in0 or None, d_in1 or None,
                                                   d_in2 or None, d_out, B, stream or None))

    def bootstrap(self, mu, x, with_keyswitch=True):
        x = _i32c(x)
        if x.ndim != 2 or x.shape[1] != self.n + 1:
            raise ValueError(f"bootstrap input must be [B][{self.n + 1}], got {x.shape}")
        B = x.shape[0]
        width = self.n + 1 if with_keyswitch else self.k * self.N + 1
        out = np.empty((B, width), np.int32)
        self._check(self._lib.tfhe_bootstrap_batch(self._h, int(mu), _ptr(x), _ptr(out), B, 1 if with_keyswitch else 0))
        return out

    def _tv_args(self, what, tables, x, index, words=None):
        x = _i32c(x)
        words = self.n + 1 if words is None else words
        if x.ndim != 2 or x.shape[1] != words:
            raise ValueError(f"{what} input must be [B][{words}], got {x.shape}")
        tables = _i32c(np.atleast_2d(tables))
        if tables.ndim != 2 or tables.shape[1] != self.N:
            raise ValueError(f"test polynomials must be [n_tv][{self.N}], got {tables.shape}")
        B = x.shape[0]
        idx = None
        if index is not None:
            idx = _i32c(index)
            if idx.shape != (B,):
                raise ValueError(f"index must have one entry per row ({B}), got {idx.shape}")
        return tables, x, idx

    def bootstrap_tv(self, tables, x, index=None, with_keyswitch=True):
        """Programmable bootstrapping (tfhe_bootstrap_tv_batch): `bootstrap` with row g's test polynomial tables[index[g]]
        (int32 [n_tv][N]; index None: table 0 for every row) instead of (mu, ..., mu).  Row g's result has the body
        v[phi] for phi in [0, N) and -v[phi - N] for phi in [N, 2N), phi = the row's modulus-switched phase (lut.py)."""
        tables, x, idx = self._tv_args("bootstrap_tv", tables, x, index)
        B = x.shape[0]
        width = self.n + 1 if with_keyswitch else self.k * self.N + 1
        out = np.empty((B, width), np.int32)
        self._check(self._lib.tfhe_bootstrap_tv_batch(self._h, _ptr(tables), tables.shape[0], _ptr(idx) if idx is not None else None,
                                                      _ptr(x), _ptr(out), B, 1 if with_keyswitch else 0))
        return out

    def bootstrap_tv_multi(self, tables, x, n_out, index=None, with_keyswitch=True):
        """Multi-output programmable bootstrapping (tfhe_bootstrap_tv_multi_batch): `bootstrap_tv` returning n_out samples per
        row from one blind rotation, int32 [B][n_out][width].  Sample j is extracted at the accumulator's coefficient j N / n_out:
        its body is v[phi + j N / n_out] where that index is below N (lut.py: make_multi_test_vector).  n_out: a power of two,
        1 <= n_out <= 32, and 1 or <= N / 4 (the library returns TFHE_ERR_INVALID_ARG otherwise)."""
        tables, x, idx = self._tv_args("bootstrap_tv_multi", tables, x, index)
        B, n_out = x.shape[0], int(n_out)
        width = self.n + 1 if with_keyswitch else self.k * self.N + 1
        out = np.empty((B, n_out if 1 <= n_out <= 32 else 0, width), np.int32)      # (an n_out the library refuses: nothing written)
        self._check(self._lib.tfhe_bootstrap_tv_multi_batch(self._h, _ptr(tables), tables.shape[0], _ptr(idx) if idx is not None else None,
                                                            n_out, _ptr(x), _ptr(out), B, 1 if with_keyswitch else 0))
        return out

    def _mk_width(self, what):
        P = getattr(self, "_mk_parties", None)
        if P is None:
            raise EngineError(3, f"{what}: multi-key keys not loaded")
        return P

    def mk_bootstrap_tv(self, tables, x, index=None, with_keyswitch=True):
        """Multi-key programmable bootstrapping (tfhe_mk_bootstrap_tv_batch): `bootstrap_tv` on multi-key samples int32 [B][P*n+1];
        the result is [B][P*n+1], or [B][P*N+1] without keyswitch."""
        return self.mk_bootstrap_tv_multi(tables, x, 1, index, with_keyswitch)[:, 0]

    def mk_bootstrap_tv_multi(self, tables, x, n_out, index=None, with_keyswitch=True):
        """Multi-key multi-output programmable bootstrapping (tfhe_mk_bootstrap_tv_multi_batch): `bootstrap_tv_multi` on multi-key
        samples, int32 [B][n_out][P*n+1] (or [B][n_out][P*N+1] without keyswitch)."""
        P = self._mk_width("mk_bootstrap_tv")
        tables, x, idx = self._tv_args("mk_bootstrap_tv", tables, x, index, P * self.n + 1)
        B, n_out = x.shape[0], int(n_out)
        width = P * self.n + 1 if with_keyswitch else P * self.N + 1
        out = np.empty((B, n_out if 1 <= n_out <= 32 else 0, width), np.int32)      # (an n_out the library refuses: nothing written)
        fn = self._lib.tfhe_mk_bootstrap_tv_multi_batch
        self._check(fn(self._h, _ptr(tables), tables.shape[0], _ptr(idx) if idx is not None else None, n_out, _ptr(x), _ptr(out), B,
                       1 if with_keyswitch else 0))
        return out

    def keyswitch(self, x):
        x = _i32c(x)
        B = x.shape[0]
        if x.ndim != 2 or x.shape[1] != self.k * self.N + 1:
            raise ValueError("keyswitch input must be [B][k*N+1]")
        out = np.empty((B, self.n + 1), np.int32)
        self._check(self._lib.tfhe_keyswitch_batch(self._h, _ptr(x), _ptr(out), B))
        return out

    # ---- leveled mode: external products and CMUX trees on the caller's own TGSW / TLWE samples ----
    def tgsw_load(self, tgsw):
        """The selector set of extern_mul / cmux_tree (tfhe_tgsw_load): int32 [S][l][k+1][k+1][N], S TGSW samples in the bootstrap
        key's canonical layout (leveled.tgsw_encrypt_bits makes them).  Replaces any earlier set."""
        t = _i32c(tgsw)
        per = self.params.bs_decomp_length * (self.k + 1) ** 2 * self.N
        if t.size == 0 or t.size % per:
            raise ValueError(f"TGSW samples have {t.size} words, expected a positive multiple of {per}")
        self._check(self._lib.tfhe_tgsw_load(self._h, _ptr(t), t.size // per))

    def extern_mul(self, tlwe, sel):
        """out[g] = selector[sel[g]] (.) tlwe[g] (tfhe_extern_mul_batch; tgsw_extern_mul, tgsw.jl:125-129): int32 [B][k+1][N]."""
        x = _i32c(tlwe)
        if x.ndim != 3 or x.shape[1:] != (self.k + 1, self.N):
            raise ValueError(f"TLWE samples must be [B][{self.k + 1}][{self.N}], got {x.shape}")
        B = x.shape[0]
        idx = _i32c(sel).reshape(-1)
        if idx.size != B:
            raise ValueError(f"sel must have one entry per row ({B}), got {idx.size}")
        out = np.empty_like(x)
        self._check(self._lib.tfhe_extern_mul_batch(self._h, _ptr(x), _ptr(idx), _ptr(out), B))
        return out

    def cmux_tree(self, data, sel, table_index=None, out_form=2):
        """CMUX-tree lookup (tfhe_cmux_tree_batch).  data: int32 [T][2^depth][k+1][N] tables of TLWE samples; sel: int32 [B][depth]
        indices into the loaded selector set, level 0 = the lowest address bit; table_index: [B] or None (table 0).  Row g's
        result is entry sum_v bit_v 2^v of its table, as a TLWE sample [k+1][N] (out_form 0), extracted at coefficient 0 [k*N+1]
        (1) or keyswitched to an LWE sample under the gate key [n+1] (2)."""
        d = _i32c(data)
        if d.ndim == 3:
            d = d[None]
        sel = _i32c(np.atleast_2d(sel))
        B, depth = sel.shape
        if d.ndim != 4 or d.shape[1:] != (1 << min(max(depth, 0), 30), self.k + 1, self.N):
            raise ValueError(f"tables must be [T][2^{depth}][{self.k + 1}][{self.N}], got {d.shape}")
        idx = None
        if table_index is not None:
            idx = _i32c(table_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"table_index must have one entry per row ({B}), got {idx.size}")
        shape = {0: (B, self.k + 1, self.N), 1: (B, self.k * self.N + 1), 2: (B, self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form the library refuses: nothing written)
        self._check(self._lib.tfhe_cmux_tree_batch(self._h, _ptr(d), d.shape[0], _ptr(idx), depth, _ptr(sel), _ptr(out), B, int(out_form)))
        return out

    def _net_args(self, data, net, sel, table_index, polys):
        """The shape checks cmux_net and mk_cmux_net share: tables [T][E][polys][N] (or one table [E][polys][N]), sel [B][V]."""
        d = _i32c(data)
        if d.ndim == 3:
            d = d[None]
        if d.ndim != 4 or d.shape[0] < 1 or d.shape[1] < 1 or d.shape[2:] != (polys, self.N):
            raise ValueError(f"tables must be [T][E][{polys}][{self.N}], got {d.shape}")
        if d.shape[1] < net.entries:
            raise ValueError(f"the network reads table entry {net.entries - 1}, the tables have {d.shape[1]}")
        sel = _i32c(np.atleast_2d(sel))
        B, V = sel.shape
        if V < net.variables:
            raise ValueError(f"the network reads variable {net.variables - 1}, sel has {V} per row")
        idx = None
        if table_index is not None:
            idx = _i32c(table_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"table_index must have one entry per row ({B}), got {idx.size}")
        return d, sel, idx

    def cmux_net(self, data, net, sel, table_index=None, out_form=2):
        """CMUX network (tfhe_cmux_net_batch).  data: int32 [T][E][k+1][N] tables of TLWE samples (or [E][k+1][N]: one table); net: a
        leveled.CmuxNet, the public wiring shared by all rows; sel: int32 [B][V] indices into the loaded selector set, one per variable
        of the network; table_index: [B] or None (table 0).  Row g's result is the F outputs of the last level: TLWE samples
        [B][F][k+1][N] (out_form 0), extracted at coefficient 0 [B][F][k*N+1] (1) or keyswitched under the gate key [B][F][n+1] (2)."""
        d, sel, idx = self._net_args(data, net, sel, table_index, self.k + 1)
        B, V = sel.shape
        F = int(net.widths[-1])
        shape = {0: (B, F, self.k + 1, self.N), 1: (B, F, self.k * self.N + 1), 2: (B, F, self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form the library refuses: nothing written)
        self._check(self._lib.tfhe_cmux_net_batch(self._h, _ptr(d), d.shape[0], d.shape[1], _ptr(idx), _ptr(net.widths), net.levels, _ptr(net.nodes),
                                                  _ptr(sel), V, _ptr(out), B, int(out_form)))
        return out

    def rot_net(self, data, net, sel, table_index=None, out_form=2):
        """CMUX network with monomial edges (tfhe_rot_net_batch): cmux_net with net a leveled.RotNet, whose records carry a public
        rotation X^rot for each source; shapes and out_forms as cmux_net (extraction at coefficient 0: a packed lookup rotates the
        wanted coefficient there)."""
        if getattr(net, "degree", None) != self.N:
            raise ValueError(f"the network's rotations are taken mod 2 * {getattr(net, 'degree', None)}, the engine's polynomials have {self.N} coefficients")
        d, sel, idx = self._net_args(data, net, sel, table_index, self.k + 1)
        B, V = sel.shape
        F = int(net.widths[-1])
        shape = {0: (B, F, self.k + 1, self.N), 1: (B, F, self.k * self.N + 1), 2: (B, F, self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form the library refuses: nothing written)
        self._check(self._lib.tfhe_rot_net_batch(self._h, _ptr(d), d.shape[0], d.shape[1], _ptr(idx), _ptr(net.widths), net.levels, _ptr(net.nodes),
                                                 _ptr(sel), V, _ptr(out), B, int(out_form)))
        return out

    def blind_rotate(self, acc, rows, sel=None, acc_index=None, in_form=0, n_out=1, out_form=2):
        """Blind rotation of the caller's TLWE accumulators (tfhe_blind_rotate_batch).  acc: int32 [T][k+1][N] TLWE samples, trivial or
        encrypted (or [k+1][N]: one accumulator); rows: int32 [B][steps+1], mask words then body — LWE samples (in_form 0) or exponents
        in [0, 2N) (in_form 1); sel: int32 [steps] indices into the loaded selector set, shared by all rows, or None (selector i for step
        i); acc_index: [B] or None (accumulator 0).  Row g's result is X^(-barb) acc rotated by the steps' exponents under the
        selectors: the TLWE sample [B][k+1][N] (out_form 0, n_out 1), its extractions at the coefficients j N / n_out
        [B][n_out][k*N+1] (1), or those keyswitched under the gate key [B][n_out][n+1] (2)."""
        a = _i32c(acc)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (self.k + 1, self.N):
            raise ValueError(f"accumulators must be [T][{self.k + 1}][{self.N}], got {a.shape}")
        r = _i32c(rows)
        if r.ndim != 2 or r.shape[1] < 2:
            raise ValueError(f"rows must be [B][steps+1] with at least one step, got {r.shape}")
        B, steps = r.shape[0], r.shape[1] - 1
        s = None
        if sel is not None:
            s = _i32c(sel).reshape(-1)
            if s.size != steps:
                raise ValueError(f"sel must have one entry per step ({steps}), got {s.size}")
        idx = None
        if acc_index is not None:
            idx = _i32c(acc_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"acc_index must have one entry per row ({B}), got {idx.size}")
        n_out = int(n_out)
        K = n_out if 1 <= n_out <= 32 else 0
        shape = {0: (B, self.k + 1, self.N), 1: (B, K, self.k * self.N + 1), 2: (B, K, self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form or n_out the library refuses: nothing written)
        self._check(self._lib.tfhe_blind_rotate_batch(self._h, _ptr(a), a.shape[0], _ptr(idx), _ptr(r), steps, int(in_form), _ptr(s), n_out, _ptr(out), B,
                                                      int(out_form)))
        return out

    def bootstrap_acc(self, acc, rows, acc_index=None, n_out=1, out_form=2):
        """blind_rotate on the gates' own kernel and key (tfhe_bootstrap_acc_batch): rows are LWE samples int32 [B][n+1], the steps are
        the context's n under the loaded bootstrapping key, no selector set is read.  acc, acc_index, n_out, out_form and the result
        are blind_rotate's, and so are the words where the selector set holds the key's n entries in order.  Served where
        get_option("bootstrap_acc") is 1 (N = 1024, k = 1).
        set_option("acc_dispatch", 1) (default 0: blind_rotate_kernel_v3_acc, one wave per row, at every B) lets the call choose its
        kernel by B as a gate batch does, under the same options (br_tiny, br_small, br_rt_l, w2_rw, v3_rw, br_split): the 4 l-wave
        kernel's ACC form up to one row per compute unit, the two-wave kernel's up to four, the one-wave form above, and a second launch
        for the last round of a batch above eight.  The words are the same; last_kernel_name() tells which ran."""
        a = _i32c(acc)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (self.k + 1, self.N):
            raise ValueError(f"accumulators must be [T][{self.k + 1}][{self.N}], got {a.shape}")
        r = _i32c(rows)
        if r.ndim != 2 or r.shape[1] != self.n + 1:
            raise ValueError(f"rows must be LWE samples [B][{self.n + 1}], got {r.shape}")
        B = r.shape[0]
        idx = None
        if acc_index is not None:
            idx = _i32c(acc_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"acc_index must have one entry per row ({B}), got {idx.size}")
        n_out = int(n_out)
        K = n_out if 1 <= n_out <= 32 else 0
        shape = {0: (B, self.k + 1, self.N), 1: (B, K, self.k * self.N + 1), 2: (B, K, self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form or n_out the library refuses: nothing written)
        self._check(self._lib.tfhe_bootstrap_acc_batch(self._h, _ptr(a), a.shape[0], _ptr(idx), _ptr(r), n_out, int(out_form), _ptr(out), B))
        return out

    # ---- leveled mode on device-resident tables: the TLWE table beside the wire table, levels that read and write both ----
    def tlwe_alloc(self, slots):
        """A device table of TLWE samples int32 [slots][k+1][N] (tfhe_tlwe_alloc); 0 frees it, reallocating discards the contents."""
        self._check(self._lib.tfhe_tlwe_alloc(self._h, int(slots)))

    def tlwe_upload(self, first, samples):
        """samples int32 [count][k+1][N] into slots [first, first + count) (tfhe_tlwe_upload), behind the levels queued so far."""
        m = _i32c(samples)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[1:] != (self.k + 1, self.N):
            raise ValueError(f"TLWE samples must be [count][{self.k + 1}][{self.N}], got {m.shape}")
        self._check(self._lib.tfhe_tlwe_upload(self._h, int(first), m.shape[0], _ptr(m)))

    def tlwe_download(self, first, count):
        """Slots [first, first + count) as int32 [count][k+1][N] (tfhe_tlwe_download), behind the levels queued so far."""
        out = np.empty((max(int(count), 0), self.k + 1, self.N), np.int32)
        self._check(self._lib.tfhe_tlwe_download(self._h, int(first), int(count), _ptr(out)))
        return out

    def tgsw_update(self, first, tgsw):
        """Replaces selectors [first, first + count) of the loaded set in place (tfhe_tgsw_update): tgsw int32 [count][l][k+1][k+1][N];
        every other selector keeps its words."""
        t = _i32c(tgsw)
        per = self.params.bs_decomp_length * (self.k + 1) ** 2 * self.N
        if t.size == 0 or t.size % per:
            raise ValueError(f"TGSW samples have {t.size} words, expected a positive multiple of {per}")
        self._check(self._lib.tfhe_tgsw_update(self._h, _ptr(t), int(first), t.size // per))

    def rot_net_level(self, net, sel, table_first=None, out_form=2, out_first=0, out_wires=None):
        """rot_net between the tables (tfhe_rot_net_level).  net: a leveled.RotNet, or a leveled.CmuxNet (its rotation-0 case);
        sel: int32 [B][V]; level 0 of row g reads source src at TLWE slot table_first[g] + src (None: absolute slots).  out_form 0:
        output node i of row g goes to slot out_first + g F + i; out_form 2: keyswitched, to wire out_wires[g F + i].  Synchronous."""
        self._rot_net_level(self._lib.tfhe_rot_net_level, net, sel, table_first, out_form, out_first, out_wires)

    def _rot_net_level(self, call, net, sel, table_first, out_form, out_first, out_wires):
        nodes = _i32c(net.nodes)
        if nodes.shape[1] == 3:      # a CmuxNet: every rotation 0
            nodes = np.ascontiguousarray(np.concatenate([nodes, np.zeros((nodes.shape[0], 2), np.int32)], axis=1))
        elif getattr(net, "degree", None) != self.N:
            raise ValueError(f"the network's rotations are taken mod 2 * {getattr(net, 'degree', None)}, the engine's polynomials have {self.N} coefficients")
        sel = _i32c(np.atleast_2d(sel))
        B, V = sel.shape
        if V < net.variables:
            raise ValueError(f"the network reads variable {net.variables - 1}, sel has {V} per row")
        first = None
        if table_first is not None:
            first = _i32c(table_first).reshape(-1)
            if first.size != B:
                raise ValueError(f"table_first must have one entry per row ({B}), got {first.size}")
        F = int(net.widths[-1])
        ow = None
        if out_wires is not None:
            ow = _i32c(out_wires).reshape(-1)
            if ow.size != B * F:
                raise ValueError(f"out_wires must have B F = {B * F} entries, got {ow.size}")
        self._check(call(self._h, _ptr(first), net.entries, _ptr(net.widths), net.levels, _ptr(nodes), _ptr(sel), V, int(out_form), int(out_first),
                         _ptr(ow), B))

    def blind_rotate_level(self, acc_slot, term_start, term_wire, term_coef, cst=None, sel=None, n_out=1, out_form=2, out_slot=None, out_wires=None):
        """blind_rotate between the tables (tfhe_blind_rotate_level).  Row g rotates the sample in TLWE slot acc_slot[g] by lut_level's
        combination of wires (term_start [B+1], term_wire, term_coef, cst) over the context's n steps; sel: int32 [n] or None.  out_form
        0: the final accumulator goes to slot out_slot[g]; out_form 2: the n_out extractions, keyswitched, to wires
        out_wires[g n_out + j].  Synchronous."""
        self._blind_rotate_level(self._lib.tfhe_blind_rotate_level, self.n, acc_slot, term_start, term_wire, term_coef, cst, sel, n_out, out_form,
                                 out_slot, out_wires)

    def bootstrap_acc_level(self, acc_slot, term_start, term_wire, term_coef, cst=None, n_out=1, out_form=2, out_slot=None, out_wires=None):
        """bootstrap_acc between the tables (tfhe_bootstrap_acc_level): blind_rotate_level on the gates' own kernel and key, without
        a selector set.  Every argument and the words are blind_rotate_level's with sel None.  Synchronous.
        Option acc_dispatch (see bootstrap_acc) chooses the kernel by the number of rows; the words are the same."""
        def call(h, acc, start, wire, coef, c, _sel, n_out_, out_form_, os_, ow, B):
            return self._lib.tfhe_bootstrap_acc_level(h, acc, start, wire, coef, c, n_out_, out_form_, os_, ow, B)
        self._blind_rotate_level(call, self.n, acc_slot, term_start, term_wire, term_coef, cst, None, n_out, out_form, out_slot, out_wires)

    def _blind_rotate_level(self, call, steps, acc_slot, term_start, term_wire, term_coef, cst, sel, n_out, out_form, out_slot, out_wires):
        acc = _i32c(acc_slot).reshape(-1)
        start = _i32c(term_start).reshape(-1)
        B = acc.size
        if start.size != B + 1:
            raise ValueError(f"term_start must have B + 1 = {B + 1} entries, got {start.size}")
        T = int(start[-1])
        wire, coef = _i32c(term_wire).reshape(-1), _i32c(term_coef).reshape(-1)
        if wire.size != coef.size or wire.size < T:
            raise ValueError(f"term_wire / term_coef must have term_start[B] = {T} entries, got {wire.size} / {coef.size}")
        c = None if cst is None else _i32c(cst).reshape(-1)
        if c is not None and c.size != B:
            raise ValueError(f"cst must have one entry per row ({B}), got {c.size}")
        s = None
        if sel is not None:
            s = _i32c(sel).reshape(-1)
            if s.size != steps:
                raise ValueError(f"sel must have one entry per step ({steps}), got {s.size}")
        n_out = int(n_out)
        os_ = None if out_slot is None else _i32c(out_slot).reshape(-1)
        if os_ is not None and os_.size != B:
            raise ValueError(f"out_slot must have one entry per row ({B}), got {os_.size}")
        ow = None if out_wires is None else _i32c(out_wires).reshape(-1)
        if ow is not None and ow.size != B * max(n_out, 1):
            raise ValueError(f"out_wires must have B n_out = {B * max(n_out, 1)} entries, got {ow.size}")
        self._check(call(self._h, _ptr(acc), _ptr(start), _ptr(wire), _ptr(coef), _ptr(c), _ptr(s), n_out, int(out_form), _ptr(os_), _ptr(ow), B))

    # ---- leveled mode under a multi-key cloud key: expanded RGSW selectors, MK TLWE samples [P+1][N] ----
    def mk_tgsw_load(self, tgsw, party_of):
        """The multi-key selector set (tfhe_mk_tgsw_load): int32 [S][2lP + 2l][N], S expanded RGSW samples laid out as the entries of
        the multi-key bootstrapping key (leveled.mk_tgsw_expand makes them), and party_of [S], the party each was expanded for.
        Replaces any earlier set."""
        P = self._mk_width("mk_tgsw_load")
        self._mk_key_extra = None      # (leveled.mk_two_stage_lookup_device: the set is no longer the one it loaded)
        t, who = _i32c(tgsw), _i32c(party_of).reshape(-1)
        per = (2 * self.params.bs_decomp_length * P + 2 * self.params.bs_decomp_length) * self.N
        if who.size == 0 or t.size != who.size * per:
            raise ValueError(f"expanded samples have {t.size} words, expected {per} for each of the {who.size} entries of party_of")
        self._check(self._lib.tfhe_mk_tgsw_load(self._h, _ptr(t), _ptr(who), who.size, P))

    def mk_tgsw_expand_load(self, pub_b, party_of, c0, c1, d0, d1, f0, f1, want_expanded=False):
        """The same selector set expanded on the device (tfhe_mk_tgsw_expand_load).  pub_b: [P][l][N]; party_of: [S]; c0 .. f1: [S][l][N],
        sample s uni-encrypted by party party_of[s] (leveled.mk_tgsw_uni_encrypt_bits).  Returns the expanded samples
        [S][2lP + 2l][N] if want_expanded."""
        P, l = self._mk_width("mk_tgsw_expand_load"), self.params.bs_decomp_length
        self._mk_key_extra = None      # (leveled.mk_two_stage_lookup_device: the set is no longer the one it loaded)
        who = _i32c(party_of).reshape(-1)
        S = who.size
        arrs = [_i32c(a) for a in (pub_b, c0, c1, d0, d1, f0, f1)]
        if arrs[0].shape != (P, l, self.N):
            raise ValueError(f"public keys must be [{P}][{l}][{self.N}], got {arrs[0].shape}")
        for a in arrs[1:]:
            if S == 0 or a.shape != (S, l, self.N):
                raise ValueError(f"uni-encryption arrays must be [{S}][{l}][{self.N}] with S >= 1, got {a.shape}")
        out = np.empty((S, 2 * l * P + 2 * l, self.N), np.int32) if want_expanded else None
        self._check(self._lib.tfhe_mk_tgsw_expand_load(self._h, P, _ptr(arrs[0]), _ptr(who), *[_ptr(a) for a in arrs[1:]], S, _ptr(out)))
        return out

    def mk_extern_mul(self, tlwe, sel):
        """out[g] = mk_tgsw_extern_mul(tlwe[g], selector[sel[g]]) (tfhe_mk_extern_mul_batch; mk_internals.jl:348-391): int32 [B][P+1][N]."""
        P = self._mk_width("mk_extern_mul")
        x = _i32c(tlwe)
        if x.ndim != 3 or x.shape[1:] != (P + 1, self.N):
            raise ValueError(f"MK TLWE samples must be [B][{P + 1}][{self.N}], got {x.shape}")
        B = x.shape[0]
        idx = _i32c(sel).reshape(-1)
        if idx.size != B:
            raise ValueError(f"sel must have one entry per row ({B}), got {idx.size}")
        out = np.empty_like(x)
        self._check(self._lib.tfhe_mk_extern_mul_batch(self._h, _ptr(x), _ptr(idx), _ptr(out), B))
        return out

    def mk_cmux_tree(self, data, sel, table_index=None, out_form=2):
        """CMUX-tree lookup on multi-key samples (tfhe_mk_cmux_tree_batch): cmux_tree with tables int32 [T][2^depth][P+1][N].  Row g's
        result is an MK TLWE sample [P+1][N] (out_form 0), extracted at coefficient 0 [P*N+1] (1) or keyswitched to a multi-key LWE
        sample [P*n+1] (2), an operand of every mk_gate."""
        P = self._mk_width("mk_cmux_tree")
        d = _i32c(data)
        if d.ndim == 3:
            d = d[None]
        sel = _i32c(np.atleast_2d(sel))
        B, depth = sel.shape
        if d.ndim != 4 or d.shape[1:] != (1 << min(max(depth, 0), 30), P + 1, self.N):
            raise ValueError(f"tables must be [T][2^{depth}][{P + 1}][{self.N}], got {d.shape}")
        idx = None
        if table_index is not None:
            idx = _i32c(table_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"table_index must have one entry per row ({B}), got {idx.size}")
        shape = {0: (B, P + 1, self.N), 1: (B, P * self.N + 1), 2: (B, P * self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form the library refuses: nothing written)
        self._check(self._lib.tfhe_mk_cmux_tree_batch(self._h, _ptr(d), d.shape[0], _ptr(idx), depth, _ptr(sel), _ptr(out), B, int(out_form)))
        return out

    def mk_cmux_net(self, data, net, sel, table_index=None, out_form=2):
        """CMUX network on multi-key samples (tfhe_mk_cmux_net_batch): cmux_net with tables int32 [T][E][P+1][N] and sel [B][V] into the
        multi-key selector set; every node multiplies for the party of its own selector.  Row g's F outputs are MK TLWE samples
        [B][F][P+1][N] (out_form 0), extracted at coefficient 0 [B][F][P*N+1] (1) or keyswitched to multi-key LWE samples [B][F][P*n+1]
        (2), operands of every mk_gate."""
        P = self._mk_width("mk_cmux_net")
        d, sel, idx = self._net_args(data, net, sel, table_index, P + 1)
        B, V = sel.shape
        F = int(net.widths[-1])
        shape = {0: (B, F, P + 1, self.N), 1: (B, F, P * self.N + 1), 2: (B, F, P * self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form the library refuses: nothing written)
        self._check(self._lib.tfhe_mk_cmux_net_batch(self._h, _ptr(d), d.shape[0], d.shape[1], _ptr(idx), _ptr(net.widths), net.levels, _ptr(net.nodes),
                                                     _ptr(sel), V, _ptr(out), B, int(out_form)))
        return out

    def mk_rot_net(self, data, net, sel, table_index=None, out_form=2):
        """CMUX network with monomial edges on multi-key samples (tfhe_mk_rot_net_batch): mk_cmux_net with net a leveled.RotNet, whose
        records carry a public rotation X^rot for each source, applied to all P + 1 polynomials; shapes and out_forms as mk_cmux_net
        (extraction at coefficient 0: a packed lookup rotates the wanted coefficient there)."""
        P = self._mk_width("mk_rot_net")
        if getattr(net, "degree", None) != self.N:
            raise ValueError(f"the network's rotations are taken mod 2 * {getattr(net, 'degree', None)}, the engine's polynomials have {self.N} coefficients")
        d, sel, idx = self._net_args(data, net, sel, table_index, P + 1)
        B, V = sel.shape
        F = int(net.widths[-1])
        shape = {0: (B, F, P + 1, self.N), 1: (B, F, P * self.N + 1), 2: (B, F, P * self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form the library refuses: nothing written)
        self._check(self._lib.tfhe_mk_rot_net_batch(self._h, _ptr(d), d.shape[0], d.shape[1], _ptr(idx), _ptr(net.widths), net.levels, _ptr(net.nodes),
                                                    _ptr(sel), V, _ptr(out), B, int(out_form)))
        return out

    def mk_blind_rotate(self, acc, rows, sel=None, acc_index=None, in_form=0, n_out=1, out_form=2):
        """Multi-key blind rotation of the caller's MK TLWE accumulators (tfhe_mk_blind_rotate_batch): blind_rotate under a multi-key
        cloud key.  acc: int32 [T][P+1][N] MK TLWE samples, trivial or encrypted (or [P+1][N]: one accumulator); rows: int32
        [B][steps+1], the step words then the body — multi-key LWE samples (in_form 0) or exponents in [0, 2N) (in_form 1); sel: int32
        [steps] indices into the multi-key selector set, shared by all rows, or None (selector i for step i), step i multiplying for
        the party of its selector; acc_index: [B] or None (accumulator 0).  Row g's result is the MK TLWE sample [B][P+1][N] (out_form
        0, n_out 1), its extractions at the coefficients j N / n_out [B][n_out][P*N+1] (1), or those keyswitched to multi-key LWE
        samples [B][n_out][P*n+1] (2), operands of every mk_gate."""
        P = self._mk_width("mk_blind_rotate")
        a = _i32c(acc)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (P + 1, self.N):
            raise ValueError(f"accumulators must be [T][{P + 1}][{self.N}], got {a.shape}")
        r = _i32c(rows)
        if r.ndim != 2 or r.shape[1] < 2:
            raise ValueError(f"rows must be [B][steps+1] with at least one step, got {r.shape}")
        B, steps = r.shape[0], r.shape[1] - 1
        s = None
        if sel is not None:
            s = _i32c(sel).reshape(-1)
            if s.size != steps:
                raise ValueError(f"sel must have one entry per step ({steps}), got {s.size}")
        idx = None
        if acc_index is not None:
            idx = _i32c(acc_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"acc_index must have one entry per row ({B}), got {idx.size}")
        n_out = int(n_out)
        K = n_out if 1 <= n_out <= 32 else 0
        shape = {0: (B, P + 1, self.N), 1: (B, K, P * self.N + 1), 2: (B, K, P * self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form or n_out the library refuses: nothing written)
        self._check(self._lib.tfhe_mk_blind_rotate_batch(self._h, _ptr(a), a.shape[0], _ptr(idx), _ptr(r), steps, int(in_form), _ptr(s), n_out, _ptr(out),
                                                         B, int(out_form)))
        return out

    def mk_bootstrap_acc(self, acc, rows, acc_index=None, n_out=1, out_form=2):
        """mk_blind_rotate on the multi-key gates' own kernel and key (tfhe_mk_bootstrap_acc_batch): rows are multi-key LWE samples int32
        [B][P*n+1], the steps are the P n entries of the loaded multi-key bootstrapping key, no selector set is read (the key need not
        be loaded a second time as selectors).  acc, acc_index, n_out, out_form and the result are mk_blind_rotate's, and so are the
        words where the selector set is mk_bootstrap_key_selectors(ck).  Served where get_option("mk_bootstrap_acc") is 1 (2 parties,
        N = 1024, l = 4); option mk_rw (0 = by B, 1, 2) sets the rotations per workgroup as for the gates."""
        P = self._mk_width("mk_bootstrap_acc")
        a = _i32c(acc)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (P + 1, self.N):
            raise ValueError(f"accumulators must be [T][{P + 1}][{self.N}], got {a.shape}")
        r = _i32c(rows)
        if r.ndim != 2 or r.shape[1] != P * self.n + 1:
            raise ValueError(f"rows must be multi-key LWE samples [B][{P * self.n + 1}], got {r.shape}")
        B = r.shape[0]
        idx = None
        if acc_index is not None:
            idx = _i32c(acc_index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"acc_index must have one entry per row ({B}), got {idx.size}")
        n_out = int(n_out)
        K = n_out if 1 <= n_out <= 32 else 0
        shape = {0: (B, P + 1, self.N), 1: (B, K, P * self.N + 1), 2: (B, K, P * self.n + 1)}.get(int(out_form), (0,))
        out = np.empty(shape, np.int32)      # (an out_form or n_out the library refuses: nothing written)
        self._check(self._lib.tfhe_mk_bootstrap_acc_batch(self._h, _ptr(a), a.shape[0], _ptr(idx), _ptr(r), n_out, int(out_form), _ptr(out), B))
        return out

    # ---- multi-key leveled mode on device-resident tables: the MK TLWE table beside the multi-key wire table ----
    def mk_tlwe_alloc(self, slots):
        """A device table of MK TLWE samples int32 [slots][P+1][N] for the parties of the loaded multi-key bootstrapping key
        (tfhe_mk_tlwe_alloc); 0 frees it, reallocating discards the contents."""
        self._check(self._lib.tfhe_mk_tlwe_alloc(self._h, int(slots)))

    def mk_tlwe_upload(self, first, samples):
        """samples int32 [count][P+1][N] into slots [first, first + count) (tfhe_mk_tlwe_upload), behind the levels queued so far."""
        P = self._mk_width("mk_tlwe_upload")
        m = _i32c(samples)
        if m.ndim == 2:
            m = m[None]
        if m.ndim != 3 or m.shape[1:] != (P + 1, self.N):
            raise ValueError(f"MK TLWE samples must be [count][{P + 1}][{self.N}], got {m.shape}")
        self._check(self._lib.tfhe_mk_tlwe_upload(self._h, int(first), m.shape[0], _ptr(m)))

    def mk_tlwe_download(self, first, count):
        """Slots [first, first + count) as int32 [count][P+1][N] (tfhe_mk_tlwe_download), behind the levels queued so far."""
        P = self._mk_width("mk_tlwe_download")
        out = np.empty((max(int(count), 0), P + 1, self.N), np.int32)
        self._check(self._lib.tfhe_mk_tlwe_download(self._h, int(first), int(count), _ptr(out)))
        return out

    def mk_tgsw_update(self, first, tgsw, party_of):
        """Replaces selectors [first, first + count) of the loaded multi-key set in place (tfhe_mk_tgsw_update): tgsw int32
        [count][2lP + 2l][N] expanded samples, party_of [count]; every other selector keeps its words."""
        P = self._mk_width("mk_tgsw_update")
        t, who = _i32c(tgsw), _i32c(party_of).reshape(-1)
        per = (2 * self.params.bs_decomp_length * P + 2 * self.params.bs_decomp_length) * self.N
        if who.size == 0 or t.size != who.size * per:
            raise ValueError(f"expanded samples have {t.size} words, expected {per} for each of the {who.size} entries of party_of")
        self._check(self._lib.tfhe_mk_tgsw_update(self._h, _ptr(t), _ptr(who), int(first), who.size, P))

    def mk_tgsw_expand_update(self, first, pub_b, party_of, c0, c1, d0, d1, f0, f1, want_expanded=False):
        """The same update expanded on the device (tfhe_mk_tgsw_expand_update).  pub_b: [P][l][N]; party_of: [count]; c0 .. f1:
        [count][l][N], sample s uni-encrypted by party party_of[s].  Returns the expanded samples [count][2lP + 2l][N] if want_expanded."""
        P, l = self._mk_width("mk_tgsw_expand_update"), self.params.bs_decomp_length
        who = _i32c(party_of).reshape(-1)
        S = who.size
        arrs = [_i32c(a) for a in (pub_b, c0, c1, d0, d1, f0, f1)]
        if arrs[0].shape != (P, l, self.N):
            raise ValueError(f"public keys must be [{P}][{l}][{self.N}], got {arrs[0].shape}")
        for a in arrs[1:]:
            if S == 0 or a.shape != (S, l, self.N):
                raise ValueError(f"uni-encryption arrays must be [{S}][{l}][{self.N}] with count >= 1, got {a.shape}")
        out = np.empty((S, 2 * l * P + 2 * l, self.N), np.int32) if want_expanded else None
        self._check(self._lib.tfhe_mk_tgsw_expand_update(self._h, P, _ptr(arrs[0]), _ptr(who), *[_ptr(a) for a in arrs[1:]], int(first), S, _ptr(out)))
        return out

    def mk_rot_net_level(self, net, sel, table_first=None, out_form=2, out_first=0, out_wires=None):
        """mk_rot_net between the tables (tfhe_mk_rot_net_level): rot_net_level with MK TLWE slots, multi-key wires and the multi-key
        selector set.  Synchronous."""
        self._mk_width("mk_rot_net_level")
        self._rot_net_level(self._lib.tfhe_mk_rot_net_level, net, sel, table_first, out_form, out_first, out_wires)

    def mk_blind_rotate_level(self, acc_slot, term_start, term_wire, term_coef, cst=None, sel=None, n_out=1, out_form=2, out_slot=None, out_wires=None):
        """mk_blind_rotate between the tables (tfhe_mk_blind_rotate_level): blind_rotate_level with MK TLWE slots, mk_lut_level's
        combination of multi-key wires over P n steps (sel: int32 [P n] or None, selector i for step i) and the multi-key keyswitch.
        Synchronous."""
        P = self._mk_width("mk_blind_rotate_level")
        self._blind_rotate_level(self._lib.tfhe_mk_blind_rotate_level, P * self.n, acc_slot, term_start, term_wire, term_coef, cst, sel, n_out,
                                 out_form, out_slot, out_wires)

    def mk_bootstrap_acc_level(self, acc_slot, term_start, term_wire, term_coef, cst=None, n_out=1, out_form=2, out_slot=None, out_wires=None):
        """mk_bootstrap_acc between the tables (tfhe_mk_bootstrap_acc_level): mk_blind_rotate_level on the multi-key gates' own kernel and
        key, without a selector set.  Every argument and the words are mk_blind_rotate_level's with sel None.  Synchronous."""
        P = self._mk_width("mk_bootstrap_acc_level")

        def call(h, acc, start, wire, coef, c, _sel, n_out_, out_form_, os_, ow, B):
            return self._lib.tfhe_mk_bootstrap_acc_level(h, acc, start, wire, coef, c, n_out_, out_form_, os_, ow, B)
        self._blind_rotate_level(call, P * self.n, acc_slot, term_start, term_wire, term_coef, cst, None, n_out, out_form, out_slot, out_wires)

    # ---- levelised circuits on the device-resident wire table ----
    def wires_alloc(self, num_wires):
        self._check(self._lib.tfhe_wires_alloc(self._h, int(num_wires)))
        self._wire_width = self.n + 1

    def mk_wires_alloc(self, num_wires):
        """A wire table of multi-key rows [num_wires][P*n+1] for the parties of the loaded multi-key keys (tfhe_mk_wires_alloc);
        wires_upload / _download / _gather then move rows of that width."""
        self._check(self._lib.tfhe_mk_wires_alloc(self._h, int(num_wires)))
        self._wire_width = self._mk_parties * self.n + 1

    def wires_upload(self, first, samples):
        m = _i32c(samples)
        if m.ndim != 2 or m.shape[1] != self._wire_width:
            raise ValueError("samples must be [count][n+1]" if self._wire_width == self.n + 1 else
                             f"samples must be [count][{self._wire_width}] (multi-key wire table)")
        self._check(self._lib.tfhe_wires_upload(self._h, int(first), m.shape[0], _ptr(m)))

    def wires_download(self, first, count):
        out = np.empty((int(count), self._wire_width), np.int32)
        self._check(self._lib.tfhe_wires_download(self._h, int(first), int(count), _ptr(out)))
        return out

    def wires_gather(self, wires):
        """Rows of the given wire indices, in one device gather + one copy."""
        idx = np.ascontiguousarray(wires, dtype=np.int32).reshape(-1)
        out = np.empty((idx.size, self._wire_width), np.int32)
        self._check(self._lib.tfhe_wires_gather(self._h, _ptr(idx), idx.size, _ptr(out)))
        return out

    def gates_level(self, opcodes, a, b, c, out):
        ops = np.ascontiguousarray(opcodes, dtype=np.uint8)
        arrs = [None if v is None else _i32c(v) for v in (a, b, c, out)]
        for v in arrs:
            if v is not None and v.shape != (ops.size,):
                raise ValueError("index arrays must have one entry per gate")
        self._check(self._lib.tfhe_gates_level(self._h, _ptr(ops), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                                               _ptr(arrs[3]), ops.size))

    def _level_terms(self, term_start, term_wire, term_coef, cst, out, per_row):
        start = _i32c(term_start).reshape(-1)
        B = start.size - 1
        if B < 0:
            raise ValueError("term_start must have B + 1 entries")
        T = int(start[-1]) if B >= 0 else 0
        wire, coef = _i32c(term_wire).reshape(-1), _i32c(term_coef).reshape(-1)
        if wire.size != coef.size or wire.size < T:
            raise ValueError(f"term_wire / term_coef must have term_start[B] = {T} entries, got {wire.size} / {coef.size}")
        c = None if cst is None else _i32c(cst).reshape(-1)
        if c is not None and c.size != B:
            raise ValueError(f"cst must have one entry per row ({B}), got {c.size}")
        o = _i32c(out).reshape(-1)
        if o.size != B * per_row:
            raise ValueError(f"out must have {B * per_row} entries (B n_out), got {o.size}")
        return start, wire, coef, c, o, B

    def lut_level(self, tables, term_start, term_wire, term_coef, cst, out, index=None, n_out=1):
        """Programmable bootstrapping on the wire table (tfhe_lut_level): row g's sample is sum_t term_coef[t] wire[term_wire[t]] over
        t in [term_start[g], term_start[g+1]), plus cst[g] on the body (mod 2^32; cst None: 0); its n_out results (bootstrap_tv_multi:
        tables[index[g]], index None: table 0) go to wires out[g n_out + j].  Asynchronous; the arrays may be reused at once."""
        self._lut_level(self._lib.tfhe_lut_level, tables, term_start, term_wire, term_coef, cst, out, index, n_out)

    def _lut_level(self, fn, tables, term_start, term_wire, term_coef, cst, out, index, n_out):
        tables = _i32c(np.atleast_2d(tables))
        if tables.ndim != 2 or tables.shape[1] != self.N:
            raise ValueError(f"test polynomials must be [n_tv][{self.N}], got {tables.shape}")
        n_out = int(n_out)
        start, wire, coef, c, o, B = self._level_terms(term_start, term_wire, term_coef, cst, out, max(n_out, 1))
        idx = None
        if index is not None:
            idx = _i32c(index).reshape(-1)
            if idx.size != B:
                raise ValueError(f"index must have one entry per row ({B}), got {idx.size}")
        self._check(fn(self._h, _ptr(tables), tables.shape[0], _ptr(idx), n_out, _ptr(start), _ptr(wire), _ptr(coef), _ptr(c), _ptr(o), B))

    def linear_level(self, term_start, term_wire, term_coef, cst, out):
        """wire[out[g]] = the combination of lut_level's row g itself, no bootstrap (tfhe_linear_level): exact mod-2^32 arithmetic."""
        self._linear_level(self._lib.tfhe_linear_level, term_start, term_wire, term_coef, cst, out)

    def _linear_level(self, fn, term_start, term_wire, term_coef, cst, out):
        start, wire, coef, c, o, B = self._level_terms(term_start, term_wire, term_coef, cst, out, 1)
        self._check(fn(self._h, _ptr(start), _ptr(wire), _ptr(coef), _ptr(c), _ptr(o), B))

    def mk_lut_level(self, tables, term_start, term_wire, term_coef, cst, out, index=None, n_out=1):
        """`lut_level` on the multi-key wire table (tfhe_mk_lut_level, mk_wires_alloc): the multi-key rotation and keyswitch."""
        self._lut_level(self._lib.tfhe_mk_lut_level, tables, term_start, term_wire, term_coef, cst, out, index, n_out)

    def mk_linear_level(self, term_start, term_wire, term_coef, cst, out):
        """`linear_level` on the multi-key wire table (tfhe_mk_linear_level)."""
        self._linear_level(self._lib.tfhe_mk_linear_level, term_start, term_wire, term_coef, cst, out)

    # ---- multi-key ----
    def mk_load_bootstrap_key(self, bk_i32, parties):
        bk = _i32c(bk_i32)
        P, l = int(parties), self.params.bs_decomp_length
        want = P * self.n * (2 * l * P + 2 * l) * self.N
        if bk.size != want:
            raise ValueError(f"multi-key bootstrap key has {bk.size} words, expected {want} for {P} parties")
        self._check(self._lib.tfhe_mk_load_bootstrap_key_i32(self._h, _ptr(bk), P))
        self._mk_parties = P

    def mk_load_bootstrap_key_spectra(self, spectra, parties):
        """The reference's stored form: complex128 [P][n][2lP + 2l][N/2]."""
        sp = np.ascontiguousarray(spectra, dtype=np.complex128)
        P, l = int(parties), self.params.bs_decomp_length
        want = P * self.n * (2 * l * P + 2 * l) * (self.N // 2)
        if sp.size != want:
            raise ValueError(f"multi-key bootstrap spectra have {sp.size} values, expected {want} for {P} parties")
        self._check(self._lib.tfhe_mk_load_bootstrap_key_c128(self._h, _ptr(sp), P))
        self._mk_parties = P

    def mk_expand_load_bootstrap_key(self, parties, pub_b, c0, c1, d0, d1, f0, f1, want_expanded=False):
        """RGSW.Expand on the device (tfhe_mk_expand_load_bootstrap_key).  pub_b: [P][l][N]; c0 .. f1: [P][n][l][N].
        Returns the expanded Int32 key [P][n][2lP + 2l][N] if want_expanded."""
        P, l = int(parties), self.params.bs_decomp_length
        arrs = [_i32c(a) for a in (pub_b, c0, c1, d0, d1, f0, f1)]
        if arrs[0].shape != (P, l, self.N):
            raise ValueError(f"public keys must be [{P}][{l}][{self.N}], got {arrs[0].shape}")
        for a in arrs[1:]:
            if a.shape != (P, self.n, l, self.N):
                raise ValueError(f"uni-encryption arrays must be [{P}][{self.n}][{l}][{self.N}], got {a.shape}")
        out = np.empty((P, self.n, 2 * l * P + 2 * l, self.N), np.int32) if want_expanded else None
        self._check(self._lib.tfhe_mk_expand_load_bootstrap_key(self._h, P, *[_ptr(a) for a in arrs], _ptr(out)))
        self._mk_parties = P
        return out

    def mk_load_keyswitch_key(self, ks, parties):
        ks = _i32c(ks)
        P, p = int(parties), self.params
        want = P * self.N * p.ks_decomp_length * ((1 << p.ks_log2_base) - 1) * (self.n + 1)
        if ks.size != want:
            raise ValueError(f"multi-key keyswitch key has {ks.size} words, expected {want} for {P} parties")
        self._check(self._lib.tfhe_mk_load_keyswitch_key(self._h, _ptr(ks), P))

    def mk_gate_nand(self, in0, in1):
        in0, in1 = _i32c(in0), _i32c(in1)
        P = getattr(self, "_mk_parties", None)
        if P is None:
            raise EngineError(3, "mk_gate_nand: multi-key keys not loaded")
        if in0.ndim != 2 or in0.shape[1] != P * self.n + 1 or in1.shape != in0.shape:
            raise ValueError(f"multi-key operands must both be [B][{P * self.n + 1}], got {in0.shape} and {in1.shape}")
        out = np.empty_like(in0)
        self._check(self._lib.tfhe_mk_gate_nand_batch(self._h, _ptr(in0), _ptr(in1), _ptr(out), in0.shape[0]))
        return out

    def mk_gates_batch(self, opcodes, in0, in1=None, in2=None, out=None):
        """Mixed batch of multi-key gates (tfhe_mk_gates_batch): operands and result int32 [B][P*n+1]; an operand no opcode
        reads may be None."""
        ops = np.ascontiguousarray(opcodes, dtype=np.uint8)
        B = ops.size
        P = getattr(self, "_mk_parties", None)
        if P is None:
            raise EngineError(3, "mk_gates_batch: multi-key keys not loaded")
        w = P * self.n + 1
        in0, in1, in2 = _i32c(in0), _i32c(in1), _i32c(in2)
        for a in (in0, in1, in2):
            if a is not None and a.shape != (B, w):
                raise ValueError(f"multi-key operand shape {a.shape}, expected {(B, w)}")
        if out is None:
            out = np.empty((B, w), np.int32)
        elif out.dtype != np.int32 or out.shape != (B, w) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous int32 array of shape {(B, w)}")
        self._check(self._lib.tfhe_mk_gates_batch(self._h, _ptr(ops), _ptr(in0), _ptr(in1), _ptr(in2), _ptr(out), B))
        return out

    def mk_gates_level(self, opcodes, a, b, c, out):
        """One level on the multi-key wire table (tfhe_mk_gates_level): the index arrays of gates_level."""
        ops = np.ascontiguousarray(opcodes, dtype=np.uint8)
        arrs = [None if v is None else _i32c(v) for v in (a, b, c, out)]
        for v in arrs:
            if v is not None and v.shape != (ops.size,):
                raise ValueError("index arrays must have one entry per gate")
        self._check(self._lib.tfhe_mk_gates_level(self._h, _ptr(ops), _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]),
                                                  _ptr(arrs[3]), ops.size))

    # ---- measurement ----
    def last_timing_ms(self, which):
        ms = C.c_float(0)
        self._check(self._lib.tfhe_last_timing_ms(self._h, int(which), C.byref(ms)))
        return float(ms.value)

    def timing_history_ms(self, which, max_calls=32):
        """Kernel-side durations (HIP events) of up to the last 32 batch calls, oldest first, read after the calls in one go
        (tfhe_timing_history_ms): no synchronisation between the calls themselves."""
        buf = (C.c_float * int(max_calls))()
        n = C.c_int32(0)
        self._check(self._lib.tfhe_timing_history_ms(self._h, int(which), buf, int(max_calls), C.byref(n)))
        return [float(buf[i]) for i in range(n.value)]

    def last_rotation_count(self):
        return int(self._lib.tfhe_last_rotation_count(self._h))

    def last_device_count(self):
        """Device contexts the last batch / level call was sharded over (1 on a one-device context)."""
        return int(self._lib.tfhe_last_device_count(self._h))

    def last_rounding_margin(self):
        m = C.c_double(0)
        self._check(self._lib.tfhe_last_rounding_margin(self._h, C.byref(m)))
        return float(m.value)

    def last_kernel_clock_mhz(self):
        m = C.c_double(0)
        self._check(self._lib.tfhe_last_kernel_clock_mhz(self._h, C.byref(m)))
        return float(m.value)

    def last_kernel_name(self):
        return self._lib.tfhe_last_kernel_name(self._h).decode()

    def device_count(self):
        return int(self._lib.tfhe_ctx_device_count(self._h))

    def set_option(self, name, value):
        self._check(self._lib.tfhe_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int64(0)
        self._check(self._lib.tfhe_get_option(self._h, name.encode(), C.byref(v)))
        return v.value
