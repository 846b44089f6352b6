/*
 * tfhe_mi355x.h — C ABI of the MI355X-native TFHE gate-bootstrapping engine (libtfhe_mi355x.so).
 *
 * The reference (nucypher/TFHE.jl) has no FFI for this path: it is plain Julia.  This header is the
 * drop-in boundary a `ccall` shim binds instead of the Julia functions cited per entry point
 * (paths relative to the reference checkout).  Plain pointers and sizes only; no C++ types, no
 * exceptions cross the boundary: every entry point catches what its C++ body throws (a std::vector or std::thread that could
 * not be had: TFHE_ERR_NOMEM; anything else: TFHE_ERR_STATE with the exception's text) and the context stays usable — under a
 * Julia `ccall` or Python `ctypes` an escaping exception would end the process.  Every function returns 0 on success or a
 * TFHE_ERR_* code; tfhe_last_error() gives the message for the last failure on that context.
 *
 * Data formats (all Torus32 = int32_t, wrapping two's-complement arithmetic):
 *   LWE sample      : int32[n+1]          = a[0..n-1], b            (lwe.jl:21-29)
 *   extracted sample: int32[k*N+1]        = a[0..kN-1], b           (tlwe.jl:55-59)
 *   bootstrapping key, canonical Int32 form:
 *       int32 [n][l][k+1][k+1][N]  = key[i].samples[p, j].a[c]      (bootstrap.jl:1-16, tgsw.jl:25-42)
 *       i.e. the inverse_transform of the spectra the reference stores (bootstrap.jl:12-14)
 *   bootstrapping key, the reference's stored form:
 *       complex128 [n][l][k+1][k+1][N/2] (re,im interleaved)        (polynomials.jl:12-14,106-112)
 *   keyswitch key   : int32 [kN][t][base-1][n+1] = key[h, j, i]     (keyswitch.jl:7-42; h fastest in Julia)
 *   MK sample       : int32[P*n+1]        = a[:,0], a[:,1], ..., b  (mk_internals.jl:6-18)
 *   MK bootstrap key: int32 [P][n][2*l*P + 2*l][N], per (party i, bit j) the polys
 *       x[l][P], y[l][P], c0[l], c1[l]                              (mk_internals.jl:243-271,442-461)
 *   MK keyswitch key: P single-key keyswitch keys back to back      (mk_api.jl:83-101)
 *
 * Ownership: the caller owns every host buffer for the duration of the call only; the library
 * copies keys to the device(s) at load time and owns all device memory.  A context made by
 * tfhe_ctx_create is bound to one device; one made by tfhe_ctx_create_multi fans every host-buffer
 * batch call out over its devices on library-owned threads and streams (keys replicated at load,
 * contiguous rotation-balanced shards, results written straight into the caller's buffer).
 *
 * Threading.  The reference is single-threaded and non-re-entrant (global transform plans with shared scratch,
 * polynomials.jl:80-103).  Here distinct contexts are independent, and calls on ONE context must not overlap: the thread
 * inside an entry point owns the context until that call returns, and a call made meanwhile from another thread fails with
 * TFHE_ERR_STATE (tfhe_last_error then tells that thread why) instead of racing on the context's workspaces.  Give every
 * host thread its own context (keys are per context), or serialise the calls (the Julia binding holds a ReentrantLock).
 * Two entry points are exempt and may be called from any thread at any time: tfhe_ctx_synchronize and tfhe_gates_batch_wait
 * (which then waits as tfhe_ctx_synchronize does) — what a finalizer needs before it frees the buffers of a submitted batch.
 * The asynchronous forms (tfhe_gates_batch_submit, tfhe_gates_batch_dev, tfhe_gates_level) return while the device works;
 * only their host side is a "call" in this sense.
 *
 * Parameter sets.  The reference validates nothing (SchemeParameters is a positional struct, tlwe_mask_size a free keyword:
 * api.jl:4-21,30,55); decode_message needs 2N to be a power of two (numeric-functions.jl:28-33) and the transform plans an even
 * length (polynomials.jl:51,69).  tfhe_ctx_create accepts EVERY such set: N any power of two from 2 to 8192, any tlwe_mask_size
 * k, any bs_decomp_length l with l * bs_log2_base <= 32, any lwe_size, any keyswitch base / length with t * gamma <= 31;
 * multi-key: any N, any number of parties, any l (k = 1 as the reference hard-wires it, mk_internals.jl:89-91,129-131).
 * What runs where (every path gives the same words):
 *   tuned kernels      N = 1024 with k = 1 and ANY l (instantiated for the shipped l = 2 and 3; the one- and two-waves-per-rotation
 *                      kernels also exist with l as a run-time value and serve every other l at the same speed); N = 1024 with
 *                      k = 2 and l = 2 or 3; N = 2048 with k = 1 and l = 3 (BASELINE config 4b); N = 512 with k = 1 and any l (the
 *                      same design with four points per lane); multi-key N = 1024: the shipped 2- / 4- / 8-party sets
 *   general kernels    everything else at N = 1024 / 2048 with k <= 4 (blind_rotate_kernel_general, ~3.5 x slower than tuned),
 *                      multi-key at N = 1024 with up to 8 parties and l <= 8 (mk_blind_rotate_kernel_general)
 *   any-N kernels      every other set (N other than 512 / 1024 / 2048, N = 512 with k > 1, k > 4, multi-key with N other than 1024, more than 8 parties or
 *                      l > 8): csrc/kernels_anyn.hpp, one workgroup per rotation, mixed-radix transforms in LDS — correct, untuned
 *   keyswitch          int8 MFMA kernel for base 4 / t = 8 (k N a multiple of 128), tiled integer kernel for base 4 / t a
 *                      multiple of 4 (k N <= 2048), gather kernel for every other base, length and size (single- and multi-key)
 * Refused: N that is no power of two (TFHE_ERR_INVALID_ARG), N > 8192 (TFHE_ERR_UNSUPPORTED: one polynomial's transform no
 * longer fits a compute unit's 160 KB of LDS — and the Float64 transform, here as in the reference, has no rounding margin
 * left there), multi-key with tlwe_mask_size != 1 (TFHE_ERR_UNSUPPORTED: as the reference).
 *
 * Exactness domain.  Like the reference (polynomials.jl:106-132) the external product goes through a Float64 transform and
 * ONE rounding per output coefficient (polynomials.jl:115-116: round(Int64, x), low 32 bits).  Every result word is the exact
 * negacyclic product mod 2^32 as long as (i) the transform's error stays below 1/2 — tfhe_last_rounding_margin measures the
 * largest distance of a pre-rounding value from an integer; 0.03 - 0.08 at the shipped sets, growing with N, l and
 * bs_log2_base — and (ii) every pre-rounding value v satisfies |v| < 2^51: the kernels round with the 1.5 * 2^52 trick, exact
 * there; the reference's round(Int64, .) is defined up to 2^63 but has lost integer precision long before.  With a real key
 * (uniform words) |v| is around sqrt((k+1) l N) * 2^(bs_log2_base + 29) = 2^44 at the 80-bit set; only a caller-supplied
 * "key" whose words all share one sign at magnitude 2^31 reaches 2^52 (k = 1, l = 2, beta = 10, N = 1024): outside the domain,
 * no guarantee there from this engine or from the reference (tests/test_any_params.py::test_worst_case_magnitude_key feeds
 * such a key and records what comes out: with every word -2^31 the values are multiples of 2^31, which Float64 still holds
 * exactly, and both still return the exact product; full-range random words with the extremes planted are exact as any key).
 */
#ifndef TFHE_MI355X_H
#define TFHE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFHE_MI355X_ABI_VERSION 7

/* Scheme parameters — the fields of SchemeParameters the hot path reads (api.jl:4-21). */
typedef struct tfhe_params {
    int32_t n;            /* lwe_size                                  api.jl:6   */
    int32_t N;            /* tlwe_polynomial_degree (power of two)     api.jl:9   */
    int32_t k;            /* tlwe_mask_size                            api.jl:10  */
    int32_t bs_l;         /* bs_decomp_length                          api.jl:12  */
    int32_t bs_log2_base; /* bs_log2_base                              api.jl:13  */
    int32_t ks_t;         /* ks_decomp_length                          api.jl:16  */
    int32_t ks_log2_base; /* ks_log2_base                              api.jl:17  */
    int32_t parties;      /* max_parties (1 = single key)              api.jl:20  */
} tfhe_params;

typedef struct tfhe_ctx tfhe_ctx;

/* error codes */
enum {
    TFHE_OK = 0,
    TFHE_ERR_INVALID_ARG = 1,  /* NULL pointer, bad size, bad opcode                       */
    TFHE_ERR_UNSUPPORTED = 2,  /* parameter set outside what the kernels are built for      */
    TFHE_ERR_NO_KEY = 3,       /* a key needed by the call has not been loaded              */
    TFHE_ERR_DEVICE = 4,       /* HIP runtime error (no device, allocation, launch, ...)    */
    TFHE_ERR_STATE = 5,        /* call not possible in the context's state: wrong kind of context, overlapping call
                                  from another thread, option after the key it decides about; unexpected C++ exception */
    TFHE_ERR_NOMEM = 6         /* host memory exhausted inside the library (std::bad_alloc); ABI v7                    */
};

/* Gate opcodes for tfhe_gates_batch — one per exported gate_* function (TFHE.jl:34-46). */
enum {
    TFHE_GATE_NAND = 0,    /* gate_nand    gates.jl:15-18   */
    TFHE_GATE_OR = 1,      /* gate_or      gates.jl:27-30   */
    TFHE_GATE_AND = 2,     /* gate_and     gates.jl:39-42   */
    TFHE_GATE_XOR = 3,     /* gate_xor     gates.jl:51-54   */
    TFHE_GATE_XNOR = 4,    /* gate_xnor    gates.jl:63-66   */
    TFHE_GATE_NOT = 5,     /* gate_not     gates.jl:76-79   (no bootstrap) */
    TFHE_GATE_NOR = 6,     /* gate_nor     gates.jl:102-105 */
    TFHE_GATE_ANDNY = 7,   /* gate_andny   gates.jl:114-117 */
    TFHE_GATE_ANDYN = 8,   /* gate_andyn   gates.jl:126-129 */
    TFHE_GATE_ORNY = 9,    /* gate_orny    gates.jl:138-141 */
    TFHE_GATE_ORYN = 10,   /* gate_oryn    gates.jl:150-153 */
    TFHE_GATE_MUX = 11,    /* gate_mux     gates.jl:163-177 (2 blind rotations + 1 keyswitch) */
    TFHE_GATE_CONST0 = 12, /* gate_constant(ck, false)  gates.jl:91-93 */
    TFHE_GATE_CONST1 = 13, /* gate_constant(ck, true)   gates.jl:91-93 */
    TFHE_GATE_COPY = 14,   /* identity (circuit plumbing; no reference counterpart needed) */
    TFHE_GATE__COUNT = 15
};

/* ---- library / context ------------------------------------------------------------------- */

/* ABI version of the loaded library (== TFHE_MI355X_ABI_VERSION it was built with).  NEGATIVE: a development build
 * (-DTFHE_EXPERIMENT, csrc/experiment.hpp: in-kernel stamps, environment-variable overrides) that a binding must refuse
 * unless its user asked for it. */
int32_t tfhe_abi_version(void);

/* Number of HIP devices visible to this process (<0: runtime error). */
int32_t tfhe_device_count(void);

/* Replaces the implicit construction of TGswParams / KeyswitchParameters / LweParams from
 * SchemeParameters (api.jl:72-82, tgsw.jl:8-21) and validates what the reference does not
 * (api.jl:4-21 has no checks): N a power of two (2 .. 8192), bs_l*bs_log2_base <= 32, ks_t*ks_log2_base <= 31. */
int32_t tfhe_ctx_create(const tfhe_params *params, int32_t device_id, tfhe_ctx **out_ctx);
void tfhe_ctx_destroy(tfhe_ctx *ctx);

/* Multi-device context (ctx_create(params, device_ids[], n_dev)): the analogue of Julia's
 * `gate_xor.(cloud_key, c1, c2)` broadcast (docs/src/manual.md:28-35) spread over all the GPUs of a node.
 * One device context per entry of device_ids[] (an id may repeat: two contexts then share that GPU on separate
 * streams).  tfhe_load_* / tfhe_mk_load_* replicate the key to every device; tfhe_gates_batch,
 * tfhe_bootstrap_batch, tfhe_keyswitch_batch, tfhe_mk_gate_nand_batch and tfhe_mk_gates_batch split the batch into contiguous
 * shards (gates: balanced by blind-rotation count, MUX = 2) that run concurrently and write into the caller's buffers.
 * There is no communication between devices: the gates of a batch are independent (gates.jl).
 * tfhe_gates_batch_dev needs n_dev == 1 (a device pointer belongs to one device).  tfhe_gates_batch_submit gives every
 * device its shard as a submit of its own, so each keeps two batches in flight.  The wire table (tfhe_wires_*) is
 * replicated on every device; tfhe_gates_level runs a level of fewer than "level_split_min" blind rotations (option,
 * default 16 per compute unit of the first device: 4096 on an MI355X) on the first device and shards a wider one over all of them.  The context tracks which replicas hold each
 * wire's current value: a device fetches the operand rows it is about to read and does not have — device to device
 * (hipMemcpyPeerAsync; peer access is switched on at creation wherever hipDeviceCanAccessPeer allows) or through pinned host
 * memory where it does not (option "level_exchange": 0 = by peer access, 1 / 2 force either path) — on the devices' own streams,
 * ordered by events: like the one-device call, tfhe_gates_level returns when the level is queued.  Rows nobody else reads
 * never travel; tfhe_wires_download / _gather bring the first device up to date for what they read.  Results are
 * bit-identical to a one-device context. */
int32_t tfhe_ctx_create_multi(const tfhe_params *params, const int32_t *device_ids, int32_t n_dev,
                              tfhe_ctx **out_ctx);
/* Number of device contexts behind ctx (1 for tfhe_ctx_create). */
int32_t tfhe_ctx_device_count(const tfhe_ctx *ctx);
/* The sharding rule of a multi-device tfhe_gates_batch: bounds[r] .. bounds[r+1] (r < shards) are the gates of
 * shard r; contiguous, balanced by blind rotations (MUX = 2, NOT / CONSTANT / COPY = 0; gates.jl:76-93,163-177).
 * opcodes may be NULL (all gates cost one rotation).  bounds: int64 [shards + 1]. */
int32_t tfhe_shard_bounds(const uint8_t *opcodes, int64_t B, int32_t shards, int64_t *bounds);

/* Message of the last error on ctx (ctx == NULL: last error of a failed tfhe_ctx_create). */
const char *tfhe_last_error(const tfhe_ctx *ctx);

/* Copies the parameters the context was created with. */
int32_t tfhe_ctx_params(const tfhe_ctx *ctx, tfhe_params *out);

/* Blocks until everything queued on ctx so far has completed: its own stream, its second stream (tfhe_gates_batch_submit),
 * every device of a multi-device context.  Takes no ownership of the context and touches none of its state: callable from ANY
 * thread, also while another thread is inside a call on ctx (ABI v7).  For code that must release the host buffers of a submitted
 * batch without being the context's caller — a garbage collector's finalizer, an error path: after it returns TFHE_OK no DMA
 * of an earlier submit is still reading or writing them. */
int32_t tfhe_ctx_synchronize(tfhe_ctx *ctx);

/* ---- keys (replace CloudKey's object graphs, api.jl:111-127) -------------------------------- */

/* BootstrapKey (bootstrap.jl:1-16) from the canonical Int32 form [n][l][k+1][k+1][N].
 * The engine forward-transforms it on the device into its own spectrum-domain layout
 * (the analogue of `forward_transform.(bk)`, bootstrap.jl:12).  Any Int32 words are accepted; results are the exact product
 * within the exactness domain stated at the top of this file (|pre-rounding value| < 2^51: every real key). */
int32_t tfhe_load_bootstrap_key_i32(tfhe_ctx *ctx, const int32_t *bk);

/* BootstrapKey from the reference's stored spectra, complex128 [n][l][k+1][k+1][N/2] as produced by
 * polynomials.jl:106-112.  The engine's spectrum domain is the reference's (same fold, twist and
 * transform sign), so loading is a permutation into the engine's order plus the 1/M scaling. */
int32_t tfhe_load_bootstrap_key_c128(tfhe_ctx *ctx, const double *bk_spectra);

/* KeyswitchKey (keyswitch.jl:7-42), Int32 [kN][t][base-1][n+1]. */
int32_t tfhe_load_keyswitch_key(tfhe_ctx *ctx, const int32_t *ks);

/* Generates the cloud key ON THE DEVICE and loads it: BootstrapKey = tgsw_encrypt(s_i) for every bit of the LWE key
 * (bootstrap.jl:6-15, tgsw.jl:52-88, tlwe.jl:63-73) and KeyswitchKey (keyswitch.jl:14-41, lwe.jl:49-55) — the work
 * CloudKey(rng, secret_key) does on the host (api.jl:111-127).  lwe_key: [n] words 0/1 (SecretKey.key, lwe.jl:11-17);
 * tlwe_key: [k][N] words 0/1 (TLweKey, tlwe.jl:11-21); the noise parameters are bs_noise_stddev / ks_noise_stddev of
 * SchemeParameters (api.jl:4-21).  Randomness is Philox4x32-10 (csrc/kernels_keygen.hpp documents the streams; the
 * reference's MersenneTwister stream is not reproduced) keyed by `seed`, SIX 32-bit words: seed[0..1] key the mask
 * words, which the cloud key publishes anyway; seed[2..5] are 128 bits that key the noise and are AS SECRET AS THE SECRET
 * KEY (with them every noise term can be subtracted and the keys solved for): draw them from a cryptographic source, keep
 * them with the secret key or discard them, never with the cloud key.  The call uploads the secret key bits to the
 * device for its duration (the context therefore sees the secret key); the scratch copies and the raw noise are zeroed
 * before their memory is released.  bk_out / ks_out (either may be NULL) receive the canonical Int32 arrays,
 * [n][l][k+1][k+1][N] and [kN][t][base-1][n+1], e.g. to serialise the key.
 * Single-key contexts; a multi-device context generates on its first device and replicates through a host copy. */
int32_t tfhe_keygen_cloud_key(tfhe_ctx *ctx, const int32_t *lwe_key, const int32_t *tlwe_key, double bs_noise_stddev,
                              double ks_noise_stddev, const uint32_t *seed /* [6] */, int32_t *bk_out, int32_t *ks_out);

/* ---- host buffers ---------------------------------------------------------------------------- */

/* Page-locked host memory for the operands and results of the host-buffer batch calls below.  Any host pointer works
 * with them; from pageable memory the runtime stages every copy through its own pinned bounce buffers at roughly half
 * the PCIe rate, from memory allocated here the copies are single DMA transfers (8.2 MB per operand of a 4096-gate
 * batch at the 80-bit set).  Not tied to a context; free with tfhe_host_free. */
int32_t tfhe_host_alloc(size_t bytes, void **out_ptr);
void tfhe_host_free(void *ptr);

/* ---- the hot path --------------------------------------------------------------------------- */

/* B independent gates: out[g] = gate_<opcode[g]>(ck, in0[g], in1[g], in2[g])   (gates.jl:15-177).
 * in0/in1/in2/out: host int32 [B][n+1].  in1 may be NULL if no opcode reads a 2nd operand,
 * in2 may be NULL if no opcode is MUX. */
int32_t tfhe_gates_batch(tfhe_ctx *ctx, const uint8_t *opcodes, const int32_t *in0, const int32_t *in1,
                         const int32_t *in2, int32_t *out, int64_t B);

/* The streaming form of tfhe_gates_batch, for a caller that feeds batch after batch from host memory: submit enqueues the
 * upload, the kernels and the download of one batch and returns; wait blocks until that batch's `out` is complete.  A
 * context runs up to two submitted batches at a time, on two streams taken in turn, so that the upload of batch i + 1
 * runs under the kernels of batch i and the download of batch i under the kernels of batch i + 1 (the PCIe time of
 * the synchronous call — ~0.7 ms of a 12 ms 4096-gate batch — disappears from the steady state); submitting a third
 * batch first waits for the oldest.  in0/in1/in2/out must stay valid and untouched until the batch has been waited
 * for, and should come from tfhe_host_alloc: the runtime stages copies from pageable memory synchronously, which
 * overlaps nothing.  `opcodes` is read before submit returns.  *ticket identifies the batch for tfhe_gates_batch_wait
 * (waiting twice, or for a batch a later submit already displaced, is harmless).  On a multi-device context every device
 * takes its shard as a submit of its own.  Contexts that cannot run two batches side by side (multi-key, measure_margin)
 * complete the batch inside submit.  The timing queries below see only the batches that ran on the context's own stream
 * (every other one). */
int32_t tfhe_gates_batch_submit(tfhe_ctx *ctx, const uint8_t *opcodes, const int32_t *in0, const int32_t *in1,
                                const int32_t *in2, int32_t *out, int64_t B, int32_t *ticket);
/* wait: callable from any thread (ABI v7).  From the thread that submitted, it waits for the ticket and releases its slot.  From any
 * other thread it never takes the context — it cannot make the submitting thread's calls fail — and waits for everything queued
 * on ctx (tfhe_ctx_synchronize); the slot is released by the submitting thread's next submit or wait. */
int32_t tfhe_gates_batch_wait(tfhe_ctx *ctx, int32_t ticket);

/* Same with DEVICE pointers for in0/in1/in2/out (opcodes stay a host array) on HIP stream `stream`
 * (a hipStream_t, NULL = the context's own stream).  Asynchronous with respect to the host except
 * for the upload of the B opcode bytes; results are ordered on `stream`.  The context's workspaces are shared by
 * all calls: every batch call records a context-owned event at its end and the next call makes its own stream wait
 * for it (device-side ordering; the host does not block and no handle of the caller's stream is kept). */
int32_t tfhe_gates_batch_dev(tfhe_ctx *ctx, const uint8_t *opcodes, const int32_t *d_in0,
                             const int32_t *d_in1, const int32_t *d_in2, int32_t *d_out, int64_t B,
                             void *stream);

/* ---- levelised circuits on device-resident ciphertexts ----------------------------------------------
 * The caller side of the path (examples/tutorial.jl:42-62 is a 16-deep XNOR->MUX chain followed by 16
 * parallel MUXes): ciphertexts stay in a device-resident table of `num_wires` LWE samples and each call
 * runs ONE level of independent gates addressed by wire index, so nothing crosses PCIe between levels. */

/* (Re)allocates the context's wire table: int32 [num_wires][n+1] on the device (0 frees it); multi-key rows:
 * tfhe_mk_wires_alloc.  Upload, download and gather move rows of the width the table was allocated with. */
int32_t tfhe_wires_alloc(tfhe_ctx *ctx, int64_t num_wires);
/* Copies `count` samples (host int32 [count][n+1]) into / out of wires [first, first+count). */
int32_t tfhe_wires_upload(tfhe_ctx *ctx, int64_t first, int64_t count, const int32_t *host);
int32_t tfhe_wires_download(tfhe_ctx *ctx, int64_t first, int64_t count, int32_t *host);
/* host[i] = wire[wires[i]] for i < count: any set of wires in ONE device gather + ONE copy (the outputs of a circuit). */
int32_t tfhe_wires_gather(tfhe_ctx *ctx, const int32_t *wires, int64_t count, int32_t *host);
/* wire[out[g]] = gate_<opcode[g]>(ck, wire[a[g]], wire[b[g]], wire[c[g]]) for g < B (host index arrays; b / c
 * may be NULL if no opcode reads them).  A level must not read a wire it writes, nor write a wire twice
 * (TFHE_ERR_INVALID_ARG).  Asynchronous: returns when the level is queued on the context's stream (multi-device context: on
 * every participating device's stream, the exchange of operand rows between devices included); ordered with later calls. */
int32_t tfhe_gates_level(tfhe_ctx *ctx, const uint8_t *opcodes, const int32_t *a, const int32_t *b,
                         const int32_t *c, const int32_t *out, int64_t B);
/* Programmable bootstrapping on the wire table (addition within ABI v7).  For every row g < B:
 *   x_g = sum over t in [term_start[g], term_start[g+1]) of term_coef[t] * wire[term_wire[t]], plus cst[g] on the body (mod 2^32)
 *   wire[out[g*n_out + j]] = keyswitch of the sample extracted at coefficient j N / n_out of the blind rotation of x_g
 *                            with test polynomial tv[tv_index[g]],   j < n_out
 * n_out, tv, n_tv, tv_index (NULL: table 0 for every row): as tfhe_bootstrap_tv_multi_batch.  cst may be NULL (all zero).
 * term_start: host int32 [B+1], from 0, never decreasing (a row without terms is the trivial sample (0, cst[g])); term_wire,
 * term_coef: [term_start[B]]; out: [B*n_out].  Every index inside the table, no output wire written twice, no term reading a wire
 * the call writes (TFHE_ERR_INVALID_ARG).  Asynchronous as tfhe_gates_level: every host array is staged before the call returns,
 * so the caller may reuse them at once.  TFHE_ERR_STATE: a multi-key context or wire table, no wire table, measure_margin on;
 * TFHE_ERR_NO_KEY: bootstrapping or keyswitch key missing.  tfhe_last_rotation_count reports B.  A multi-device context runs a
 * level below "level_split_min" rows on its first device and cuts a wider one into equal contiguous shards, as tfhe_gates_level. */
int32_t tfhe_lut_level(tfhe_ctx *ctx, const int32_t *tv, int32_t n_tv, const int32_t *tv_index, int32_t n_out,
                       const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef, const int32_t *cst,
                       const int32_t *out, int64_t B);
/* wire[out[g]] = x_g as above, with no bootstrap (exact mod-2^32 arithmetic: LweSampleArray's +, integer scale, add_constant).
 * Arguments, checks, errors (but TFHE_ERR_NO_KEY and measure_margin) and asynchrony as tfhe_lut_level. */
int32_t tfhe_linear_level(tfhe_ctx *ctx, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                          const int32_t *cst, const int32_t *out, int64_t B);

/* bootstrap(bk, ks, mu, x) (bootstrap.jl:92-95) if with_keyswitch != 0, else
 * bootstrap_wo_keyswitch(bk, mu, x) (bootstrap.jl:69-82).
 * in: host int32 [B][n+1]; out: host int32 [B][n+1] or [B][k*N+1]. */
int32_t tfhe_bootstrap_batch(tfhe_ctx *ctx, int32_t mu, const int32_t *in, int32_t *out, int64_t B,
                             int32_t with_keyswitch);

/* Programmable bootstrapping (addition within ABI v7).
 * blind_rotate_and_extract(v, bk, barb, bara) (bootstrap.jl:50-59) after the modulus switch of bootstrap_wo_keyswitch
 * (bootstrap.jl:69-82) with testvect = tv[tv_index[g]] instead of repeat([mu], N); keyswitched (bootstrap.jl:92-95)
 * if with_keyswitch != 0.  tv: host int32 [n_tv][N]; tv_index: host int32 [B] in [0, n_tv), or NULL = table 0 for every row.
 * in: host int32 [B][n+1]; out: host int32 [B][n+1] or [B][k*N+1].
 * Row g's body is v[phi] for phi in [0, N) and -v[phi - N] for phi in [N, 2N), phi = barb - sum(bara_i s_i) mod 2N.
 * TFHE_ERR_INVALID_ARG: a NULL buffer, n_tv < 1 or an index outside [0, n_tv) (checked before anything is uploaded; the message
 * names the first bad row); TFHE_ERR_STATE: a multi-key context, or measure_margin on (no DIAG form of these kernels);
 * TFHE_ERR_NO_KEY: keys not loaded.  A multi-device context splits the rows; every device receives all tables. */
int32_t tfhe_bootstrap_tv_batch(tfhe_ctx *ctx, const int32_t *tv, int32_t n_tv, const int32_t *tv_index,
                                const int32_t *in, int32_t *out, int64_t B, int32_t with_keyswitch);

/* Multi-output programmable bootstrapping (addition within ABI v7): tfhe_bootstrap_tv_batch returning n_out samples per row, from
 * ONE blind rotation.  Sample j of row g is tlwe_extract_sample (tlwe.jl:55-59) of the final accumulator at coefficient
 * c_j = j N / n_out instead of 0: mask polynomial i = X^{c_j} times mask polynomial i of the index-0 extraction (a[u] = e[u - c_j] for
 * u >= c_j, -e[N + u - c_j] for u < c_j), body = coefficient c_j of the accumulator's body; each is keyswitched if with_keyswitch.
 * Sample 0 is tfhe_bootstrap_tv_batch's result.  Its body is v[phi + c_j] for phi + c_j < N: a table packing f_j(m) at window
 * j p + m of Z_{p n_out} gives f_j(m) for a message m of Z_p encrypted in Z_{p n_out} (tfhe_jl_amd.lut, make_multi_test_vector).
 * out: host int32 [B][n_out][n+1], or [B][n_out][k*N+1] without keyswitch.  n_out: a power of two, 1 <= n_out <= 32, and n_out = 1
 * or n_out <= N/4, else TFHE_ERR_INVALID_ARG before anything is uploaded.  Other arguments and errors as tfhe_bootstrap_tv_batch;
 * tfhe_last_rotation_count reports B. */
int32_t tfhe_bootstrap_tv_multi_batch(tfhe_ctx *ctx, const int32_t *tv, int32_t n_tv, const int32_t *tv_index, int32_t n_out,
                                      const int32_t *in, int32_t *out, int64_t B, int32_t with_keyswitch);

/* keyswitch(ks, sample) (keyswitch.jl:45-80). in: host int32 [B][k*N+1]; out: host int32 [B][n+1]. */
int32_t tfhe_keyswitch_batch(tfhe_ctx *ctx, const int32_t *in, int32_t *out, int64_t B);

/* ---- multi-key (mk_gates.jl:7-12, mk_internals.jl:348-411,464-515) --------------------------- */

/* MKBootstrapKey from Int32 [P][n][2*l*P + 2*l][N] (see top of file); 2 <= P <= the context's `parties` (mk_api.jl:94). */
int32_t tfhe_mk_load_bootstrap_key_i32(tfhe_ctx *ctx, const int32_t *bk, int32_t parties);
/* The same key in the form the reference stores it (MKBootstrapKey.key[j, i] :: MKTransformedTGswExpSample,
 * mk_internals.jl:274-288,442-461): complex128 [P][n][2*l*P + 2*l][N/2] spectra of polynomials.jl:106-112.  Loading
 * is a permutation into the engine's order plus the 1/M scaling: nothing is re-transformed or rounded. */
int32_t tfhe_mk_load_bootstrap_key_c128(tfhe_ctx *ctx, const double *bk_spectra, int32_t parties);
/* MKBootstrapKey built ON THE DEVICE from what the parties publish: RGSW.Expand (mk_tgsw_expand, mk_internals.jl:304-345)
 * of every party's uni-encrypted key bits against all public keys, then the forward transform (MKBootstrapKey,
 * :442-461).  pub_b: Int32 [P][l][N] (PublicKey.b, :116-139); c0, c1, d0, d1, f0, f1: Int32 [P][n][l][N]
 * (MKTGswUESample of bit j of party i, :185-227).  The host only decomposes the public-key differences; the
 * P (P-1) n l^2 polynomial products run on the GPU (exact, like the external product).  If expanded_out is not NULL it
 * receives the expanded key in the Int32 layout tfhe_mk_load_bootstrap_key_i32 takes ([P][n][2 l P + 2 l][N]). */
int32_t tfhe_mk_expand_load_bootstrap_key(tfhe_ctx *ctx, int32_t parties, const int32_t *pub_b, const int32_t *c0,
                                          const int32_t *c1, const int32_t *d0, const int32_t *d1, const int32_t *f0,
                                          const int32_t *f1, int32_t *expanded_out);
/* P single-key KeyswitchKeys back to back, each [N][t][base-1][n+1]; any base and length (mk_internals.jl:397-411 calls the
 * single-key keyswitch per party). */
int32_t tfhe_mk_load_keyswitch_key(tfhe_ctx *ctx, const int32_t *ks, int32_t parties);
/* out[g] = mk_gate_nand(ck, in0[g], in1[g]); all host int32 [B][P*n+1]. */
int32_t tfhe_mk_gate_nand_batch(tfhe_ctx *ctx, const int32_t *in0, const int32_t *in1, int32_t *out,
                                int64_t B);

/* Multi-key gate set and multi-key circuits: additions within ABI v7 (a library that exports them still reports 7).
 * Every opcode of tfhe_gates_batch over multi-key samples (gates.jl's formulas, the constants as mk_lwe_noiseless_trivial,
 * mk_gates.jl:8-10 for NAND): each bootstrapped gate is ONE multi-key blind rotation with mu = 1/8 and one multi-key
 * keyswitch; MUX is two rotations whose extracted samples are summed, (0, 1/8) added once, then one keyswitch; NOT / COPY /
 * CONST0 / CONST1 bootstrap nothing (constants: all-zero masks, b = +-1/8).
 * out[g] = gate_<opcodes[g]>(in0[g], in1[g], in2[g]); host int32 [B][P*n+1], P = the parties of the loaded multi-key keys.
 * TFHE_ERR_STATE on a single-key context, TFHE_ERR_NO_KEY without multi-key keys.  A multi-device context splits the batch
 * by rotations (tfhe_shard_bounds; MUX counts two). */
int32_t tfhe_mk_gates_batch(tfhe_ctx *ctx, const uint8_t *opcodes, const int32_t *in0, const int32_t *in1,
                            const int32_t *in2, int32_t *out, int64_t B);
/* (Re)allocates the context's wire table with multi-key rows: int32 [num_wires][P*n+1], P = the parties of the loaded
 * multi-key bootstrapping key, fixed for the table's lifetime.  tfhe_wires_upload / _download / _gather then move rows of
 * that width; tfhe_wires_alloc makes a single-key table again.  TFHE_ERR_NO_KEY without a multi-key bootstrapping key;
 * TFHE_ERR_STATE on a single-key or a multi-device context (multi-key tables are single-device). */
int32_t tfhe_mk_wires_alloc(tfhe_ctx *ctx, int64_t num_wires);
/* tfhe_gates_level on the multi-key wire table: same index arrays, checks and asynchrony.  TFHE_ERR_STATE on a single-key
 * table, or when the keys now loaded are for a party count other than the table's. */
int32_t tfhe_mk_gates_level(tfhe_ctx *ctx, const uint8_t *opcodes, const int32_t *a, const int32_t *b,
                            const int32_t *c, const int32_t *out, int64_t B);

/* Multi-key programmable bootstrapping (additions within ABI v7): tfhe_bootstrap_tv_batch / tfhe_bootstrap_tv_multi_batch on
 * multi-key samples.  The multi-key blind rotation (mk_internals.jl:464-495) starts its body polynomial from X^{-barb} tv[tv_index[g]]
 * instead of X^{-barb} (mu, ..., mu) (the masks from zero); sample j of row g is mk_tlwe_extract_sample (mk_internals.jl:88-95) at
 * coefficient j N / n_out, then mk_keyswitch (mk_internals.jl:397-411) if with_keyswitch.  in: host int32 [B][P*n+1]; out: host
 * int32 [B][n_out][P*n+1], or [B][n_out][P*N+1] without keyswitch.  Tables, tv_index, n_out and TFHE_ERR_INVALID_ARG as the
 * single-key pair (checked before anything is uploaded).  TFHE_ERR_STATE: a single-key context, measure_margin on, or (with
 * keyswitch) keys loaded for different party counts; TFHE_ERR_NO_KEY: multi-key keys not loaded.  A multi-device context splits
 * the rows; every device receives all tables.  The single-key entry points keep refusing multi-key contexts. */
int32_t tfhe_mk_bootstrap_tv_batch(tfhe_ctx *ctx, const int32_t *tv, int32_t n_tv, const int32_t *tv_index,
                                   const int32_t *in, int32_t *out, int64_t B, int32_t with_keyswitch);
int32_t tfhe_mk_bootstrap_tv_multi_batch(tfhe_ctx *ctx, const int32_t *tv, int32_t n_tv, const int32_t *tv_index, int32_t n_out,
                                         const int32_t *in, int32_t *out, int64_t B, int32_t with_keyswitch);
/* tfhe_lut_level / tfhe_linear_level on the multi-key wire table (rows [P*n+1]; the multi-key rotation and keyswitch): same index
 * arrays, checks, staging and asynchrony.  TFHE_ERR_STATE on a single-key context or table, measure_margin on (LUT form), or (LUT
 * form) when the keys now loaded are for a party count other than the table's; TFHE_ERR_NO_KEY (LUT form): multi-key keys missing. */
int32_t tfhe_mk_lut_level(tfhe_ctx *ctx, const int32_t *tv, int32_t n_tv, const int32_t *tv_index, int32_t n_out,
                          const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef, const int32_t *cst,
                          const int32_t *out, int64_t B);
int32_t tfhe_mk_linear_level(tfhe_ctx *ctx, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                             const int32_t *cst, const int32_t *out, int64_t B);

/* ---- leveled mode: external products and CMUX trees on the caller's own samples (additions within ABI v7) ------------
 * The blind rotation applies the external product to the bootstrapping key alone.  These entry points apply it to TGSW and TLWE
 * samples the caller made: a 2^depth-entry table of TLWE samples is folded by depth levels of CMUXes d0 + C (.) (d1 - d0) (the
 * form of bootstrap.jl:19-23) down to the entry that `depth` TGSW-encrypted address bits name, at 2^depth - 1 external products
 * and no blind rotation; the result can leave as an LWE sample under the gate key and go into tfhe_gates_batch.
 * Formats: TLWE sample int32 [k+1][N] = a[0..k-1], b (tlwe.jl:34-41); TGSW sample int32 [l][k+1][k+1][N] = samples[p, j].a[c]
 * (tgsw.jl:25-32), exactly one entry of the bootstrapping key's canonical form.  One kernel (csrc/kernels_leveled.hpp) serves every
 * parameter set a context accepts; tfhe_last_kernel_name reports "cmux_level_kernel(N=..,k=..,l=..[,spec=global])" (the option "anyn_spec"
 * = 1 puts the spectrum accumulators in global memory, as for the network kernels; the multi-key tree kernel reads it the same way).
 * Exactness: as the rotation, (k+1) l digit-by-selector products are summed in Float64 before the one rounding per coefficient:
 * "exact_domain" (tfhe_get_option) applies unchanged, with the selector words in the place of the key words.
 * All three follow the one-caller-at-a-time rule and return TFHE_ERR_STATE on a multi-key context and on a multi-device context
 * (leveled operations on several devices are out of scope: use one device context per GPU); the two batch calls also with
 * measure_margin on (no DIAG form of the kernel).  tfhe_last_timing_ms: 0 = the CMUX levels, 1 = the keyswitch, 2 = both. */

/* forward_transform(::TGswSample) (tgsw.jl:120-121) for S samples, host int32 [S][l][k+1][k+1][N]: the selector set the two calls
 * below index.  Replaces any earlier set (the context is quiesced first).  TFHE_ERR_INVALID_ARG: NULL or S < 1; TFHE_ERR_NOMEM: the
 * set does not fit the device's free memory (nothing is loaded then). */
int32_t tfhe_tgsw_load(tfhe_ctx *ctx, const int32_t *tgsw, int64_t S);

/* tgsw_extern_mul(accum, gsw) (tgsw.jl:125-129) for B rows: tlwe_out[g] = selector[sel[g]] (.) tlwe_in[g].  tlwe_in / tlwe_out: host
 * int32 [B][k+1][N]; sel: host int32 [B] in [0, S).  TFHE_ERR_NO_KEY: no selector set; TFHE_ERR_INVALID_ARG: a selector out of
 * range (checked before anything is uploaded). */
int32_t tfhe_extern_mul_batch(tfhe_ctx *ctx, const int32_t *tlwe_in, const int32_t *sel, int32_t *tlwe_out, int64_t B);

/* CMUX tree.  data: host int32 [T][2^depth][k+1][N], T tables shared by the rows; row g folds table table_index[g] (host int32 [B] in
 * [0, T); NULL = table 0 for every row).  Level v (0 = the lowest address bit) replaces each pair (d0, d1) = entries (2i, 2i + 1)
 * by d0 + selector[sel[g][v]] (.) (d1 - d0)  (tgsw.jl:99-129, bootstrap.jl:19-23); sel: host int32 [B][depth] in [0, S).  After
 * depth levels one sample is left, entry sum_v bit_v 2^v of the table when selector sel[g][v] encrypts bit_v.
 * out_form 0: the TLWE sample, out int32 [B][k+1][N]; 1: tlwe_extract_sample at coefficient 0 (tlwe.jl:55-59), [B][k*N+1];
 * 2: that keyswitched (keyswitch.jl:45-80), [B][n+1], an LWE sample under the gate key.
 * Workspace: two device buffers of B 2^(depth-1) and B 2^(depth-2) TLWE samples plus the T tables, grown on demand and kept; the
 * sizes are compared with the device's free memory BEFORE anything is allocated: TFHE_ERR_NOMEM if they do not fit, the context
 * stays usable.  TFHE_ERR_INVALID_ARG: NULL buffer, depth outside 1 ... 12, T < 1, out_form outside 0 ... 2, a selector or table index
 * out of range (all checked in O(B depth) before anything is uploaded); TFHE_ERR_NO_KEY: no selector set, or out_form 2 without
 * the keyswitch key. */
int32_t tfhe_cmux_tree_batch(tfhe_ctx *ctx, const int32_t *data, int64_t T, const int32_t *table_index, int32_t depth,
                             const int32_t *sel, int32_t *out, int64_t B, int32_t out_form);

/* CMUX network (addition within ABI v7): the same CMUX wired by a public netlist instead of by halving — the backward evaluation of a
 * deterministic automaton or an ordered decision diagram on TGSW-encrypted variables.  The network is shared by all rows: `levels`
 * levels (1 ... 1024), level v with widths[v] nodes (1 ... 4096); nodes: host int32 [sum widths][3] = (src0, src1, var) in level order.
 * Node i of level v of row g is  in[src0] + selector[sel[g][var]] (.) (in[src1] - in[src0])  — a selector that encrypts 1 picks src1 —
 * where `in` is, for v = 0, the E TLWE samples of the row's table data[table_index[g]] (E >= 1, any count) and, for v > 0, the outputs
 * of level v - 1.  var indexes the row's V selectors, sel: host int32 [B][V] in [0, S), and is per node.  A node with src0 == src1 is
 * a copy: no product, no noise, the same words.  All F = widths[levels-1] nodes of the last level are outputs.
 * data: host int32 [T][E][k+1][N]; table_index: host int32 [B] in [0, T) or NULL = table 0.  out_form 0: out int32 [B][F][k+1][N];
 * 1: extracted at coefficient 0, [B][F][k*N+1]; 2: that keyswitched, [B][F][n+1].  One launch per level
 * (csrc/kernels_cmux_net.hpp; tfhe_last_kernel_name reports "cmux_net_level_kernel(N=..,k=..,l=..[,spec=global])", the option
 * "anyn_spec" = 1 puts the spectrum accumulators in global memory as for the any-N rotation).  A tree-shaped network equals
 * tfhe_cmux_tree_batch word for word.
 * Workspace: two device buffers of B max(widths of the even levels) and B max(widths of the odd levels) TLWE samples plus the T
 * tables; as above the sizes are compared with the device's free memory BEFORE anything is allocated (TFHE_ERR_NOMEM, the context
 * stays usable).  Everything is validated on the host in O(B V + nodes) before anything is uploaded, the message naming the
 * offender — TFHE_ERR_INVALID_ARG: NULL buffer, levels / a width / E / V / T out of range, a source negative or not below the width
 * of the level below (E at level 0), var outside [0, V), a selector or table index out of range, out_form outside 0 ... 2, B * width
 * above one launch; TFHE_ERR_NO_KEY: no selector set, or out_form 2 without the keyswitch key; TFHE_ERR_STATE as the calls above.
 * B = 0 returns TFHE_OK. */
int32_t tfhe_cmux_net_batch(tfhe_ctx *ctx, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths,
                            int32_t levels, const int32_t *nodes, const int32_t *sel, int32_t V, int32_t *out, int64_t B, int32_t out_form);

/* CMUX network with a public monomial on every edge (addition within ABI v7): tfhe_cmux_net_batch's contract with one difference, a node
 * record of five words, nodes: host int32 [sum widths][5] = (src0, src1, var, rot0, rot1).  Node i of level v of row g is
 *     X^rot0 in[src0] + selector[sel[g][var]] (.) (X^rot1 in[src1] - X^rot0 in[src0])
 * where X^r p is mul_by_monomial(p, r) (bootstrap.jl:21, :54) on every polynomial of the sample, mask and body: coefficient j moves to
 * j + r mod 2N and changes sign past N.  rot0, rot1 are public, in [0, 2N).  A node with src0 == src1 and rot0 == rot1 is a rotated
 * copy: no product, no noise, the exact words of X^rot0 in[src0].  A node with src0 == src1 and rot0 != rot1 is a true product:
 * CMUX(C_b; acc, X^(2N - 2^b) acc) for b = 0 ... r-1 rotates acc by minus an encrypted r-bit index (the blind rotation by TGSW bits),
 * which brings entry `index` of a table packed N entries to a sample to coefficient 0, where out_form 1 and 2 extract: a 2^d-entry
 * table costs 2^(d - log2 N) - 1 + log2 N external products per lookup instead of 2^d - 1.  X^w on the transitions of an automaton
 * gives weighted automata (output X^(sum of weights) table[end state]).  With every rotation 0 the call equals tfhe_cmux_net_batch
 * word for word.
 * Everything else is tfhe_cmux_net_batch's: the limits (1024 levels, width 4096, B * width within one launch), data, table_index, sel,
 * the three out_forms (extraction at coefficient 0), the two workspaces sized per level parity and TFHE_ERR_NOMEM before any
 * allocation, the order of the refusals, B = 0, the tfhe_last_timing_ms slots.  TFHE_ERR_INVALID_ARG also for a rotation outside
 * [0, 2N), the message naming node, level and field (rot0 / rot1), before anything is uploaded.  One launch per level
 * (csrc/kernels_rot_net.hpp; tfhe_last_kernel_name reports "rot_net_level_kernel(N=..,k=..,l=..[,spec=global])"; the option
 * "anyn_spec" is honoured). */
int32_t tfhe_rot_net_batch(tfhe_ctx *ctx, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths,
                           int32_t levels, const int32_t *nodes, const int32_t *sel, int32_t V, int32_t *out, int64_t B, int32_t out_form);

/* Blind rotation of the caller's TLWE accumulators (addition within ABI v7): blind_rotate (bootstrap.jl:26-41) on an accumulator the
 * caller supplies, returning the accumulator the caller asks for — the way from the bootstrapped half (gates, lookups: LWE samples) to
 * the leveled one.  For row g
 *     A_0 = X^(-barb_g) acc[acc_index[g]]                            on all k + 1 polynomials, the mask included
 *     A_(i+1) = A_i + selector[sel[i]] (.) (X^(e_g,i) A_i - A_i)     i = 0 ... steps - 1        (bootstrap.jl:19-23, :32-39)
 * with the selectors of tfhe_tgsw_load: an entry of the bootstrapping key in canonical form is a TGSW selector, so loading the key's n
 * entries (and address-bit selectors in the same set, if wanted) makes this the bootstrap's rotation, whichever kernel family serves
 * the gates.  With an encrypted test polynomial as acc the server evaluates a lookup table it cannot read; with the output of a CMUX
 * tree (out_form 0 there) as acc, a table of p 2^d entries is addressed in part by an LWE digit computed by gates; with out_form 0
 * here, a bootstrap's result leaves as a TLWE sample that tfhe_cmux_tree_batch / tfhe_cmux_net_batch accept as `data`.
 * acc: host int32 [T][k+1][N], TLWE samples, trivial or encrypted; acc_index: host int32 [B] in [0, T), or NULL = accumulator 0 for
 * every row.  rows: host int32 [B][steps+1], mask words then body; in_form 0: LWE samples under the key whose bits the selectors
 * encrypt, switched to Z_2N in the kernel (bootstrap.jl:74-75); in_form 1: the exponents themselves, every word in [0, 2N).  A zero
 * exponent adds exactly zero.  sel: host int32 [steps] in [0, S), shared by all rows, or NULL = selector i for step i.  steps: 1 ...
 * 65536.  out_form 0: the final accumulator, out int32 [B][k+1][N] (n_out must be 1); 1: for j < n_out its extraction at coefficient
 * j N / n_out (tfhe_bootstrap_tv_multi_batch's rule), [B][n_out][k*N+1]; 2: those keyswitched, [B][n_out][n+1].  n_out: a power of
 * two <= 32, and 1 or <= N / 4.  With acc = (0, tv), in_form 0, sel NULL and the bootstrapping key as selectors the call equals
 * tfhe_bootstrap_tv_multi_batch word for word; with B = 1 and out_form 0 it equals the tfhe_rot_net_batch chain "rotated copy by
 * 2N - barb, then `steps` levels of width 1 with records (0, 0, i, 0, e_i)" word for word, in one launch instead of steps + 1.
 * Noise: the accumulator's own noise passes through unrefreshed, and the rotation adds what a bootstrap's rotation adds.
 * One kernel, one workgroup per row (csrc/kernels_blind_rotate_tlwe.hpp; tfhe_last_kernel_name reports
 * "tlwe_rotate_kernel(N=..,k=..,l=..,steps=..[,spec=global])"; the option "anyn_spec" is honoured); tfhe_last_rotation_count = B;
 * tfhe_last_timing_ms: 0 = the rotation, 1 = the keyswitch, 2 = both.  Everything is validated on the host before anything is uploaded
 * — TFHE_ERR_INVALID_ARG: NULL buffer, B < 0, steps / in_form / out_form / T / n_out out of range, n_out != 1 with out_form 0, a
 * selector or accumulator index out of range, sel NULL with fewer than `steps` selectors loaded, with in_form 1 a word outside
 * [0, 2N) (the message names row and column); TFHE_ERR_NO_KEY: no selector set, or out_form 2 without the keyswitch key;
 * TFHE_ERR_STATE: a multi-key context, a multi-device context, measure_margin on.  The workspaces (the T accumulators, two samples
 * per row, the rows, the extractions) are compared with the device's free memory BEFORE anything is allocated: TFHE_ERR_NOMEM, the
 * context stays usable.  B = 0 returns TFHE_OK.  The multi-key form is tfhe_mk_blind_rotate_batch below.  The form on the gates'
 * own kernel and key layout is tfhe_bootstrap_acc_batch below (N = 1024, k = 1); this call reads the selector set alone. */
int32_t tfhe_blind_rotate_batch(tfhe_ctx *ctx, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t steps,
                                int32_t in_form, const int32_t *sel, int32_t n_out, int32_t *out, int64_t B, int32_t out_form);

/* ---- leveled mode on device-resident tables (additions within ABI v7) -----------------------------------
 * The leveled half's own table beside the wire table: TLWE samples that stay on the device between leveled calls, and level calls
 * that read and write both tables, so that a program of gates, private lookups and gates crosses PCIe only at its ends.  No new
 * cryptography, no new key material: every result equals, word for word, the host-buffer batch call above on the same samples.
 * Single-key, one-device contexts only (TFHE_ERR_STATE otherwise).
 *
 * tfhe_tlwe_alloc: a device table int32 [slots][k+1][N]; slots = 0 frees it; reallocating discards the old contents.  The size is
 * compared with the device's free memory (the table being replaced counted as free) before anything is freed or allocated:
 * TFHE_ERR_NOMEM, the context and its present table stay as they were.  Waits for the levels queued on the context.
 * tfhe_tlwe_upload / tfhe_tlwe_download: slots [first, first + count) from / to host int32 [count][k+1][N], ordered behind the levels
 * queued on the context; both return with the copy done.  TFHE_ERR_STATE without a table, TFHE_ERR_INVALID_ARG for a range outside
 * it or a NULL buffer with count > 0. */
int32_t tfhe_tlwe_alloc(tfhe_ctx *ctx, int64_t slots);
int32_t tfhe_tlwe_upload(tfhe_ctx *ctx, int64_t first, int64_t count, const int32_t *host);
int32_t tfhe_tlwe_download(tfhe_ctx *ctx, int64_t first, int64_t count, int32_t *host);

/* Replaces selectors [first, first + count) of the set tfhe_tgsw_load loaded, in place: tgsw is int32 [count][l][k+1][k+1][N]; every
 * other selector keeps its exact words, and the replaced ones are what a fresh tfhe_tgsw_load of the edited set would hold.  For a
 * set "the key's n selectors, then a request's address bits": the key is loaded once and the address bits are swapped behind it.
 * Waits for the work queued on the context first.  TFHE_ERR_NO_KEY: no set loaded; TFHE_ERR_INVALID_ARG: NULL pointer, count < 1, a
 * range outside [0, S); TFHE_ERR_STATE: a multi-key or multi-device context. */
int32_t tfhe_tgsw_update(tfhe_ctx *ctx, const int32_t *tgsw, int64_t first, int64_t count);

/* tfhe_rot_net_batch between the tables.  Level 0 of row g reads source `src` at TLWE slot table_first[g] + src (table_first: host
 * int32 [B]; NULL = 0 for every row, so src is an absolute slot); the network (E, widths, levels, nodes, sel, V) is that call's.
 * out_form 0: output node i of row g goes to slot out_first + g F + i (F = widths[levels-1]); the range must lie inside the table and
 * must not meet any row's read range [table_first[g], + E).  out_form 2: the sample extracted at coefficient 0 and keyswitched goes
 * to wire out_wires[g F + i] (host int32 [B F]) of the single-key wire table; no wire may be named twice.  out_form 1 is refused
 * (extracted rows have no table).  The words equal tfhe_rot_net_batch on the same samples — with every rotation 0 that is
 * tfhe_cmux_net_batch, with a tree's netlist tfhe_cmux_tree_batch: one level call covers all three.  The same kernel
 * (rot_net_level_kernel), unchanged; timing slots and tfhe_last_kernel_name as tfhe_rot_net_batch.
 *
 * tfhe_blind_rotate_batch between the tables.  Row g's rotating sample is formed exactly as tfhe_lut_level forms it,
 *     x_g = sum over t in [term_start[g], term_start[g+1]) of term_coef[t] * wire[term_wire[t]], plus cst[g] on the body   (mod 2^32)
 * (cst NULL: 0; a row without terms is the trivial sample), read as in_form 0 with steps = the context's n;
 * A_0 = X^(-barb_g) slot[acc_slot[g]] (host int32 [B]; slots may repeat); sel: host int32 [n] or NULL, as in the batch call.
 * out_form 0 (n_out must be 1): the final accumulator goes to slot out_slot[g] (host int32 [B]); the slots must be distinct and none
 * may be an acc_slot of the same call.  out_form 2: the n_out extractions, keyswitched, go to wires out_wires[g n_out + j] (host int32
 * [B n_out]); no wire may be named twice and none may be a term wire of the same call.  The unused one of out_slot / out_wires may
 * be NULL.  The words equal tfhe_blind_rotate_batch(acc = those slots' samples, rows = x_g, steps = n, in_form 0, sel, n_out,
 * out_form).  tfhe_lut_level's prologue stages the rows (linear_prologue_kernel), then one kernel, one workgroup per row
 * (csrc/kernels_tlwe_levels.hpp; tfhe_last_kernel_name reports "tlwe_rotate_level_kernel(N=..,k=..,l=..,steps=..[,spec=global])";
 * "anyn_spec" is honoured); tfhe_last_rotation_count = B; tfhe_last_timing_ms as the batch call.
 *
 * Both level calls: everything is validated on the host before anything is uploaded or written, the message names the offender, and
 * a refused call changes no slot and no wire.  In this order — TFHE_ERR_STATE: a multi-key context, a multi-device context,
 * measure_margin on, no TLWE table, no wire table when out_form 2 or terms need one, a wire table with multi-key rows;
 * TFHE_ERR_INVALID_ARG: everything about the arguments; TFHE_ERR_NO_KEY: no selector set, or out_form 2 without the keyswitch key
 * (a selector index is checked against the loaded set after that).  The workspaces are compared with the device's free memory
 * before anything is allocated (TFHE_ERR_NOMEM, the context stays usable).  B = 0 returns TFHE_OK.  The calls are ordered behind
 * the asynchronous levels queued on the context (tfhe_gates_level, tfhe_lut_level, ...) and SYNCHRONISE before they return: the
 * slots and wires they wrote are complete, and the caller's arrays are free, on return. */
int32_t tfhe_rot_net_level(tfhe_ctx *ctx, const int32_t *table_first, int32_t E, const int32_t *widths, int32_t levels, const int32_t *nodes,
                           const int32_t *sel, int32_t V, int32_t out_form, int64_t out_first, const int32_t *out_wires, int64_t B);
int32_t tfhe_blind_rotate_level(tfhe_ctx *ctx, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire,
                                const int32_t *term_coef, const int32_t *cst, const int32_t *sel, int32_t n_out, int32_t out_form,
                                const int32_t *out_slot, const int32_t *out_wires, int64_t B);

/* The same two rotations on the gates' own kernel and key (additions within ABI v7): tfhe_blind_rotate_batch and
 * tfhe_blind_rotate_level with steps = the context's n, in_form 0 and sel NULL, run by the ACC form of the one-wave-per-rotation
 * kernel of the gates (csrc/kernels_v3.hpp, compiled a third time in csrc/engine_bootstrap_acc.hip): the accumulator stays in LDS for
 * all n steps and a row costs one wave, not one workgroup.  The calls read the context's bootstrapping key in the layout the gates
 * read (tfhe_load_bootstrap_key_*, tfhe_keygen_cloud_key); they need no selector set and leave a loaded one alone.  The result
 * equals, word for word, that of tfhe_blind_rotate_batch(acc, T, acc_index, rows, steps = n, in_form 0, sel NULL, n_out, out, B,
 * out_form), respectively tfhe_blind_rotate_level(..., sel NULL, ...), where the selector set holds the loaded bootstrapping key's n
 * entries in order.
 * Buffer shapes (acc, acc_index, out), the n_out rule, the out_forms 0 / 1 / 2 and, for the level call, the terms, the slot, wire and
 * overlap rules are those of tfhe_blind_rotate_batch and tfhe_blind_rotate_level above.  rows: host int32 [B][n+1], LWE samples, staged
 * by tfhe_bootstrap_tv_batch's modulus switch; the level call's rows by tfhe_lut_level's prologue, as tfhe_blind_rotate_level's.
 * Geometry: the gates' — four rotations per workgroup from 6 rotations per CU up (option "v3_rw": 0 = by batch size, 1, 4), the
 * l = 2 and l = 3 instantiations and the run-time-l one for every other l (option "br_rt_l").  tfhe_last_kernel_name reports
 * "blind_rotate_kernel_v3_acc<L,8,tw2reg[,rw4]>" ("<0,...>(l=..)" for the run-time-l form); tfhe_last_rotation_count = B;
 * tfhe_last_timing_ms: 0 = the rotation, 1 = the keyswitch, 2 = both.
 * Everything is validated on the host before anything is uploaded, and a refused call changes no slot and no wire.  TFHE_ERR_STATE:
 * a multi-key context, a multi-device context, measure_margin on (the level call: and a missing or unfit table, as
 * tfhe_blind_rotate_level), then a shape the kernel does not serve (N != 1024 or k != 1) or a key that is not in its layout (option
 * "br_anyn") — the message names the shape and points to tfhe_blind_rotate_batch; TFHE_ERR_INVALID_ARG: as the two calls above;
 * TFHE_ERR_NO_KEY: no bootstrapping key, or out_form 2 without the keyswitch key; TFHE_ERR_NOMEM: the workspaces compared with the
 * device's free memory before anything is allocated.  B = 0 returns TFHE_OK.  tfhe_get_option(ctx, "bootstrap_acc") answers 1
 * where the context's shape and key layout are served, 0 otherwise.
 * Option "acc_dispatch" (tfhe_set_option; 0 or 1, anything else TFHE_ERR_INVALID_ARG; default 0 = everything above): with 1 both calls
 * choose kernel and geometry by batch size as a gate batch of B rotations does, under the same options ("br_tiny", "br_small",
 * "br_rt_l", "w2_rw", "v3_rw", "br_split"): up to br_tiny rows (one per CU; l = 2, 3) the ACC form of the 4 l-wave kernel,
 * "blind_rotate_kernel_h2_acc<L>"; up to br_small rows (four per CU) that of the two-wave kernel,
 * "blind_rotate_kernel_w2_acc<L[,rw2]>"; above, the one-wave form; and a batch above 8 rows per CU whose last round is at most
 * br_small rows is two launches on the context's stream, "blind_rotate_kernel_v3_acc<..> + blind_rotate_kernel_w2_acc<..>" (or
 * h2_acc).  The words, the checks, the refusals and the timing slots do not depend on the option (csrc/engine_bootstrap_acc_small.hip).
 * Out of scope: k = 2, N = 512 and N = 2048.  The multi-key forms are tfhe_mk_bootstrap_acc_batch / _level, further down. */
int32_t tfhe_bootstrap_acc_batch(tfhe_ctx *ctx, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t n_out,
                                 int32_t out_form, int32_t *out, int64_t B);
int32_t tfhe_bootstrap_acc_level(tfhe_ctx *ctx, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire,
                                 const int32_t *term_coef, const int32_t *cst, int32_t n_out, int32_t out_form, const int32_t *out_slot,
                                 const int32_t *out_wires, int64_t B);

/* ---- leveled mode under a multi-key cloud key (additions within ABI v7) ---------------------------------
 * The same two operations on multi-key samples, with no blind rotation: the selectors are the parties' uni-encryptions of address
 * bits (mk_tgsw_encrypt, RGSW.UniEnc, mk_internals.jl:185-227) expanded against all public keys (mk_tgsw_expand, :304-345), the
 * product is mk_tgsw_extern_mul (:348-391) — which the reference applies to the bootstrapping key only — on the caller's own
 * MKTLweSample (:46-57; tlwe_mask_size = 1, :89-90).  P = the parties of the loaded multi-key bootstrapping key, per = 2 l P + 2 l.
 * One-device multi-key contexts only: TFHE_ERR_STATE on a single-key context (its calls are the three above, which in turn keep
 * refusing a multi-key context), on a multi-device context, and with "measure_margin" on; TFHE_ERR_NO_KEY without the multi-key
 * bootstrapping key or without a selector set.  Same exactness domain as the multi-key rotation: (P + 1) l products per rounding.
 * tfhe_last_kernel_name: "mk_cmux_level_kernel(N=..,P=..,l=..[,spec=global])"; tfhe_last_timing_ms: 0 = levels, 1 = keyswitch, 2 = both.
 *
 * The selector set.  tgsw: host int32 [S][per][N], S expanded samples (MKTGswExpSample, :243-271), each laid out exactly as one
 * (party, bit) entry of tfhe_mk_load_bootstrap_key_i32: x [l][P], y [l][P], c0 [l], c1 [l]; party_of: host int32 [S] in [0, P), the
 * party whose expansion sample s is.  Forward-transformed once (forward_transform(::MKTGswExpSample), :291-301) into the any-N
 * kernels' spectrum order whichever kernel family serves the rotation; replaces any earlier multi-key selector set; a multi-key
 * bootstrapping key loaded later for ANOTHER party count drops it.  `parties` must equal P: TFHE_ERR_STATE otherwise.
 * TFHE_ERR_INVALID_ARG: NULL pointer, S < 1, a party_of entry out of range (checked before anything is uploaded). */
int32_t tfhe_mk_tgsw_load(tfhe_ctx *ctx, const int32_t *tgsw, const int32_t *party_of, int64_t S, int32_t parties);

/* The same store built on the device from what the parties publish (mk_tgsw_expand, mk_internals.jl:304-345, for S samples): pub_b
 * host int32 [P][l][N] (PublicKey.b, :116-139); c0, c1, d0, d1, f0, f1 host int32 [S][l][N], sample s uni-encrypted by party
 * party_of[s].  The selectors are grouped by party and every group runs the expand path of tfhe_mk_expand_load_bootstrap_key with the
 * group's size in the place of n.  expanded_out: NULL, or host int32 [S][per][N] receiving the expanded samples in the caller's
 * order — word for word what a host expansion followed by tfhe_mk_tgsw_load holds. */
int32_t tfhe_mk_tgsw_expand_load(tfhe_ctx *ctx, int32_t parties, const int32_t *pub_b, const int32_t *party_of, const int32_t *c0,
                                 const int32_t *c1, const int32_t *d0, const int32_t *d1, const int32_t *f0, const int32_t *f1, int64_t S,
                                 int32_t *expanded_out);

/* tlwe_out[g] = mk_tgsw_extern_mul(tlwe_in[g], selector[sel[g]], party_of[sel[g]], P)  (mk_internals.jl:348-391) for B rows.  Rows: host
 * int32 [B][P+1][N] = a_0 ... a_{P-1}, b (MKTLweSample, :46-57); sel: host int32 [B] in [0, S).  TFHE_ERR_INVALID_ARG: a selector out
 * of range (checked before anything is uploaded). */
int32_t tfhe_mk_extern_mul_batch(tfhe_ctx *ctx, const int32_t *tlwe_in, const int32_t *sel, int32_t *tlwe_out, int64_t B);

/* CMUX tree on multi-key samples: tfhe_cmux_tree_batch's contract with data host int32 [T][2^depth][P+1][N].  Level v replaces each pair
 * (d0, d1) by d0 + selector[sel[g][v]] (.) (d1 - d0): mk_mux_rotate (mk_internals.jl:464-471) without the monomial.  out_form 0: the
 * MK TLWE sample, out int32 [B][P+1][N]; 1: mk_tlwe_extract_sample (:88-95), [B][P*N+1]; 2: that through mk_keyswitch (:397-411),
 * [B][P*n+1], a multi-key LWE sample every tfhe_mk_gate* call accepts.  Depth 1 ... 12; two ping-pong workspaces whose sizes are
 * compared with the device's free memory BEFORE anything is allocated (TFHE_ERR_NOMEM, the context stays usable).
 * TFHE_ERR_INVALID_ARG as tfhe_cmux_tree_batch; TFHE_ERR_NO_KEY also for out_form 2 without the multi-key keyswitch key. */
int32_t tfhe_mk_cmux_tree_batch(tfhe_ctx *ctx, const int32_t *data, int64_t T, const int32_t *table_index, int32_t depth,
                                const int32_t *sel, int32_t *out, int64_t B, int32_t out_form);

/* CMUX network on multi-key samples (addition within ABI v7): tfhe_cmux_net_batch's contract — the same netlist, limits, validation and
 * messages — with data host int32 [T][E][P+1][N] and sel: host int32 [B][V] into the multi-key selector set.  Node i of level v of row
 * g is  in[src0] + selector[sel[g][var]] (.) (in[src1] - in[src0])  with mk_tgsw_extern_mul for the party of THAT selector: the party
 * is per node, so one level may mix the parties' variables.  A node with src0 == src1 is a copy.  out_form 0: out int32 [B][F][P+1][N];
 * 1: mk_tlwe_extract_sample at coefficient 0, [B][F][P*N+1]; 2: that through mk_keyswitch, [B][F][P*n+1], multi-key LWE samples every
 * tfhe_mk_gate* call accepts.  One launch per level (csrc/kernels_mk_cmux_net.hpp; tfhe_last_kernel_name reports
 * "mk_cmux_net_level_kernel(N=..,P=..,l=..[,spec=global])"; the option "anyn_spec" = 1 puts the three spectrum accumulators in global
 * memory, where they are anyway from N = 4096 up).  A tree-shaped network equals tfhe_mk_cmux_tree_batch word for word.  The jointly
 * encrypted comparison of two 16-bit integers held by two parties is 32 levels and 48 products per row.
 * Workspace and TFHE_ERR_NOMEM as tfhe_cmux_net_batch, on samples of P + 1 polynomials.  Refused in this order: TFHE_ERR_STATE on a
 * single-key context, a multi-device context, with "measure_margin" on; TFHE_ERR_NO_KEY without the multi-key bootstrapping key or a
 * selector set; TFHE_ERR_INVALID_ARG as tfhe_cmux_net_batch; TFHE_ERR_NO_KEY for out_form 2 without the multi-key keyswitch key.
 * B = 0 returns TFHE_OK. */
int32_t tfhe_mk_cmux_net_batch(tfhe_ctx *ctx, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index,
                               const int32_t *widths, int32_t levels, const int32_t *nodes, const int32_t *sel, int32_t V,
                               int32_t *out, int64_t B, int32_t out_form);

/* CMUX network with a public monomial on every edge, on multi-key samples (addition within ABI v7): tfhe_mk_cmux_net_batch's contract
 * with tfhe_rot_net_batch's one difference, a node record of five words, nodes: host int32 [sum widths][5] = (src0, src1, var, rot0,
 * rot1).  Node i of level v of row g is
 *     X^rot0 in[src0] + selector[sel[g][var]] (.) (X^rot1 in[src1] - X^rot0 in[src0])
 * with mk_tgsw_extern_mul for the party of that selector and X^r p = mul_by_monomial(p, r) on all P + 1 polynomials of the MK TLWE
 * sample; rot0, rot1 are public, in [0, 2N).  src0 == src1 with rot0 == rot1 is a rotated copy (no product, no noise, the exact words
 * of X^rot0 in[src0]); src0 == src1 with rot0 != rot1 is a true product.  A table packed N entries to an MK TLWE sample is read at an
 * address whose bits several parties own at 2^(d - log2 N) - 1 + log2 N multi-key external products instead of 2^d - 1, and a
 * 2^16-entry table, beyond tfhe_mk_cmux_tree_batch's depth 12, at 63 + 10 products under N = 1024; a one-state automaton with weights
 * 0 and 2N - 1 returns f(popcount) of bits from several parties.  With every rotation 0 the call equals tfhe_mk_cmux_net_batch word
 * for word.
 * Everything else is tfhe_mk_cmux_net_batch's: data, table_index, sel, the limits, the three out_forms (extraction at coefficient 0),
 * the workspaces and TFHE_ERR_NOMEM before any allocation, B = 0, the timing slots, and the order of the refusals, with
 * TFHE_ERR_INVALID_ARG also for a rotation outside [0, 2N), the message naming node, level and field (rot0 / rot1), before anything
 * is uploaded.  One launch per level (csrc/kernels_mk_rot_net.hpp; tfhe_last_kernel_name reports
 * "mk_rot_net_level_kernel(N=..,P=..,l=..[,spec=global])"; the option "anyn_spec" is honoured).  A single-key context is refused with
 * TFHE_ERR_STATE, as a multi-key context is by tfhe_rot_net_batch. */
int32_t tfhe_mk_rot_net_batch(tfhe_ctx *ctx, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index,
                              const int32_t *widths, int32_t levels, const int32_t *nodes, const int32_t *sel, int32_t V,
                              int32_t *out, int64_t B, int32_t out_form);

/* Multi-key blind rotation of the caller's MK TLWE accumulators (addition within ABI v7): tfhe_blind_rotate_batch's contract, argument
 * for argument, under a multi-key cloud key — mk_blind_rotate (mk_internals.jl:473-485) on an accumulator the caller supplies.  For row g
 *     A_0 = X^(-barb_g) acc[acc_index[g]]                            on all P + 1 polynomials (mk_mul_by_monomial, :79-85)
 *     A_(i+1) = A_i + selector[sel[i]] (.) (X^(e_g,i) A_i - A_i)     i = 0 ... steps - 1        (mk_mux_rotate, :464-470)
 * with the expanded RGSW selectors of tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load, step i multiplying for party_of[sel[i]]
 * (mk_tgsw_extern_mul).  A (party, bit) entry of the multi-key bootstrapping key is such a selector: with the key's P n entries loaded
 * party-major as selectors 0 ... P n - 1, sel NULL and steps = P n, a row is a multi-key LWE sample as it lies in memory and the call
 * is the reference's rotation, whichever kernel family serves the gates.  With MK TLWE encryptions of test polynomials as acc one
 * party's private table is evaluated on jointly encrypted data; with the output of tfhe_mk_cmux_tree_batch (out_form 0 there) as acc a
 * table of p 2^d entries is addressed in part by a digit computed by multi-key gates or lookups; with out_form 0 here a multi-key
 * bootstrap's result leaves as an MK TLWE sample that the multi-key trees and networks accept as `data`.
 * acc: host int32 [T][P+1][N], trivial or encrypted; acc_index: host int32 [B] in [0, T), or NULL = accumulator 0.  rows: host int32
 * [B][steps+1], the step words then the body; in_form 0: LWE words, switched to Z_2N in the kernel (:502-503); in_form 1: exponents in
 * [0, 2N).  A zero exponent adds exactly zero.  sel: host int32 [steps] in [0, S), shared by all rows, or NULL = selector i for step i.
 * steps: 1 ... 65536.  out_form 0: the final accumulator, out int32 [B][P+1][N] (n_out must be 1); 1: for j < n_out its extraction at
 * coefficient j N / n_out (tfhe_mk_bootstrap_tv_multi_batch's rule), [B][n_out][P*N+1]; 2: those through the multi-key keyswitch,
 * [B][n_out][P*n+1], operands of every multi-key gate.  n_out: a power of two <= 32, and 1 or <= N / 4.  With acc = (0, ..., 0, tv) and
 * the bootstrapping key as selectors the call equals tfhe_mk_bootstrap_tv_multi_batch word for word; with B = 1 and out_form 0 it
 * equals the tfhe_mk_rot_net_batch chain "rotated copy by 2N - barb, then `steps` levels of width 1 with records (0, 0, i, 0, e_i)"
 * word for word, in one launch instead of steps + 1.
 * One kernel, one workgroup per row (csrc/kernels_mk_blind_rotate_tlwe.hpp; tfhe_last_kernel_name reports
 * "mk_tlwe_rotate_kernel(N=..,P=..,l=..,steps=..[,spec=global])"; the option "anyn_spec" is honoured); tfhe_last_rotation_count = B;
 * tfhe_last_timing_ms: 0 = the rotation, 1 = the keyswitch, 2 = both.  The refusals come in tfhe_blind_rotate_batch's order, everything
 * validated on the host before anything is uploaded — TFHE_ERR_STATE: a single-key context, a multi-device context, measure_margin on,
 * and with out_form 2 a keyswitch key loaded for another party count; TFHE_ERR_NO_KEY: no multi-key bootstrapping key, no selector
 * set, or out_form 2 without the multi-key keyswitch key; TFHE_ERR_INVALID_ARG: NULL buffer, B < 0, steps / in_form / out_form / T /
 * n_out out of range, n_out != 1 with out_form 0, a selector or accumulator index out of range, sel NULL with fewer than `steps`
 * selectors loaded, with in_form 1 a word outside [0, 2N) (the message names row and column).  The workspaces are compared with the
 * device's free memory BEFORE anything is allocated: TFHE_ERR_NOMEM, the context stays usable.  B = 0 returns TFHE_OK.
 * tfhe_blind_rotate_batch keeps refusing a multi-key context.  Out of scope: an LDS-resident accumulator, and forms on the tuned
 * multi-key families' key layouts (the call reads the selector set alone). */
int32_t tfhe_mk_blind_rotate_batch(tfhe_ctx *ctx, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows,
                                   int32_t steps, int32_t in_form, const int32_t *sel, int32_t n_out, int32_t *out, int64_t B,
                                   int32_t out_form);

/* ---- multi-key leveled mode on device-resident tables (additions within ABI v7) ---------------------------
 * The single-key block "leveled mode on device-resident tables" above, under a multi-key cloud key: MK TLWE samples that stay on the
 * device between leveled calls, an in-place update of the expanded selector set, and two level calls between the MK TLWE table and
 * the multi-key wire table (tfhe_mk_wires_alloc).  No new cryptography, no new key material: every result equals, word for word,
 * tfhe_mk_rot_net_batch / tfhe_mk_blind_rotate_batch on the same samples.  P = the parties of the loaded multi-key bootstrapping key;
 * a sample is int32 [P+1][N], a wire row P n + 1 words.  One-device multi-key contexts only (TFHE_ERR_STATE otherwise; the single-key
 * calls above keep refusing a multi-key context).
 *
 * tfhe_mk_tlwe_alloc: a device table int32 [slots][P+1][N]; slots = 0 frees it; reallocating discards the old contents.  The table
 * records the party count it was allocated for, as tfhe_mk_wires_alloc does for the wires: TFHE_ERR_NO_KEY without the multi-key
 * bootstrapping key (it fixes P).  The size is compared with the device's free memory (the table being replaced counted as free)
 * before anything is freed or allocated: TFHE_ERR_NOMEM, the context and its present table stay as they were.  Waits for the levels
 * queued on the context.  Freed with the context.
 * tfhe_mk_tlwe_upload / tfhe_mk_tlwe_download: slots [first, first + count) from / to host int32 [count][P+1][N], ordered behind the
 * levels queued on the context; both return with the copy done.  TFHE_ERR_STATE without a table, TFHE_ERR_INVALID_ARG for a range
 * outside it or a NULL buffer with count > 0. */
int32_t tfhe_mk_tlwe_alloc(tfhe_ctx *ctx, int64_t slots);
int32_t tfhe_mk_tlwe_upload(tfhe_ctx *ctx, int64_t first, int64_t count, const int32_t *host);
int32_t tfhe_mk_tlwe_download(tfhe_ctx *ctx, int64_t first, int64_t count, int32_t *host);

/* Replace selectors [first, first + count) of the set tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load loaded, in place, spectra and
 * party_of entries alike: every other selector keeps its exact words, and the replaced ones are what a fresh load of the edited set
 * would hold.  tfhe_mk_tgsw_update: tgsw is int32 [count][2 l P + 2 l][N] (expanded samples), party_of int32 [count].
 * tfhe_mk_tgsw_expand_update: the uni-encryptions c0 ... f1, int32 [count][l][N] each, and party_of [count], expanded against pub_b
 * [P][l][N] with tfhe_mk_tgsw_expand_load's per-party grouping over the count new samples only; expanded_out, if not NULL, receives
 * int32 [count][2 l P + 2 l][N].  For a set "the key's P n selectors, then a request's address bits": the key is loaded once and the
 * address bits are swapped behind it.  Both wait for the work queued on the context first.  TFHE_ERR_STATE: a single-key or
 * multi-device context, parties other than the bootstrapping key's; TFHE_ERR_NO_KEY: no set loaded; TFHE_ERR_INVALID_ARG: a NULL
 * pointer, count < 1, a range outside [0, S), a party outside [0, P); TFHE_ERR_NOMEM: the staging does not fit the device's free
 * memory, before anything is allocated. */
int32_t tfhe_mk_tgsw_update(tfhe_ctx *ctx, const int32_t *tgsw, const int32_t *party_of, int64_t first, int64_t count, int32_t parties);
int32_t tfhe_mk_tgsw_expand_update(tfhe_ctx *ctx, int32_t parties, const int32_t *pub_b, const int32_t *party_of, const int32_t *c0,
                                   const int32_t *c1, const int32_t *d0, const int32_t *d1, const int32_t *f0, const int32_t *f1,
                                   int64_t first, int64_t count, int32_t *expanded_out);

/* tfhe_mk_rot_net_batch between the tables: tfhe_rot_net_level's contract argument for argument, with "slot" an MK TLWE slot, "wire"
 * a row of the multi-key wire table and the keyswitch the multi-key one.  The words equal tfhe_mk_rot_net_batch on the same samples —
 * with every rotation 0 that is tfhe_mk_cmux_net_batch, with a tree's netlist tfhe_mk_cmux_tree_batch.  The same kernel
 * (mk_rot_net_level_kernel), unchanged; timing slots and tfhe_last_kernel_name as tfhe_mk_rot_net_batch.
 *
 * tfhe_mk_blind_rotate_batch between the tables: tfhe_blind_rotate_level's contract with steps = P n.  Row g's rotating sample x_g is
 * tfhe_mk_lut_level's combination of multi-key wire rows (cst NULL: 0; a row without terms is the trivial sample and reads no wire);
 * A_0 = X^(-barb_g) slot[acc_slot[g]] (slots may repeat); sel: host int32 [P n] or NULL = selector i for step i (the key loaded
 * party-major).  out_form 0 (n_out must be 1): the final accumulator goes to slot out_slot[g]; the slots must be distinct and none may
 * be an acc_slot of the same call.  out_form 2: the n_out extractions go through the multi-key keyswitch to wires
 * out_wires[g n_out + j]; no wire may be named twice and none may be a term wire of the same call.  The words equal
 * tfhe_mk_blind_rotate_batch(acc = those slots' samples, rows = x_g, steps = P n, in_form 0, sel, n_out, out_form).
 * tfhe_mk_lut_level's prologue stages the rows (linear_prologue_kernel), then one kernel, one workgroup per row
 * (csrc/kernels_mk_tlwe_levels.hpp; tfhe_last_kernel_name reports "mk_tlwe_rotate_level_kernel(N=..,P=..,l=..,steps=..[,spec=global])";
 * "anyn_spec" is honoured); tfhe_last_rotation_count = B; tfhe_last_timing_ms as the batch call.
 *
 * Both level calls: everything is validated on the host before anything is uploaded or written, the message names the offender, and
 * a refused call changes no slot and no wire.  In this order — TFHE_ERR_STATE: a single-key context, a multi-device context,
 * measure_margin on, no MK TLWE table, no wire table when out_form 2 or terms need one, a wire table with single-key rows, a table,
 * wire table or keyswitch key whose parties differ from the bootstrapping key's; TFHE_ERR_NO_KEY: no multi-key bootstrapping key;
 * TFHE_ERR_INVALID_ARG: everything about the arguments, by the single-key calls' slot / wire / overlap rules; TFHE_ERR_NO_KEY: no
 * selector set, or out_form 2 without the multi-key keyswitch key (a selector index is checked against the loaded set after that).
 * The workspaces are compared with the device's free memory before anything is allocated (TFHE_ERR_NOMEM, the context stays usable).
 * B = 0 returns TFHE_OK.  The calls are ordered behind the asynchronous levels queued on the context (tfhe_mk_gates_level,
 * tfhe_mk_lut_level, ...) and SYNCHRONISE before they return.  Out of scope: multi-device contexts, circuits (Circuit.run keeps
 * refusing TLWE nodes under a multi-key cloud key). */
int32_t tfhe_mk_rot_net_level(tfhe_ctx *ctx, const int32_t *table_first, int32_t E, const int32_t *widths, int32_t levels,
                              const int32_t *nodes, const int32_t *sel, int32_t V, int32_t out_form, int64_t out_first,
                              const int32_t *out_wires, int64_t B);
int32_t tfhe_mk_blind_rotate_level(tfhe_ctx *ctx, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire,
                                   const int32_t *term_coef, const int32_t *cst, const int32_t *sel, int32_t n_out, int32_t out_form,
                                   const int32_t *out_slot, const int32_t *out_wires, int64_t B);

/* The same two multi-key rotations on the multi-key gates' own kernel and key (additions within ABI v7): tfhe_mk_blind_rotate_batch and
 * tfhe_mk_blind_rotate_level with steps = P n, in_form 0 and sel NULL, run by the ACC form of the two-waves-per-rotation kernel of the
 * 2-party gates (mk_blind_rotate_kernel_w2 in csrc/kernels_multikey.hpp, compiled once more in csrc/engine_mk_bootstrap_acc.hip): the
 * three polynomials of the accumulator stay in LDS for all P n steps.  The calls read the multi-key bootstrapping key in the layout the
 * gates read (tfhe_mk_load_bootstrap_key_*, tfhe_mk_expand_load_bootstrap_key); they need no selector set — the key need not be
 * expanded and loaded a second time as P n selectors — and leave a loaded one alone.  The result equals, word for word, that of
 * tfhe_mk_blind_rotate_batch(acc, T, acc_index, rows, steps = P n, in_form 0, sel NULL, n_out, out, B, out_form), respectively
 * tfhe_mk_blind_rotate_level(..., sel NULL, ...), where the selector set holds the loaded bootstrapping key's P n entries in order.
 * Served: 2 parties (those of the loaded key), N = 1024, l = 4, the tuned key layout — mktfhe_parameters_2party.  Option "mk_general" is
 * ignored: there is one ACC family, and the tuned and the any-party kernel read the same key layout.
 * Buffer shapes (acc [T][P+1][N], acc_index, out), the n_out rule, the out_forms 0 / 1 / 2 and, for the level call, the terms, the slot,
 * wire and overlap rules are those of tfhe_mk_blind_rotate_batch and tfhe_mk_blind_rotate_level above.  rows: host int32 [B][P n + 1],
 * multi-key LWE samples, staged by tfhe_mk_bootstrap_tv_batch's modulus switch; the level call's rows by tfhe_mk_lut_level's prologue
 * (a call without terms stages its rows on the host and needs no wire table), as tfhe_mk_blind_rotate_level's.
 * Geometry: the gates' — option "mk_rw": 0 = one rotation per workgroup up to one row per CU and pairs in lockstep beyond, 1, 2 (an odd
 * count in pairs gets a padding rotation that stores nothing).  tfhe_last_kernel_name reports "mk_blind_rotate_kernel_w2_acc<4[,rw2]>";
 * tfhe_last_rotation_count = B; tfhe_last_timing_ms: 0 = the rotation, 1 = the keyswitch, 2 = both.
 * Everything is validated on the host before anything is uploaded, and a refused call changes no slot and no wire.  TFHE_ERR_STATE:
 * a single-key context, a multi-device context, measure_margin on (the level call: and a missing or unfit table, as
 * tfhe_mk_blind_rotate_level), then a shape the kernel does not serve (parties != 2, l != 4, N != 1024) or a key that is not in its
 * layout (the any-N kernels' layout) — the message names the shape and points to tfhe_mk_blind_rotate_batch; TFHE_ERR_INVALID_ARG: as
 * the two calls above; TFHE_ERR_NO_KEY: no multi-key bootstrapping key, or out_form 2 without the multi-key keyswitch key;
 * TFHE_ERR_NOMEM: the workspaces compared with the device's free memory before anything is allocated.  B = 0 returns TFHE_OK.
 * tfhe_get_option(ctx, "mk_bootstrap_acc") answers 1 where the context's shape, its key's parties and its key layout are served, 0
 * otherwise.  The single-key tfhe_bootstrap_acc_batch / _level keep refusing a multi-key context.
 * Out of scope: the 4- and 8-party sets (mk_g2 and the any-party kernel have no ACC form), dispatch by batch size beyond "mk_rw". */
int32_t tfhe_mk_bootstrap_acc_batch(tfhe_ctx *ctx, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows,
                                    int32_t n_out, int32_t out_form, int32_t *out, int64_t B);
int32_t tfhe_mk_bootstrap_acc_level(tfhe_ctx *ctx, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire,
                                    const int32_t *term_coef, const int32_t *cst, int32_t n_out, int32_t out_form, const int32_t *out_slot,
                                    const int32_t *out_wires, int64_t B);

/* ---- measurement ---------------------------------------------------------------------------- */

/* Timing of the most recent batch call on ctx, from HIP events recorded on the stream the kernels
 * were launched on.  which: 0 = blind-rotate kernel(s), 1 = keyswitch kernel(s), 2 = whole batch
 * (prologue .. last kernel, device side).  Blocks until those kernels have finished.  After a host-buffer call that ran as
 * two halves on two streams (tfhe_gates_batch from "pipeline_min" gates up; default 16 per compute unit: 4096 on an MI355X): from the start of the phase on the stream that
 * started first to the later of the two streams' ends. */
int32_t tfhe_last_timing_ms(tfhe_ctx *ctx, int32_t which, float *ms);

/* The same timing of up to the last 32 batch calls on a one-device ctx, oldest first, read in ONE go after the calls: a
 * caller timing a sequence of asynchronous calls need not synchronise (and so serialise its host work with the device)
 * after each one.  ms: room for max_calls floats; *n_out = entries written (<= max_calls, <= 32, <= calls made).  A call
 * that failed part-way is not counted.  The history is per stream: after tfhe_gates_batch_submit it holds the batches that
 * took the context's own stream (every other one); a blocking host-buffer call that ran as two halves contributes the half
 * on the own stream (tfhe_last_timing_ms spans both). */
int32_t tfhe_timing_history_ms(tfhe_ctx *ctx, int32_t which, float *ms, int32_t max_calls, int32_t *n_out);

/* Number of device contexts that took part in the most recent batch / level call (1 on a one-device context; on a
 * multi-device context: how many devices the call was sharded over — a narrow circuit level runs on the first one).  ABI v5. */
int32_t tfhe_last_device_count(const tfhe_ctx *ctx);

/* Number of blind rotations the most recent batch call executed (MUX counts 2). */
int64_t tfhe_last_rotation_count(const tfhe_ctx *ctx);

/* Name of the blind-rotate kernel instantiation the most recent batch call launched (e.g.
 * "blind_rotate_kernel_v3<2,16>"); valid until the next call on ctx. */
const char *tfhe_last_kernel_name(const tfhe_ctx *ctx);

/* Exactness evidence for the Float64 transform: after tfhe_set_option(ctx, "measure_margin", 1), batch calls run
 * the DIAG instantiation of whichever blind-rotate kernel the dispatcher selects (every kernel that rounds has one:
 * single key N = 1024 / 2048, k = 1 / 2, two-wave, multi-key 2-party and any-party) and record, per blind rotation,
 * the largest distance of any pre-rounding value from an integer (polynomials.jl:115-116 rounds; a flipped rounding
 * needs 0.5).  Returns the maximum over the last call. */
int32_t tfhe_last_rounding_margin(tfhe_ctx *ctx, double *worst);

/* Same DIAG run: the shader clock the blind-rotate kernel actually held, in MHz = s_memtime ticks / s_memrealtime
 * ticks x 100 MHz around the kernel body, median over the workgroups that ran for at least 10 us (what FP64-issue roofline
 * figures are priced at).  TFHE_ERR_STATE if no workgroup ran that long: the 100 MHz counter is too coarse for a shorter one.
 * A kernel of a few tens of microseconds right after the device woke up reads the clock of the DVFS ramp, not the sustained
 * one: price rooflines with the reading of a launch that lasts milliseconds. */
int32_t tfhe_last_kernel_clock_mhz(tfhe_ctx *ctx, double *mhz);

/* Options by name.  NONE of them changes a result word: they choose among kernels that compute the same thing (the tests
 * force every kernel through them and compare with the oracle), switch diagnostics on, or move a dispatch threshold.  Defaults
 * are what the measurements of DESIGN.md chose; thresholds given per compute unit scale with the device (256 CUs on an MI355X).
 *
 *   what runs                  "measure_margin" 0|1       the DIAG instantiation of the chosen kernel: rounding margin + in-kernel clock
 *                              "timing_events"  1|0       0: no per-phase HIP events (each costs the stream ~5 us; tfhe_last_timing_ms then reports nothing)
 *   host-buffer pipeline       "pipeline_min"   n         tfhe_gates_batch from n gates up runs as two halves on two streams (default 16 per CU; < 0 never)
 *   multi-device context       "level_split_min" n        levels of at least n rotations are sharded over the devices (default 16 per CU; < 0 never)
 *                              "level_exchange" 0|1|2     rows between devices: by peer access | device to device | pinned host staging
 *   kernel by batch size       "br_tiny"  n               up to n rotations: 4 l waves per rotation (h2); default one per CU, -1 never
 *    (N = 1024, k = 1)         "br_small" n               up to n rotations: two waves per rotation (w2); default 4 per CU, -1 never
 *                              "br_split" 1|0             a batch above what the chip holds sends its last partly filled round to the two-wave kernel
 *                              "w2_rw" 0|1|2, "v3_rw" 0|1|4   rotations per workgroup in lockstep (0: by batch size)
 *                              "br_prio_pct" 0..100       a wave lowers its issue priority over this share of its steps (default 90)
 *                              "br_rt_l" 0|1              l = 2 / 3 on the run-time-l instantiations too (a comparison switch)
 *   other shapes               "k2_w3" -1|0|1, "k2_rw" 0|1|7       k = 2: three waves per rotation (by size | never | always), lockstep groups
 *                              "n2048_rw" 0|1|2           N = 2048: rotations per workgroup
 *                              "n512_w2" -1|0|1, "n512_rw" 0|1|4   N = 512
 *                              "br_general" 0|1           every single-key rotation on blind_rotate_kernel_general (cross-check)
 *                              "br_anyn" 0|1, "anyn_spec" -1|0|1   the any-N kernel where a tuned one exists (decides a KEY LAYOUT: choose before
 *                                                         loading the bootstrapping key, TFHE_ERR_STATE otherwise); its spectrum accumulators in LDS / global memory
 *   multi-key                  "mk_rw" 0|1|2, "mk_general" 0|1, "mkg_variant" 0|1, "mkg_rw" 0|1|2|4, "mkg_acc" -1|0|1
 *   keyswitch                  "ks_variant" 4|3|1         int8 MFMA | tiled integer | gather (decides a KEY LAYOUT: before loading the keyswitch key)
 *                              "ks_slices" 1|2|4          K-split of the MFMA kernel for large batches
 *   read-only (tfhe_get_option) "exact_domain", "exact_bound_log2_x1000", "exact_margin_x1e6" (below), "peer_pairs" (multi-device context:
 *                              ordered pairs of different device contexts that copy device to device)
 *   tests                      "debug_fail_alloc_after" n (ctx may be NULL; process-wide): see tfhe_get_option */
int32_t tfhe_set_option(tfhe_ctx *ctx, const char *name, int64_t value);
/* Read-only names of tfhe_get_option (ABI v7), decided by tfhe_ctx_create from the parameter set alone — is it inside what a
 * Float64 transform computes exactly ("Exactness domain" above)?
 *   "exact_domain"            2 = every result word is the exact product for ANY Int32 key words: the worst-case pre-rounding
 *                                 magnitude np N 2^(beta-1) 2^31 (np = (k+1) l products per output; multi-key (P+1) l) is below 2^51
 *                                 and the predicted rounding margin below 1/4  (tfhe_parameters_128, the multi-key sets);
 *                             1 = the same for every REAL key (uniform mask words: 8 x rms magnitude below 2^51), but not for an
 *                                 adversarial one  (tfhe_parameters_80: its all-keys bound is exactly 2^52);
 *                             0 = outside: the predicted margin reaches 1/4 (or the magnitude 2^51).  The engine still computes —
 *                                 the reference does too and warns (polynomials.jl:135-144) — but a word may differ from the exact
 *                                 product; tfhe_last_rounding_margin measures.  The Python and Julia constructors warn once.
 *   "exact_bound_log2_x1000"  1000 x log2 of that worst-case magnitude
 *   "exact_margin_x1e6"       10^6 x the predicted margin = 4.5 x 2^-53 x rms x max(log2(N/2), 4), rms = sqrt(np N) 2^(beta+32) / 12; every
 *                             measured margin of rounds 2-6 lies between 0.31 and 0.90 of it
 * "debug_fail_alloc_after" (set / get, ctx may be NULL, process-wide, default 0 = off): the n-th allocation checkpoint inside the
 * library from now on throws std::bad_alloc — how the tests show that TFHE_ERR_NOMEM comes back and the context survives. */
/* The current value of an option (ABI v6): a caller that changes one for a while can put it back.  "br_anyn" (the any-N kernel
 * where a tuned one exists; like "ks_variant" it decides a key layout and must be chosen before the bootstrapping key is
 * loaded), "anyn_spec", "level_exchange", "k2_w3", "n512_rw", "n512_w2" (which N = 512 / k = 2 kernel a batch size takes) are new in v6. */
int32_t tfhe_get_option(tfhe_ctx *ctx, const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* TFHE_MI355X_H */
