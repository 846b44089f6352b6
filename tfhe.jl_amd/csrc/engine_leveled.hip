// engine_leveled.hip — leveled mode: tfhe_extern_mul_batch and tfhe_cmux_tree_batch on a caller's TGSW selectors (tfhe_tgsw_load,
// engine_keys.hip) and TLWE samples; the CMUX level kernel (kernels_leveled.hpp) is compiled here and nowhere else
#define TFHE_EMIT_LEVELED_KERNELS
#include "engine.hpp"
#include "kernels_leveled.hpp"

// what both entry points refuse before they look at their arguments
static int32_t leveled_state(tfhe_ctx *c, const char *who)
{
    if (c->P.parties != 1) return c->set_err(TFHE_ERR_STATE, "%s: context is multi-key (leveled operations are single-key)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", who);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the CMUX level kernel has no DIAG instantiation)", who);
    return TFHE_OK;
}

// Grows the workspaces of one call, all or none: what they would have to grow by is compared with the device's free memory
// BEFORE anything is allocated, so a request the device cannot hold is refused (TFHE_ERR_NOMEM) without a failed hipMalloc
// behind it, and the buffers the context already holds stay as they are.
int32_t leveled_reserve(tfhe_ctx *c, const char *who, const LvlWant *want, int count)
{
    double grow = 0.0;      // (a double: the sum of an absurd request must not wrap)
    for (int i = 0; i < count; i++)
        if (want[i].bytes > want[i].buf->cap) grow += (double)want[i].bytes * 1.25 + 256.0;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    if (grow > (double)free_b)
        return c->set_err(TFHE_ERR_NOMEM, "%s: the workspaces need %.0f MB more device memory, %.0f MB are free", who, grow / 1048576.0, (double)free_b / 1048576.0);
    for (int i = 0; i < count; i++) {
        const hipError_t e = want[i].buf->reserve(want[i].bytes);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            return c->set_err(TFHE_ERR_NOMEM, "%s: out of device memory (%zu bytes)", who, want[i].bytes);
        }
        if (e != hipSuccess) return c->set_err(TFHE_ERR_DEVICE, "%s: hipMalloc failed: %s", who, hipGetErrorString(e));
    }
    return TFHE_OK;
}

// One validated call on a device context: `depth` CMUX levels over B rows, level 0 reading row g's 2^depth samples at
// in[row_index[g]] (d0_zero: depth 1 and the one sample in[g], the plain external product).  Host arrays: in [in_rows][2^depth or
// 1][k+1][N], row_index [B] or NULL = row 0 (d0_zero: row g), sel [B][depth].  out_form 0: the TLWE sample [k+1][N], 1: extracted at
// coefficient 0 [kN+1], 2: that keyswitched [n+1].  Timing events as the gate entry points: levels in slot 0, keyswitch in slot 1.
static int32_t run_levels(tfhe_ctx *c, const char *who, const int32_t *in, int64_t in_rows, const int32_t *row_index, int32_t depth, bool d0_zero,
                          const int32_t *sel, int32_t *out, int64_t B, int32_t out_form)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int N = c->P.N, K1 = c->P.k + 1, M = N / 2 > 0 ? N / 2 : 1, n = c->P.n, kNn = c->P.k * N;
    const size_t sample = (size_t)K1 * N;
    const size_t per_row_in = d0_zero ? 1 : (size_t)1 << depth;
    const size_t nodes0 = (size_t)1 << (depth - 1);                 // output nodes of level 0 per row: the widest level
    const size_t ws_bytes = (size_t)B * nodes0 * sample * 4;        // B 2^(depth-1) TLWE samples per buffer
    const bool in_lds = leveled::lds_bytes(N, K1) <= 160 * 1024;
    const bool fits = c->anyn_spec < 0 ? in_lds : (c->anyn_spec == 0 && in_lds);      // option anyn_spec, as the network kernels read it: 1 = accumulators in global memory
    const size_t B_ = (size_t)B, Sd = B_ * (size_t)depth;
    auto up = [](size_t words) { return (words + 63) / 64 * 64; };
    const size_t o_idx = up(B_), o_sel = o_idx + up(B_), map_bytes = (o_sel + Sd) * 4;      // e0 [B] | row_index [B] | sel [B][depth]
    const LvlWant want[] = {
        {&c->lvl_data, (size_t)in_rows * per_row_in * sample * 4},
        {&c->lvl_ws[0], ws_bytes},
        {&c->lvl_ws[1], depth > 1 ? ws_bytes / 2 : 0},
        {&c->lvl_spec, fits ? 0 : (size_t)B * nodes0 * K1 * M * sizeof(cplx)},
        {&c->ext, out_form >= 1 ? (size_t)B * (kNn + 1) * 4 : 0},
        {&c->io[3], out_form == 2 ? (size_t)B * (n + 1) * 4 : 0},
        {&c->map, map_bytes},
    };
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }       // (the workspaces may still be in use by a call on another stream)
    int32_t rc = leveled_reserve(c, who, want, (int)(sizeof want / sizeof want[0]));
    if (rc) return rc;
    if ((double)B * (double)nodes0 > 2147483647.0)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B * 2^(depth-1) = %.0f workgroups exceed one launch", who, (double)B * (double)nodes0);

    rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h = (int32_t *)c->h_map;
    for (size_t g = 0; g < B_; g++) h[g] = (int32_t)g;
    if (row_index) memcpy(h + o_idx, row_index, B_ * 4);
    else for (size_t g = 0; g < B_; g++) h[o_idx + g] = d0_zero ? (int32_t)g : 0;
    memcpy(h + o_sel, sel, Sd * 4);
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->lvl_data.p, in, (size_t)in_rows * per_row_in * sample * 4, hipMemcpyHostToDevice, s));
    const int32_t *d_map = (const int32_t *)c->map.p;

    leveled::Args a;
    a.sel = d_map + o_sel;
    a.tgsw = c->d_tgsw;
    a.spec_g = fits ? nullptr : (cplx *)c->lvl_spec.p;
    a.wtab = c->d_anyn_tab; a.twist = c->d_anyn_tab + N / 2;
    a.g = c->g;
    a.K1 = K1; a.L = c->P.bs_l; a.log2N = ilog2i(N);
    a.depth = depth;
    a.d0_zero = d0_zero ? 1 : 0;
    const size_t lds = leveled::lds_bytes(N, fits ? K1 : 0);
    if (lds > 64 * 1024) LDS_TRY(c, lds, leveled::cmux_level_kernel);
    const unsigned nt = (unsigned)anyn::threads_for(N);

    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    const int32_t *final_tlwe = nullptr;
    for (int lv = 0; lv < depth; lv++) {
        const size_t nodes_out = (size_t)1 << (depth - 1 - lv);
        const bool last = lv == depth - 1;
        a.in = lv == 0 ? (const int32_t *)c->lvl_data.p : (const int32_t *)c->lvl_ws[(lv - 1) & 1].p;
        a.row_index = lv == 0 ? d_map + o_idx : nullptr;
        a.row_words = (int64_t)(lv == 0 ? per_row_in * sample : 2 * nodes_out * sample);
        a.level = lv;
        a.nodes_out = (int32_t)nodes_out;
        a.out = last && out_form != 0 ? nullptr : (int32_t *)c->lvl_ws[lv & 1].p;
        a.ext = last && out_form != 0 ? (int32_t *)c->ext.p : nullptr;
        if (last) final_tlwe = a.out;
        hipLaunchKernelGGL(leveled::cmux_level_kernel, dim3((unsigned)(B_ * nodes_out)), dim3(nt), lds, s, a);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (out_form == 2) {
        rc = launch_keyswitch(c, B_, d_map, nullptr, nullptr, (const int32_t *)c->ext.p, (int32_t *)c->io[3].p, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    if (out_form == 0) HIP_TRY(c, hipMemcpyAsync(out, final_tlwe, B_ * sample * 4, hipMemcpyDeviceToHost, s));
    else if (out_form == 1) HIP_TRY(c, hipMemcpyAsync(out, c->ext.p, B_ * (kNn + 1) * 4, hipMemcpyDeviceToHost, s));
    else HIP_TRY(c, hipMemcpyAsync(out, c->io[3].p, B_ * (n + 1) * 4, hipMemcpyDeviceToHost, s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = 0;
    c->diag_rows = 0;
    name_kernel(c, fits ? "cmux_level_kernel(N=%d,k=%d,l=%d)" : "cmux_level_kernel(N=%d,k=%d,l=%d,spec=global)", N, c->P.k, c->P.bs_l);
    return TFHE_OK;
}

static int32_t check_selectors(tfhe_ctx *c, const char *who, const int32_t *sel, int64_t B, int32_t depth)
{
    for (int64_t e = 0; e < B * depth; e++)
        if (sel[e] < 0 || sel[e] >= c->tgsw_count)
            return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel[%lld][%d] = %d is outside the %lld loaded selectors", who, (long long)(e / depth), (int)(e % depth),
                              sel[e], (long long)c->tgsw_count);
    return TFHE_OK;
}

int32_t tfhe_extern_mul_batch(tfhe_ctx *c, const int32_t *tlwe_in, const int32_t *sel, int32_t *tlwe_out, int64_t B) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!tlwe_in || !sel || !tlwe_out))) return c->set_err(TFHE_ERR_INVALID_ARG, "extern_mul_batch: NULL argument or negative B");
    int32_t rc = leveled_state(c, "extern_mul_batch");
    if (rc) return rc;
    if (!c->d_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "extern_mul_batch: no selector set loaded (tfhe_tgsw_load)");
    rc = check_selectors(c, "extern_mul_batch", sel, B, 1);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    return run_levels(c, "extern_mul_batch", tlwe_in, B, nullptr, 1, true, sel, tlwe_out, B, 0);
}
ABI_CATCH(c, "tfhe_extern_mul_batch")

int32_t tfhe_cmux_tree_batch(tfhe_ctx *c, const int32_t *data, int64_t T, const int32_t *table_index, int32_t depth, const int32_t *sel, int32_t *out,
                             int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!data || !sel || !out))) return c->set_err(TFHE_ERR_INVALID_ARG, "cmux_tree_batch: NULL argument or negative B");
    int32_t rc = leveled_state(c, "cmux_tree_batch");
    if (rc) return rc;
    if (depth < 1 || depth > 12) return c->set_err(TFHE_ERR_INVALID_ARG, "cmux_tree_batch: depth = %d (1 ... 12)", depth);
    if (T < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "cmux_tree_batch: T = %lld (at least one table)", (long long)T);
    if (out_form < 0 || out_form > 2) return c->set_err(TFHE_ERR_INVALID_ARG, "cmux_tree_batch: out_form = %d (0 TLWE, 1 extracted, 2 key-switched)", out_form);
    if (!c->d_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "cmux_tree_batch: no selector set loaded (tfhe_tgsw_load)");
    if (out_form == 2 && !c->have_ks()) return c->set_err(TFHE_ERR_NO_KEY, "cmux_tree_batch: out_form 2 needs the keyswitch key");
    rc = check_selectors(c, "cmux_tree_batch", sel, B, depth);
    if (rc) return rc;
    if (table_index)
        for (int64_t g = 0; g < B; g++)
            if (table_index[g] < 0 || table_index[g] >= T)
                return c->set_err(TFHE_ERR_INVALID_ARG, "cmux_tree_batch: table_index[%lld] = %d is outside [0, %lld)", (long long)g, table_index[g], (long long)T);
    if (B == 0) return TFHE_OK;
    return run_levels(c, "cmux_tree_batch", data, T, table_index, depth, false, sel, out, B, out_form);
}
ABI_CATCH(c, "tfhe_cmux_tree_batch")
