// engine_mk_tlwe_levels.hip — the multi-key leveled half's device-resident table: MK TLWE samples int32 [slots][P+1][N] beside the
// multi-key wire table (tfhe_mk_tlwe_alloc / _upload / _download), and tfhe_mk_blind_rotate_level: tfhe_mk_blind_rotate_batch with the
// accumulator read from a slot, the rotating multi-key LWE sample formed from wire-table rows as tfhe_mk_lut_level forms it, and the
// result left in a slot or, keyswitched, in wires: engine_tlwe_levels.hip under a multi-key cloud key.  The kernel
// (kernels_mk_tlwe_levels.hpp) is compiled here and nowhere else.  (tfhe_mk_rot_net_level: engine_mk_rot_net.hip; tfhe_mk_tgsw_update
// and tfhe_mk_tgsw_expand_update: engine_keys.hip.)
#define TFHE_EMIT_MK_TLWE_LEVEL_KERNELS
#include "engine.hpp"
#include "kernels_mk_tlwe_levels.hpp"
#include "leveled_checks.hpp"
#include <unordered_set>

// ---- the table --------------------------------------------------------------------------------------------------------------------
static int32_t mk_tlwe_state(tfhe_ctx *c, const char *who)
{
    if (c->P.parties < 2) return c->set_err(TFHE_ERR_STATE, "%s: context is single-key (tfhe_tlwe_alloc is its TLWE table)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (the MK TLWE table exists on one-device contexts only)", who);
    return TFHE_OK;
}

int32_t tfhe_mk_tlwe_alloc(tfhe_ctx *c, int64_t slots) try
{
    ENTER_CTX(c);
    int32_t rc = mk_tlwe_state(c, "mk_tlwe_alloc");
    if (rc) return rc;
    if (!c->have_mk_bk) return c->set_err(TFHE_ERR_NO_KEY, "mk_tlwe_alloc: multi-key bootstrapping key not loaded (it fixes the sample width)");
    if (slots < 0 || slots > 2147483647LL) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_tlwe_alloc: slots = %lld (0 ... 2^31 - 1)", (long long)slots);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->done_pending) { HIP_TRY(c, hipEventSynchronize(c->done_ev)); c->done_pending = false; }      // a level still running on a caller's stream
    const size_t sample = (size_t)(c->mk_parties + 1) * c->P.N * 4;
    if (slots > 0) {
        // (the table being replaced is freed first: its bytes count as free; a refused call keeps it)
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        const double held = (double)c->mk_tlwe_slots * (double)(c->mk_tlwe_parties + 1) * (double)c->P.N * 4;
        if ((double)slots * (double)sample > (double)free_b + held)
            return c->set_err(TFHE_ERR_NOMEM, "mk_tlwe_alloc: %lld slots of %zu bytes do not fit the device's free memory (%zu bytes)", (long long)slots, sample, free_b);
    }
    if (c->d_mk_tlwe) { (void)hipFree(c->d_mk_tlwe); c->d_mk_tlwe = nullptr; c->mk_tlwe_slots = 0; c->mk_tlwe_parties = 0; }
    if (slots == 0) return TFHE_OK;
    const hipError_t e = hipMalloc((void **)&c->d_mk_tlwe, (size_t)slots * sample);
    if (e != hipSuccess) {
        c->d_mk_tlwe = nullptr;
        (void)hipGetLastError();
        return c->set_err(TFHE_ERR_NOMEM, "mk_tlwe_alloc: hipMalloc of %lld slots failed: %s", (long long)slots, hipGetErrorString(e));
    }
    c->mk_tlwe_slots = slots;
    c->mk_tlwe_parties = c->mk_parties;
    return TFHE_OK;
}
ABI_CATCH(c, "tfhe_mk_tlwe_alloc")

static int32_t mk_tlwe_range_ok(tfhe_ctx *c, const char *who, int64_t first, int64_t count, const void *host)
{
    const int32_t rc = mk_tlwe_state(c, who);
    if (rc) return rc;
    if (!c->d_mk_tlwe) return c->set_err(TFHE_ERR_STATE, "%s: no MK TLWE table allocated (tfhe_mk_tlwe_alloc)", who);
    if (first < 0 || count < 0 || first > c->mk_tlwe_slots || count > c->mk_tlwe_slots - first || (count > 0 && !host))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: slot range [%lld, %lld + %lld) outside the table of %lld slots or NULL buffer", who, (long long)first,
                          (long long)first, (long long)count, (long long)c->mk_tlwe_slots);
    return TFHE_OK;
}

// (both copies go through the context's stream, behind the levels queued on it, and are waited for: the caller's buffer is free, or
//  filled, on return; a slot is as wide as the table was allocated for)
int32_t tfhe_mk_tlwe_upload(tfhe_ctx *c, int64_t first, int64_t count, const int32_t *host) try
{
    ENTER_CTX(c);
    const int32_t rc = mk_tlwe_range_ok(c, "mk_tlwe_upload", first, count, host);
    if (rc || count == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    { const int32_t rc0 = enter_stream(c, c->stream); if (rc0) return rc0; }
    const size_t sample = (size_t)(c->mk_tlwe_parties + 1) * c->P.N * 4;
    HIP_TRY(c, hipMemcpyAsync((char *)c->d_mk_tlwe + (size_t)first * sample, host, (size_t)count * sample, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return TFHE_OK;
}
ABI_CATCH(c, "tfhe_mk_tlwe_upload")

int32_t tfhe_mk_tlwe_download(tfhe_ctx *c, int64_t first, int64_t count, int32_t *host) try
{
    ENTER_CTX(c);
    const int32_t rc = mk_tlwe_range_ok(c, "mk_tlwe_download", first, count, host);
    if (rc || count == 0) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    { const int32_t rc0 = enter_stream(c, c->stream); if (rc0) return rc0; }
    const size_t sample = (size_t)(c->mk_tlwe_parties + 1) * c->P.N * 4;
    HIP_TRY(c, hipMemcpyAsync(host, (const char *)c->d_mk_tlwe + (size_t)first * sample, (size_t)count * sample, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return TFHE_OK;
}
ABI_CATCH(c, "tfhe_mk_tlwe_download")

// ---- tfhe_mk_blind_rotate_level ---------------------------------------------------------------------------------------------------
static const char *const WHO = "mk_blind_rotate_level";

struct MkRotateLevel {
    const int32_t *acc_slot, *term_start, *term_wire, *term_coef, *cst, *sel, *out_slot, *out_wires;
    int32_t n_out, out_form;
    int64_t B;
};

// One validated call on a device context: the prologue that stages the rows (timed with the upload, outside slot 0), one launch over
// B rows, then the multi-key keyswitch of the B n_out extractions into their wires if asked.  run_rotate_level's
// (engine_tlwe_levels.hip) protocol on samples of P + 1 polynomials and three spectrum accumulators whatever P is; nothing is
// downloaded.  A call without terms reads no wire (it may have no wire table at all): its rows, (0, ..., 0, cst[g]) switched to Z_2N,
// are staged by the host with the maps.
static int32_t run_mk_rotate_level(tfhe_ctx *c, const MkRotateLevel &L)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int N = c->P.N, M = N / 2 > 0 ? N / 2 : 1, NP = c->mk_parties, steps = NP * c->P.n;
    const size_t sample = (size_t)(NP + 1) * N, ext_w = (size_t)NP * N + 1, row_w = (size_t)steps + 1;
    const size_t B_ = (size_t)L.B, G = B_ * (size_t)L.n_out, T = (size_t)L.term_start[B_];
    const bool fits = leveled::lds_bytes(N, 3) <= 160 * 1024;
    const bool spec_lds = c->anyn_spec < 0 ? fits : (c->anyn_spec == 0 && fits);      // option anyn_spec: 1 = accumulators in global memory
    auto up = [](size_t words) { return (words + 63) / 64 * 64; };
    // e0 [G] (the keyswitch's identity map) | acc_slot [B] | sel [steps] | term_start [B + 1] | term_wire [T] | term_coef [T] | cst [B] |
    // out_slot [B] or out_wires [G] | without terms: the rows [B][steps + 1]
    const size_t o_idx = up(G), o_sel = o_idx + up(B_), o_start = o_sel + up((size_t)steps), o_wire = o_start + up(B_ + 1), o_coef = o_wire + up(T);
    const size_t o_cst = o_coef + up(T), o_out = o_cst + (L.cst ? up(B_) : 0), o_rows = o_out + up(L.out_form == 0 ? B_ : G);
    const size_t map_bytes = (T ? o_out + (L.out_form == 0 ? B_ : G) : o_rows + B_ * row_w) * 4;
    const LvlWant want[] = {
        {&c->lvl_ws[0], B_ * 2 * sample * 4},
        {&c->lvl_spec, spec_lds ? 0 : B_ * 3 * M * sizeof(cplx)},
        {&c->bara, T ? B_ * row_w * 4 : 0},
        {&c->ext, L.out_form == 2 ? G * ext_w * 4 : 0},
        {&c->map, map_bytes},
    };
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }       // (the workspaces may still be in use by a call on another stream)
    int32_t rc = leveled_reserve(c, WHO, want, (int)(sizeof want / sizeof want[0]));
    if (rc) return rc;

    rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h = (int32_t *)c->h_map;
    for (size_t r = 0; r < G; r++) h[r] = (int32_t)r;
    memcpy(h + o_idx, L.acc_slot, B_ * 4);
    if (L.sel) memcpy(h + o_sel, L.sel, (size_t)steps * 4);
    else for (int32_t i = 0; i < steps; i++) h[o_sel + i] = i;
    memcpy(h + o_start, L.term_start, (B_ + 1) * 4);
    if (T) {
        memcpy(h + o_wire, L.term_wire, T * 4);
        memcpy(h + o_coef, L.term_coef, T * 4);
    }
    if (L.cst) memcpy(h + o_cst, L.cst, B_ * 4);
    if (L.out_form == 0) memcpy(h + o_out, L.out_slot, B_ * 4);
    else memcpy(h + o_out, L.out_wires, G * 4);
    if (!T) {
        const int shift = 32 - (ilog2i(N) + 1);      // decode_message(., 2N), numeric-functions.jl:31-34
        memset(h + o_rows, 0, B_ * row_w * 4);
        if (L.cst)
            for (size_t g = 0; g < B_; g++) h[o_rows + g * row_w + (size_t)steps] = (int32_t)((uint32_t)L.cst[g] + (1u << (shift - 1))) >> shift;
    }
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    const int32_t *d_map = (const int32_t *)c->map.p;

    leveled::MkRotateLevelArgs a;
    a.in = c->d_mk_tlwe;
    a.row_index = d_map + o_idx;
    a.sel = d_map + o_sel;
    a.tgsw = c->d_mk_tgsw;
    a.out = L.out_form == 0 ? c->d_mk_tlwe : nullptr;
    a.ext = L.out_form == 0 ? nullptr : (int32_t *)c->ext.p;
    a.spec_g = spec_lds ? nullptr : (cplx *)c->lvl_spec.p;
    a.wtab = c->d_anyn_tab; a.twist = c->d_anyn_tab + N / 2;
    a.g = c->g;
    a.row_words = (int64_t)sample;
    a.L = c->P.bs_l; a.log2N = ilog2i(N);
    a.nodes_out = 1;
    a.rows = T ? (const int32_t *)c->bara.p : d_map + o_rows;
    a.party_of = c->d_mk_tgsw_party;
    a.out_slot = d_map + o_out;
    a.ws = (int32_t *)c->lvl_ws[0].p;
    a.parties = NP, a.steps = steps, a.log2_n_out = ilog2i(L.n_out);
    const size_t lds = leveled::lds_bytes(N, spec_lds ? 3 : 0);
    if (lds > 64 * 1024) LDS_TRY(c, lds, leveled::mk_tlwe_rotate_level_kernel);
    const unsigned nt = (unsigned)anyn::threads_for(N);

    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    if (T) {
        // x_g, switched to Z_2N, into bara: tfhe_mk_lut_level's prologue on rows of P n + 1 words (a row without terms reads no wire)
        rc = launch_linear_prologue(c, true, B_, d_map + o_start, d_map + o_wire, d_map + o_coef, L.cst ? d_map + o_cst : nullptr, nullptr, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    hipLaunchKernelGGL(leveled::mk_tlwe_rotate_level_kernel, dim3((unsigned)B_), dim3(nt), lds, s, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (L.out_form == 2) {
        rc = launch_keyswitch(c, G, d_map, nullptr, d_map + o_out, (const int32_t *)c->ext.p, c->d_wires, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = L.B;
    c->diag_rows = 0;
    name_kernel(c, "mk_tlwe_rotate_level_kernel(N=%d,P=%d,l=%d,steps=%d%s)", N, NP, c->P.bs_l, steps, spec_lds ? "" : ",spec=global");
    return TFHE_OK;
}

int32_t tfhe_mk_blind_rotate_level(tfhe_ctx *c, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                                   const int32_t *cst, const int32_t *sel, int32_t n_out, int32_t out_form, const int32_t *out_slot,
                                   const int32_t *out_wires, int64_t B) try
{
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc_slot || !term_start)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc_slot, term_start)", WHO);
    const bool needs_wires = out_form == 2 || (B > 0 && term_start[B] > 0);
    int32_t rc = mk_level_state(c, WHO, needs_wires, out_form == 2);
    if (rc) return rc;

    const int N = c->P.N, steps = c->mk_parties * c->P.n;
    const int64_t slots = c->mk_tlwe_slots;
    if (B > (int64_t)1 << 30) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld rows exceed one launch", WHO, (long long)B);
    if (out_form != 0 && out_form != 2)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_form = %d (0 into MK TLWE slots, 2 key-switched into wires; extracted rows have no table)", WHO, out_form);
    if (n_out < 1 || n_out > 32 || (n_out & (n_out - 1)) || (n_out > 1 && n_out > N / 4))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: n_out = %d (a power of two, at most 32, and 1 or at most N / 4 = %d)", WHO, n_out, N / 4);
    if (out_form == 0 && n_out != 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: n_out = %d with out_form 0 (the accumulator is one sample: n_out must be 1)", WHO, n_out);
    if ((double)B * (double)n_out > 2147483647.0)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B * n_out = %.0f rows exceed one launch", WHO, (double)B * (double)n_out);
    if (B > 0 && !(out_form == 0 ? out_slot : out_wires))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL %s with out_form %d", WHO, out_form == 0 ? "out_slot" : "out_wires", out_form);
    if (B > 0) {
        if (term_start[0] != 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term_start[0] = %d (must be 0)", WHO, term_start[0]);
        for (int64_t g = 0; g < B; g++)
            if (term_start[g + 1] < term_start[g]) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term_start decreases at row %lld", WHO, (long long)g);
        const int64_t T = term_start[B], G = B * n_out;
        if (T > 0 && (!term_wire || !term_coef)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: %lld terms and a NULL term array", WHO, (long long)T);
        for (int64_t t = 0; t < T; t++)
            if (term_wire[t] < 0 || term_wire[t] >= c->num_wires)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term %lld reads wire %d, outside the table of %lld wires", WHO, (long long)t, term_wire[t], (long long)c->num_wires);
        for (int64_t g = 0; g < B; g++)
            if (acc_slot[g] < 0 || acc_slot[g] >= slots)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: acc_slot[%lld] = %d is outside the table of %lld slots", WHO, (long long)g, acc_slot[g], (long long)slots);
        alloc_checkpoint();
        std::unordered_set<int32_t> written;
        written.reserve((size_t)G * 2);
        if (out_form == 0) {
            for (int64_t g = 0; g < B; g++) {
                if (out_slot[g] < 0 || out_slot[g] >= slots)
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_slot[%lld] = %d is outside the table of %lld slots", WHO, (long long)g, out_slot[g], (long long)slots);
                if (!written.insert(out_slot[g]).second) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: slot %d written twice in one call", WHO, out_slot[g]);
            }
            for (int64_t g = 0; g < B; g++)
                if (written.count(acc_slot[g]))
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: acc_slot[%lld] = %d is an output slot of the same call", WHO, (long long)g, acc_slot[g]);
        } else {
            for (int64_t g = 0; g < G; g++) {
                if (out_wires[g] < 0 || out_wires[g] >= c->num_wires)
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: output %lld is wire %d, outside the table of %lld wires", WHO, (long long)g, out_wires[g], (long long)c->num_wires);
                if (!written.insert(out_wires[g]).second) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: wire %d written twice in one call", WHO, out_wires[g]);
            }
            for (int64_t t = 0; t < T; t++)
                if (written.count(term_wire[t]))
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term %lld reads wire %d, which the same call writes", WHO, (long long)t, term_wire[t]);
        }
    }
    if (!c->d_mk_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "%s: no selector set loaded (tfhe_mk_tgsw_load)", WHO);
    if (out_form == 2 && !c->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the multi-key keyswitch key", WHO);
    if (sel) {
        for (int32_t i = 0; i < steps; i++)
            if (sel[i] < 0 || sel[i] >= c->mk_tgsw_count)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel[%d] = %d is outside the %lld loaded selectors", WHO, (int)i, sel[i], (long long)c->mk_tgsw_count);
    } else if (steps > c->mk_tgsw_count) {
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel NULL names selector i for step i, P n = %d steps, %lld selectors are loaded", WHO, steps, (long long)c->mk_tgsw_count);
    }
    if (B == 0) return TFHE_OK;
    return run_mk_rotate_level(c, MkRotateLevel{acc_slot, term_start, term_wire, term_coef, cst, sel, out_slot, out_wires, n_out, out_form, B});
}
ABI_CATCH(c, "tfhe_mk_blind_rotate_level")
