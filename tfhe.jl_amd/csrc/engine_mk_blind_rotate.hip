// engine_mk_blind_rotate.hip — tfhe_mk_blind_rotate_batch: the multi-key blind rotation of the caller's MK TLWE accumulators by
// multi-key LWE samples (or by exponents), on the caller's expanded RGSW selectors (tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load,
// engine_keys.hip), returning the final accumulator, its extractions or those keyswitched: engine_blind_rotate.hip's call under a
// multi-key cloud key.  The kernel (kernels_mk_blind_rotate_tlwe.hpp) is compiled here and nowhere else.
#define TFHE_EMIT_MK_BLIND_ROTATE_TLWE_KERNELS
#include "engine.hpp"
#include "kernels_mk_blind_rotate_tlwe.hpp"
#include "leveled_checks.hpp"

static const char *const WHO = "mk_blind_rotate_batch";
enum { ROTATE_MAX_STEPS = 65536 };

// One validated call on a device context: one launch over B rows, then the multi-key keyswitch of the B n_out extractions if asked.
// run_rotate's (engine_blind_rotate.hip) protocol on samples of P + 1 polynomials and three spectrum accumulators whatever P is.
static int32_t run_mk_rotate(tfhe_ctx *c, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t steps, int32_t in_form,
                             const int32_t *sel, int32_t n_out, int32_t *out, int64_t B, int32_t out_form)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int N = c->P.N, M = N / 2 > 0 ? N / 2 : 1, NP = c->mk_parties;
    const size_t sample = (size_t)(NP + 1) * N, ext_w = (size_t)NP * N + 1, ks_w = (size_t)NP * c->P.n + 1;
    const size_t B_ = (size_t)B, G = B_ * (size_t)n_out, row_w = (size_t)steps + 1;
    const bool fits = leveled::lds_bytes(N, 3) <= 160 * 1024;
    const bool spec_lds = c->anyn_spec < 0 ? fits : (c->anyn_spec == 0 && fits);      // option anyn_spec: 1 = accumulators in global memory
    auto up = [](size_t words) { return (words + 63) / 64 * 64; };
    // e0 [B n_out] (the keyswitch's identity map) | acc_index [B] | sel [steps]
    const size_t o_idx = up(G), o_sel = o_idx + up(B_), map_bytes = (o_sel + (size_t)steps) * 4;
    const size_t acc_bytes = (size_t)T * sample * 4;
    const LvlWant want[] = {
        {&c->lvl_data, acc_bytes},
        {&c->lvl_ws[0], B_ * 2 * sample * 4},
        {&c->lvl_ws[1], out_form == 0 ? B_ * sample * 4 : 0},
        {&c->lvl_spec, spec_lds ? 0 : B_ * 3 * M * sizeof(cplx)},
        {&c->bara, B_ * row_w * 4},
        {&c->ext, out_form >= 1 ? G * ext_w * 4 : 0},
        {&c->io[3], out_form == 2 ? G * ks_w * 4 : 0},
        {&c->map, map_bytes},
    };
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }       // (the workspaces may still be in use by a call on another stream)
    int32_t rc = leveled_reserve(c, WHO, want, (int)(sizeof want / sizeof want[0]));
    if (rc) return rc;

    rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h = (int32_t *)c->h_map;
    for (size_t r = 0; r < G; r++) h[r] = (int32_t)r;
    if (acc_index) memcpy(h + o_idx, acc_index, B_ * 4);
    else memset(h + o_idx, 0, B_ * 4);
    if (sel) memcpy(h + o_sel, sel, (size_t)steps * 4);
    else for (int32_t i = 0; i < steps; i++) h[o_sel + i] = i;
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->lvl_data.p, acc, acc_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->bara.p, rows, B_ * row_w * 4, hipMemcpyHostToDevice, s));
    const int32_t *d_map = (const int32_t *)c->map.p;

    leveled::MkRotateArgs a;
    a.in = (const int32_t *)c->lvl_data.p;
    a.row_index = d_map + o_idx;
    a.sel = d_map + o_sel;
    a.tgsw = c->d_mk_tgsw;
    a.out = out_form == 0 ? (int32_t *)c->lvl_ws[1].p : nullptr;
    a.ext = out_form == 0 ? nullptr : (int32_t *)c->ext.p;
    a.spec_g = spec_lds ? nullptr : (cplx *)c->lvl_spec.p;
    a.wtab = c->d_anyn_tab; a.twist = c->d_anyn_tab + N / 2;
    a.g = c->g;
    a.row_words = (int64_t)sample;
    a.L = c->P.bs_l; a.log2N = ilog2i(N);
    a.nodes_out = 1;
    a.rows = (const int32_t *)c->bara.p;
    a.party_of = c->d_mk_tgsw_party;
    a.ws = (int32_t *)c->lvl_ws[0].p;
    a.parties = NP, a.steps = steps, a.in_form = in_form, a.log2_n_out = ilog2i(n_out);
    const size_t lds = leveled::lds_bytes(N, spec_lds ? 3 : 0);
    if (lds > 64 * 1024) LDS_TRY(c, lds, leveled::mk_tlwe_rotate_kernel);
    const unsigned nt = (unsigned)anyn::threads_for(N);

    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    hipLaunchKernelGGL(leveled::mk_tlwe_rotate_kernel, dim3((unsigned)B_), dim3(nt), lds, s, a);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (out_form == 2) {
        rc = launch_keyswitch(c, G, d_map, nullptr, nullptr, (const int32_t *)c->ext.p, (int32_t *)c->io[3].p, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    if (out_form == 0) HIP_TRY(c, hipMemcpyAsync(out, c->lvl_ws[1].p, B_ * sample * 4, hipMemcpyDeviceToHost, s));
    else if (out_form == 1) HIP_TRY(c, hipMemcpyAsync(out, c->ext.p, G * ext_w * 4, hipMemcpyDeviceToHost, s));
    else HIP_TRY(c, hipMemcpyAsync(out, c->io[3].p, G * ks_w * 4, hipMemcpyDeviceToHost, s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = B;
    c->diag_rows = 0;
    name_kernel(c, "mk_tlwe_rotate_kernel(N=%d,P=%d,l=%d,steps=%d%s)", N, NP, c->P.bs_l, steps, spec_lds ? "" : ",spec=global");
    return TFHE_OK;
}

int32_t tfhe_mk_blind_rotate_batch(tfhe_ctx *c, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t steps, int32_t in_form,
                                   const int32_t *sel, int32_t n_out, int32_t *out, int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc || !rows || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc, rows, out)", WHO);
    int32_t rc = mk_leveled_state(c, WHO);
    if (rc) return rc;
    const int N = c->P.N;
    if (steps < 1 || steps > ROTATE_MAX_STEPS) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: steps = %d (1 ... %d)", WHO, steps, (int)ROTATE_MAX_STEPS);
    if (in_form < 0 || in_form > 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: in_form = %d (0 LWE samples, 1 exponents)", WHO, in_form);
    if (out_form < 0 || out_form > 2) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_form = %d (0 TLWE, 1 extracted, 2 key-switched)", WHO, out_form);
    if (T < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: T = %lld (at least one accumulator)", WHO, (long long)T);
    if (T > 2147483647LL) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: T = %lld accumulators (at most 2^31 - 1)", WHO, (long long)T);
    if (n_out < 1 || n_out > 32 || (n_out & (n_out - 1)) || (n_out > 1 && n_out > N / 4))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: n_out = %d (a power of two, at most 32, and 1 or at most N / 4 = %d)", WHO, n_out, N / 4);
    if (out_form == 0 && n_out != 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: n_out = %d with out_form 0 (the accumulator is one sample: n_out must be 1)", WHO, n_out);
    if ((double)B * (double)n_out > 2147483647.0)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B * n_out = %.0f rows exceed one launch", WHO, (double)B * (double)n_out);
    if (out_form == 2 && !c->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the multi-key keyswitch key", WHO);
    // (the keyswitch addresses rows by ITS key's parties, the rotation writes them by the bootstrapping key's: they must agree)
    if (out_form == 2 && c->ks.parties != c->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "%s: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties", WHO,
                          c->mk_parties, c->ks.parties);
    if (sel) {
        for (int32_t i = 0; i < steps; i++)
            if (sel[i] < 0 || sel[i] >= c->mk_tgsw_count)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel[%d] = %d is outside the %lld loaded selectors", WHO, (int)i, sel[i], (long long)c->mk_tgsw_count);
    } else if (steps > c->mk_tgsw_count) {
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel NULL names selector i for step i, steps = %d, %lld selectors are loaded", WHO, steps, (long long)c->mk_tgsw_count);
    }
    if (acc_index)
        for (int64_t g = 0; g < B; g++)
            if (acc_index[g] < 0 || acc_index[g] >= T)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: acc_index[%lld] = %d is outside [0, %lld)", WHO, (long long)g, acc_index[g], (long long)T);
    if (in_form == 1)
        for (int64_t g = 0; g < B; g++)
            for (int32_t i = 0; i <= steps; i++) {
                const int32_t e = rows[g * ((int64_t)steps + 1) + i];
                if (e < 0 || e >= 2 * N)
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: rows[%lld][%d] = %d is outside [0, %d) (in_form 1: exponents)", WHO, (long long)g, (int)i, e, 2 * N);
            }
    if (B == 0) return TFHE_OK;
    return run_mk_rotate(c, acc, T, acc_index, rows, steps, in_form, sel, n_out, out, B, out_form);
}
ABI_CATCH(c, "tfhe_mk_blind_rotate_batch")
