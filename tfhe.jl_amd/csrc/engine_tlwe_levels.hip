// engine_tlwe_levels.hip — the leveled half's device-resident table: TLWE samples int32 [slots][k+1][N] beside the wire table
// (tfhe_tlwe_alloc / _upload / _download), its multi-key form of MK TLWE samples [slots][P+1][N] beside the multi-key wire table
// (tfhe_mk_tlwe_alloc / _upload / _download: the same three bodies), and tfhe_blind_rotate_level: tfhe_blind_rotate_batch with the
// accumulator read from a slot, the rotating LWE sample formed from wire-table rows as tfhe_lut_level forms it, and the result left in a
// slot or, keyswitched, in wires.  The kernel (kernels_tlwe_levels.hpp) is compiled here and nowhere else.  (tfhe_rot_net_level:
// engine_rot_net.hip; tfhe_mk_blind_rotate_level: engine_mk_tlwe_levels.hip.)
#define TFHE_EMIT_TLWE_LEVEL_KERNELS
#include "engine.hpp"
#include "kernels_tlwe_levels.hpp"
#include "leveled_checks.hpp"
#include "rotate_run.hpp"

// ---- the table --------------------------------------------------------------------------------------------------------------------
// One table per context (tfhe_ctx::tlwe), of the context's kind: `who` names the caller, `mk` its kind.
static int32_t tlwe_state(tfhe_ctx *c, const char *who, bool mk)
{
    if (!mk && c->P.parties != 1) return c->set_err(TFHE_ERR_STATE, "%s: context is multi-key (the TLWE table holds single-key samples)", who);
    if (mk && c->P.parties < 2) return c->set_err(TFHE_ERR_STATE, "%s: context is single-key (tfhe_tlwe_alloc is its TLWE table)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (the %s table exists on one-device contexts only)", who, mk ? "MK TLWE" : "TLWE");
    return TFHE_OK;
}

static int32_t tlwe_alloc(tfhe_ctx *c, const char *who, bool mk, int64_t slots)
{
    int32_t rc = tlwe_state(c, who, mk);
    if (rc) return rc;
    if (mk && !c->have_mk_bk) return c->set_err(TFHE_ERR_NO_KEY, "%s: multi-key bootstrapping key not loaded (it fixes the sample width)", who);
    if (slots < 0 || slots > 2147483647LL) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: slots = %lld (0 ... 2^31 - 1)", who, (long long)slots);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->done_pending) { HIP_TRY(c, hipEventSynchronize(c->done_ev)); c->done_pending = false; }      // a level still running on a caller's stream
    const int parties = mk ? c->mk_parties : 0;
    const size_t sample = (size_t)(mk ? parties + 1 : c->P.k + 1) * c->P.N * 4;
    if (slots > 0) {
        // (the table being replaced is freed first: its bytes count as free; a refused call keeps it)
        size_t free_b = 0, total_b = 0;
        HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
        const double held = (double)c->tlwe.slots * (double)c->sample_words() * 4;
        if ((double)slots * (double)sample > (double)free_b + held)
            return c->set_err(TFHE_ERR_NOMEM, "%s: %lld slots of %zu bytes do not fit the device's free memory (%zu bytes)", who, (long long)slots, sample, free_b);
    }
    if (c->tlwe.d) { (void)hipFree(c->tlwe.d); c->tlwe = {}; }
    if (slots == 0) return TFHE_OK;
    const hipError_t e = hipMalloc((void **)&c->tlwe.d, (size_t)slots * sample);
    if (e != hipSuccess) {
        c->tlwe.d = nullptr;
        (void)hipGetLastError();
        return c->set_err(TFHE_ERR_NOMEM, "%s: hipMalloc of %lld slots failed: %s", who, (long long)slots, hipGetErrorString(e));
    }
    c->tlwe.slots = slots;
    c->tlwe.parties = parties;
    return TFHE_OK;
}

// Slots [first, first + count) to (`up`) or from the caller's buffer.  The copy goes through the context's stream, behind the levels
// queued on it, and is waited for: the caller's buffer is free, or filled, on return; a slot is as wide as the table was allocated for.
static int32_t tlwe_copy(tfhe_ctx *c, const char *who, bool mk, bool up, int64_t first, int64_t count, int32_t *host)
{
    const int32_t rc = tlwe_state(c, who, mk);
    if (rc) return rc;
    if (!c->tlwe.d) return c->set_err(TFHE_ERR_STATE, "%s: no %s table allocated (%s)", who, mk ? "MK TLWE" : "TLWE", mk ? "tfhe_mk_tlwe_alloc" : "tfhe_tlwe_alloc");
    if (first < 0 || count < 0 || first > c->tlwe.slots || count > c->tlwe.slots - first || (count > 0 && !host))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: slot range [%lld, %lld + %lld) outside the table of %lld slots or NULL buffer", who, (long long)first,
                          (long long)first, (long long)count, (long long)c->tlwe.slots);
    if (count == 0) return TFHE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    { const int32_t rc0 = enter_stream(c, c->stream); if (rc0) return rc0; }
    const size_t sample = c->sample_words();
    int32_t *dev = c->tlwe.d + (size_t)first * sample;
    HIP_TRY(c, hipMemcpyAsync(up ? dev : host, up ? host : dev, (size_t)count * sample * 4, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return TFHE_OK;
}

int32_t tfhe_tlwe_alloc(tfhe_ctx *c, int64_t slots) try
{
    ENTER_CTX(c);
    return tlwe_alloc(c, "tlwe_alloc", false, slots);
}
ABI_CATCH(c, "tfhe_tlwe_alloc")

int32_t tfhe_tlwe_upload(tfhe_ctx *c, int64_t first, int64_t count, const int32_t *host) try
{
    ENTER_CTX(c);
    return tlwe_copy(c, "tlwe_upload", false, true, first, count, const_cast<int32_t *>(host));
}
ABI_CATCH(c, "tfhe_tlwe_upload")

int32_t tfhe_tlwe_download(tfhe_ctx *c, int64_t first, int64_t count, int32_t *host) try
{
    ENTER_CTX(c);
    return tlwe_copy(c, "tlwe_download", false, false, first, count, host);
}
ABI_CATCH(c, "tfhe_tlwe_download")

int32_t tfhe_mk_tlwe_alloc(tfhe_ctx *c, int64_t slots) try
{
    ENTER_CTX(c);
    return tlwe_alloc(c, "mk_tlwe_alloc", true, slots);
}
ABI_CATCH(c, "tfhe_mk_tlwe_alloc")

int32_t tfhe_mk_tlwe_upload(tfhe_ctx *c, int64_t first, int64_t count, const int32_t *host) try
{
    ENTER_CTX(c);
    return tlwe_copy(c, "mk_tlwe_upload", true, true, first, count, const_cast<int32_t *>(host));
}
ABI_CATCH(c, "tfhe_mk_tlwe_upload")

int32_t tfhe_mk_tlwe_download(tfhe_ctx *c, int64_t first, int64_t count, int32_t *host) try
{
    ENTER_CTX(c);
    return tlwe_copy(c, "mk_tlwe_download", true, false, first, count, host);
}
ABI_CATCH(c, "tfhe_mk_tlwe_download")

// ---- tfhe_blind_rotate_level ------------------------------------------------------------------------------------------------------
static const char *const WHO = "blind_rotate_level";

int32_t tfhe_blind_rotate_level(tfhe_ctx *c, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                                const int32_t *cst, const int32_t *sel, int32_t n_out, int32_t out_form, const int32_t *out_slot, const int32_t *out_wires,
                                int64_t B) try
{
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc_slot || !term_start)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc_slot, term_start)", WHO);
    const bool needs_wires = out_form == 2 || (B > 0 && term_start[B] > 0);
    int32_t rc = level_state(c, WHO, SINGLE_KEY, needs_wires, out_form == 2);
    if (rc) return rc;
    const int32_t steps = c->P.n;
    rc = rotate_level_check(c, WHO, SINGLE_KEY, acc_slot, term_start, term_wire, term_coef, n_out, out_form, out_slot, out_wires, B);
    if (rc) return rc;
    rc = rotate_check_selectors(c, WHO, SINGLE_KEY, out_form, sel, steps, "the context's n = ", "");
    if (rc || B == 0) return rc;
    RotatePlan p = {single_key_shape(c, "tlwe_rotate_level_kernel"), steps, sel, n_out, out_form, B};
    p.acc_slot = acc_slot, p.term_start = term_start, p.term_wire = term_wire, p.term_coef = term_coef, p.cst = cst;
    p.out_slot = out_slot, p.out_wires = out_wires;
    return run_rotation<leveled::RotateLevelArgs, leveled::tlwe_rotate_level_kernel>(
        c, WHO, p, [&](leveled::RotateLevelArgs &a, const int32_t *d_rows, const int32_t *d_out_slot) {
            a.tgsw = c->d_tgsw;
            a.rows = d_rows;
            a.out_slot = d_out_slot;
            a.ws = (int32_t *)c->lvl_ws[0].p;
            a.K1 = p.shape.polys, a.steps = steps, a.log2_n_out = ilog2i(n_out);
        });
}
ABI_CATCH(c, "tfhe_blind_rotate_level")
