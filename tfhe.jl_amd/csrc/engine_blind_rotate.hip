// engine_blind_rotate.hip — tfhe_blind_rotate_batch: the blind rotation of the caller's TLWE accumulators by LWE samples (or by
// exponents), on the caller's TGSW selectors (tfhe_tgsw_load, engine_keys.hip), returning the final accumulator, its extractions or
// those keyswitched.  The bridge from the bootstrapped half to the leveled one: private lookup tables, two-stage lookups, gate outputs
// as table entries.  The kernel (kernels_blind_rotate_tlwe.hpp) is compiled here and nowhere else.
#define TFHE_EMIT_BLIND_ROTATE_TLWE_KERNELS
#include "engine.hpp"
#include "kernels_blind_rotate_tlwe.hpp"
#include "leveled_checks.hpp"
#include "rotate_run.hpp"

static const char *const WHO = "blind_rotate_batch";

int32_t tfhe_blind_rotate_batch(tfhe_ctx *c, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t steps, int32_t in_form,
                                const int32_t *sel, int32_t n_out, int32_t *out, int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc || !rows || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc, rows, out)", WHO);
    int32_t rc = leveled_state(c, WHO);
    if (rc) return rc;
    rc = rotate_batch_check(c, WHO, SINGLE_KEY, T, acc_index, rows, steps, in_form, sel, n_out, B, out_form);
    if (rc || B == 0) return rc;
    RotatePlan p = {single_key_shape(c, "tlwe_rotate_kernel"), steps, sel, n_out, out_form, B};
    p.acc = acc, p.T = T, p.acc_index = acc_index, p.rows = rows, p.in_form = in_form, p.out = out;
    return run_rotation<leveled::RotateArgs, leveled::tlwe_rotate_kernel>(c, WHO, p, [&](leveled::RotateArgs &a, const int32_t *d_rows, const int32_t *) {
        a.tgsw = c->d_tgsw;
        a.rows = d_rows;
        a.ws = (int32_t *)c->lvl_ws[0].p;
        a.K1 = p.shape.polys, a.steps = steps, a.in_form = in_form, a.log2_n_out = ilog2i(n_out);
    });
}
ABI_CATCH(c, "tfhe_blind_rotate_batch")
