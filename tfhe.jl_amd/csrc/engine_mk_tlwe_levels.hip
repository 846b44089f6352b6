// engine_mk_tlwe_levels.hip — tfhe_mk_blind_rotate_level: tfhe_mk_blind_rotate_batch with the accumulator read from a slot of the MK
// TLWE table (tfhe_mk_tlwe_alloc / _upload / _download: engine_tlwe_levels.hip, with the single-key table), the rotating multi-key LWE
// sample formed from wire-table rows as tfhe_mk_lut_level forms it, and the result left in a slot or, keyswitched, in wires:
// engine_tlwe_levels.hip's call under a multi-key cloud key.  The kernel (kernels_mk_tlwe_levels.hpp) is compiled here and nowhere
// else.  (tfhe_mk_rot_net_level: engine_mk_rot_net.hip; tfhe_mk_tgsw_update and tfhe_mk_tgsw_expand_update: engine_keys.hip.)
#define TFHE_EMIT_MK_TLWE_LEVEL_KERNELS
#include "engine.hpp"
#include "kernels_mk_tlwe_levels.hpp"
#include "leveled_checks.hpp"
#include "rotate_run.hpp"

static const char *const WHO = "mk_blind_rotate_level";

int32_t tfhe_mk_blind_rotate_level(tfhe_ctx *c, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                                   const int32_t *cst, const int32_t *sel, int32_t n_out, int32_t out_form, const int32_t *out_slot,
                                   const int32_t *out_wires, int64_t B) try
{
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc_slot || !term_start)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc_slot, term_start)", WHO);
    const bool needs_wires = out_form == 2 || (B > 0 && term_start[B] > 0);
    int32_t rc = level_state(c, WHO, MULTI_KEY, needs_wires, out_form == 2);
    if (rc) return rc;
    const int32_t steps = c->mk_parties * c->P.n;
    rc = rotate_level_check(c, WHO, MULTI_KEY, acc_slot, term_start, term_wire, term_coef, n_out, out_form, out_slot, out_wires, B);
    if (rc) return rc;
    rc = rotate_check_selectors(c, WHO, MULTI_KEY, out_form, sel, steps, "P n = ", " steps");
    if (rc || B == 0) return rc;
    RotatePlan p = {multi_key_shape(c, "mk_tlwe_rotate_level_kernel"), steps, sel, n_out, out_form, B};
    p.acc_slot = acc_slot, p.term_start = term_start, p.term_wire = term_wire, p.term_coef = term_coef, p.cst = cst;
    p.host_rows_without_terms = true;
    p.out_slot = out_slot, p.out_wires = out_wires;
    return run_rotation<leveled::MkRotateLevelArgs, leveled::mk_tlwe_rotate_level_kernel>(
        c, WHO, p, [&](leveled::MkRotateLevelArgs &a, const int32_t *d_rows, const int32_t *d_out_slot) {
            a.tgsw = c->d_mk_tgsw;
            a.rows = d_rows;
            a.party_of = c->d_mk_tgsw_party;
            a.out_slot = d_out_slot;
            a.ws = (int32_t *)c->lvl_ws[0].p;
            a.parties = c->mk_parties, a.steps = steps, a.log2_n_out = ilog2i(n_out);
        });
}
ABI_CATCH(c, "tfhe_mk_blind_rotate_level")
