// engine_mk_leveled.hip — leveled mode under a multi-key cloud key: tfhe_mk_extern_mul_batch and tfhe_mk_cmux_tree_batch on a caller's
// expanded RGSW selectors (tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load, engine_keys.hip) and MK TLWE samples; the multi-key CMUX level
// kernel (kernels_mk_leveled.hpp) is compiled here and nowhere else
#define TFHE_EMIT_MK_LEVELED_KERNELS
#include "engine.hpp"
#include "kernels_mk_leveled.hpp"
#include "leveled_run.hpp"
#include "leveled_checks.hpp"

// engine_leveled.hip's run_tree on MK samples of (P + 1) polynomials
static int32_t run_mk_tree(tfhe_ctx *c, const char *who, const int32_t *in, int64_t in_rows, const int32_t *row_index, int32_t depth, bool d0_zero,
                           const int32_t *sel, int32_t *out, int64_t B, int32_t out_form)
{
    int32_t widths[12];
    tree_widths(widths, depth);
    LevelPlan p = {in, in_rows, d0_zero ? 1 : 1 << depth, row_index, d0_zero, sel, depth, widths, depth, "2^(depth-1)", nullptr, 0};
    p.shape = multi_key_shape(c, "mk_cmux_level_kernel");
    p.B = B, p.out = out, p.out_form = out_form;
    return run_leveled<leveled::MkArgs, leveled::mk_cmux_level_kernel>(c, who, p, [&](leveled::MkArgs &a, int lv, const int32_t *) {
        a.tgsw = c->d_mk_tgsw;
        a.party_of = c->d_mk_tgsw_party;
        a.parties = c->mk_parties;
        a.depth = depth, a.level = lv;
        a.d0_zero = d0_zero ? 1 : 0;
    });
}

int32_t tfhe_mk_extern_mul_batch(tfhe_ctx *c, const int32_t *tlwe_in, const int32_t *sel, int32_t *tlwe_out, int64_t B) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!tlwe_in || !sel || !tlwe_out))) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_extern_mul_batch: NULL argument or negative B");
    int32_t rc = mk_leveled_state(c, "mk_extern_mul_batch");
    if (rc) return rc;
    rc = net_check_rows(c, "mk_extern_mul_batch", sel, 1, B, c->mk_tgsw_count, nullptr, B);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    return run_mk_tree(c, "mk_extern_mul_batch", tlwe_in, B, nullptr, 1, true, sel, tlwe_out, B, 0);
}
ABI_CATCH(c, "tfhe_mk_extern_mul_batch")

int32_t tfhe_mk_cmux_tree_batch(tfhe_ctx *c, const int32_t *data, int64_t T, const int32_t *table_index, int32_t depth, const int32_t *sel, int32_t *out,
                                int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!data || !sel || !out))) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_cmux_tree_batch: NULL argument or negative B");
    if (c->P.parties < 2 || c->multi() || c->measure_margin) return mk_leveled_state(c, "mk_cmux_tree_batch");
    if (depth < 1 || depth > 12) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_cmux_tree_batch: depth = %d (1 ... 12)", depth);
    if (T < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_cmux_tree_batch: T = %lld (at least one table)", (long long)T);
    if (out_form < 0 || out_form > 2) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_cmux_tree_batch: out_form = %d (0 TLWE, 1 extracted, 2 key-switched)", out_form);
    int32_t rc = mk_leveled_state(c, "mk_cmux_tree_batch");
    if (rc) return rc;
    if (out_form == 2 && !c->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "mk_cmux_tree_batch: out_form 2 needs the multi-key keyswitch key");
    // (the keyswitch addresses rows by ITS key's parties, the levels write them by the bootstrapping key's: they must agree)
    if (out_form == 2 && c->ks.parties != c->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "mk_cmux_tree_batch: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties",
                          c->mk_parties, c->ks.parties);
    rc = net_check_rows(c, "mk_cmux_tree_batch", sel, depth, B, c->mk_tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    return run_mk_tree(c, "mk_cmux_tree_batch", data, T, table_index, depth, false, sel, out, B, out_form);
}
ABI_CATCH(c, "tfhe_mk_cmux_tree_batch")
