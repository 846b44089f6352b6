// engine_leveled.hip — leveled mode: tfhe_extern_mul_batch and tfhe_cmux_tree_batch on a caller's TGSW selectors (tfhe_tgsw_load,
// engine_keys.hip) and TLWE samples; the CMUX level kernel (kernels_leveled.hpp) is compiled here and nowhere else
#define TFHE_EMIT_LEVELED_KERNELS
#include "engine.hpp"
#include "kernels_leveled.hpp"
#include "leveled_run.hpp"
#include "leveled_checks.hpp"

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

// `depth` CMUX levels over B rows, level 0 reading row g's 2^depth samples at in[row_index[g]] (d0_zero: depth 1 and the one sample
// in[g], the plain external product): the network of widths 2^(depth-1) ... 1 whose kernel halves instead of reading records
static int32_t run_tree(tfhe_ctx *c, const char *who, const int32_t *in, int64_t in_rows, const int32_t *row_index, int32_t depth, bool d0_zero,
                        const int32_t *sel, int32_t *out, int64_t B, int32_t out_form)
{
    int32_t widths[12];
    tree_widths(widths, depth);
    LevelPlan p = {in, in_rows, d0_zero ? 1 : 1 << depth, row_index, d0_zero, sel, depth, widths, depth, "2^(depth-1)", nullptr, 0};
    p.shape = single_key_shape(c, "cmux_level_kernel");
    p.B = B, p.out = out, p.out_form = out_form;
    return run_leveled<leveled::Args, leveled::cmux_level_kernel>(c, who, p, [&](leveled::Args &a, int lv, const int32_t *) {
        a.tgsw = c->d_tgsw;
        a.K1 = p.shape.polys;
        a.depth = depth, a.level = lv;
        a.d0_zero = d0_zero ? 1 : 0;
    });
}

int32_t tfhe_extern_mul_batch(tfhe_ctx *c, const int32_t *tlwe_in, const int32_t *sel, int32_t *tlwe_out, int64_t B) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!tlwe_in || !sel || !tlwe_out))) return c->set_err(TFHE_ERR_INVALID_ARG, "extern_mul_batch: NULL argument or negative B");
    int32_t rc = leveled_state(c, "extern_mul_batch");
    if (rc) return rc;
    if (!c->d_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "extern_mul_batch: no selector set loaded (tfhe_tgsw_load)");
    rc = net_check_rows(c, "extern_mul_batch", sel, 1, B, c->tgsw_count, nullptr, B);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    return run_tree(c, "extern_mul_batch", tlwe_in, B, nullptr, 1, true, sel, tlwe_out, B, 0);
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
    rc = net_check_rows(c, "cmux_tree_batch", sel, depth, B, c->tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    return run_tree(c, "cmux_tree_batch", data, T, table_index, depth, false, sel, out, B, out_form);
}
ABI_CATCH(c, "tfhe_cmux_tree_batch")
