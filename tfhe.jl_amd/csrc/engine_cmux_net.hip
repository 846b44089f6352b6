// engine_cmux_net.hip — leveled mode: tfhe_cmux_net_batch, CMUX networks (automata, decision diagrams) wired by a public netlist on a
// caller's TGSW selectors (tfhe_tgsw_load, engine_keys.hip) and TLWE samples; the network level kernel (kernels_cmux_net.hpp) is
// compiled here and nowhere else
#define TFHE_EMIT_CMUX_NET_KERNELS
#include "engine.hpp"
#include "kernels_cmux_net.hpp"
#include "leveled_run.hpp"
#include "leveled_checks.hpp"

static const char *const WHO = "cmux_net_batch";

int32_t tfhe_cmux_net_batch(tfhe_ctx *c, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths, int32_t levels,
                            const int32_t *nodes, const int32_t *sel, int32_t V, int32_t *out, int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (!widths || !nodes) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL network (widths, nodes)", WHO);
    if (B > 0 && (!data || !sel || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (data, sel, out)", WHO);
    int32_t rc = leveled_state(c, WHO);
    if (rc) return rc;
    size_t total_nodes = 0;
    rc = net_check_netlist(c, WHO, T, E, widths, levels, nodes, V, B, out_form, &total_nodes);
    if (rc) return rc;
    if (!c->d_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "%s: no selector set loaded (tfhe_tgsw_load)", WHO);
    if (out_form == 2 && !c->have_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the keyswitch key", WHO);
    rc = net_check_rows(c, WHO, sel, V, B, c->tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    LevelPlan p = {data, T, E, table_index, false, sel, V, widths, levels, "the widest level", nodes, 3};
    p.shape = single_key_shape(c, "cmux_net_level_kernel");
    p.B = B, p.out = out, p.out_form = out_form;
    return run_leveled<leveled::NetArgs, leveled::cmux_net_level_kernel>(c, WHO, p, [&](leveled::NetArgs &a, int, const int32_t *d_nodes) {
        a.tgsw = c->d_tgsw;
        a.nodes = d_nodes;
        a.K1 = p.shape.polys;
        a.V = V;
    });
}
ABI_CATCH(c, "tfhe_cmux_net_batch")
