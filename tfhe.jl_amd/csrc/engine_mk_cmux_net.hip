// engine_mk_cmux_net.hip — leveled mode under a multi-key cloud key: tfhe_mk_cmux_net_batch, CMUX networks (automata, decision diagrams)
// wired by a public netlist on a caller's expanded RGSW selectors (tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load, engine_keys.hip) and
// MK TLWE samples; the multi-key network level kernel (kernels_mk_cmux_net.hpp) is compiled here and nowhere else
#define TFHE_EMIT_MK_CMUX_NET_KERNELS
#include "engine.hpp"
#include "kernels_mk_cmux_net.hpp"
#include "leveled_run.hpp"
#include "leveled_checks.hpp"

static const char *const WHO = "mk_cmux_net_batch";

int32_t tfhe_mk_cmux_net_batch(tfhe_ctx *c, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths, int32_t levels,
                               const int32_t *nodes, const int32_t *sel, int32_t V, int32_t *out, int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (!widths || !nodes) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL network (widths, nodes)", WHO);
    if (B > 0 && (!data || !sel || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (data, sel, out)", WHO);
    int32_t rc = mk_leveled_state(c, WHO);
    if (rc) return rc;
    size_t total_nodes = 0;
    rc = net_check_netlist(c, WHO, T, E, widths, levels, nodes, V, B, out_form, &total_nodes);
    if (rc) return rc;
    if (out_form == 2 && !c->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the multi-key keyswitch key", WHO);
    // (the keyswitch addresses rows by ITS key's parties, the levels write them by the bootstrapping key's: they must agree)
    if (out_form == 2 && c->ks.parties != c->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "%s: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties", WHO,
                          c->mk_parties, c->ks.parties);
    rc = net_check_rows(c, WHO, sel, V, B, c->mk_tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    LevelPlan p = {data, T, E, table_index, false, sel, V, widths, levels, "the widest level", nodes, 3};
    p.shape = multi_key_shape(c, "mk_cmux_net_level_kernel");
    p.B = B, p.out = out, p.out_form = out_form;
    return run_leveled<leveled::MkNetArgs, leveled::mk_cmux_net_level_kernel>(c, WHO, p, [&](leveled::MkNetArgs &a, int, const int32_t *d_nodes) {
        a.tgsw = c->d_mk_tgsw;
        a.nodes = d_nodes;
        a.party_of = c->d_mk_tgsw_party;
        a.parties = c->mk_parties;
        a.V = V;
    });
}
ABI_CATCH(c, "tfhe_mk_cmux_net_batch")
