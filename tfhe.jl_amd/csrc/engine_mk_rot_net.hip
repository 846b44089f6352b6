// engine_mk_rot_net.hip — leveled mode under a multi-key cloud key: tfhe_mk_rot_net_batch, CMUX networks with a public monomial X^rot
// on every edge (packed tables read at jointly encrypted addresses, weighted automata over bits of several parties) on a caller's
// expanded RGSW selectors (tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load, engine_keys.hip) and MK TLWE samples: engine_mk_cmux_net.hip's
// call with five-word node records; the level kernel (kernels_mk_rot_net.hpp) is compiled here and nowhere else
#define TFHE_EMIT_MK_ROT_NET_KERNELS
#include "engine.hpp"
#include "kernels_mk_rot_net.hpp"
#include "leveled_run.hpp"
#include "leveled_checks.hpp"

static const char *const WHO = "mk_rot_net_batch";

int32_t tfhe_mk_rot_net_batch(tfhe_ctx *c, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths, int32_t levels,
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
    rc = rot_check_netlist(c, WHO, T, E, widths, levels, nodes, V, c->P.N, B, out_form, &total_nodes);
    if (rc) return rc;
    if (out_form == 2 && !c->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the multi-key keyswitch key", WHO);
    // (the keyswitch addresses rows by ITS key's parties, the levels write them by the bootstrapping key's: they must agree)
    if (out_form == 2 && c->ks.parties != c->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "%s: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties", WHO,
                          c->mk_parties, c->ks.parties);
    rc = net_check_rows(c, WHO, sel, V, B, c->mk_tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    LevelPlan p = {data, T, E, table_index, false, sel, V, widths, levels, "the widest level", nodes, 5};
    p.shape = multi_key_shape(c, "mk_rot_net_level_kernel");
    p.B = B, p.out = out, p.out_form = out_form;
    return run_leveled<leveled::MkRotNetArgs, leveled::mk_rot_net_level_kernel>(c, WHO, p, [&](leveled::MkRotNetArgs &a, int, const int32_t *d_nodes) {
        a.tgsw = c->d_mk_tgsw;
        a.nodes = d_nodes;
        a.party_of = c->d_mk_tgsw_party;
        a.parties = c->mk_parties;
        a.V = V;
    });
}
ABI_CATCH(c, "tfhe_mk_rot_net_batch")

// tfhe_mk_rot_net_batch between the device-resident tables: level 0 of row g reads source `src` at slot table_first[g] + src of the MK
// TLWE table (tfhe_mk_tlwe_alloc); the F outputs go to the slots out_first + g F + i (out_form 0) or, through the multi-key keyswitch,
// to the wires out_wires[g F + i] of the multi-key wire table (out_form 2).  tfhe_rot_net_level's contract argument for argument: the
// same kernel, unchanged, through the same runner: `in` is the table, row_index = table_first and a row is one sample wide; the last
// level's `out` is slot out_first, or its `ext` the keyswitch's input.
static const char *const WHO_LEVEL = "mk_rot_net_level";

int32_t tfhe_mk_rot_net_level(tfhe_ctx *c, const int32_t *table_first, int32_t E, const int32_t *widths, int32_t levels, const int32_t *nodes,
                              const int32_t *sel, int32_t V, int32_t out_form, int64_t out_first, const int32_t *out_wires, int64_t B) try
{
    ENTER_CTX(c);
    const char *const who = WHO_LEVEL;
    const LevelKind &K = MULTI_KEY;
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", who, (long long)B);
    if (!widths || !nodes) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL network (widths, nodes)", who);
    if (B > 0 && !sel) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (sel)", who);
    int32_t rc = level_state(c, who, K, out_form == 2, out_form == 2);
    if (rc) return rc;
    if (out_form != 0 && out_form != 2)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_form = %d (0 into %s slots, 2 key-switched into wires; extracted rows have no table)", who, out_form, K.tlwe);
    size_t total_nodes = 0;
    rc = rot_check_netlist(c, who, 1, E, widths, levels, nodes, V, c->P.N, B, out_form, &total_nodes);
    if (rc) return rc;
    rc = net_level_check(c, who, K, table_first, E, B * widths[levels - 1], B, out_form, out_first, out_wires);
    if (rc) return rc;
    rc = level_keys_check(c, who, K, out_form);
    if (rc) return rc;
    rc = net_check_rows(c, who, sel, V, B, K.selectors(c), nullptr, 1);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    LevelPlan p = {nullptr, 1, E, table_first, false, sel, V, widths, levels, "the widest level", nodes, 5};
    p.shape = multi_key_shape(c, "mk_rot_net_level_kernel");
    p.B = B, p.out = nullptr, p.out_form = out_form;
    p.d_data = c->tlwe.d, p.data_row_words = (int64_t)c->sample_words();
    if (out_form == 0) p.d_out = c->tlwe.d + (size_t)out_first * c->sample_words();
    else p.dst_rows = out_wires, p.d_ks_out = c->d_wires;
    return run_leveled<leveled::MkRotNetArgs, leveled::mk_rot_net_level_kernel>(c, who, p, [&](leveled::MkRotNetArgs &a, int, const int32_t *d_nodes) {
        a.tgsw = c->d_mk_tgsw;
        a.nodes = d_nodes;
        a.party_of = c->d_mk_tgsw_party;
        a.parties = c->mk_parties;
        a.V = V;
    });
}
ABI_CATCH(c, "tfhe_mk_rot_net_level")
