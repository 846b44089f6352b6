// engine_rot_net.hip — leveled mode: tfhe_rot_net_batch, CMUX networks with a public monomial X^rot on every edge (blind rotation by
// TGSW bits for packed tables, weighted automata) on a caller's TGSW selectors (tfhe_tgsw_load, engine_keys.hip) and TLWE samples:
// engine_cmux_net.hip's call with five-word node records; the level kernel (kernels_rot_net.hpp) is compiled here and nowhere else
#define TFHE_EMIT_ROT_NET_KERNELS
#include "engine.hpp"
#include "kernels_rot_net.hpp"
#include "leveled_run.hpp"
#include "leveled_checks.hpp"

static const char *const WHO = "rot_net_batch";

int32_t tfhe_rot_net_batch(tfhe_ctx *c, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths, int32_t levels,
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
    rc = rot_check_netlist(c, WHO, T, E, widths, levels, nodes, V, c->P.N, B, out_form, &total_nodes);
    if (rc) return rc;
    if (!c->d_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "%s: no selector set loaded (tfhe_tgsw_load)", WHO);
    if (out_form == 2 && !c->have_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the keyswitch key", WHO);
    rc = net_check_rows(c, WHO, sel, V, B, c->tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    LevelPlan p = {data, T, E, table_index, false, sel, V, widths, levels, "the widest level", nodes, 5};
    p.shape = single_key_shape(c, "rot_net_level_kernel");
    p.B = B, p.out = out, p.out_form = out_form;
    return run_leveled<leveled::RotNetArgs, leveled::rot_net_level_kernel>(c, WHO, p, [&](leveled::RotNetArgs &a, int, const int32_t *d_nodes) {
        a.tgsw = c->d_tgsw;
        a.nodes = d_nodes;
        a.K1 = p.shape.polys;
        a.V = V;
    });
}
ABI_CATCH(c, "tfhe_rot_net_batch")

// tfhe_rot_net_batch between the device-resident tables: level 0 of row g reads source `src` at slot table_first[g] + src of the TLWE
// table (tfhe_tlwe_alloc); the F outputs go to the slots out_first + g F + i (out_form 0) or, keyswitched, to the wires
// out_wires[g F + i] (out_form 2).  The same kernel, unchanged, through the same runner: `in` is the table, row_index = table_first
// and a row is one sample wide; the last level's `out` is slot out_first, or its `ext` the keyswitch's input.
static const char *const WHO_LEVEL = "rot_net_level";
// (the single-key nouns, but this call has no terms to name when it has no wire table)
static const LevelKind ROT_NET_LEVEL = [] { LevelKind K = SINGLE_KEY; K.no_wires = "out_form 2 writes wires"; return K; }();

int32_t tfhe_rot_net_level(tfhe_ctx *c, const int32_t *table_first, int32_t E, const int32_t *widths, int32_t levels, const int32_t *nodes, const int32_t *sel,
                           int32_t V, int32_t out_form, int64_t out_first, const int32_t *out_wires, int64_t B) try
{
    ENTER_CTX(c);
    const char *const who = WHO_LEVEL;
    const LevelKind &K = ROT_NET_LEVEL;
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
    p.shape = single_key_shape(c, "rot_net_level_kernel");
    p.B = B, p.out = nullptr, p.out_form = out_form;
    p.d_data = c->tlwe.d, p.data_row_words = (int64_t)c->sample_words();
    if (out_form == 0) p.d_out = c->tlwe.d + (size_t)out_first * c->sample_words();
    else p.dst_rows = out_wires, p.d_ks_out = c->d_wires;
    return run_leveled<leveled::RotNetArgs, leveled::rot_net_level_kernel>(c, who, p, [&](leveled::RotNetArgs &a, int, const int32_t *d_nodes) {
        a.tgsw = c->d_tgsw;
        a.nodes = d_nodes;
        a.K1 = p.shape.polys;
        a.V = V;
    });
}
ABI_CATCH(c, "tfhe_rot_net_level")
