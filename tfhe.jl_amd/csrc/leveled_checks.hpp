// leveled_checks.hpp — host-only checks that more than one leveled unit makes before anything is uploaded: the state a multi-key
// leveled call needs (engine_mk_leveled.hip, engine_mk_cmux_net.hip, engine_mk_rot_net.hip, engine_mk_blind_rotate.hip; on the device-resident
// tables: engine_mk_rot_net.hip, engine_mk_tlwe_levels.hip) and the netlist of a CMUX network
// (engine_cmux_net.hip, engine_mk_cmux_net.hip; with monomial edges: engine_rot_net.hip, engine_mk_rot_net.hip).  Every function sets
// the context's error message, naming the caller `who`, and returns its code.
#pragma once
#include "engine.hpp"

enum { NET_MAX_LEVELS = 1024, NET_MAX_WIDTH = 4096 };

// what the single-key leveled entry points refuse before they look at their arguments
inline int32_t leveled_state(tfhe_ctx *c, const char *who)
{
    if (c->P.parties != 1) return c->set_err(TFHE_ERR_STATE, "%s: context is multi-key (leveled operations are single-key)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", who);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the CMUX level kernel has no DIAG instantiation)", who);
    return TFHE_OK;
}

// what the multi-key leveled entry points refuse before they look at their arguments
inline int32_t mk_leveled_state(tfhe_ctx *c, const char *who)
{
    if (c->P.parties < 2) return c->set_err(TFHE_ERR_STATE, "%s: context is single-key (tfhe_extern_mul_batch / tfhe_cmux_tree_batch are its leveled calls)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", who);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the CMUX level kernel has no DIAG instantiation)", who);
    if (!c->have_mk_bk) return c->set_err(TFHE_ERR_NO_KEY, "%s: no multi-key bootstrapping key loaded", who);
    if (!c->d_mk_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "%s: no selector set loaded (tfhe_mk_tgsw_load)", who);
    return TFHE_OK;
}

// what the multi-key level calls on the device-resident tables (tfhe_mk_rot_net_level, tfhe_mk_blind_rotate_level) refuse before they
// look at their arguments: the state first, then the key that fixes P.  `needs_wires`: the call reads or writes the wire table;
// `keyswitches`: out_form 2.  (The selector set and the keyswitch key are asked for after the arguments, as in the single-key calls.)
inline int32_t mk_level_state(tfhe_ctx *c, const char *who, bool needs_wires, bool keyswitches)
{
    if (c->P.parties < 2) return c->set_err(TFHE_ERR_STATE, "%s: context is single-key (tfhe_rot_net_level / tfhe_blind_rotate_level are its level calls)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", who);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the CMUX level kernel has no DIAG instantiation)", who);
    if (!c->d_mk_tlwe) return c->set_err(TFHE_ERR_STATE, "%s: no MK TLWE table allocated (tfhe_mk_tlwe_alloc)", who);
    if (needs_wires && !c->d_wires) return c->set_err(TFHE_ERR_STATE, "%s: no wire table allocated (out_form 2 and terms need one)", who);
    if (needs_wires && !c->wires_parties)
        return c->set_err(TFHE_ERR_STATE, "%s: the wire table has single-key rows (tfhe_wires_alloc): allocate it with tfhe_mk_wires_alloc", who);
    if (c->have_mk_bk) {
        if (c->mk_tlwe_parties != c->mk_parties)
            return c->set_err(TFHE_ERR_STATE, "%s: the MK TLWE table holds %d-party samples, the bootstrapping key is for %d parties", who, c->mk_tlwe_parties,
                              c->mk_parties);
        if (needs_wires && c->wires_parties != c->mk_parties)
            return c->set_err(TFHE_ERR_STATE, "%s: the wire table holds %d-party rows, the bootstrapping key is for %d parties", who, c->wires_parties, c->mk_parties);
        // (the keyswitch addresses rows by ITS key's parties, the levels write them by the bootstrapping key's: they must agree)
        if (keyswitches && c->have_mk_ks() && c->ks.parties != c->mk_parties)
            return c->set_err(TFHE_ERR_STATE, "%s: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties", who,
                              c->mk_parties, c->ks.parties);
    }
    if (!c->have_mk_bk) return c->set_err(TFHE_ERR_NO_KEY, "%s: no multi-key bootstrapping key loaded", who);
    return TFHE_OK;
}

// The public part of a CMUX-network call, O(nodes): the scalar arguments, every width (and B * width within one launch), every
// record's sources against the level below (E at level 0) and its var against V.  *total_nodes = sum of the widths.  A record has
// `words` words: (src0, src1, var), and with words = 5 the rotations (rot0, rot1) of a network with monomial edges, each in [0, two_n).
inline int32_t net_check_records(tfhe_ctx *c, const char *who, int64_t T, int32_t E, const int32_t *widths, int32_t levels, const int32_t *nodes,
                                 int32_t V, int64_t B, int32_t out_form, size_t *total_nodes, int words, int32_t two_n)
{
    if (levels < 1 || levels > NET_MAX_LEVELS) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: levels = %d (1 ... %d)", who, levels, (int)NET_MAX_LEVELS);
    if (E < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: E = %d (at least one table entry)", who, E);
    if (V < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: V = %d (at least one variable)", who, V);
    if (T < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: T = %lld (at least one table)", who, (long long)T);
    if ((double)T * (double)E > 2147483647.0)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: T * E = %.0f table entries (at most 2^31 - 1)", who, (double)T * (double)E);
    if (out_form < 0 || out_form > 2) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_form = %d (0 TLWE, 1 extracted, 2 key-switched)", who, out_form);
    size_t total = 0;
    for (int lv = 0; lv < levels; lv++) {
        if (widths[lv] < 1 || widths[lv] > NET_MAX_WIDTH)
            return c->set_err(TFHE_ERR_INVALID_ARG, "%s: widths[%d] = %d (1 ... %d)", who, lv, widths[lv], (int)NET_MAX_WIDTH);
        if ((double)B * (double)widths[lv] > 2147483647.0)
            return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B * widths[%d] = %.0f workgroups exceed one launch", who, lv, (double)B * (double)widths[lv]);
        total += (size_t)widths[lv];
    }
    const int32_t *rec = nodes;
    for (int lv = 0; lv < levels; lv++) {
        const int32_t below = lv == 0 ? E : widths[lv - 1];
        for (int i = 0; i < widths[lv]; i++, rec += words) {
            for (int e = 0; e < 2; e++)
                if (rec[e] < 0 || rec[e] >= below)
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: node %d of level %d: src%d = %d is outside the %d %s below", who, i, lv, e, rec[e], below,
                                      lv == 0 ? "table entries" : "nodes");
            if (rec[2] < 0 || rec[2] >= V)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: node %d of level %d: var = %d is outside [0, %d)", who, i, lv, rec[2], V);
            for (int e = 3; e < words; e++)
                if (rec[e] < 0 || rec[e] >= two_n)
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: node %d of level %d: rot%d = %d is outside [0, %d)", who, i, lv, e - 3, rec[e], two_n);
        }
    }
    *total_nodes = total;
    return TFHE_OK;
}

// the netlist of tfhe_cmux_net_batch / tfhe_mk_cmux_net_batch: records (src0, src1, var)
inline int32_t net_check_netlist(tfhe_ctx *c, const char *who, int64_t T, int32_t E, const int32_t *widths, int32_t levels, const int32_t *nodes,
                                 int32_t V, int64_t B, int32_t out_form, size_t *total_nodes)
{
    return net_check_records(c, who, T, E, widths, levels, nodes, V, B, out_form, total_nodes, 3, 0);
}

// the netlist of tfhe_rot_net_batch / tfhe_mk_rot_net_batch: records (src0, src1, var, rot0, rot1), the rotations public exponents of X in [0, 2N)
inline int32_t rot_check_netlist(tfhe_ctx *c, const char *who, int64_t T, int32_t E, const int32_t *widths, int32_t levels, const int32_t *nodes,
                                 int32_t V, int32_t N, int64_t B, int32_t out_form, size_t *total_nodes)
{
    return net_check_records(c, who, T, E, widths, levels, nodes, V, B, out_form, total_nodes, 5, 2 * N);
}

// The per-row part, O(B V): every selector against the `selectors` loaded ones, every table index against T (a CMUX tree: V = depth).
inline int32_t net_check_rows(tfhe_ctx *c, const char *who, const int32_t *sel, int32_t V, int64_t B, int64_t selectors, const int32_t *table_index, int64_t T)
{
    for (int64_t g = 0; g < B; g++)
        for (int32_t v = 0; v < V; v++) {
            const int32_t e = sel[g * V + v];
            if (e < 0 || e >= selectors)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel[%lld][%d] = %d is outside the %lld loaded selectors", who, (long long)g, (int)v, e,
                                  (long long)selectors);
        }
    if (table_index)
        for (int64_t g = 0; g < B; g++)
            if (table_index[g] < 0 || table_index[g] >= T)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: table_index[%lld] = %d is outside [0, %lld)", who, (long long)g, table_index[g], (long long)T);
    return TFHE_OK;
}
