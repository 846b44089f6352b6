// leveled_checks.hpp — host-only checks that more than one leveled unit makes before anything is uploaded: the state a leveled call
// needs (leveled_state: engine_leveled.hip, engine_cmux_net.hip, engine_rot_net.hip, engine_blind_rotate.hip; mk_leveled_state: their
// engine_mk_* forms; level_state: the four level calls on the device-resident tables, engine_rot_net.hip, engine_mk_rot_net.hip,
// engine_tlwe_levels.hip, engine_mk_tlwe_levels.hip), the arguments of the four TLWE rotation calls (rotate_check_*: the two batch units
// and the two level units), those of the level calls (rotate_level_check, net_level_check) and the netlist of a CMUX network
// (engine_cmux_net.hip, engine_mk_cmux_net.hip; with monomial edges: engine_rot_net.hip, engine_mk_rot_net.hip).  Every function sets
// the context's error message, naming the caller `who`, and returns its code.  The order of the refusals is behaviour.
#pragma once
#include "engine.hpp"
#include <unordered_set>

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

// The nouns by which the single-key and the multi-key calls on the device-resident tables differ where their checks do not, and the
// selector set and keyswitch key each kind asks for.  (no_wires is tfhe_rot_net_level's own: it has no terms to name.)
struct LevelKind {
    bool mk;
    const char *other_kind;     // what a context of the other kind is told
    const char *tlwe;           // the table's name
    const char *tlwe_alloc, *tgsw_load;
    const char *ks_key;
    const char *no_wires;       // the parenthetical of the "no wire table" refusal
    const char *other_wires;    // what a wire table of the other kind is told
    bool gate_key = false;      // the selectors are the context's bootstrapping key in the gates' layout, its n entries in order
    bool has_selectors(const tfhe_ctx *c) const { return gate_key ? (mk ? c->have_mk_bk : c->have_bk) : mk ? c->d_mk_tgsw != nullptr : c->d_tgsw != nullptr; }
    int64_t selectors(const tfhe_ctx *c) const { return gate_key ? (mk ? (int64_t)c->mk_parties * c->P.n : c->P.n) : mk ? c->mk_tgsw_count : c->tgsw_count; }
    bool has_ks(const tfhe_ctx *c) const { return mk ? c->have_mk_ks() : c->have_ks(); }
};
inline const LevelKind SINGLE_KEY = {false, "context is multi-key (leveled operations are single-key)", "TLWE", "tfhe_tlwe_alloc", "tfhe_tgsw_load",
                                     "the keyswitch key", "out_form 2 and terms need one", "the wire table has multi-key rows (tfhe_mk_wires_alloc)"};
inline const LevelKind MULTI_KEY = {true, "context is single-key (tfhe_rot_net_level / tfhe_blind_rotate_level are its level calls)", "MK TLWE",
                                    "tfhe_mk_tlwe_alloc", "tfhe_mk_tgsw_load", "the multi-key keyswitch key", "out_form 2 and terms need one",
                                    "the wire table has single-key rows (tfhe_wires_alloc): allocate it with tfhe_mk_wires_alloc"};
// the single-key calls that rotate on the gates' key and kernel (tfhe_bootstrap_acc_batch / _level): no selector set is read
inline const LevelKind GATE_KEY = {false, "context is multi-key (leveled operations are single-key)", "TLWE", "tfhe_tlwe_alloc", "tfhe_load_bootstrap_key_i32",
                                   "the keyswitch key", "out_form 2 and terms need one", "the wire table has multi-key rows (tfhe_mk_wires_alloc)", true};
// the multi-key calls that rotate on the multi-key gates' key and kernel (tfhe_mk_bootstrap_acc_batch / _level): the selectors are the
// multi-key bootstrapping key's P n entries in order, no selector set is read
inline const LevelKind MK_GATE_KEY = {true, "context is single-key (tfhe_bootstrap_acc_batch / tfhe_bootstrap_acc_level are its calls)", "MK TLWE",
                                      "tfhe_mk_tlwe_alloc", "tfhe_mk_load_bootstrap_key_i32", "the multi-key keyswitch key", "out_form 2 and terms need one",
                                      "the wire table has single-key rows (tfhe_wires_alloc): allocate it with tfhe_mk_wires_alloc", true};

// what the level calls on the device-resident tables (tfhe_[mk_]rot_net_level, tfhe_[mk_]blind_rotate_level) refuse before they look at
// their arguments: the state first, then (multi-key) the key that fixes P.  `needs_wires`: the call reads or writes the wire table;
// `keyswitches`: out_form 2.  (The selector set and the keyswitch key are asked for after the arguments: level_keys_check.)
inline int32_t level_state(tfhe_ctx *c, const char *who, const LevelKind &K, bool needs_wires, bool keyswitches)
{
    if (K.mk ? c->P.parties < 2 : c->P.parties != 1) return c->set_err(TFHE_ERR_STATE, "%s: %s", who, K.other_kind);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", who);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the CMUX level kernel has no DIAG instantiation)", who);
    if (!c->tlwe.d) return c->set_err(TFHE_ERR_STATE, "%s: no %s table allocated (%s)", who, K.tlwe, K.tlwe_alloc);
    if (needs_wires && !c->d_wires) return c->set_err(TFHE_ERR_STATE, "%s: no wire table allocated (%s)", who, K.no_wires);
    if (needs_wires && (c->wires_parties != 0) != K.mk) return c->set_err(TFHE_ERR_STATE, "%s: %s", who, K.other_wires);
    if (!K.mk) return TFHE_OK;
    if (c->have_mk_bk) {
        if (c->tlwe.parties != c->mk_parties)
            return c->set_err(TFHE_ERR_STATE, "%s: the MK TLWE table holds %d-party samples, the bootstrapping key is for %d parties", who, c->tlwe.parties,
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

// the selector set and, for out_form 2, the keyswitch key of a call of kind K: asked for after the call's arguments
inline int32_t level_keys_check(tfhe_ctx *c, const char *who, const LevelKind &K, int32_t out_form)
{
    if (!K.has_selectors(c)) return c->set_err(TFHE_ERR_NO_KEY, K.gate_key ? "%s: no bootstrapping key loaded (%s)" : "%s: no selector set loaded (%s)", who, K.tgsw_load);
    if (out_form == 2 && !K.has_ks(c)) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs %s", who, K.ks_key);
    // (the keyswitch addresses rows by ITS key's parties, the rotation writes them by the bootstrapping key's: they must agree; level_state
    //  has asked the level calls already)
    if (K.mk && out_form == 2 && c->ks.parties != c->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "%s: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties", who,
                          c->mk_parties, c->ks.parties);
    return TFHE_OK;
}

// What the four TLWE rotation entry points (tfhe_[mk_]blind_rotate_batch, tfhe_[mk_]blind_rotate_level) check alike, in the two places
// where they check it: the extractions of a row after the call's out_form ...
inline int32_t rotate_check_outputs(tfhe_ctx *c, const char *who, int32_t n_out, int32_t out_form, int64_t B)
{
    const int N = c->P.N;
    if (n_out < 1 || n_out > 32 || (n_out & (n_out - 1)) || (n_out > 1 && n_out > N / 4))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: n_out = %d (a power of two, at most 32, and 1 or at most N / 4 = %d)", who, n_out, N / 4);
    if (out_form == 0 && n_out != 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: n_out = %d with out_form 0 (the accumulator is one sample: n_out must be 1)", who, n_out);
    if ((double)B * (double)n_out > 2147483647.0)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B * n_out = %.0f rows exceed one launch", who, (double)B * (double)n_out);
    return TFHE_OK;
}

// ... and, after its other arguments, the keys and `sel` against the loaded selectors (NULL: selector i for step i).  A call names its
// step count "<steps_is><steps><steps_unit>".
inline int32_t rotate_check_selectors(tfhe_ctx *c, const char *who, const LevelKind &K, int32_t out_form, const int32_t *sel, int32_t steps, const char *steps_is,
                                      const char *steps_unit)
{
    const int32_t rc = level_keys_check(c, who, K, out_form);
    if (rc) return rc;
    const int64_t count = K.selectors(c);
    if (sel) {
        for (int32_t i = 0; i < steps; i++)
            if (sel[i] < 0 || sel[i] >= count)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel[%d] = %d is outside the %lld loaded selectors", who, (int)i, sel[i], (long long)count);
    } else if (steps > count) {
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: sel NULL names selector i for step i, %s%d%s, %lld selectors are loaded", who, steps_is, steps, steps_unit,
                          (long long)count);
    }
    return TFHE_OK;
}

// The arguments of tfhe_[mk_]blind_rotate_batch after [mk_]leveled_state: the scalars, the keys, then every index and, with in_form 1,
// every exponent.
enum { ROTATE_MAX_STEPS = 65536 };
inline int32_t rotate_batch_check(tfhe_ctx *c, const char *who, const LevelKind &K, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t steps,
                                  int32_t in_form, const int32_t *sel, int32_t n_out, int64_t B, int32_t out_form)
{
    const int N = c->P.N;
    if (steps < 1 || steps > ROTATE_MAX_STEPS) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: steps = %d (1 ... %d)", who, steps, (int)ROTATE_MAX_STEPS);
    if (in_form < 0 || in_form > 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: in_form = %d (0 LWE samples, 1 exponents)", who, in_form);
    if (out_form < 0 || out_form > 2) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_form = %d (0 TLWE, 1 extracted, 2 key-switched)", who, out_form);
    if (T < 1) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: T = %lld (at least one accumulator)", who, (long long)T);
    if (T > 2147483647LL) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: T = %lld accumulators (at most 2^31 - 1)", who, (long long)T);
    int32_t rc = rotate_check_outputs(c, who, n_out, out_form, B);
    if (rc) return rc;
    rc = rotate_check_selectors(c, who, K, out_form, sel, steps, "steps = ", "");
    if (rc) return rc;
    if (acc_index)
        for (int64_t g = 0; g < B; g++)
            if (acc_index[g] < 0 || acc_index[g] >= T)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: acc_index[%lld] = %d is outside [0, %lld)", who, (long long)g, acc_index[g], (long long)T);
    if (in_form == 1)
        for (int64_t g = 0; g < B; g++)
            for (int32_t i = 0; i <= steps; i++) {
                const int32_t e = rows[g * ((int64_t)steps + 1) + i];
                if (e < 0 || e >= 2 * N)
                    return c->set_err(TFHE_ERR_INVALID_ARG, "%s: rows[%lld][%d] = %d is outside [0, %d) (in_form 1: exponents)", who, (long long)g, (int)i, e, 2 * N);
            }
    return TFHE_OK;
}

// The arguments of tfhe_[mk_]blind_rotate_level after level_state: the scalars, then every term, slot and wire against the tables,
// no slot or wire written twice and none that the same call reads.
inline int32_t rotate_level_check(tfhe_ctx *c, const char *who, const LevelKind &K, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire,
                                  const int32_t *term_coef, int32_t n_out, int32_t out_form, const int32_t *out_slot, const int32_t *out_wires, int64_t B)
{
    const int64_t slots = c->tlwe.slots;
    if (B > (int64_t)1 << 30) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld rows exceed one launch", who, (long long)B);
    if (out_form != 0 && out_form != 2)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_form = %d (0 into %s slots, 2 key-switched into wires; extracted rows have no table)", who, out_form, K.tlwe);
    const int32_t rc = rotate_check_outputs(c, who, n_out, out_form, B);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    if (!(out_form == 0 ? out_slot : out_wires))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL %s with out_form %d", who, out_form == 0 ? "out_slot" : "out_wires", out_form);
    if (term_start[0] != 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term_start[0] = %d (must be 0)", who, term_start[0]);
    for (int64_t g = 0; g < B; g++)
        if (term_start[g + 1] < term_start[g]) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term_start decreases at row %lld", who, (long long)g);
    const int64_t T = term_start[B], G = B * n_out;
    if (T > 0 && (!term_wire || !term_coef)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: %lld terms and a NULL term array", who, (long long)T);
    for (int64_t t = 0; t < T; t++)
        if (term_wire[t] < 0 || term_wire[t] >= c->num_wires)
            return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term %lld reads wire %d, outside the table of %lld wires", who, (long long)t, term_wire[t], (long long)c->num_wires);
    for (int64_t g = 0; g < B; g++)
        if (acc_slot[g] < 0 || acc_slot[g] >= slots)
            return c->set_err(TFHE_ERR_INVALID_ARG, "%s: acc_slot[%lld] = %d is outside the table of %lld slots", who, (long long)g, acc_slot[g], (long long)slots);
    alloc_checkpoint();
    std::unordered_set<int32_t> written;
    written.reserve((size_t)G * 2);
    if (out_form == 0) {
        for (int64_t g = 0; g < B; g++) {
            if (out_slot[g] < 0 || out_slot[g] >= slots)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: out_slot[%lld] = %d is outside the table of %lld slots", who, (long long)g, out_slot[g], (long long)slots);
            if (!written.insert(out_slot[g]).second) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: slot %d written twice in one call", who, out_slot[g]);
        }
        for (int64_t g = 0; g < B; g++)
            if (written.count(acc_slot[g]))
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: acc_slot[%lld] = %d is an output slot of the same call", who, (long long)g, acc_slot[g]);
    } else {
        for (int64_t g = 0; g < G; g++) {
            if (out_wires[g] < 0 || out_wires[g] >= c->num_wires)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: output %lld is wire %d, outside the table of %lld wires", who, (long long)g, out_wires[g], (long long)c->num_wires);
            if (!written.insert(out_wires[g]).second) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: wire %d written twice in one call", who, out_wires[g]);
        }
        for (int64_t t = 0; t < T; t++)
            if (written.count(term_wire[t]))
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: term %lld reads wire %d, which the same call writes", who, (long long)t, term_wire[t]);
    }
    return TFHE_OK;
}

// The arguments of tfhe_[mk_]rot_net_level after its netlist (rot_check_netlist): the E entries every row reads and the G = B F
// outputs against the table, the output slots against the slots read, or the output wires against the wire table and each other.
inline int32_t net_level_check(tfhe_ctx *c, const char *who, const LevelKind &K, const int32_t *table_first, int32_t E, int64_t G, int64_t B, int32_t out_form,
                               int64_t out_first, const int32_t *out_wires)
{
    const int64_t slots = c->tlwe.slots;
    if (E > slots) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: E = %d entries, the %s table has %lld slots", who, E, K.tlwe, (long long)slots);
    if (table_first)
        for (int64_t g = 0; g < B; g++)
            if (table_first[g] < 0 || table_first[g] > slots - E)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: table_first[%lld] = %d: slots [%d, %d + %d) are outside the table of %lld slots", who, (long long)g,
                                  table_first[g], table_first[g], table_first[g], E, (long long)slots);
    if (B > 0 && out_form == 0) {
        if (out_first < 0 || out_first > slots || G > slots - out_first)
            return c->set_err(TFHE_ERR_INVALID_ARG, "%s: output slots [%lld, %lld + %lld) are outside the table of %lld slots", who, (long long)out_first,
                              (long long)out_first, (long long)G, (long long)slots);
        for (int64_t g = 0; g < B; g++) {
            const int64_t lo = table_first ? table_first[g] : 0;
            if (lo < out_first + G && out_first < lo + E)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: output slots [%lld, %lld + %lld) meet the slots [%lld, %lld + %d) that row %lld reads", who,
                                  (long long)out_first, (long long)out_first, (long long)G, (long long)lo, (long long)lo, E, (long long)g);
            if (!table_first) break;      // (every row reads the same range)
        }
    }
    if (B > 0 && out_form == 2) {
        if (!out_wires) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL out_wires with out_form 2", who);
        alloc_checkpoint();
        std::unordered_set<int32_t> written;
        written.reserve((size_t)G * 2);
        for (int64_t r = 0; r < G; r++) {
            if (out_wires[r] < 0 || out_wires[r] >= c->num_wires)
                return c->set_err(TFHE_ERR_INVALID_ARG, "%s: output %lld is wire %d, outside the table of %lld wires", who, (long long)r, out_wires[r], (long long)c->num_wires);
            if (!written.insert(out_wires[r]).second) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: wire %d written twice in one call", who, out_wires[r]);
        }
    }
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
