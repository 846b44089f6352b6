// engine_rot_net.hip — leveled mode: tfhe_rot_net_batch, CMUX networks with a public monomial X^rot on every edge (blind rotation by
// TGSW bits for packed tables, weighted automata) on a caller's TGSW selectors (tfhe_tgsw_load, engine_keys.hip) and TLWE samples:
// engine_cmux_net.hip's call with five-word node records; the level kernel (kernels_rot_net.hpp) is compiled here and nowhere else
#define TFHE_EMIT_ROT_NET_KERNELS
#include "engine.hpp"
#include "kernels_leveled.hpp"
#include "kernels_rot_net.hpp"
#include "leveled_checks.hpp"

static const char *const WHO = "rot_net_batch";

// what the entry point refuses before it looks at its arguments (the conditions of engine_leveled.hip's entry points)
static int32_t rot_net_state(tfhe_ctx *c)
{
    if (c->P.parties != 1) return c->set_err(TFHE_ERR_STATE, "%s: context is multi-key (leveled operations are single-key)", WHO);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", WHO);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the network level kernel has no DIAG instantiation)", WHO);
    return TFHE_OK;
}

// One validated call on a device context: `levels` launches over B rows.  Level 0 reads row g's E samples at data[table_index[g]],
// level v > 0 the widths[v-1] outputs of the level below; the F = widths[levels-1] outputs of the last level are the result.
// Workspaces: buffer 0 holds the outputs of the even levels, buffer 1 those of the odd ones, each sized by its own widest level.
static int32_t run_rot_net(tfhe_ctx *c, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths, int32_t levels,
                           const int32_t *nodes, size_t total_nodes, const int32_t *sel, int32_t V, int32_t *out, int64_t B, int32_t out_form)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int N = c->P.N, K1 = c->P.k + 1, M = N / 2 > 0 ? N / 2 : 1, n = c->P.n, kNn = c->P.k * N;
    const size_t sample = (size_t)K1 * N;
    size_t wmax[2] = {0, 0}, wall = 0;                              // the widest even level, the widest odd level, the widest level
    for (int lv = 0; lv < levels; lv++) {
        const size_t w = (size_t)widths[lv];
        if (w > wmax[lv & 1]) wmax[lv & 1] = w;
        if (w > wall) wall = w;
    }
    const size_t B_ = (size_t)B, F = (size_t)widths[levels - 1], G = B_ * F;
    const bool fits = leveled::lds_bytes(N, K1) <= 160 * 1024;
    const bool spec_lds = c->anyn_spec < 0 ? fits : (c->anyn_spec == 0 && fits);
    auto up = [](size_t words) { return (words + 63) / 64 * 64; };
    // e0 [B F] (the keyswitch's identity map) | table_index [B] | sel [B][V] | nodes [total][5]
    const size_t o_idx = up(G), o_sel = o_idx + up(B_), o_nodes = o_sel + up(B_ * (size_t)V), map_bytes = (o_nodes + 5 * total_nodes) * 4;
    const size_t data_bytes = (size_t)T * (size_t)E * sample * 4;
    const LvlWant want[] = {
        {&c->lvl_data, data_bytes},
        {&c->lvl_ws[0], B_ * wmax[0] * sample * 4},
        {&c->lvl_ws[1], B_ * wmax[1] * sample * 4},
        {&c->lvl_spec, spec_lds ? 0 : B_ * wall * K1 * M * sizeof(cplx)},
        {&c->ext, out_form >= 1 ? G * (kNn + 1) * 4 : 0},
        {&c->io[3], out_form == 2 ? G * (n + 1) * 4 : 0},
        {&c->map, map_bytes},
    };
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }       // (the workspaces may still be in use by a call on another stream)
    int32_t rc = leveled_reserve(c, WHO, want, (int)(sizeof want / sizeof want[0]));
    if (rc) return rc;

    rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h = (int32_t *)c->h_map;
    for (size_t r = 0; r < G; r++) h[r] = (int32_t)r;
    if (table_index) memcpy(h + o_idx, table_index, B_ * 4);
    else memset(h + o_idx, 0, B_ * 4);
    memcpy(h + o_sel, sel, B_ * (size_t)V * 4);
    memcpy(h + o_nodes, nodes, 5 * total_nodes * 4);
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->lvl_data.p, data, data_bytes, hipMemcpyHostToDevice, s));
    const int32_t *d_map = (const int32_t *)c->map.p;

    leveled::RotNetArgs a;
    a.sel = d_map + o_sel;
    a.tgsw = c->d_tgsw;
    a.spec_g = spec_lds ? nullptr : (cplx *)c->lvl_spec.p;
    a.wtab = c->d_anyn_tab; a.twist = c->d_anyn_tab + N / 2;
    a.g = c->g;
    a.K1 = K1; a.L = c->P.bs_l; a.log2N = ilog2i(N);
    a.V = V;
    const size_t lds = leveled::lds_bytes(N, spec_lds ? K1 : 0);
    if (lds > 64 * 1024) LDS_TRY(c, lds, leveled::rot_net_level_kernel);
    const unsigned nt = (unsigned)anyn::threads_for(N);

    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    const int32_t *final_tlwe = nullptr;
    size_t first_node = 0;
    for (int lv = 0; lv < levels; lv++) {
        const size_t w = (size_t)widths[lv];
        const bool last = lv == levels - 1;
        a.in = lv == 0 ? (const int32_t *)c->lvl_data.p : (const int32_t *)c->lvl_ws[(lv - 1) & 1].p;
        a.row_index = lv == 0 ? d_map + o_idx : nullptr;
        a.row_words = (int64_t)((lv == 0 ? (size_t)E : (size_t)widths[lv - 1]) * sample);
        a.nodes = d_map + o_nodes + 5 * first_node;
        a.nodes_out = (int32_t)w;
        a.out = last && out_form != 0 ? nullptr : (int32_t *)c->lvl_ws[lv & 1].p;
        a.ext = last && out_form != 0 ? (int32_t *)c->ext.p : nullptr;
        if (last) final_tlwe = a.out;
        hipLaunchKernelGGL(leveled::rot_net_level_kernel, dim3((unsigned)(B_ * w)), dim3(nt), lds, s, a);
        HIP_TRY(c, hipGetLastError());
        first_node += w;
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (out_form == 2) {
        rc = launch_keyswitch(c, G, d_map, nullptr, nullptr, (const int32_t *)c->ext.p, (int32_t *)c->io[3].p, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    if (out_form == 0) HIP_TRY(c, hipMemcpyAsync(out, final_tlwe, G * sample * 4, hipMemcpyDeviceToHost, s));
    else if (out_form == 1) HIP_TRY(c, hipMemcpyAsync(out, c->ext.p, G * (kNn + 1) * 4, hipMemcpyDeviceToHost, s));
    else HIP_TRY(c, hipMemcpyAsync(out, c->io[3].p, G * (n + 1) * 4, hipMemcpyDeviceToHost, s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = 0;
    c->diag_rows = 0;
    name_kernel(c, spec_lds ? "rot_net_level_kernel(N=%d,k=%d,l=%d)" : "rot_net_level_kernel(N=%d,k=%d,l=%d,spec=global)", N, c->P.k, c->P.bs_l);
    return TFHE_OK;
}

int32_t tfhe_rot_net_batch(tfhe_ctx *c, const int32_t *data, int64_t T, int32_t E, const int32_t *table_index, const int32_t *widths, int32_t levels,
                           const int32_t *nodes, const int32_t *sel, int32_t V, int32_t *out, int64_t B, int32_t out_form) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (!widths || !nodes) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL network (widths, nodes)", WHO);
    if (B > 0 && (!data || !sel || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (data, sel, out)", WHO);
    int32_t rc = rot_net_state(c);
    if (rc) return rc;
    size_t total_nodes = 0;
    rc = rot_check_netlist(c, WHO, T, E, widths, levels, nodes, V, c->P.N, B, out_form, &total_nodes);
    if (rc) return rc;
    if (!c->d_tgsw) return c->set_err(TFHE_ERR_NO_KEY, "%s: no selector set loaded (tfhe_tgsw_load)", WHO);
    if (out_form == 2 && !c->have_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: out_form 2 needs the keyswitch key", WHO);
    rc = net_check_rows(c, WHO, sel, V, B, c->tgsw_count, table_index, T);
    if (rc) return rc;
    if (B == 0) return TFHE_OK;
    return run_rot_net(c, data, T, E, table_index, widths, levels, nodes, total_nodes, sel, V, out, B, out_form);
}
ABI_CATCH(c, "tfhe_rot_net_batch")
