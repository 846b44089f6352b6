// leveled_run.hpp — host-only: the one runner behind the leveled entry points (engine_leveled.hip, engine_mk_leveled.hip,
// engine_cmux_net.hip, engine_rot_net.hip, engine_mk_cmux_net.hip, engine_mk_rot_net.hip).  An entry point validates its arguments, describes the call in a
// LevelPlan and names its kernel; the workspace protocol, the uploads, the level loop, the keyswitch, the download and the timing are
// here and nowhere else.  tfhe_rot_net_level and tfhe_mk_rot_net_level run through it too: their sources and destinations are the
// device-resident (MK) TLWE and wire tables (LevelPlan's d_* fields), so nothing is uploaded but the maps and nothing is downloaded.
// (The four single-launch rotations have a runner of their own, rotate_run.hpp, on the same SampleShape.)
#pragma once
#include "engine.hpp"
#include "kernels_leveled_core.hpp"

// The samples a leveled call works on and the kernel it names: single_key_shape / multi_key_shape below.
struct SampleShape {
    int polys, nspec;         // polynomials per sample (k + 1 | P + 1); spectrum accumulators per workgroup (k + 1 | 3)
    size_t ext_w, ks_w;       // words of an extracted row (k N + 1 | P N + 1) and of a key-switched row (n + 1 | P n + 1)
    const char *kernel;       // tfhe_last_kernel_name: "<kernel>(N=..,<mid_name>=<mid>,l=..[,spec=global])"
    const char *mid_name;
    int mid;
};

// One validated call on a device context: `levels` launches over B rows.  Level 0 reads row g's E samples at data[row_index[g]],
// level v > 0 the widths[v-1] outputs of the level below; the F = widths[levels-1] outputs of the last level are the result.  A CMUX
// tree of depth d is the network of widths 2^(d-1) ... 1 over E = 2^d entries without node records (the kernel halves), the plain
// external product the one-level network of width 1 over E = 1 whose row g reads sample g.
struct LevelPlan {
    const int32_t *data;      // host [T][E][polys][N]
    int64_t T;
    int32_t E;
    const int32_t *row_index; // host [B], or NULL: every row reads row 0 (row_default_g: row g reads row g)
    bool row_default_g;
    const int32_t *sel;       // host [B][V]
    int32_t V;
    const int32_t *widths;    // host [levels]
    int32_t levels;
    const char *widest;       // how the caller's refusal of more than one launch's workgroups names its widest level
    const int32_t *nodes;     // host [sum of widths][words], or NULL with words = 0
    int words;
    SampleShape shape;
    int64_t B;
    int32_t *out;             // host, by out_form 0: the samples [B F][polys][N], 1: extracted at coefficient 0 [B F][ext_w], 2: that
    int32_t out_form;         //   keyswitched [B F][ks_w] (launch_keyswitch with identity maps)
    // device-resident sources and destinations (tfhe_rot_net_level; all NULL for the host-buffer calls above):
    const int32_t *d_data;    // level 0 reads this device table instead of an upload of `data` (`data` NULL): row g's E samples at
                              //   d_data[row_index[g]] with `data_row_words` words between two indices (0: E samples)
    int64_t data_row_words;
    int32_t *d_out;           // out_form 0: the last level writes its B F samples here, nothing is downloaded (`out` NULL)
    const int32_t *dst_rows;  // out_form 2: host [B F], the row of `d_ks_out` each keyswitched sample goes to (launch_keyswitch's dst
    int32_t *d_ks_out;        //   map), nothing is downloaded (`out` NULL)
};

// KERNEL takes A, one of the argument structs on leveled::LevelArgs; set(a, lv, d_nodes) fills the fields A adds to it, with d_nodes the
// device copy of level lv's records.  Workspaces: buffer 0 holds the outputs of the even levels, buffer 1 those of the odd ones, each
// sized by its own widest level.  Timing events as the gate entry points: levels in slot 0, keyswitch in slot 1.
template <class A, void (*KERNEL)(A), class Set>
static int32_t run_leveled(tfhe_ctx *c, const char *who, const LevelPlan &p, Set set)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int N = c->P.N, M = N / 2 > 0 ? N / 2 : 1;
    const size_t sample = (size_t)p.shape.polys * N;
    size_t wmax[2] = {0, 0}, wall = 0, total_nodes = 0;             // the widest even level, the widest odd level, the widest level
    for (int lv = 0; lv < p.levels; lv++) {
        const size_t w = (size_t)p.widths[lv];
        if (w > wmax[lv & 1]) wmax[lv & 1] = w;
        if (w > wall) wall = w;
        total_nodes += w;
    }
    const size_t B_ = (size_t)p.B, F = (size_t)p.widths[p.levels - 1], G = B_ * F;
    const bool fits = leveled::lds_bytes(N, p.shape.nspec) <= 160 * 1024;
    const bool spec_lds = c->anyn_spec < 0 ? fits : (c->anyn_spec == 0 && fits);      // option anyn_spec: 1 = accumulators in global memory
    auto up = [](size_t words) { return (words + 63) / 64 * 64; };
    // e0 [B F] (the keyswitch's identity map) | row_index [B] | sel [B][V] | nodes [total][words] | dst_rows [B F] (if any)
    const size_t o_idx = up(G), o_sel = o_idx + up(B_), o_nodes = o_sel + up(B_ * (size_t)p.V);
    const size_t o_dst = p.dst_rows ? o_nodes + up(p.words * total_nodes) : 0, map_bytes = p.dst_rows ? (o_dst + G) * 4 : (o_nodes + p.words * total_nodes) * 4;
    const size_t data_bytes = p.d_data ? 0 : (size_t)p.T * (size_t)p.E * sample * 4;
    const LvlWant want[] = {
        {&c->lvl_data, data_bytes},
        {&c->lvl_ws[0], B_ * wmax[0] * sample * 4},
        {&c->lvl_ws[1], B_ * wmax[1] * sample * 4},
        {&c->lvl_spec, spec_lds ? 0 : B_ * wall * p.shape.nspec * M * sizeof(cplx)},
        {&c->ext, p.out_form >= 1 ? G * p.shape.ext_w * 4 : 0},
        {&c->io[3], p.out_form == 2 && !p.d_ks_out ? G * p.shape.ks_w * 4 : 0},
        {&c->map, map_bytes},
    };
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }       // (the workspaces may still be in use by a call on another stream)
    int32_t rc = leveled_reserve(c, who, want, (int)(sizeof want / sizeof want[0]));
    if (rc) return rc;
    if ((double)p.B * (double)wall > 2147483647.0)
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B * %s = %.0f workgroups exceed one launch", who, p.widest, (double)p.B * (double)wall);

    rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h = (int32_t *)c->h_map;
    for (size_t r = 0; r < G; r++) h[r] = (int32_t)r;
    if (p.row_index) memcpy(h + o_idx, p.row_index, B_ * 4);
    else for (size_t g = 0; g < B_; g++) h[o_idx + g] = p.row_default_g ? (int32_t)g : 0;
    memcpy(h + o_sel, p.sel, B_ * (size_t)p.V * 4);
    if (p.words) memcpy(h + o_nodes, p.nodes, p.words * total_nodes * 4);
    if (p.dst_rows) memcpy(h + o_dst, p.dst_rows, G * 4);
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    if (!p.d_data) HIP_TRY(c, hipMemcpyAsync(c->lvl_data.p, p.data, data_bytes, hipMemcpyHostToDevice, s));
    const int32_t *d_map = (const int32_t *)c->map.p;

    A a;
    a.sel = d_map + o_sel;
    a.spec_g = spec_lds ? nullptr : (cplx *)c->lvl_spec.p;
    a.wtab = c->d_anyn_tab; a.twist = c->d_anyn_tab + N / 2;
    a.g = c->g;
    a.L = c->P.bs_l; a.log2N = ilog2i(N);
    const size_t lds = leveled::lds_bytes(N, spec_lds ? p.shape.nspec : 0);
    if (lds > 64 * 1024) {      // (LDS_TRY's call, spelt out: the macro would name the template parameter, not the kernel, in its error)
        rc = ensure_dyn_lds(c, (const void *)KERNEL, lds, (std::string("leveled::") + p.shape.kernel).c_str());
        if (rc) return rc;
    }
    const unsigned nt = (unsigned)anyn::threads_for(N);

    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    const int32_t *final_tlwe = nullptr;
    size_t first_node = 0;
    for (int lv = 0; lv < p.levels; lv++) {
        const size_t w = (size_t)p.widths[lv];
        const bool last = lv == p.levels - 1;
        a.in = lv == 0 ? (p.d_data ? p.d_data : (const int32_t *)c->lvl_data.p) : (const int32_t *)c->lvl_ws[(lv - 1) & 1].p;
        a.row_index = lv == 0 ? d_map + o_idx : nullptr;
        a.row_words = lv == 0 && p.d_data && p.data_row_words ? p.data_row_words : (int64_t)((lv == 0 ? (size_t)p.E : (size_t)p.widths[lv - 1]) * sample);
        a.nodes_out = (int32_t)w;
        a.out = last && p.out_form != 0 ? nullptr : last && p.d_out ? p.d_out : (int32_t *)c->lvl_ws[lv & 1].p;
        a.ext = last && p.out_form != 0 ? (int32_t *)c->ext.p : nullptr;
        set(a, lv, d_map + o_nodes + p.words * first_node);
        if (last) final_tlwe = a.out;
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)(B_ * w)), dim3(nt), lds, s, a);
        HIP_TRY(c, hipGetLastError());
        first_node += w;
    }
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (p.out_form == 2) {
        rc = launch_keyswitch(c, G, d_map, nullptr, p.dst_rows ? d_map + o_dst : nullptr, (const int32_t *)c->ext.p,
                              p.d_ks_out ? p.d_ks_out : (int32_t *)c->io[3].p, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    if (p.out_form == 0 ? p.d_out != nullptr : p.d_ks_out != nullptr) { /* the result stays on the device */ }
    else if (p.out_form == 0) HIP_TRY(c, hipMemcpyAsync(p.out, final_tlwe, G * sample * 4, hipMemcpyDeviceToHost, s));
    else if (p.out_form == 1) HIP_TRY(c, hipMemcpyAsync(p.out, c->ext.p, G * p.shape.ext_w * 4, hipMemcpyDeviceToHost, s));
    else HIP_TRY(c, hipMemcpyAsync(p.out, c->io[3].p, G * p.shape.ks_w * 4, hipMemcpyDeviceToHost, s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = 0;
    c->diag_rows = 0;
    name_kernel(c, "%s(N=%d,%s=%d,l=%d%s)", p.shape.kernel, N, p.shape.mid_name, p.shape.mid, c->P.bs_l, spec_lds ? "" : ",spec=global");
    return TFHE_OK;
}

// the single-key sample shape of a context: k + 1 polynomials and as many accumulators, rows of k N + 1 and n + 1 words
inline SampleShape single_key_shape(const tfhe_ctx *c, const char *kernel)
{
    return {c->P.k + 1, c->P.k + 1, (size_t)c->P.k * c->P.N + 1, (size_t)c->P.n + 1, kernel, "k", c->P.k};
}

// the multi-key one: P + 1 polynomials, three accumulators whatever P is, rows of P N + 1 and P n + 1 words
inline SampleShape multi_key_shape(const tfhe_ctx *c, const char *kernel)
{
    return {c->mk_parties + 1, 3, (size_t)c->mk_parties * c->P.N + 1, (size_t)c->mk_parties * c->P.n + 1, kernel, "P", c->mk_parties};
}

// the widths of a CMUX tree of `depth` <= 12 levels: 2^(depth-1-lv)
inline void tree_widths(int32_t (&widths)[12], int32_t depth)
{
    for (int lv = 0; lv < depth; lv++) widths[lv] = 1 << (depth - 1 - lv);
}
