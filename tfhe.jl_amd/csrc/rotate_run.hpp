// rotate_run.hpp — host-only: the one runner behind the four single-launch rotations of TLWE accumulators (tfhe_blind_rotate_batch:
// engine_blind_rotate.hip, tfhe_mk_blind_rotate_batch: engine_mk_blind_rotate.hip, tfhe_blind_rotate_level: engine_tlwe_levels.hip,
// tfhe_mk_blind_rotate_level: engine_mk_tlwe_levels.hip) and the two on the gates' kernel (tfhe_bootstrap_acc_batch, tfhe_bootstrap_acc_level:
// engine_bootstrap_acc.hip).  An entry point validates its arguments (leveled_checks.hpp), describes the
// call in a RotatePlan and names its kernel; the workspace protocol, the map, the uploads, the prologue, the launch, the keyswitch, the
// download and the timing are here and nowhere else: leveled_run.hpp's protocol for a call that is one launch and not a level loop.
// The launch itself is the caller's (run_rotation_on's launcher): AnyNRotation below for the four, V3AccRotation or, under option
// acc_dispatch, AccDispatchRotation for the two; MkW2AccRotation for their multi-key twins (tfhe_mk_bootstrap_acc_batch, tfhe_mk_bootstrap_acc_level:
// engine_mk_bootstrap_acc.hip).
#pragma once
#include "engine.hpp"
#include "leveled_run.hpp"

// One validated call on a device context: one launch over B rows of `steps` steps each, then the keyswitch of the B n_out extractions if
// asked.  The accumulators and the rotating rows come from the caller's buffers (acc != NULL: the batch calls) or from the device-resident
// tables (acc NULL: the level calls, row g's accumulator in slot acc_slot[g], its rows formed from wire-table rows by the terms); the
// result goes to the caller's buffer (out != NULL), to the slots out_slot (out_form 0) or, keyswitched, to the wires out_wires (2).
struct RotatePlan {
    SampleShape shape;
    int32_t steps;
    const int32_t *sel;         // host [steps], or NULL: selector i for step i
    int32_t n_out, out_form;
    int64_t B;
    // source, the caller's buffers:
    const int32_t *acc;         // host [T][polys][N]
    int64_t T;
    const int32_t *acc_index;   // host [B], or NULL: every row rotates accumulator 0
    const int32_t *rows;        // host [B][steps + 1]: LWE samples (in_form 0) or exponents (1)
    int32_t in_form;
    // source, the tables:
    const int32_t *acc_slot;    // host [B]
    const int32_t *term_start, *term_wire, *term_coef, *cst;      // tfhe_lut_level's combination: host [B + 1], [terms], [terms], [B] or NULL
    // A call without terms reads no wire: its rows are (0, ..., 0, cst[g]) switched to Z_2N.  The multi-key level call stages those on
    // the host with the map and launches no prologue, because the prologue takes the row width from the wire table, which such a call
    // may not have (the single-key one always has rows of n + 1 words, and always launches it).
    bool host_rows_without_terms;
    // destination:
    int32_t *out;               // host, by out_form 0: [B][polys][N], 1: [B n_out][ext_w], 2: [B n_out][ks_w]
    const int32_t *out_slot;    // host [B] (out_form 0)
    const int32_t *out_wires;   // host [B n_out] (out_form 2)
};

// The device side of one call as the runner staged it: what a launcher builds its kernel's arguments from.
struct RotateDev {
    const int32_t *in;          // the accumulators: the uploaded ones, or the TLWE table
    const int32_t *index;       // [B] acc_index or acc_slot (never NULL)
    const int32_t *sel;         // [steps]
    const int32_t *rows;        // [B][steps + 1] the staged rows
    const int32_t *out_slot;    // [B] out_slot or [G] out_wires (meaningful from the tables only)
    int32_t *out;               // out_form 0: the caller's samples [B][polys][N] or the TLWE table (rows out_slot); else NULL
    int32_t *ext;               // out_form 1, 2: [G][ext_w]; else NULL
    bool spec_lds;              // any-N kernels: spectrum accumulators in LDS
};

// The runner, over the launch.  A launcher L has
//   L.kGateRows       true: the kernel reads rows already switched to Z_2N, as the gates' kernels do: the batch calls' rows go through the
//                     modulus switch of tfhe_bootstrap_tv_batch (launch_modswitch) between events 0 and 1, and there are no per-row
//                     ping-pong samples and no global spectrum accumulators; false: the any-N rotation kernels, which switch themselves
//   L.prepare(c, d)   the kernel's arguments from d, the LDS grant of each kernel it will launch; before the timing slot is taken
//   L.launch(c, s)    the rotation's launch on s: one, or (AccDispatchRotation's split call) two over disjoint rows, one after the other
//   L.name(c, d)      tfhe_last_kernel_name
// Timing events as the gate entry points: what stages the rows between events 0 and 1 (outside slot 0), the rotation in slot 0, the
// keyswitch in slot 1.
template <class Launcher>
static int32_t run_rotation_on(tfhe_ctx *c, const char *who, const RotatePlan &p, Launcher &L)
{
    constexpr bool gate_rows = Launcher::kGateRows;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const SampleShape &sh = p.shape;
    const int N = c->P.N, M = N / 2 > 0 ? N / 2 : 1;
    const bool tables = !p.acc;
    const size_t sample = (size_t)sh.polys * N, steps = (size_t)p.steps, row_w = steps + 1;
    const size_t B_ = (size_t)p.B, G = B_ * (size_t)p.n_out, T = tables ? (size_t)p.term_start[B_] : 0, n_dst = p.out_form == 0 ? B_ : G;
    const bool host_rows = tables && !T && p.host_rows_without_terms;
    const bool fits = gate_rows || leveled::lds_bytes(N, sh.nspec) <= 160 * 1024;
    const bool spec_lds = gate_rows || (c->anyn_spec < 0 ? fits : (c->anyn_spec == 0 && fits));      // option anyn_spec: 1 = accumulators in global memory
    // e0 [G] (the keyswitch's identity map) | acc_index or acc_slot [B] | sel [steps] | and from the tables: term_start [B + 1] |
    // term_wire [T] | term_coef [T] | cst [B] (if any) | out_slot [B] or out_wires [G] | the rows [B][steps + 1] (if the host stages them)
    size_t end = 0;
    auto seg = [&end](size_t words) { const size_t at = (end + 63) / 64 * 64; end = at + words; return at; };
    const size_t o_e0 = seg(G), o_idx = seg(B_), o_sel = seg(steps);
    size_t o_start = 0, o_wire = 0, o_coef = 0, o_cst = 0, o_dst = 0, o_rows = 0;
    if (tables) {
        o_start = seg(B_ + 1), o_wire = seg(T), o_coef = seg(T);
        if (p.cst) o_cst = seg(B_);
        o_dst = seg(n_dst);
        if (host_rows) o_rows = seg(B_ * row_w);
    }
    const size_t map_bytes = end * 4, acc_bytes = tables ? 0 : (size_t)p.T * sample * 4;
    LvlWant want[9];
    int wants = 0;
    if (!tables) want[wants++] = {&c->lvl_data, acc_bytes};
    if (!gate_rows) want[wants++] = {&c->lvl_ws[0], B_ * 2 * sample * 4};
    if (gate_rows && !tables) want[wants++] = {&c->io[0], B_ * row_w * 4};      // the rows as uploaded, in front of the modulus switch
    if (p.out) want[wants++] = {&c->lvl_ws[1], p.out_form == 0 ? B_ * sample * 4 : 0};
    if (!gate_rows) want[wants++] = {&c->lvl_spec, spec_lds ? 0 : B_ * sh.nspec * M * sizeof(cplx)};
    want[wants++] = {&c->bara, host_rows ? 0 : B_ * row_w * 4};
    want[wants++] = {&c->ext, p.out_form >= 1 ? G * sh.ext_w * 4 : 0};
    if (p.out) want[wants++] = {&c->io[3], p.out_form == 2 ? G * sh.ks_w * 4 : 0};
    want[wants++] = {&c->map, map_bytes};
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }       // (the workspaces may still be in use by a call on another stream)
    int32_t rc = leveled_reserve(c, who, want, wants);
    if (rc) return rc;

    rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h = (int32_t *)c->h_map;
    for (size_t r = 0; r < G; r++) h[o_e0 + r] = (int32_t)r;
    const int32_t *index = tables ? p.acc_slot : p.acc_index;
    if (index) memcpy(h + o_idx, index, B_ * 4);
    else memset(h + o_idx, 0, B_ * 4);
    if (p.sel) memcpy(h + o_sel, p.sel, steps * 4);
    else for (int32_t i = 0; i < p.steps; i++) h[o_sel + i] = i;
    if (tables) {
        memcpy(h + o_start, p.term_start, (B_ + 1) * 4);
        if (T) {
            memcpy(h + o_wire, p.term_wire, T * 4);
            memcpy(h + o_coef, p.term_coef, T * 4);
        }
        if (p.cst) memcpy(h + o_cst, p.cst, B_ * 4);
        memcpy(h + o_dst, p.out_form == 0 ? p.out_slot : p.out_wires, n_dst * 4);
        if (host_rows) {
            const int shift = 32 - (ilog2i(N) + 1);      // decode_message(., 2N), numeric-functions.jl:31-34
            memset(h + o_rows, 0, B_ * row_w * 4);
            if (p.cst)
                for (size_t g = 0; g < B_; g++) h[o_rows + g * row_w + steps] = (int32_t)((uint32_t)p.cst[g] + (1u << (shift - 1))) >> shift;
        }
    }
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    if (!tables) {
        HIP_TRY(c, hipMemcpyAsync(c->lvl_data.p, p.acc, acc_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(c, hipMemcpyAsync(gate_rows ? c->io[0].p : c->bara.p, p.rows, B_ * row_w * 4, hipMemcpyHostToDevice, s));
    }
    const int32_t *d_map = (const int32_t *)c->map.p;

    RotateDev d;
    d.in = tables ? c->tlwe.d : (const int32_t *)c->lvl_data.p;
    d.index = d_map + o_idx;
    d.sel = d_map + o_sel;
    d.rows = host_rows ? d_map + o_rows : (const int32_t *)c->bara.p;
    d.out_slot = d_map + o_dst;
    d.out = p.out_form != 0 ? nullptr : tables ? c->tlwe.d : (int32_t *)c->lvl_ws[1].p;
    d.ext = p.out_form == 0 ? nullptr : (int32_t *)c->ext.p;
    d.spec_lds = spec_lds;
    rc = L.prepare(c, d);
    if (rc) return rc;

    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    if (tables && !host_rows) {
        // x_g, switched to Z_2N, into bara: tfhe_[mk_]lut_level's prologue (a row without terms reads no wire)
        rc = launch_linear_prologue(c, true, B_, d_map + o_start, d_map + o_wire, d_map + o_coef, p.cst ? d_map + o_cst : nullptr, nullptr, s);
        if (rc) return rc;
    }
    if (gate_rows && !tables) {
        rc = launch_modswitch(c, B_, (const int32_t *)c->io[0].p, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    rc = L.launch(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (p.out_form == 2) {
        rc = launch_keyswitch(c, G, d_map + o_e0, nullptr, tables ? d_map + o_dst : nullptr, (const int32_t *)c->ext.p, tables ? c->d_wires : (int32_t *)c->io[3].p, s);
        if (rc) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    if (!p.out) { /* the result stays on the device */ }
    else if (p.out_form == 0) HIP_TRY(c, hipMemcpyAsync(p.out, c->lvl_ws[1].p, B_ * sample * 4, hipMemcpyDeviceToHost, s));
    else if (p.out_form == 1) HIP_TRY(c, hipMemcpyAsync(p.out, c->ext.p, G * sh.ext_w * 4, hipMemcpyDeviceToHost, s));
    else HIP_TRY(c, hipMemcpyAsync(p.out, c->io[3].p, G * sh.ks_w * 4, hipMemcpyDeviceToHost, s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = p.B;
    c->diag_rows = 0;
    L.name(c, d);
    return TFHE_OK;
}

// The launch of the four any-N rotation kernels.  KERNEL takes A, one of the rotation argument structs on leveled::LevelArgs;
// set(a, d_rows, d_out_slot) fills the fields A adds to it and `tgsw`, with d_rows the staged rows and d_out_slot the device copy of
// out_slot.  One workgroup per row.
template <class A, void (*KERNEL)(A), class Set>
struct AnyNRotation {
    static constexpr bool kGateRows = false;
    const RotatePlan &p;
    Set set;
    A a;
    size_t lds;
    int32_t prepare(tfhe_ctx *c, const RotateDev &d)
    {
        const SampleShape &sh = p.shape;
        const int N = c->P.N;
        a.in = d.in;
        a.row_index = d.index;
        a.sel = d.sel;
        a.out = d.out;
        a.ext = d.ext;
        a.spec_g = d.spec_lds ? nullptr : (cplx *)c->lvl_spec.p;
        a.wtab = c->d_anyn_tab; a.twist = c->d_anyn_tab + N / 2;
        a.g = c->g;
        a.row_words = (int64_t)((size_t)sh.polys * N);
        a.L = c->P.bs_l; a.log2N = ilog2i(N);
        a.nodes_out = 1;
        set(a, d.rows, d.out_slot);
        lds = leveled::lds_bytes(N, d.spec_lds ? sh.nspec : 0);
        if (lds > 64 * 1024)        // (LDS_TRY's call, spelt out: the macro would name the template parameter, not the kernel, in its error)
            return ensure_dyn_lds(c, (const void *)KERNEL, lds, (std::string("leveled::") + sh.kernel).c_str());
        return TFHE_OK;
    }
    int32_t launch(tfhe_ctx *c, hipStream_t s)
    {
        hipLaunchKernelGGL(KERNEL, dim3((unsigned)p.B), dim3((unsigned)anyn::threads_for(c->P.N)), lds, s, a);
        HIP_TRY(c, hipGetLastError());
        return TFHE_OK;
    }
    void name(tfhe_ctx *c, const RotateDev &d)
    {
        const SampleShape &sh = p.shape;
        name_kernel(c, "%s(N=%d,%s=%d,l=%d,steps=%d%s)", sh.kernel, c->P.N, sh.mid_name, sh.mid, c->P.bs_l, p.steps, d.spec_lds ? "" : ",spec=global");
    }
};
template <class A, void (*KERNEL)(A), class Set>
static int32_t run_rotation(tfhe_ctx *c, const char *who, const RotatePlan &p, Set set)
{
    AnyNRotation<A, KERNEL, Set> L{p, set, A(), 0};
    return run_rotation_on(c, who, p, L);
}
