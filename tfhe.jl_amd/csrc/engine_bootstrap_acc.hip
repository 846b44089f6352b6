// engine_bootstrap_acc.hip — tfhe_bootstrap_acc_batch and tfhe_bootstrap_acc_level: tfhe_blind_rotate_batch's and tfhe_blind_rotate_level's
// rotation of the caller's TLWE accumulators (private lookup tables, two-stage lookups, a bootstrap's result as a table entry) on the
// gates' own kernel and key.  This unit compiles blind_rotate_kernel_v3 with TFHE_ACC_KERNELS (kernels_common.hpp): its ACC form,
// blind_rotate_kernel_v3_acc, starts rotation w from X^{-barb} acc[acc_index[w]] on both polynomials and leaves the whole accumulator
// and / or its n_out extractions; the step loop between the two is the kernel's, the accumulator LDS-resident, one WAVE per row.  The
// key is the context's bootstrapping key in the layout the gates read (c->d_bk): no selector set is needed and a loaded one is left
// alone.  Exactly the forms br_launch_v3 names without DIAG are instantiated: <2 | 3 | 0, 8, tw2reg, no DIAG, 1 | 4>.  The unit's
// compiler report is build/resource_usage_bootstrap_acc.txt (tests/test_bootstrap_acc_resources.py).  The host side of a call is
// rotate_run.hpp's, shared with the four calls on the any-N rotation kernels; the checks are leveled_checks.hpp's.
// Option acc_dispatch (0 by default: everything above, at every batch size) = 1 sends a call to the family a gate batch of its size
// takes: the ACC forms of blind_rotate_kernel_h2 and blind_rotate_kernel_w2 (engine_bootstrap_acc_small.hip, a unit and a report of their
// own) for small batches, this unit's v3 form above them, and the split of launch_blind_rotate (AccDispatchRotation below).
#define TFHE_ACC_KERNELS
#include "engine.hpp"
#include "leveled_checks.hpp"
#include "rotate_run.hpp"

// The arguments of a call's rotation as the runner staged it, all B rows: what every family's ACC form reads.
static WithAcc<BrArgs> acc_args(tfhe_ctx *c, const RotatePlan &p, const RotateDev &d)
{
    WithAcc<BrArgs> a;
    a.diag = DiagArgs{nullptr, nullptr, nullptr};
    a.bara = d.rows;
    a.bk = c->d_bk;
    static_cast<BrArgs &>(a).ext = nullptr;      // (hidden by WithAcc's; the ACC form never reads it)
    a.T = c->T;
    a.tan2 = reinterpret_cast<const double *>(c->d_tables + kTan2TableOffset);
    a.g = c->g;
    a.n = c->P.n;
    a.mu = 0;
    a.prio_steps = (int32_t)((int64_t)c->P.n * c->br_prio_pct / 100);
    a.R = (int32_t)p.B;
    a.l = c->P.bs_l;
    a.grp_big = a.grp_q = 0;
    a.acc = d.in;
    a.acc_index = d.index;
    a.out = d.out;
    a.out_index = p.acc ? nullptr : d.out_slot;      // (the tables: the final accumulator of row g goes to slot out_slot[g])
    a.ext = d.ext;
    a.log2_n_out = ilog2i(p.n_out);
    return a;
}
// ... and of rows [first, first + count) alone: the second launch of a split call
static WithAcc<BrArgs> acc_rows(WithAcc<BrArgs> a, size_t first, size_t count)
{
    a.bara += first * (size_t)(a.n + 1);
    a.acc_index += first;
    if (a.out_index) a.out_index += first;
    else if (a.out) a.out += first * (size_t)(2 * kN);
    if (a.ext) a.ext += (first << a.log2_n_out) * (size_t)(kN + 1);
    a.R = (int32_t)count;
    return a;
}

// One launch of the ACC form with v3's geometry: four rotations per workgroup in lockstep from 6 rotations per CU up (option v3_rw: 0 =
// by batch size, 1, 4), L = 2 / 3 / 0 by br_inst_l — what launch_blind_rotate_part decides for the kernel it was compiled from.  Rows
// [0, count) of the call (count 0: all of them).
struct V3AccRotation {
    static constexpr bool kGateRows = true;
    const RotatePlan &p;
    size_t count = 0;
    WithAcc<BrArgs> a;
    BrLaunch g;
    const void *kernel;

    template <int L>
    void pick()
    {
        if (g.rw == 4) kernel = (const void *)blind_rotate_kernel_v3_acc<L, 8, true, false, 4>;
        else kernel = (const void *)blind_rotate_kernel_v3_acc<L, 8, true, false, 1>;
    }
    int32_t prepare(tfhe_ctx *c, const RotateDev &d)
    {
        const size_t R = count ? count : (size_t)p.B;
        a = acc_rows(acc_args(c, p, d), 0, R);
        g = br_geo_v3(c, R, false);
        switch (g.L) {
        case 2: pick<2>(); break;
        case 3: pick<3>(); break;
        default: pick<0>(); break;
        }
        if (g.lds > 64 * 1024) return ensure_dyn_lds(c, kernel, g.lds, "blind_rotate_kernel_v3_acc");
        return TFHE_OK;
    }
    int32_t launch(tfhe_ctx *c, hipStream_t s)
    {
        void *args[] = {(void *)&a};
        HIP_TRY(c, hipLaunchKernel(kernel, g.grid, g.block, args, g.lds, s));
        return TFHE_OK;
    }
    void name(tfhe_ctx *c, const RotateDev &) { name_br(c, "v3_acc", g.L, g.rw == 4 ? ",8,tw2reg,rw4" : ",8,tw2reg"); }
};

// One launch of a multi-wave family's ACC form (engine_bootstrap_acc_small.hip) over rows [first, first + count) of the call, with the
// geometry launch_blind_rotate_part gives a gate batch of `count` rotations: blind_rotate_kernel_h2_acc where br_takes_h2 (4 l waves per
// row, one row per workgroup), else blind_rotate_kernel_w2_acc (two waves per row, pairs of rows by option w2_rw).
struct SmallAccLaunch {
    size_t first, count;
    bool h2;
    WithAcc<BrArgs> a;
    H2Tables ht;
    BrLaunch g;
    const void *kernel;

    int32_t prepare(tfhe_ctx *c, const WithAcc<BrArgs> &all)
    {
        a = acc_rows(all, first, count);
        h2 = br_takes_h2(c, count);
        ht = br_h2_tables(c);
        g = h2 ? br_geo_h2(c, count, false) : br_geo_w2(c, count, false);
        kernel = h2 ? acc_kernel_h2(g.L) : acc_kernel_w2(g.L, g.rw);
        if (!kernel) return c->set_err(TFHE_ERR_STATE, "bootstrap_acc: no ACC kernel for bs_l = %d (%s)", c->P.bs_l, h2 ? "h2" : "w2");
        if (g.lds > 64 * 1024) return ensure_dyn_lds(c, kernel, g.lds, h2 ? "blind_rotate_kernel_h2_acc" : "blind_rotate_kernel_w2_acc");
        return TFHE_OK;
    }
    int32_t launch(tfhe_ctx *c, hipStream_t s)
    {
        void *args[] = {(void *)&a, (void *)&ht};      // (the two-wave kernel takes the first alone)
        HIP_TRY(c, hipLaunchKernel(kernel, g.grid, g.block, args, g.lds, s));
        return TFHE_OK;
    }
    void name(tfhe_ctx *c)
    {
        if (h2) name_br(c, "h2_acc", g.L);
        else name_br(c, "w2_acc", g.L, g.rw == 2 ? ",rw2" : "");
    }
};

// Option acc_dispatch = 1: family and geometry by batch size, by the rules launch_blind_rotate / launch_blind_rotate_part apply to a gate
// batch at N = 1024, k = 1 (engine_dispatch.hip: br_takes_*, br_geo_*, br_split_tail; options br_tiny, br_small, br_rt_l, w2_rw, v3_rw,
// br_split).  Up to br_tiny rows h2_acc, up to br_small w2_acc, else v3_acc; a call above what the chip holds on the one-wave kernel whose
// last round is at most br_small rows is two launches on the same stream, the whole rounds on v3_acc and the tail on what its size takes.
struct AccDispatchRotation {
    static constexpr bool kGateRows = true;
    const RotatePlan &p;
    V3AccRotation v3;          // rule 3, and the whole rounds of a split call
    SmallAccLaunch small;      // rules 1 and 2, and the tail of a split call
    bool use_v3, use_small;

    explicit AccDispatchRotation(const RotatePlan &plan) : p(plan), v3{plan}, small(), use_v3(false), use_small(false) {}
    int32_t prepare(tfhe_ctx *c, const RotateDev &d)
    {
        const size_t R = (size_t)p.B, tail = br_split_tail(c, R);
        const bool whole_small = br_takes_h2(c, R) || br_takes_w2(c, R);
        use_small = whole_small || tail > 0;
        use_v3 = !whole_small;
        if (use_v3) {
            v3.count = R - tail;
            const int32_t rc = v3.prepare(c, d);
            if (rc) return rc;
        }
        if (use_small) {
            small.first = whole_small ? 0 : R - tail;
            small.count = whole_small ? R : tail;
            return small.prepare(c, acc_args(c, p, d));
        }
        return TFHE_OK;
    }
    int32_t launch(tfhe_ctx *c, hipStream_t s)
    {
        if (use_v3) {
            const int32_t rc = v3.launch(c, s);
            if (rc) return rc;
        }
        return use_small ? small.launch(c, s) : TFHE_OK;
    }
    void name(tfhe_ctx *c, const RotateDev &d)
    {
        std::string head;
        if (use_v3) {
            v3.name(c, d);
            head = c->last_kernel;
        }
        if (!use_small) return;
        small.name(c);
        if (use_v3) c->last_kernel = head + " + " + c->last_kernel;
    }
};

// the launcher of a call by option acc_dispatch
static int32_t run_acc_rotation(tfhe_ctx *c, const char *who, const RotatePlan &p)
{
    if (c->acc_dispatch) {
        AccDispatchRotation L(p);
        return run_rotation_on(c, who, p, L);
    }
    V3AccRotation L{p};
    return run_rotation_on(c, who, p, L);
}

// what both calls refuse after the state of a leveled call: a shape the kernel does not serve, a key that is not in its layout
static int32_t acc_shape(tfhe_ctx *c, const char *who)
{
    if (c->P.N != kN || c->P.k != 1)
        return c->set_err(TFHE_ERR_STATE, "%s: N = %d, k = %d: the kernel serves N = %d, k = 1 (tfhe_blind_rotate_batch serves every shape)", who, c->P.N, c->P.k, kN);
    if (c->anyn())
        return c->set_err(TFHE_ERR_STATE, "%s: N = %d, k = %d with br_anyn: the key is in the any-N kernels' layout (tfhe_blind_rotate_batch serves it)", who,
                          c->P.N, c->P.k);
    return TFHE_OK;
}

int32_t tfhe_bootstrap_acc_batch(tfhe_ctx *c, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t n_out, int32_t out_form,
                                 int32_t *out, int64_t B) try
{
    static const char *const WHO = "bootstrap_acc_batch";
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc || !rows || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc, rows, out)", WHO);
    int32_t rc = leveled_state(c, WHO);
    if (rc) return rc;
    rc = acc_shape(c, WHO);
    if (rc) return rc;
    const int32_t steps = c->P.n;
    rc = rotate_batch_check(c, WHO, GATE_KEY, T, acc_index, rows, steps, 0, nullptr, n_out, B, out_form);
    if (rc || B == 0) return rc;
    RotatePlan p = {single_key_shape(c, "blind_rotate_kernel_v3_acc"), steps, nullptr, n_out, out_form, B};
    p.acc = acc, p.T = T, p.acc_index = acc_index, p.rows = rows, p.in_form = 0, p.out = out;
    return run_acc_rotation(c, WHO, p);
}
ABI_CATCH(c, "tfhe_bootstrap_acc_batch")

int32_t tfhe_bootstrap_acc_level(tfhe_ctx *c, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                                 const int32_t *cst, int32_t n_out, int32_t out_form, const int32_t *out_slot, const int32_t *out_wires, int64_t B) try
{
    static const char *const WHO = "bootstrap_acc_level";
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc_slot || !term_start)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc_slot, term_start)", WHO);
    const bool needs_wires = out_form == 2 || (B > 0 && term_start[B] > 0);
    int32_t rc = level_state(c, WHO, GATE_KEY, needs_wires, out_form == 2);
    if (rc) return rc;
    rc = acc_shape(c, WHO);
    if (rc) return rc;
    const int32_t steps = c->P.n;
    rc = rotate_level_check(c, WHO, GATE_KEY, acc_slot, term_start, term_wire, term_coef, n_out, out_form, out_slot, out_wires, B);
    if (rc) return rc;
    rc = rotate_check_selectors(c, WHO, GATE_KEY, out_form, nullptr, steps, "the context's n = ", "");
    if (rc || B == 0) return rc;
    RotatePlan p = {single_key_shape(c, "blind_rotate_kernel_v3_acc"), steps, nullptr, n_out, out_form, B};
    p.acc_slot = acc_slot, p.term_start = term_start, p.term_wire = term_wire, p.term_coef = term_coef, p.cst = cst;
    p.out_slot = out_slot, p.out_wires = out_wires;
    return run_acc_rotation(c, WHO, p);
}
ABI_CATCH(c, "tfhe_bootstrap_acc_level")
