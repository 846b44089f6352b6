// engine_mk_bootstrap_acc.hip — tfhe_mk_bootstrap_acc_batch and tfhe_mk_bootstrap_acc_level: tfhe_mk_blind_rotate_batch's and
// tfhe_mk_blind_rotate_level's rotation of the caller's MK TLWE accumulators (one party's private table on jointly encrypted data, two-stage
// lookups) on the multi-key gates' own kernel and key: engine_bootstrap_acc.hip's calls under a multi-key cloud key.  This unit compiles
// mk_blind_rotate_kernel_w2 with TFHE_ACC_KERNELS (kernels_common.hpp, kernels_multikey.hpp): its ACC form,
// mk_blind_rotate_kernel_w2_acc, starts rotation w from X^{-barb} acc[acc_index[w]] on all three polynomials (mk_init_acc before the first
// barrier) and leaves the whole accumulator and / or its n_out extractions (mk_store_acc after the last hand-off); the step loop between
// the two is the kernel's, two waves per row, the accumulator LDS-resident.  The key is the multi-key bootstrapping key in the layout the
// gates read (c->d_mk_bk): no selector set is needed and a loaded one is left alone.  Exactly the two forms launch_mk_blind_rotate's
// `special` branch names without DIAG are instantiated: <4, no DIAG, 1 | 2>, that is 2 parties, N = 1024, l = 4.  There is one ACC family
// and the tuned and the any-party kernel read the same key layout, so option mk_general is ignored here.  The unit's compiler report is
// build/resource_usage_mk_bootstrap_acc.txt (tests/test_mk_bootstrap_acc_resources.py).  The host side of a call is rotate_run.hpp's,
// shared with the other rotation calls; the checks are leveled_checks.hpp's.
#define TFHE_ACC_KERNELS
#include "engine.hpp"
#include "leveled_checks.hpp"
#include "rotate_run.hpp"

// One launch of the ACC form with the geometry, LDS and rotations per workgroup of launch_mk_blind_rotate's `special` branch: option mk_rw,
// 0 = one rotation per workgroup up to one row per CU, pairs in lockstep beyond (an odd count gets a padding rotation).
struct MkW2AccRotation {
    static constexpr bool kGateRows = true;
    const RotatePlan &p;
    WithAcc<MkBrArgs> a;
    int rw;
    unsigned nblk;
    size_t lds;
    const void *kernel;

    int32_t prepare(tfhe_ctx *c, const RotateDev &d)
    {
        constexpr int NP = 2;
        const size_t R = (size_t)p.B;
        a.diag = DiagArgs{nullptr, nullptr, nullptr};
        a.R = (int32_t)R;
        a.bara = d.rows;
        a.bk = c->d_mk_bk;
        static_cast<MkBrArgs &>(a).ext = nullptr;      // (hidden by WithAcc's; the ACC form never reads it)
        a.T = c->T;
        a.g = c->g;
        a.n = c->P.n;
        a.mu = 0;
        a.prio_steps = (int32_t)((int64_t)NP * c->P.n * c->br_prio_pct / 100);
        a.acc = d.in;
        a.acc_index = d.index;
        a.out = d.out;
        a.out_index = p.acc ? nullptr : d.out_slot;      // (the tables: the final accumulator of row g goes to slot out_slot[g])
        a.ext = d.ext;
        a.log2_n_out = ilog2i(p.n_out);
        rw = c->mk_rw ? c->mk_rw : (R <= (size_t)c->cu_count ? 1 : 2);
        lds = (size_t)rw * ((NP + 1) * kImg * 4 + (2 * kXchElems + kM) * sizeof(cplx)) + 64 * sizeof(cplx) + 64;      // (+ the hand-off words of the pairs)
        nblk = (unsigned)((R + rw - 1) / rw);
        kernel = rw == 2 ? (const void *)mk_blind_rotate_kernel_w2_acc<4, false, 2> : (const void *)mk_blind_rotate_kernel_w2_acc<4, false, 1>;
        if (lds > 64 * 1024) return ensure_dyn_lds(c, kernel, lds, "mk_blind_rotate_kernel_w2_acc");
        return TFHE_OK;
    }
    int32_t launch(tfhe_ctx *c, hipStream_t s)
    {
        void *args[] = {(void *)&a};
        HIP_TRY(c, hipLaunchKernel(kernel, dim3(nblk), dim3(128 * rw), args, lds, s));
        return TFHE_OK;
    }
    void name(tfhe_ctx *c, const RotateDev &) { name_kernel(c, rw == 2 ? "mk_blind_rotate_kernel_w2_acc<%d,rw2>" : "mk_blind_rotate_kernel_w2_acc<%d>", c->P.bs_l); }
};

// what both calls refuse before they look at their arguments: the state of a multi-key leveled call (without the keys, which come after
// the arguments) ...
static int32_t mk_acc_state(tfhe_ctx *c, const char *who)
{
    if (c->P.parties < 2) return c->set_err(TFHE_ERR_STATE, "%s: context is single-key (tfhe_bootstrap_acc_batch / tfhe_bootstrap_acc_level are its calls)", who);
    if (c->multi()) return c->set_err(TFHE_ERR_STATE, "%s: multi-device context (leveled operations run on a one-device context)", who);
    if (c->measure_margin) return c->set_err(TFHE_ERR_STATE, "%s: measure_margin is on (the ACC form has no DIAG instantiation)", who);
    return TFHE_OK;
}
// ... and a shape the kernel does not serve, a key that is not in its layout
static int32_t mk_acc_shape(tfhe_ctx *c, const char *who)
{
    if (c->mk_bootstrap_acc()) return TFHE_OK;
    return c->set_err(TFHE_ERR_STATE,
                      "%s: %d parties, N = %d, l = %d%s: the kernel serves 2 parties, N = %d, l = 4 in the tuned key layout (tfhe_mk_blind_rotate_batch / "
                      "tfhe_mk_blind_rotate_level serve every shape)",
                      who, c->mk_acc_parties(), c->P.N, c->P.bs_l, c->anyn() ? " with the key in the any-N kernels' layout" : "", kN);
}

int32_t tfhe_mk_bootstrap_acc_batch(tfhe_ctx *c, const int32_t *acc, int64_t T, const int32_t *acc_index, const int32_t *rows, int32_t n_out, int32_t out_form,
                                    int32_t *out, int64_t B) try
{
    static const char *const WHO = "mk_bootstrap_acc_batch";
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc || !rows || !out)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc, rows, out)", WHO);
    int32_t rc = mk_acc_state(c, WHO);
    if (rc) return rc;
    rc = mk_acc_shape(c, WHO);
    if (rc) return rc;
    const int32_t steps = 2 * c->P.n;
    rc = rotate_batch_check(c, WHO, MK_GATE_KEY, T, acc_index, rows, steps, 0, nullptr, n_out, B, out_form);
    if (rc || B == 0) return rc;
    RotatePlan p = {multi_key_shape(c, "mk_blind_rotate_kernel_w2_acc"), steps, nullptr, n_out, out_form, B};
    p.acc = acc, p.T = T, p.acc_index = acc_index, p.rows = rows, p.in_form = 0, p.out = out;
    MkW2AccRotation L{p};
    return run_rotation_on(c, WHO, p, L);
}
ABI_CATCH(c, "tfhe_mk_bootstrap_acc_batch")

int32_t tfhe_mk_bootstrap_acc_level(tfhe_ctx *c, const int32_t *acc_slot, const int32_t *term_start, const int32_t *term_wire, const int32_t *term_coef,
                                    const int32_t *cst, int32_t n_out, int32_t out_form, const int32_t *out_slot, const int32_t *out_wires, int64_t B) try
{
    static const char *const WHO = "mk_bootstrap_acc_level";
    ENTER_CTX(c);
    if (B < 0) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: B = %lld is negative", WHO, (long long)B);
    if (B > 0 && (!acc_slot || !term_start)) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: NULL argument (acc_slot, term_start)", WHO);
    const bool needs_wires = out_form == 2 || (B > 0 && term_start[B] > 0);
    int32_t rc = level_state(c, WHO, MK_GATE_KEY, needs_wires, out_form == 2);
    if (rc) return rc;
    rc = mk_acc_shape(c, WHO);
    if (rc) return rc;
    const int32_t steps = 2 * c->P.n;
    rc = rotate_level_check(c, WHO, MK_GATE_KEY, acc_slot, term_start, term_wire, term_coef, n_out, out_form, out_slot, out_wires, B);
    if (rc) return rc;
    rc = rotate_check_selectors(c, WHO, MK_GATE_KEY, out_form, nullptr, steps, "P n = ", " steps");
    if (rc || B == 0) return rc;
    RotatePlan p = {multi_key_shape(c, "mk_blind_rotate_kernel_w2_acc"), steps, nullptr, n_out, out_form, B};
    p.acc_slot = acc_slot, p.term_start = term_start, p.term_wire = term_wire, p.term_coef = term_coef, p.cst = cst;
    p.host_rows_without_terms = true;
    p.out_slot = out_slot, p.out_wires = out_wires;
    MkW2AccRotation L{p};
    return run_rotation_on(c, WHO, p, L);
}
ABI_CATCH(c, "tfhe_mk_bootstrap_acc_level")
