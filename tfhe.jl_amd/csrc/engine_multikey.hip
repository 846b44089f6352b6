// engine_multikey.hip — multi-key: tfhe_mk_gate_nand_batch (mk_gates.jl:7-12), the multi-key gate set (tfhe_mk_gates_batch,
// tfhe_mk_gates_level's body run_mk_gates) and the launch of their kernels
#include "engine.hpp"
#ifndef TFHE_NO_G2
#include "mk_g2_launch.hpp"
#endif

// The multi-key blind rotations of R samples: bara [R][P n + 1] -> ext [R][P N + 1], mu = encode_message(1, 8).  Picks the kernel
// by parameter set and batch size (the tuned 2-party kernel, the shipped 4- / 8-party two-wave kernels, the any-party kernel,
// the any-N kernel) and launches it on stream s; tfhe_last_kernel_name names it.  With tv, rotation w starts its body from
// X^{-barb} tv->tv[tv->index[w]] (the multi-key TV kernels, engine_mk_tv.hip and the mk_g2_tv objects: same family, geometry and LDS;
// "+tv" in the name); tv->bodies as launch_blind_rotate.
int32_t launch_mk_blind_rotate(tfhe_ctx *c, size_t R, hipStream_t s, const TvPtrs *tv)
{
    const int NP = c->mk_parties, n = c->P.n, Nn = c->P.N /* (1024 in every tuned branch below) */;
    if (tv && c->measure_margin) return c->set_err(TFHE_ERR_STATE, "mk_bootstrap_tv: no DIAG instantiation of the multi-key TV kernels (measure_margin is on)");
    MkBrArgs a;
    int32_t rc = prepare_diag(c, R, s, a.diag);
    if (rc) return rc;
    const bool dg = c->measure_margin;
    a.bara = (const int32_t *)c->bara.p; a.bk = c->d_mk_bk; a.ext = (int32_t *)c->ext.p; a.T = c->T; a.g = c->g;
    a.n = n; a.mu = (int32_t)(1u << 29); a.R = (int32_t)R;
    a.prio_steps = (int32_t)((int64_t)NP * n * c->br_prio_pct / 100);
    const size_t lds = (size_t)(NP + 1) * kImg * 4 + (kXchElems + 64) * sizeof(cplx);
    // 2 parties with l = 4 (mktfhe_parameters_2party, mk_api.jl:4-10): the tuned two-wave kernel; any other shape, and option
    // mk_general, the any-party kernel (round 3's one-wave 2-party kernel is gone: the any-party kernel is the cross-check)
    const bool special = (NP == 2 && c->P.bs_l == 4 && !c->mk_force_general);
    if (c->anyn()) {
        // any N, any number of parties, any l (kernels_anyn.hpp): one workgroup per rotation, accumulators in global memory
        const int M = Nn / 2;
        anyn::Args g;
        g.diag = a.diag; g.bara = a.bara; g.bk = a.bk; g.ext = a.ext; g.g = c->g; g.n = n; g.mu = a.mu; g.K1 = NP + 1; g.L = c->P.bs_l; g.R = (int32_t)R;
        g.log2N = ilog2i(Nn); g.parties = NP;
        g.wtab = c->d_anyn_tab; g.twist = c->d_anyn_tab + M;
        HIP_TRY(c, c->mk_acc.reserve(R * (NP + 1) * Nn * sizeof(int32_t)));
        g.acc = (int32_t *)c->mk_acc.p;
        const bool fits = anyn::lds_bytes(Nn, 3) <= 160 * 1024;
        const bool spec_lds = c->anyn_spec < 0 ? fits : (c->anyn_spec == 0 && fits);
        g.spec_g = nullptr;
        if (!spec_lds) {
            HIP_TRY(c, c->spec.reserve(R * 3 * (M > 0 ? M : 1) * sizeof(cplx)));
            g.spec_g = (cplx *)c->spec.p;
        }
        const size_t ldsa = anyn::lds_bytes(Nn, spec_lds ? 3 : 0);
        const unsigned nt = (unsigned)anyn::threads_for(Nn);
        if (tv) {
            rc = mk_tv_launch_anyn(c, with_tv(g, *tv), (unsigned)R, nt, ldsa, s);
            if (rc) return rc;
        } else if (dg) {
            if (ldsa > 64 * 1024) LDS_TRY(c, ldsa, anyn::mk_blind_rotate_kernel<true>);
            hipLaunchKernelGGL((anyn::mk_blind_rotate_kernel<true>), dim3((unsigned)R), dim3(nt), ldsa, s, g);
        } else {
            if (ldsa > 64 * 1024) LDS_TRY(c, ldsa, anyn::mk_blind_rotate_kernel<false>);
            hipLaunchKernelGGL((anyn::mk_blind_rotate_kernel<false>), dim3((unsigned)R), dim3(nt), ldsa, s, g);
        }
        name_kernel(c, spec_lds ? "mk_blind_rotate_kernel_anyn(N=%d,P=%d,l=%d)" : "mk_blind_rotate_kernel_anyn(N=%d,P=%d,l=%d,spec=global)", Nn, NP, c->P.bs_l);
    } else if (special) {
        // two waves per rotation: acc[3][N] | xch[2] | second hand-off slot [M] | tw2   (39.4 KB: four workgroups per CU)
        // mk_rw rotations per workgroup in lockstep (2: default: 78.8 KB, two workgroups per CU; 1: 39.4 KB, four; DIAG: 1)
        const int rw = dg ? 1 : c->mk_rw ? c->mk_rw : (R <= (size_t)c->cu_count ? 1 : 2);
        const size_t lds2 = (size_t)rw * ((NP + 1) * kImg * 4 + (2 * kXchElems + kM) * sizeof(cplx)) + 64 * sizeof(cplx) + 64;      // (+ the hand-off words of the pairs)
        const unsigned nblk = (unsigned)((R + rw - 1) / rw);
        a.R = (int32_t)R;
#define LAUNCH_MK2(LL, DG, RWV)                                                                                    \
        do {                                                                                                       \
            if (lds2 > 64 * 1024)                                                                                  \
                LDS_TRY(c, lds2, mk_blind_rotate_kernel_w2<LL, DG, RWV>); \
            hipLaunchKernelGGL((mk_blind_rotate_kernel_w2<LL, DG, RWV>), dim3(nblk), dim3(128 * RWV), lds2, s, a);  \
        } while (0)
        if (tv) {
            rc = mk_tv_launch_w2(c, with_tv(a, *tv), rw, nblk, lds2, s);
            if (rc) return rc;
        } else if (dg) LAUNCH_MK2(4, true, 1);
        else if (rw == 2) LAUNCH_MK2(4, false, 2);
        else LAUNCH_MK2(4, false, 1);
#undef LAUNCH_MK2
        name_kernel(c, "mk_blind_rotate_kernel_w2<%d>", c->P.bs_l);
#ifndef TFHE_NO_G2      // (-DTFHE_NO_G2: quick development builds without the many-party two-wave kernel, 1 instead of 5 minutes)
    } else if (!c->mk_force_general && c->mkg_variant != 1 && ((NP == 4 && c->P.bs_l == 5) || (NP == 8 && c->P.bs_l == 8))) {
        // the shipped 4- and 8-party sets (mk_api.jl:16-34): compile-time (parties, l), two waves per rotation at two waves per
        // SIMD, accumulators in global memory.  LDS: two transposition buffers per rotation and the pass-B twiddle table;
        // two rotations per workgroup in lockstep (a single rotation gets a padding partner)
        MkGenArgs ga;
        ga.diag = a.diag; ga.R = (int32_t)R; ga.bara = a.bara; ga.bk = a.bk; ga.ext = a.ext; ga.T = a.T; ga.g = a.g; ga.n = n; ga.mu = a.mu; ga.parties = NP; ga.L = c->P.bs_l;
        ga.prio_steps = a.prio_steps;
        // rotations per workgroup, in lockstep (they share their key fetches): "mkg_rw" 2 | 4, default 4 = one workgroup of
        // eight waves per CU.  The 8-party key is 4.7 GB as spectra: with pairs the launch moves 2.2 TB beyond L2 (4.9 TB/s,
        // L2 hit 59 %, profiles/r03/r03l_mk8: every pair streams the whole key for itself) and takes 450 ms; four rotations
        // per workgroup halve that traffic: 388 ms.  4 parties: 73.1 vs 73.9 ms.  The DIAG instantiation exists for pairs only.
        // (Measured dead end: pacing the workgroups of an XCD — a counter per XCD, one lane per workgroup waiting, bounded,
        //  until its XCD's workgroups have all finished the step, so that they share key lines in their L2 — costs more in
        //  waiting for the slowest of 32 than it saves: 8 parties 424 vs 403 ms, 4 parties 94 vs 80 ms on one device.)
        // (up to two rotations per CU the pairs win: 4 parties 54 vs 69 ms at 512 rotations, 62 vs 79 ms for a single gate;
        //  8 parties 298 vs 374 ms at 256 — profiles/r03/r03j_*)
        // 4 parties: the five accumulator images (21.8 KB per rotation) fit LDS beside the transposition buffers at four
        // rotations per CU — 81 408 B per pair of rotations = 40 LDS granules of 2 KB, two pairs or one group of four per CU —
        // so the step needs neither the trip to L2 nor the workgroup-scope fence (round 4: 66.2 vs 73.6 ms; at 8 parties nine
        // images do not fit and the accumulators stay in global memory)
        const bool acc_lds = NP == 4;
        const int rw = dg ? 2 : (c->mkg_rw == 2 || c->mkg_rw == 4) ? c->mkg_rw : (R <= 2 * (size_t)c->cu_count ? 2 : 4);
        const size_t ldsg2 = (size_t)rw * 2 * kXchElems * sizeof(cplx) + 64 * sizeof(cplx) + (acc_lds ? (size_t)rw * (NP + 1) * kImg * sizeof(int32_t) : 0);
        const unsigned nblk = (unsigned)((R + rw - 1) / rw);
        ga.acc = nullptr;
        if (!acc_lds) {
            HIP_TRY(c, c->mk_acc.reserve((size_t)nblk * rw * (NP + 1) * kImg * sizeof(int32_t)));
            ga.acc = (int32_t *)c->mk_acc.p;
        }
        if (tv) HIP_TRY(c, tfhe_launch_mk_g2_tv(NP, rw, nblk, ldsg2, s, with_tv(ga, *tv)));
        else HIP_TRY(c, tfhe_launch_mk_g2(NP, dg, rw, acc_lds, nblk, ldsg2, s, ga));
        name_kernel(c, acc_lds ? "mk_blind_rotate_kernel_g2<%d,%d,acc=lds>" : "mk_blind_rotate_kernel_g2<%d,%d>", NP, c->P.bs_l);
#endif
    } else {
        MkGenArgs ga;
        ga.diag = a.diag; ga.R = (int32_t)R; ga.bara = a.bara; ga.bk = a.bk; ga.ext = a.ext; ga.T = a.T; ga.g = a.g; ga.n = n; ga.mu = a.mu; ga.parties = NP; ga.L = c->P.bs_l;
        // the kernel needs a whole SIMD's registers, so a CU holds four waves whatever the grouping: as many rotations per
        // workgroup (in lockstep, sharing their key fetches) as fit in LDS, four at most
        // accumulators in global memory: LDS holds only the transposition buffer, eight waves fit a CU whatever P is
        const bool accg = c->mkg_acc < 0 ? NP > 4 : c->mkg_acc != 0;
        const size_t lds_rot = accg ? (kXchElems + 64) * sizeof(cplx) : lds;
        // (two rotations per workgroup: 82 vs 86 ms with four or one at 4 parties, 476 vs 481 / 765 at 8 — round 2; the three- and
        //  four-rotation instantiations are gone)
        int rw = (int)std::min<size_t>(2, (160 * 1024) / lds_rot);
        if (c->mkg_rw == 1 || R < 2 || rw < 1 || dg) rw = 1;       // (the DIAG instantiations exist for single rotations only)
        const size_t ldsg = (size_t)rw * lds_rot;
        const unsigned nblk = (unsigned)((R + rw - 1) / rw);
        ga.acc = nullptr;
        ga.prio_steps = 0;
        if (accg) {
            HIP_TRY(c, c->mk_acc.reserve((size_t)nblk * rw * (NP + 1) * kImg * sizeof(int32_t)));
            ga.acc = (int32_t *)c->mk_acc.p;
        }
#define LAUNCH_MKG(DG, RWV)                                                                                        \
        do {                                                                                                       \
            if (ldsg > 64 * 1024)                                                                                  \
                LDS_TRY(c, ldsg, mk_blind_rotate_kernel_general<DG, RWV, false>); \
            if (accg) hipLaunchKernelGGL((mk_blind_rotate_kernel_general<DG, RWV, true>), dim3(nblk), dim3(64 * RWV), ldsg, s, ga); \
            else hipLaunchKernelGGL((mk_blind_rotate_kernel_general<DG, RWV, false>), dim3(nblk), dim3(64 * RWV), ldsg, s, ga); \
        } while (0)
        if (tv) {
            rc = mk_tv_launch_general(c, with_tv(ga, *tv), rw, accg, nblk, ldsg, s);
            if (rc) return rc;
        } else if (dg) LAUNCH_MKG(true, 1);
        else if (rw == 2) LAUNCH_MKG(false, 2);
        else LAUNCH_MKG(false, 1);
#undef LAUNCH_MKG
        name_kernel(c, accg ? "mk_blind_rotate_kernel_general(P=%d,L=%d,acc=global)" : "mk_blind_rotate_kernel_general(P=%d,L=%d)", NP, c->P.bs_l);
    }
    if (tv) c->last_kernel += "+tv";
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tfhe_mk_gate_nand_batch(tfhe_ctx *c, const int32_t *in0, const int32_t *in1, int32_t *out, int64_t B) try
{
    ENTER_CTX(c);
    if (!c) return TFHE_ERR_INVALID_ARG;
    if (B < 0 || (B > 0 && (!in0 || !in1 || !out))) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_gate_nand_batch: NULL argument or negative B");
    if (B == 0) return TFHE_OK;
    if (c->multi()) {
        const tfhe_ctx *k0 = c->kids[0];
        if (!k0->have_mk_bk || !k0->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "mk_gate_nand_batch: multi-key keys not loaded");
        const size_t w = (size_t)k0->mk_parties * c->P.n + 1;
        return multi_rows(c, B, [&](tfhe_ctx *k, int64_t s0, int64_t cnt) { return tfhe_mk_gate_nand_batch(k, in0 + (size_t)s0 * w, in1 + (size_t)s0 * w, out + (size_t)s0 * w, cnt); });
    }
    if (!c->have_mk_bk || !c->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "mk_gate_nand_batch: multi-key keys not loaded");
    // (the keyswitch addresses rows by ITS key's parties, the rotation writes them by the bootstrapping key's: they must agree)
    if (c->ks.parties != c->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "mk_gate_nand_batch: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties",
                          c->mk_parties, c->ks.parties);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }
    const int NP = c->mk_parties, n = c->P.n, nw = NP * n + 1, Nn = c->P.N /* (1024 in every tuned branch below) */, ew = NP * Nn + 1;
    const size_t bytes = (size_t)B * nw * 4;
    for (int i = 0; i < 2; i++) {
        HIP_TRY(c, c->io[i].reserve(bytes));
        HIP_TRY(c, hipMemcpyAsync(c->io[i].p, i == 0 ? in0 : in1, bytes, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(c, c->io[3].reserve(bytes));
    HIP_TRY(c, c->bara.reserve(bytes));
    HIP_TRY(c, c->ext.reserve((size_t)B * ew * 4));
    // maps: rot_gate[g] = g, kind = NAND, e0[g] = g
    int32_t rc = ensure_host_map(c, (size_t)B * 5);
    if (rc) return rc;
    int32_t *h_gate = (int32_t *)c->h_map;
    uint8_t *h_kind = (uint8_t *)(h_gate + B);
    for (int64_t g = 0; g < B; g++) { h_gate[g] = (int32_t)g; h_kind[g] = TFHE_GATE_NAND; }
    HIP_TRY(c, c->map.reserve((size_t)B * 5));
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, (size_t)B * 5, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipEventRecord(c->map_ev, s));
    c->map_cur->pending = true;
    const int32_t *d_gate = (const int32_t *)c->map.p;
    const uint8_t *d_kind = (const uint8_t *)(d_gate + B);
    next_timing_slot(c);
    HIP_TRY(c, hipEventRecord(c->ev[0], s));
    // mk_gate_nand prologue (mk_gates.jl:8-10) = the NAND affine form over P*n+1 words, then mod-switch
    rc = launch_prologue(c, (size_t)B, (const int32_t *)c->io[0].p, (const int32_t *)c->io[1].p, nullptr, d_gate, d_gate, d_kind, NP * n, s);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[1], s));
    rc = launch_mk_blind_rotate(c, (size_t)B, s);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[2], s));
    rc = launch_keyswitch(c, (size_t)B, d_gate, nullptr, nullptr, (const int32_t *)c->ext.p, (int32_t *)c->io[3].p, s);
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(c->ev[3], s));
    HIP_TRY(c, hipMemcpyAsync(out, c->io[3].p, bytes, hipMemcpyDeviceToHost, s));
    rc = leave_stream(c, s);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(s));
    commit_timing_slot(c);
    c->last_rotations = B;
    return TFHE_OK;
}
ABI_CATCH(c, "tfhe_mk_gate_nand_batch")

// The multi-key counterpart of run_gates: gates.jl's formulas over multi-key samples of P n + 1 words.  Common body of
// tfhe_mk_gates_batch (operands = rows g of three device arrays, ia = ib = ic = io = NULL) and tfhe_mk_gates_level (operands =
// rows ia[g], ib[g], ic[g] of the multi-key wire table, result row io[g]; operands an opcode does not read are replaced by
// row 0).  Every bootstrapped gate is one multi-key rotation (MUX: two, summed before the keyswitch), then one multi-key
// keyswitch; NOT / COPY / CONST0 / CONST1 are trivial.  The caller has checked that the multi-key keys are loaded for the same
// parties.
int32_t run_mk_gates(tfhe_ctx *c, const char *who, const uint8_t *opcodes, int64_t B, const int32_t *d_in0, const int32_t *d_in1,
                     const int32_t *d_in2, int32_t *d_out, const int32_t *ia, const int32_t *ib, const int32_t *ic, const int32_t *io,
                     hipStream_t s)
{
    // classify gates: rotations (R), keyswitches (G), trivial (T)
    size_t R = 0, G = 0, Tn = 0;
    bool need1 = false, need2 = false, need0 = false;
    for (int64_t g = 0; g < B; g++) {
        const int op = opcodes[g];
        if (op >= TFHE_GATE__COUNT) return c->set_err(TFHE_ERR_INVALID_ARG, "%s: bad opcode %d at gate %lld", who, op, (long long)g);
        if (op == TFHE_GATE_MUX) { R += 2; G += 1; need0 = need1 = need2 = true; }
        else if (op == TFHE_GATE_NOT || op == TFHE_GATE_COPY) { Tn++; need0 = true; }
        else if (op == TFHE_GATE_CONST0 || op == TFHE_GATE_CONST1) { Tn++; }
        else { R += 1; G += 1; need0 = need1 = true; }
    }
    if ((need0 && !d_in0) || (need1 && !d_in1) || (need2 && !d_in2))
        return c->set_err(TFHE_ERR_INVALID_ARG, "%s: an operand array required by the opcodes is NULL", who);
    {
        const int32_t rc0 = enter_stream(c, s);
        if (rc0) return rc0;
    }
    // index maps, one pinned staging block (as run_gates):
    //   rot_a[R] | rot_b[R] | ks_e0[G] | ks_e1[G] | ks_dst[G] | triv_src[T] | triv_dst[T] | rot_kind[R] | triv_op[T]
    const size_t map_bytes = (2 * R + 3 * G + 2 * Tn) * 4 + R + Tn;
    int32_t rc = ensure_host_map(c, map_bytes);
    if (rc) return rc;
    int32_t *h_ra = (int32_t *)c->h_map, *h_rb = h_ra + R;
    int32_t *h_e0 = h_rb + R, *h_e1 = h_e0 + G, *h_dst = h_e1 + G, *h_ts = h_dst + G, *h_td = h_ts + Tn;
    uint8_t *h_kind = (uint8_t *)(h_td + Tn), *h_top = h_kind + R;
    {
        size_t r = 0, k = 0, t = 0;
        for (int64_t g = 0; g < B; g++) {
            const int op = opcodes[g];
            const int32_t ra = ia ? (op_has_a(op) ? ia[g] : 0) : (int32_t)g;
            const int32_t rb = ib ? (op_has_b(op) ? ib[g] : 0) : (int32_t)g;
            const int32_t rcw = ic ? (op == TFHE_GATE_MUX ? ic[g] : 0) : (int32_t)g;
            const int32_t ro = io ? io[g] : (int32_t)g;
            if (op == TFHE_GATE_MUX) {
                h_ra[r] = ra; h_rb[r] = rb; h_kind[r] = 100;                // AND(x, y)      gates.jl:166
                h_ra[r + 1] = ra; h_rb[r + 1] = rcw; h_kind[r + 1] = 101;   // AND(NOT x, z)  gates.jl:170
                h_e0[k] = (int32_t)r; h_e1[k] = (int32_t)(r + 1); h_dst[k] = ro;
                r += 2; k++;
            } else if (op == TFHE_GATE_NOT || op == TFHE_GATE_COPY || op == TFHE_GATE_CONST0 || op == TFHE_GATE_CONST1) {
                h_ts[t] = ra; h_td[t] = ro; h_top[t] = (uint8_t)op; t++;
            } else {
                h_ra[r] = ra; h_rb[r] = rb; h_kind[r] = (uint8_t)op;
                h_e0[k] = (int32_t)r; h_e1[k] = -1; h_dst[k] = ro;
                r++; k++;
            }
        }
    }
    HIP_TRY(c, c->map.reserve(map_bytes));
    HIP_TRY(c, hipMemcpyAsync(c->map.p, c->h_map, map_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipEventRecord(c->map_ev, s));
    c->map_cur->pending = true;
    const int32_t *d_ra = (const int32_t *)c->map.p, *d_rb = d_ra + R;
    const int32_t *d_e0 = d_rb + R, *d_e1 = d_e0 + G, *d_dst = d_e1 + G, *d_ts = d_dst + G, *d_td = d_ts + Tn;
    const uint8_t *d_kind = (const uint8_t *)(d_td + Tn), *d_top = d_kind + R;

    const int NP = c->mk_parties, n = c->P.n, nw = NP * n + 1, ew = NP * c->P.N + 1;
    const bool no_ev = !c->timing_events;
    next_timing_slot(c);
    if (!no_ev) HIP_TRY(c, hipEventRecord(c->ev[0], s));
    if (R > 0) {
        HIP_TRY(c, c->bara.reserve(R * (size_t)nw * 4));
        HIP_TRY(c, c->ext.reserve(R * (size_t)ew * 4));
        // the gate's affine form over all P n + 1 words (mk_gates.jl:8-10 for NAND), then mod-switch
        rc = launch_prologue(c, R, d_in0, d_in1, d_in2, d_ra, d_rb, d_kind, NP * n, s);
        if (rc) return rc;
    }
    if (!no_ev) HIP_TRY(c, hipEventRecord(c->ev[1], s));
    if (R > 0) {
        rc = launch_mk_blind_rotate(c, R, s);
        if (rc) return rc;
    } else {
        c->diag_rows = 0;
    }
    if (!no_ev) HIP_TRY(c, hipEventRecord(c->ev[2], s));
    if (G > 0) {
        rc = launch_keyswitch(c, G, d_e0, d_e1, d_dst, (const int32_t *)c->ext.p, d_out, s);
        if (rc) return rc;
    }
    if (!no_ev) HIP_TRY(c, hipEventRecord(c->ev[3], s));
    if (Tn > 0) {
        rc = launch_trivial(c, Tn, d_in0, d_ts, d_td, d_top, d_out, NP * n, s);
        if (rc) return rc;
    }
    if (!no_ev) commit_timing_slot(c);
    c->last_rotations = (int64_t)R;
    return leave_stream(c, s);
}

// multi-key keys loaded, for the same parties (the keyswitch addresses rows by its key's parties, the rotation by the bootstrapping key's)
static int32_t mk_keys_ready(tfhe_ctx *c, const tfhe_ctx *k, const char *who)
{
    if (!k->have_mk_bk || !k->have_mk_ks()) return c->set_err(TFHE_ERR_NO_KEY, "%s: multi-key keys not loaded", who);
    if (k->ks.parties != k->mk_parties)
        return c->set_err(TFHE_ERR_STATE, "%s: the bootstrapping key was loaded for %d parties, the keyswitch key for %d: load both for the same parties",
                          who, k->mk_parties, k->ks.parties);
    return TFHE_OK;
}

int32_t tfhe_mk_gates_batch(tfhe_ctx *c, const uint8_t *opcodes, const int32_t *in0, const int32_t *in1, const int32_t *in2,
                            int32_t *out, int64_t B) try
{
    ENTER_CTX(c);
    if (B < 0 || (B > 0 && (!opcodes || !out))) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_gates_batch: NULL argument or negative B");
    if (B == 0) return TFHE_OK;
    if (B > (int64_t)1 << 30) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_gates_batch: B too large");
    if (c->P.parties == 1) return c->set_err(TFHE_ERR_STATE, "mk_gates_batch: context is single-key");
    {
        const int32_t rck = mk_keys_ready(c, c->multi() ? c->kids[0] : c, "mk_gates_batch");
        if (rck) return rck;
    }
    // which operand arrays do the opcodes read at all?  (an array nobody reads is not uploaded)
    bool need[3] = {false, false, false};
    for (int64_t g = 0; g < B; g++) {
        const int op = opcodes[g];
        if (op >= TFHE_GATE__COUNT) return c->set_err(TFHE_ERR_INVALID_ARG, "mk_gates_batch: bad opcode %d at gate %lld", op, (long long)g);
        need[0] = need[0] || op_has_a(op); need[1] = need[1] || op_has_b(op); need[2] = need[2] || op == TFHE_GATE_MUX;
    }
    const int32_t *hin[3] = {in0, in1, in2};
    if ((need[0] && !in0) || (need[1] && !in1) || (need[2] && !in2))
        return c->set_err(TFHE_ERR_INVALID_ARG, "mk_gates_batch: an operand array required by the opcodes is NULL");
    if (c->multi()) {
        // contiguous shards balanced by blind rotations (tfhe_shard_bounds: MUX = 2), as tfhe_gates_batch
        const int nk = (int)c->kids.size();
        const size_t w = (size_t)c->kids[0]->mk_parties * c->P.n + 1;
        alloc_checkpoint();
        std::vector<int64_t> bounds((size_t)nk + 1);
        shard_bounds_by_rotations(opcodes, B, nk, bounds.data());
        std::vector<int> which;
        for (int r = 0; r < nk; r++)
            if (bounds[(size_t)r + 1] > bounds[(size_t)r]) which.push_back(r);
        return fan_out(c, which, [&](int r) {
            const int64_t s0 = bounds[(size_t)r], cnt = bounds[(size_t)r + 1] - s0;
            auto off = [&](const int32_t *p) { return p ? p + (size_t)s0 * w : nullptr; };
            return tfhe_mk_gates_batch(c->kids[(size_t)r], opcodes + s0, off(in0), off(in1), off(in2), out + (size_t)s0 * w, cnt);
        });
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    { const int32_t rc0 = enter_stream(c, s); if (rc0) return rc0; }
    const size_t bytes = (size_t)B * ((size_t)c->mk_parties * c->P.n + 1) * 4;
    int32_t *din[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < 3; i++) {
        if (!hin[i] || !need[i]) continue;
        HIP_TRY(c, c->io[i].reserve(bytes));
        HIP_TRY(c, hipMemcpyAsync(c->io[i].p, hin[i], bytes, hipMemcpyHostToDevice, s));
        din[i] = (int32_t *)c->io[i].p;
    }
    HIP_TRY(c, c->io[3].reserve(bytes));
    int32_t rc = run_mk_gates(c, "mk_gates_batch", opcodes, B, din[0], din[1], din[2], (int32_t *)c->io[3].p, nullptr, nullptr, nullptr, nullptr, s);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, c->io[3].p, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    return TFHE_OK;
}
ABI_CATCH(c, "tfhe_mk_gates_batch")
