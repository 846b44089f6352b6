// kernels_mk_tlwe_levels.hpp — the multi-key blind rotation of kernels_mk_blind_rotate_tlwe.hpp between the two device-resident tables
// of a multi-key context: tfhe_mk_blind_rotate_level, the multi-key mirror of kernels_tlwe_levels.hpp.  Row g rotates the MK TLWE sample
// in slot acc_slot[g] of the MK TLWE table (tfhe_mk_tlwe_alloc) by the multi-key LWE sample
//     x_g = sum over t in [term_start[g], term_start[g+1]) of term_coef[t] * wires[term_wire[t]], plus cst[g] on the body
// (mod 2^32: linear_prologue_kernel's combination of multi-key wire rows, kernels_gates.hpp; a row without terms is the trivial
// sample), and leaves the final accumulator in slot out_slot[g] or its extractions for the multi-key keyswitch that writes them into
// the wire table.
//
// It is mk_tlwe_rotate_kernel's loop on the same leveled::copy_node / leveled::mk_cmux / rot_read, so its words are that kernel's words
// on the same samples.  Two things differ: the accumulator is read from its table slot, and the result goes to a table slot.  The rows
// arrive staged: linear_prologue_kernel<true> has formed x_g and switched it to Z_2N in one launch before this one, so there is no
// in_form here.  (The term sum is not formed in this kernel: the single-key level kernel measured that form and dropped it, DESIGN
// §4.18.)  The call's host checks keep every slot and wire it writes apart from every one it reads.
// One workgroup per row; workgroup barriers only; every loop is bounded by an argument.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

// LevelArgs as the level kernels read it, with: in = the MK TLWE table [slots][P+1][N], row_index = acc_slot [B] (never NULL), row_words
// = (P+1) N, nodes_out = 1, sel = [steps] shared by all rows, tgsw = the expanded selectors [S][2 L P + 2 L][M], out = the MK TLWE table
// or NULL, ext = [B][n_out][P N + 1] or NULL
struct MkRotateLevelArgs : LevelArgs {
    const int32_t *rows;        // [B][steps + 1] x_g switched to Z_2N (decode_message(., 2N), any representative mod 2N), step words then body
    const int32_t *party_of;    // [S] the party whose expansion selector s is
    const int32_t *out_slot;    // [B] the slot row g's final accumulator goes to (with out)
    int32_t *ws;                // [B][2][P+1][N] the two samples row g's accumulator alternates between
    int32_t parties, steps;
    int32_t log2_n_out;         // ext: sample j < n_out is extracted at coefficient j N / n_out
};

#ifdef TFHE_EMIT_MK_TLWE_LEVEL_KERNELS      // (defined by engine_mk_tlwe_levels.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void mk_tlwe_rotate_level_kernel(MkRotateLevelArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, 3);
    const int N = f.N, two_n_mask = 2 * N - 1, NP = P.parties;
    const size_t sample = (size_t)(NP + 1) * N;
    const int32_t *words = P.rows + f.g * ((size_t)P.steps + 1);
    auto exponent = [&](int i) { return words[i] & two_n_mask; };
    int32_t *cur = P.ws + f.g * 2 * sample, *nxt = cur + sample;

    // A_0 = X^(-barb) slot[acc_slot[g]]: a rotated copy of every polynomial     mk_internals.jl:504
    copy_node(f, Src<SRC_ROTATED>{f.row, (2 * N - exponent(P.steps)) & two_n_mask}, NP, cur, nullptr);
    __syncthreads();

#pragma unroll 1
    for (int i = 0; i < P.steps; i++) {                                        // mk_internals.jl:476-483
        const int e = exponent(i);
        if (e == 0) continue;                                                  // :478-480 (uniform over the workgroup)
        const int si = P.sel[i];
        mk_cmux(f, P.g, P.tgsw, si, P.party_of[si], Src<SRC_ROTATED>{cur, e}, Src<SRC_PLAIN>{cur, 0}, NP, nxt, nullptr);      // (ends on a barrier)
        int32_t *t = cur; cur = nxt; nxt = t;
    }

    if (P.out) copy_node(f, Src<SRC_PLAIN>{cur, 0}, NP, P.out + (size_t)P.out_slot[f.g] * sample, nullptr);
    if (P.ext) {
        // mk_tlwe_extract_sample (mk_internals.jl:88-95) at coefficient c instead of 0: mask word u of party s is coefficient c of
        // X^u a_s, the body is b[c]
        const int n_out = 1 << P.log2_n_out;
        const size_t ext_w = (size_t)NP * N + 1;
#pragma unroll 1
        for (int j = 0; j < n_out; j++) {
            const int c = j << (P.log2N - P.log2_n_out);
            int32_t *ext = P.ext + (f.g * n_out + j) * ext_w;
            for (int e = f.tid; e < NP * N; e += f.nt) ext[e] = rot_read(cur + (size_t)(e >> P.log2N) * N, c, e & (N - 1), N);
            if (f.tid == 0) ext[(size_t)NP * N] = cur[(size_t)NP * N + c];
        }
    }
}
#endif  // TFHE_EMIT_MK_TLWE_LEVEL_KERNELS

}  // namespace leveled
