// kernels_mk_blind_rotate_tlwe.hpp — the multi-key blind rotation (mk_blind_rotate, mk_internals.jl:473-485) on an MK TLWE
// accumulator the caller supplies, returning the accumulator the caller asks for: tfhe_mk_blind_rotate_batch, the multi-key mirror of
// kernels_blind_rotate_tlwe.hpp.  Row g starts from a full MK TLWE sample,
//     A_0 = X^(-barb_g) acc[acc_index[g]]             on every one of the P + 1 polynomials (mk_mul_by_monomial, :79-85)
// (every other multi-key rotation kernel starts its masks from zero and its body from a public test polynomial), and runs
//     A_(i+1) = A_i + C_sel[i] (.) (X^(e_g,i) A_i - A_i)          i = 0 ... steps - 1          (mk_mux_rotate, :464-470)
// with C_s expanded RGSW selector s of the loaded set, multiplied for party_of[s] (tfhe_mk_tgsw_load / tfhe_mk_tgsw_expand_load: a
// (party, bit) entry of the multi-key bootstrapping key IS such a selector).  The exponents come from the row's steps + 1 words, step
// words then body: an MK LWE sample switched to Z_2N here (:502-503), or exponents as they are.
//
// It is tfhe_mk_rot_net_batch's chain for one row — a rotated copy by 2N - barb, then `steps` levels of width 1 with records
// (0, 0, i, 0, e_i) — fused into one launch with per-row exponents: the same function, leveled::mk_cmux (kernels_leveled_core.hpp), on
// a rotated and a plain read of the same sample, so the words are that chain's, and with a trivial accumulator (0, ..., 0, tv) the
// any-N multi-key rotation's.  The accumulator ping-pongs between two per-row samples in global memory (L2-resident; ordered by the
// workgroup barrier); a zero exponent adds exactly zero and is skipped, as :478-480 does.
// One workgroup per row; workgroup barriers only; every loop is bounded by an argument.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

// LevelArgs as the level kernels read it, with: in = the accumulators [T][P+1][N], row_index = acc_index [B] (never NULL), row_words =
// (P+1) N, nodes_out = 1, sel = [steps] shared by all rows, tgsw = the expanded selectors [S][2 L P + 2 L][M], out = [B][P+1][N] or
// NULL, ext = [B][n_out][P N + 1] or NULL
struct MkRotateArgs : LevelArgs {
    const int32_t *rows;      // [B][steps + 1] step words then body
    const int32_t *party_of;  // [S] the party whose expansion selector s is
    int32_t *ws;              // [B][2][P+1][N] the two samples row g's accumulator alternates between
    int32_t parties, steps;
    int32_t in_form;          // 0: rows are MK LWE samples (modulus switch here), 1: exponents in [0, 2N)
    int32_t log2_n_out;       // ext: sample j < n_out is extracted at coefficient j N / n_out
};

#ifdef TFHE_EMIT_MK_BLIND_ROTATE_TLWE_KERNELS      // (defined by engine_mk_blind_rotate.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void mk_tlwe_rotate_kernel(MkRotateArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, 3);
    const int N = f.N, two_n_mask = 2 * N - 1, NP = P.parties;
    const size_t sample = (size_t)(NP + 1) * N;
    const int32_t *words = P.rows + f.g * ((size_t)P.steps + 1);
    const int log2_2N = P.log2N + 1;
    // decode_message(v, 2N) (numeric-functions.jl:31-34), then mod 2N
    auto exponent = [&](int32_t w) {
        const int32_t e = P.in_form == 0 ? (int32_t)((uint32_t)w + (1u << (32 - log2_2N - 1))) >> (32 - log2_2N) : w;
        return e & two_n_mask;
    };
    int32_t *cur = P.ws + f.g * 2 * sample, *nxt = cur + sample;

    // A_0 = X^(-barb) acc: a rotated copy of every polynomial     mk_internals.jl:504
    copy_node(f, Src<SRC_ROTATED>{f.row, (2 * N - exponent(words[P.steps])) & two_n_mask}, NP, cur, nullptr);
    __syncthreads();

#pragma unroll 1
    for (int i = 0; i < P.steps; i++) {                                        // mk_internals.jl:476-483
        const int e = exponent(words[i]);
        if (e == 0) continue;                                                  // :478-480 (uniform over the workgroup)
        const int si = P.sel[i];
        mk_cmux(f, P.g, P.tgsw, si, P.party_of[si], Src<SRC_ROTATED>{cur, e}, Src<SRC_PLAIN>{cur, 0}, NP, nxt, nullptr);      // (ends on a barrier)
        int32_t *t = cur; cur = nxt; nxt = t;
    }

    if (P.out) copy_node(f, Src<SRC_PLAIN>{cur, 0}, NP, P.out + f.g * sample, nullptr);
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
#endif  // TFHE_EMIT_MK_BLIND_ROTATE_TLWE_KERNELS

}  // namespace leveled
