// kernels_blind_rotate_tlwe.hpp — the blind rotation (bootstrap.jl:26-41) on an accumulator the caller supplies, returning the
// accumulator the caller asks for: tfhe_blind_rotate_batch.  Row g starts from a full TLWE sample,
//     A_0 = X^(-barb_g) acc[acc_index[g]]             on every one of the k + 1 polynomials, the mask included
// (every other rotation kernel starts its mask from zero and its body from a public test polynomial), and runs
//     A_(i+1) = A_i + C_sel[i] (.) (X^(e_g,i) A_i - A_i)          i = 0 ... steps - 1          (bootstrap.jl:19-23, :32-39)
// with C_s selector s of the loaded set (tfhe_tgsw_load: an entry of the bootstrapping key IS a TGSW selector).  The exponents come
// from the row's steps + 1 words, mask words then body: an LWE sample switched to Z_2N here (bootstrap.jl:74-75), or exponents as they are.
//
// It is tfhe_rot_net_batch's chain for one row — a rotated copy by 2N - barb, then `steps` levels of width 1 with records
// (0, 0, i, 0, e_i) — fused into one launch with per-row exponents: the same function, leveled::cmux (kernels_leveled_core.hpp), on a
// rotated and a plain read of the same sample, so the words are that chain's, and with a trivial accumulator (0, tv) the any-N
// rotation's.  The accumulator ping-pongs between two per-row samples in global memory (L2-resident; ordered by the workgroup
// barrier, as anyn::blind_rotate_kernel's in-place one); a zero exponent adds exactly zero and is skipped, as bootstrap.jl:34 does.
// One workgroup per row; workgroup barriers only; every loop is bounded by an argument.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

// LevelArgs as the level kernels read it, with: in = the accumulators [T][K1][N], row_index = acc_index [B] (never NULL), row_words =
// K1 N, nodes_out = 1, sel = [steps] shared by all rows, tgsw = the selector set [S][L][K1][K1][M], out = [B][K1][N] or NULL, ext =
// [B][n_out][(K1-1) N + 1] or NULL
struct RotateArgs : LevelArgs {
    const int32_t *rows;      // [B][steps + 1] mask words then body
    int32_t *ws;              // [B][2][K1][N] the two samples row g's accumulator alternates between
    int32_t K1, steps;
    int32_t in_form;          // 0: rows are LWE samples (modulus switch here), 1: exponents in [0, 2N)
    int32_t log2_n_out;       // ext: sample j < n_out is extracted at coefficient j N / n_out
};

#ifdef TFHE_EMIT_BLIND_ROTATE_TLWE_KERNELS      // (defined by engine_blind_rotate.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void tlwe_rotate_kernel(RotateArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, P.K1);
    const int N = f.N, two_n_mask = 2 * N - 1, masks = P.K1 - 1;
    const size_t sample = (size_t)P.K1 * N;
    const int32_t *words = P.rows + f.g * ((size_t)P.steps + 1);
    const int log2_2N = P.log2N + 1;
    // decode_message(v, 2N) (numeric-functions.jl:31-34), then mod 2N
    auto exponent = [&](int32_t w) {
        const int32_t e = P.in_form == 0 ? (int32_t)((uint32_t)w + (1u << (32 - log2_2N - 1))) >> (32 - log2_2N) : w;
        return e & two_n_mask;
    };
    int32_t *cur = P.ws + f.g * 2 * sample, *nxt = cur + sample;

    // A_0 = X^(-barb) acc: a rotated copy of every polynomial     bootstrap.jl:54-56
    copy_node(f, Src<SRC_ROTATED>{f.row, (2 * N - exponent(words[P.steps])) & two_n_mask}, masks, cur, nullptr);
    __syncthreads();

#pragma unroll 1
    for (int i = 0; i < P.steps; i++) {                                        // bootstrap.jl:32-39
        const int e = exponent(words[i]);
        if (e == 0) continue;                                                  // :34 (uniform over the workgroup)
        cmux(f, P.g, P.tgsw, P.sel[i], Src<SRC_ROTATED>{cur, e}, Src<SRC_PLAIN>{cur, 0}, P.K1, nxt, nullptr);      // (ends on a barrier)
        int32_t *t = cur; cur = nxt; nxt = t;
    }

    if (P.out) copy_node(f, Src<SRC_PLAIN>{cur, 0}, masks, P.out + f.g * sample, nullptr);
    if (P.ext) {
        // tlwe_extract_sample (tlwe.jl:55-59) at coefficient c instead of 0: mask word u is coefficient c of X^u a, the body is b[c]
        const int n_out = 1 << P.log2_n_out;
        const size_t ext_w = (size_t)masks * N + 1;
#pragma unroll 1
        for (int j = 0; j < n_out; j++) {
            const int c = j << (P.log2N - P.log2_n_out);
            int32_t *ext = P.ext + (f.g * n_out + j) * ext_w;
            for (int e = f.tid; e < masks * N; e += f.nt) ext[e] = rot_read(cur + (size_t)(e >> P.log2N) * N, c, e & (N - 1), N);
            if (f.tid == 0) ext[(size_t)masks * N] = cur[(size_t)masks * N + c];
        }
    }
}
#endif  // TFHE_EMIT_BLIND_ROTATE_TLWE_KERNELS

}  // namespace leveled
