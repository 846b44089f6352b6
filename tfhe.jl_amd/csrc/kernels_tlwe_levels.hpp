// kernels_tlwe_levels.hpp — the blind rotation of kernels_blind_rotate_tlwe.hpp between the two device-resident tables of a context:
// tfhe_blind_rotate_level.  Row g rotates the TLWE sample in slot acc_slot[g] of the TLWE table (tfhe_tlwe_alloc) by the LWE sample
//     x_g = sum over t in [term_start[g], term_start[g+1]) of term_coef[t] * wires[term_wire[t]], plus cst[g] on the body
// (mod 2^32: linear_prologue_kernel's combination, kernels_gates.hpp; a row without terms is the trivial sample), and leaves the final
// accumulator in slot out_slot[g] or its extractions for the keyswitch that writes them into the wire table.
//
// It is tlwe_rotate_kernel's loop on the same leveled::copy_node / leveled::cmux / rot_read, so its words are that kernel's words on
// the same samples.  Two things differ: the accumulator is read from its table slot, and the result goes to a table slot.  The rows
// arrive staged: linear_prologue_kernel<true> (kernels_gates.hpp, the prologue of tfhe_lut_level) has formed x_g and switched it to Z_2N
// in one launch before this one.  (Forming each exponent in this kernel where it is read — the term sum of word i, uniform over the
// workgroup — was built first and measured: two dependent loads in front of every step cost 0.34 ms over 500 steps at B = 1024, fifteen
// times the baseline's spread)  The call's host checks keep every slot and wire it writes apart from every one it reads.
// One workgroup per row; workgroup barriers only; every loop is bounded by an argument.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

// LevelArgs as the level kernels read it, with: in = the TLWE table [slots][K1][N], row_index = acc_slot [B] (never NULL), row_words =
// K1 N, nodes_out = 1, sel = [steps] shared by all rows, tgsw = the selector set [S][L][K1][K1][M], out = the TLWE table or NULL, ext =
// [B][n_out][(K1-1) N + 1] or NULL
struct RotateLevelArgs : LevelArgs {
    const int32_t *rows;        // [B][steps + 1] x_g switched to Z_2N (decode_message(., 2N), any representative mod 2N), mask words then body
    const int32_t *out_slot;    // [B] the slot row g's final accumulator goes to (with out)
    int32_t *ws;                // [B][2][K1][N] the two samples row g's accumulator alternates between
    int32_t K1, steps;
    int32_t log2_n_out;         // ext: sample j < n_out is extracted at coefficient j N / n_out
};

#ifdef TFHE_EMIT_TLWE_LEVEL_KERNELS      // (defined by engine_tlwe_levels.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void tlwe_rotate_level_kernel(RotateLevelArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, P.K1);
    const int N = f.N, two_n_mask = 2 * N - 1, masks = P.K1 - 1;
    const size_t sample = (size_t)P.K1 * N;
    const int32_t *words = P.rows + f.g * ((size_t)P.steps + 1);
    auto exponent = [&](int i) { return words[i] & two_n_mask; };
    int32_t *cur = P.ws + f.g * 2 * sample, *nxt = cur + sample;

    // A_0 = X^(-barb) slot[acc_slot[g]]: a rotated copy of every polynomial     bootstrap.jl:54-56
    copy_node(f, Src<SRC_ROTATED>{f.row, (2 * N - exponent(P.steps)) & two_n_mask}, masks, cur, nullptr);
    __syncthreads();

#pragma unroll 1
    for (int i = 0; i < P.steps; i++) {                                        // bootstrap.jl:32-39
        const int e = exponent(i);
        if (e == 0) continue;                                                  // :34 (uniform over the workgroup)
        cmux(f, P.g, P.tgsw, P.sel[i], Src<SRC_ROTATED>{cur, e}, Src<SRC_PLAIN>{cur, 0}, P.K1, nxt, nullptr);      // (ends on a barrier)
        int32_t *t = cur; cur = nxt; nxt = t;
    }

    if (P.out) copy_node(f, Src<SRC_PLAIN>{cur, 0}, masks, P.out + (size_t)P.out_slot[f.g] * sample, nullptr);
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
#endif  // TFHE_EMIT_TLWE_LEVEL_KERNELS

}  // namespace leveled
