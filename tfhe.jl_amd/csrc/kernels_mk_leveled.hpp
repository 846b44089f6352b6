// kernels_mk_leveled.hpp — the leveled mode under a multi-key cloud key: one CMUX d0 + C (.) (d1 - d0) per workgroup, with a caller's
// expanded RGSW sample C (MKTGswExpSample, mk_internals.jl:243-271, of party `party`) and a caller's MKTLweSample d0, d1
// (mk_internals.jl:46-57: a_0 ... a_{P-1}, b) — the form of mk_mux_rotate (mk_internals.jl:464-471) without the monomial, with
// mk_tgsw_extern_mul (:348-391) on operands that are not the bootstrapping key and not a rotating accumulator.  A level of a CMUX
// tree halves a row's table exactly as kernels_leveled.hpp's does; a plain external product is the same kernel with d0 = 0.
//
// The body is leveled::mk_cmux (kernels_leveled_core.hpp: the formulas, the three live spectrum accumulators), built on the any-N
// blocks, so the kernel is correct for every multi-key parameter set a context accepts; the selector spectra are
// anyn::bk_prepare_kernel's (fft_fwd's order, scaled 1/M).
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

struct MkArgs : LevelArgs {   // sel: [B][depth] which selector row g uses at each level; ext: nodes_out = 1
    const int32_t *party_of;  // [S] the party whose expansion selector s is, checked by the host
    int32_t parties;
    int32_t depth, level;     // sel's row length and the column this level reads
    int32_t d0_zero;          // 1: the plain external product, d0 = 0 and d1 = input node i (instead of nodes 2 i, 2 i + 1)
};

#ifdef TFHE_EMIT_MK_LEVELED_KERNELS       // (defined by engine_mk_leveled.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void mk_cmux_level_kernel(MkArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, 3);
    const int NP = P.parties;
    const size_t sample = (size_t)(NP + 1) * f.N;
    const Src<SRC_OR_ZERO> d0{P.d0_zero ? nullptr : f.row + 2 * f.i * sample, 0};
    const Src<SRC_PLAIN> d1{P.d0_zero ? f.row + f.i * sample : f.row + (2 * f.i + 1) * sample, 0};
    const int si = P.sel[f.g * (size_t)P.depth + P.level];
    // (the outputs addressed by (g, i) and the extraction by g, not by blockIdx.x as node_out does: the same addresses, since a tree
    // extracts only where nodes_out = 1, but with node_out this kernel measured 0.2 - 0.4 % slower at 1024 rows than in this form)
    int32_t *out = P.out ? P.out + (f.g * (size_t)P.nodes_out + f.i) * sample : nullptr;
    int32_t *ext = P.ext ? P.ext + f.g * ((size_t)NP * f.N + 1) : nullptr;
    mk_cmux(f, P.g, P.tgsw, si, P.party_of[si], d1, d0, NP, out, ext);
}
#endif  // TFHE_EMIT_MK_LEVELED_KERNELS

}  // namespace leveled
