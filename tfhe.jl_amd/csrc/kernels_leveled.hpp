// kernels_leveled.hpp — the leveled mode: one CMUX d0 + C (.) (d1 - d0) per workgroup, with a caller's TGSW sample C and a
// caller's TLWE samples d0, d1 (the form of bootstrap.jl:19-23 with tgsw_extern_mul, tgsw.jl:125-129, on operands that are
// not the bootstrapping key and not a rotating accumulator).  A level of a CMUX tree halves a row's table: output node i of
// row g is CMUX(sel[g][level]; in[2 i], in[2 i + 1]); 2^depth - 1 external products fold a 2^depth-entry table down to the
// entry an encrypted address names, with no blind rotation.  A plain external product is the same kernel with d0 = 0.
//
// The body is leveled::cmux (kernels_leveled_core.hpp), built on the any-N blocks with selector spectra in fft_fwd's order scaled 1/M
// (anyn::bk_prepare_kernel makes them: tgsw_prepare, engine_keys.hip), so the kernel is correct for every parameter set a context
// accepts: any power-of-two N, any k, any (l, beta).  Rounding is the rotation's (round_to_torus32), and so is the exactness domain:
// (k + 1) l products are summed before the one rounding.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

struct Args : LevelArgs {     // sel: [B][depth] which selector row g uses at each level; ext: nodes_out = 1
    int32_t K1;
    int32_t depth, level;     // sel's row length and the column this level reads
    int32_t d0_zero;          // 1: the plain external product, d0 = 0 and d1 = input node i (instead of nodes 2 i, 2 i + 1)
};

#ifdef TFHE_EMIT_LEVELED_KERNELS       // (defined by engine_leveled.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void cmux_level_kernel(Args P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, P.K1);
    const size_t sample = (size_t)P.K1 * f.N;
    const Src<SRC_OR_ZERO> d0{P.d0_zero ? nullptr : f.row + 2 * f.i * sample, 0};
    const Src<SRC_PLAIN> d1{P.d0_zero ? f.row + f.i * sample : f.row + (2 * f.i + 1) * sample, 0};
    cmux(f, P.g, P.tgsw, P.sel[f.g * (size_t)P.depth + P.level], d1, d0, P.K1, node_out(P.out, sample), node_out(P.ext, (size_t)(P.K1 - 1) * f.N + 1));
}
#endif  // TFHE_EMIT_LEVELED_KERNELS

}  // namespace leveled
