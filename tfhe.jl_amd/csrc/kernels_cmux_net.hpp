// kernels_cmux_net.hpp — the leveled mode's CMUX networks: the CMUX d0 + C (.) (d1 - d0) of kernels_leveled.hpp wired by a public
// netlist instead of by halving.  Output node i of a level of row g is CMUX(selector[sel[g][var]]; in[src0], in[src1]) with
// (src0, src1, var) the node's record, `in` the row's table entries (level 0) or the outputs of the level below: the backward
// evaluation of a deterministic automaton or an ordered decision diagram (the TFHE paper's leveled tool beside the CMUX tree), at
// one external product per node that has two different sources.  A node with src0 == src1 is a copy: no product, no noise, and
// word for word what the formula gives (the product of the zero difference is exactly zero).
//
// The arithmetic is cmux_level_kernel's because it is the same function, leveled::cmux (kernels_leveled_core.hpp): a tree-shaped
// network equals tfhe_cmux_tree_batch in every word.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

struct NetArgs : LevelArgs {
    const int32_t *nodes;     // [nodes_out][3] this level's records (src0, src1, var), checked by the host; with monomial edges
                              // (RotNetArgs) [nodes_out][5]: (src0, src1, var, rot0, rot1)
    int32_t K1;
    int32_t V;                // sel's row length
};

#ifdef TFHE_EMIT_CMUX_NET_KERNELS      // (defined by engine_cmux_net.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void cmux_net_level_kernel(NetArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, P.K1);
    const size_t sample = (size_t)P.K1 * f.N;
    const int32_t *rec = P.nodes + 3 * f.i;
    const int32_t src0 = rec[0], src1 = rec[1], var = rec[2];
    const Src<SRC_PLAIN> d0{f.row + (size_t)src0 * sample, 0}, d1{f.row + (size_t)src1 * sample, 0};
    int32_t *out = node_out(P.out, sample), *ext = node_out(P.ext, (size_t)(P.K1 - 1) * f.N + 1);
    if (src0 == src1) return copy_node(f, d0, P.K1 - 1, out, ext);
    cmux(f, P.g, P.tgsw, P.sel[f.g * (size_t)P.V + var], d1, d0, P.K1, out, ext);
}
#endif  // TFHE_EMIT_CMUX_NET_KERNELS

}  // namespace leveled
