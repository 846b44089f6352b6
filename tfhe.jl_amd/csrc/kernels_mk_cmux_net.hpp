// kernels_mk_cmux_net.hpp — CMUX networks under a multi-key cloud key: the multi-key CMUX d0 + C (.) (d1 - d0) of kernels_mk_leveled.hpp
// (mk_tgsw_extern_mul, mk_internals.jl:348-391, with an expanded RGSW selector C of party `party`) wired by the public netlist of
// kernels_cmux_net.hpp instead of by halving.  Output node i of a level of row g is CMUX(selector[sel[g][var]]; in[src0], in[src1]) with
// (src0, src1, var) the node's record and `in` the row's table entries (level 0) or the outputs of the level below; the selector, and
// with it the party, is per node.  A node with src0 == src1 is a copy: no product, no noise, and word for word what the formula gives.
//
// The arithmetic is mk_cmux_level_kernel's because it is the same function, leveled::mk_cmux (kernels_leveled_core.hpp): a tree-shaped
// network equals tfhe_mk_cmux_tree_batch in every word.
#pragma once
#include "kernels_leveled_core.hpp"

namespace leveled {

struct MkNetArgs : LevelArgs {
    const int32_t *nodes;     // [nodes_out][3] this level's records (src0, src1, var), checked by the host
    const int32_t *party_of;  // [S] the party whose expansion selector s is, checked by the host
    int32_t parties;
    int32_t V;                // sel's row length
};

#ifdef TFHE_EMIT_MK_CMUX_NET_KERNELS      // (defined by engine_mk_cmux_net.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void mk_cmux_net_level_kernel(MkNetArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, 3);
    const int NP = P.parties;
    const size_t sample = (size_t)(NP + 1) * f.N;
    const int32_t *rec = P.nodes + 3 * f.i;
    const int32_t src0 = rec[0], src1 = rec[1], var = rec[2];
    const Src<SRC_PLAIN> d0{f.row + (size_t)src0 * sample, 0}, d1{f.row + (size_t)src1 * sample, 0};
    int32_t *out = node_out(P.out, sample), *ext = node_out(P.ext, (size_t)NP * f.N + 1);
    if (src0 == src1) return copy_node(f, d0, NP, out, ext);
    const int si = P.sel[f.g * (size_t)P.V + var];
    mk_cmux(f, P.g, P.tgsw, si, P.party_of[si], d1, d0, NP, out, ext);
}
#endif  // TFHE_EMIT_MK_CMUX_NET_KERNELS

}  // namespace leveled
