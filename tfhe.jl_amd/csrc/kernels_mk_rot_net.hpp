// kernels_mk_rot_net.hpp — CMUX networks with a public monomial on every edge under a multi-key cloud key: the network of
// kernels_mk_cmux_net.hpp whose node record is (src0, src1, var, rot0, rot1), as kernels_rot_net.hpp's is of kernels_cmux_net.hpp's.
// Output node i of a level of row g is
//     X^rot0 in[src0] + selector[sel[g][var]] (.) (X^rot1 in[src1] - X^rot0 in[src0])
// with the selector an expanded RGSW sample multiplied for party_of[that selector] (mk_tgsw_extern_mul, mk_internals.jl:348-391) and
// X^r the reference's mul_by_monomial(p, r) on all P + 1 polynomials of the MK TLWE sample.  CMUX(C_b; acc, X^(-2^b) acc) for
// b = 0 ... r-1 reads a table packed N entries to a sample at jointly encrypted address bits; X^w on the transitions of an automaton
// gives weighted automata over bits of several parties.  A node with src0 == src1 and rot0 == rot1 is a rotated copy: no product, no
// noise, the exact words of X^rot0 in[src0]; with src0 == src1 and rot0 != rot1 it is a true product.
//
// The arithmetic is mk_cmux_net_level_kernel's because it is the same function, leveled::mk_cmux (kernels_leveled_core.hpp), on
// sources of the rotated kind: with every rotation 0 the network equals tfhe_mk_cmux_net_batch in every word.  The only other
// arithmetic is the rotated read (rot_read there) in the difference, the final + d0 and the copy path.
#pragma once
#include "kernels_mk_cmux_net.hpp"     // MkNetArgs (its kernel is emitted by engine_mk_cmux_net.hip only)

namespace leveled {

struct MkRotNetArgs : MkNetArgs {};   // nodes: [nodes_out][5] records (src0, src1, var, rot0, rot1)

#ifdef TFHE_EMIT_MK_ROT_NET_KERNELS   // (defined by engine_mk_rot_net.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void mk_rot_net_level_kernel(MkRotNetArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, 3);
    const int NP = P.parties;
    const size_t sample = (size_t)(NP + 1) * f.N;
    const int32_t *rec = P.nodes + 5 * f.i;
    const int32_t src0 = rec[0], src1 = rec[1], var = rec[2], rot0 = rec[3], rot1 = rec[4];
    const Src<SRC_ROTATED> d0{f.row + (size_t)src0 * sample, rot0}, d1{f.row + (size_t)src1 * sample, rot1};
    int32_t *out = node_out(P.out, sample), *ext = node_out(P.ext, (size_t)NP * f.N + 1);
    if (src0 == src1 && rot0 == rot1) return copy_node(f, d0, NP, out, ext);      // a rotated copy: the exact words of X^rot0 in[src0]
    const int si = P.sel[f.g * (size_t)P.V + var];
    mk_cmux(f, P.g, P.tgsw, si, P.party_of[si], d1, d0, NP, out, ext);
}
#endif  // TFHE_EMIT_MK_ROT_NET_KERNELS

}  // namespace leveled
