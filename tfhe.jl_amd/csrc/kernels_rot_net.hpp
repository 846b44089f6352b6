// kernels_rot_net.hpp — the leveled mode's CMUX networks with a public monomial on every edge: the network of kernels_cmux_net.hpp whose
// node record is (src0, src1, var, rot0, rot1).  Output node i of a level of row g is
//     X^rot0 in[src0] + selector[sel[g][var]] (.) (X^rot1 in[src1] - X^rot0 in[src0])
// with X^r p the reference's mul_by_monomial(p, r) on every polynomial of the sample (bootstrap.jl:21, :54): coefficient j moves to
// j + r mod 2N and changes sign past N.  CMUX(C_b; acc, X^(-2^b) acc) for b = 0 ... r-1 is the blind rotation by TGSW bits, which reads
// a table packed N entries to a sample; X^w on the transitions of an automaton gives weighted automata.  A node with src0 == src1 and
// rot0 == rot1 is a rotated copy: no product, no noise, the exact words of X^rot0 in[src0].
//
// The arithmetic is cmux_net_level_kernel's because it is the same function, leveled::cmux (kernels_leveled_core.hpp), on sources of
// the rotated kind: with every rotation 0 the network equals tfhe_cmux_net_batch in every word.  The only other arithmetic is the
// rotated read (rot_read there) in the difference, the final + d0 and the copy path.
#pragma once
#include "kernels_cmux_net.hpp"        // NetArgs (its kernel is emitted by engine_cmux_net.hip only)

namespace leveled {

struct RotNetArgs : NetArgs {};       // nodes: [nodes_out][5] records (src0, src1, var, rot0, rot1)

#ifdef TFHE_EMIT_ROT_NET_KERNELS      // (defined by engine_rot_net.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void rot_net_level_kernel(RotNetArgs P)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Frame f = frame(P, smem, P.K1);
    const size_t sample = (size_t)P.K1 * f.N;
    const int32_t *rec = P.nodes + 5 * f.i;
    const int32_t src0 = rec[0], src1 = rec[1], var = rec[2], rot0 = rec[3], rot1 = rec[4];
    const Src<SRC_ROTATED> d0{f.row + (size_t)src0 * sample, rot0}, d1{f.row + (size_t)src1 * sample, rot1};
    int32_t *out = node_out(P.out, sample), *ext = node_out(P.ext, (size_t)(P.K1 - 1) * f.N + 1);
    if (src0 == src1 && rot0 == rot1) return copy_node(f, d0, P.K1 - 1, out, ext);      // a rotated copy: the exact words of X^rot0 in[src0]
    cmux(f, P.g, P.tgsw, P.sel[f.g * (size_t)P.V + var], d1, d0, P.K1, out, ext);
}
#endif  // TFHE_EMIT_ROT_NET_KERNELS

}  // namespace leveled
