// kernels_mk_cmux_net.hpp — CMUX networks under a multi-key cloud key: the multi-key CMUX d0 + C (.) (d1 - d0) of kernels_mk_leveled.hpp
// (mk_tgsw_extern_mul, mk_internals.jl:348-391, with an expanded RGSW selector C of party `party`) wired by the public netlist of
// kernels_cmux_net.hpp instead of by halving.  Output node i of a level of row g is CMUX(selector[sel[g][var]]; in[src0], in[src1]) with
// (src0, src1, var) the node's record and `in` the row's table entries (level 0) or the outputs of the level below; the selector, and
// with it the party, is per node.  A node with src0 == src1 is a copy: no product, no noise, and word for word what the formula gives.
//
// The arithmetic is mk_cmux_level_kernel's, statement for statement: the same any-N blocks, the same loop over the P + 1 sources with
// three live spectrum accumulators (self | party | body), the same accumulation order and rounding — a tree-shaped network equals
// tfhe_mk_cmux_tree_batch in every word.  Workgroup barriers only; every loop is bounded by a parameter; inputs are read-only and the
// outputs go to the other buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "br_core.hpp"
#include "kernels_anyn.hpp"
#include "kernels_mk_leveled.hpp"      // mk_lds_bytes (its kernel is emitted by engine_mk_leveled.hip only)

using namespace tfhe;

namespace leveled {

struct MkNetArgs {
    const int32_t *in;        // the level's input samples: row r's nodes at in + r * row_words, node m at + m * (P + 1) * N
    const int32_t *row_index; // [B] row g reads input row row_index[g] (level 0: its table), or NULL: row g
    const int32_t *nodes;     // [nodes_out][3] this level's records (src0, src1, var), checked by the host
    const int32_t *sel;       // [B][V] the selector behind each of row g's variables, checked by the host
    const int32_t *party_of;  // [S] the party whose expansion selector s is, checked by the host
    const cplx *tgsw;         // [S][2 L P + 2 L][M] selector spectra x[L][P] | y[L][P] | c0[L] | c1[L], fft_fwd's order, scaled 1/M
    int32_t *out;             // [B][nodes_out][P + 1][N] the level's output samples, or NULL when only `ext` is wanted
    int32_t *ext;             // [B][nodes_out][P N + 1] every output extracted at coefficient 0 (mk_internals.jl:88-95), or NULL
    cplx *spec_g;             // [workgroups][3][M] spectrum accumulators when they are not in LDS, else NULL
    const cplx *wtab;         // [M]  e^{-2 pi i t / M}
    const cplx *twist;        // [M]  e^{-i pi j / N}
    Gadget g;
    int64_t row_words;        // words between two input rows
    int32_t parties, L, log2N;
    int32_t V;                // sel's row length
    int32_t nodes_out;        // output nodes per row
};

#ifdef TFHE_EMIT_MK_CMUX_NET_KERNELS      // (defined by engine_mk_cmux_net.hip, the one translation unit that launches it)
// one pair of output words (coefficients j and j + M of polynomial d) to the sample and / or its extraction at coefficient 0:
// mk_tlwe_extract_sample (mk_internals.jl:88-95): per party a'[0] = p[0], a'[m] = -p[N - m]; b = body[0]
__device__ __forceinline__ void mk_net_store(int32_t *out, int32_t *ext, int d, int j, int32_t lo, int32_t hi, int NP, int N, int M)
{
    const size_t e = (size_t)d * N + j;
    if (out) { out[e] = lo; out[e + M] = hi; }
    if (ext) {
        if (d < NP) {
            int32_t *a = ext + (size_t)d * N;
            if (j == 0) a[0] = lo; else a[N - j] = (int32_t)(0u - (uint32_t)lo);
            a[N - (j + M)] = (int32_t)(0u - (uint32_t)hi);
        } else if (j == 0) {
            ext[(size_t)NP * N] = lo;
        }
    }
}

// blockIdx.x = g * nodes_out + i: the workgroups of a row sit together and share its selector spectra in L2
__global__ __launch_bounds__(512) void mk_cmux_net_level_kernel(MkNetArgs P)
{
    using namespace anyn;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = 1 << P.log2N, M = N >> 1, log2M = P.log2N - 1, Mp = padded_len(M);
    const int NP = P.parties, L = P.L;
    const bool spec_lds = P.spec_g == nullptr;
    cplx *buf = reinterpret_cast<cplx *>(smem);
    cplx *spec = spec_lds ? buf + Mp : P.spec_g + (size_t)blockIdx.x * 3 * M;      // [self | party | body]
    const int ss = spec_lds ? Mp : M;
    int32_t *tmp = reinterpret_cast<int32_t *>(buf + (size_t)(spec_lds ? 4 : 1) * Mp);
    const size_t g = blockIdx.x / (unsigned)P.nodes_out, i = blockIdx.x % (unsigned)P.nodes_out;
    const size_t sample = (size_t)(NP + 1) * N;
    const int32_t *rec = P.nodes + 3 * i;
    const int32_t src0 = rec[0], src1 = rec[1], var = rec[2];
    const int32_t *row = P.in + (size_t)(P.row_index ? P.row_index[g] : (int64_t)g) * (size_t)P.row_words;
    const int32_t *d0 = row + (size_t)src0 * sample;
    const int32_t *d1 = row + (size_t)src1 * sample;
    int32_t *out = P.out ? P.out + (size_t)blockIdx.x * sample : nullptr;
    int32_t *ext = P.ext ? P.ext + (size_t)blockIdx.x * ((size_t)NP * N + 1) : nullptr;

    if (src0 == src1) {       // a copy node (uniform over the workgroup: the record depends on blockIdx alone)
#pragma unroll 1
        for (int d = 0; d <= NP; d++)
            for (int j = tid; j < M; j += nt) mk_net_store(out, ext, d, j, d0[(size_t)d * N + j], d0[(size_t)d * N + j + M], NP, N, M);
        return;
    }

    const int si = P.sel[g * (size_t)P.V + var];
    const int party = P.party_of[si];
    const int per = 2 * L * NP + 2 * L;
    const cplx *key = P.tgsw + (size_t)si * per * M;
    const int beta = P.g.log2_base;
    const int32_t xormask = gadget_xor_mask(L, beta);

    auto finish = [&](int which, int d) {      // inverse transform of spectrum accumulator `which`, round, + d0's polynomial d, store as d
        cplx *y = spec + (size_t)which * ss;
        if (!spec_lds) {
            for (int f = tid; f < M; f += nt) buf[phys(f)] = y[f];
            __syncthreads();
            y = buf;
        }
        fft_inv(y, P.wtab, log2M, tid, nt);
        // conj(y_j) e^{-i pi j/N}: real -> coefficient j, imaginary -> j + M (polynomials.jl:127-129), rounded (polynomials.jl:115-116)
        for (int j = tid; j < M; j += nt) {
            const cplx v = y[phys(j)], w = P.twist[j];
            const double re = v.x * w.x + v.y * w.y, im = v.x * w.y - v.y * w.x;
            const size_t e = (size_t)d * N + j;
            const int32_t lo = (int32_t)((uint32_t)d0[e] + (uint32_t)round_to_torus32(re));
            const int32_t hi = (int32_t)((uint32_t)d0[e + M] + (uint32_t)round_to_torus32(im));
            mk_net_store(out, ext, d, j, lo, hi, NP, N, M);
        }
        __syncthreads();
    };

    bool first_pb = true;
#pragma unroll 1
    for (int s = 0; s <= NP; s++) {
        const bool is_body = (s == NP), has_self = (!is_body && s != party);
        // tmp = ((d1 - d0)[s] + offset) ^ xormask: digit2 then reads the signed digits of tgsw.jl:99-117
        for (int j = tid; j < N; j += nt) {
            const uint32_t v = (uint32_t)d1[(size_t)s * N + j] - (uint32_t)d0[(size_t)s * N + j];
            tmp[j] = (int32_t)((v + (uint32_t)P.g.offset) ^ (uint32_t)xormask);
        }
        __syncthreads();
#pragma unroll 1
        for (int p = 0; p < L; p++) {
            digits_to_buf(tmp, p + 1, beta, M, P.twist, buf, tid, nt);
            __syncthreads();
            fft_fwd(buf, P.wtab, log2M, tid, nt);
            const cplx *k_party = key + (size_t)(is_body ? 2 * L * NP + L + p : L * NP + p * NP + s) * M;   // c1[p] | y[p, s]
            const cplx *k_body = key + (size_t)(is_body ? 2 * L * NP + p : p * NP + s) * M;                 // c0[p] | x[p, s]
            mac(buf, k_party, spec + (size_t)1 * ss, spec_lds, first_pb, M, tid, nt);
            mac(buf, k_body, spec + (size_t)2 * ss, spec_lds, first_pb, M, tid, nt);
            first_pb = false;
            if (has_self) mac(buf, key + (size_t)(L * NP + p * NP + party) * M, spec, spec_lds, p == 0, M, tid, nt);   // y[p, party]
            __syncthreads();
        }
        if (has_self) finish(0, s);
    }
    finish(1, party);
    finish(2, NP);
}
#endif  // TFHE_EMIT_MK_CMUX_NET_KERNELS

}  // namespace leveled
