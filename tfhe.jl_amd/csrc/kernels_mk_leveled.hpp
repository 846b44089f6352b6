// kernels_mk_leveled.hpp — the leveled mode under a multi-key cloud key: one CMUX d0 + C (.) (d1 - d0) per workgroup, with a caller's
// expanded RGSW sample C (MKTGswExpSample, mk_internals.jl:243-271, of party `party`) and a caller's MKTLweSample d0, d1
// (mk_internals.jl:46-57: a_0 ... a_{P-1}, b) — the form of mk_mux_rotate (mk_internals.jl:464-471) without the monomial, with
// mk_tgsw_extern_mul (:348-391) on operands that are not the bootstrapping key and not a rotating accumulator.  A level of a CMUX
// tree halves a row's table exactly as kernels_leveled.hpp's does; a plain external product is the same kernel with d0 = 0.
//
// With digits da[p, s] of mask s of d1 - d0 and db[p] of its body (spectrum-domain sums, as every MK kernel here):
//   a'_s     = d0.a_s     + sum_p da[p, s] (*) y[p, party]                          for every s != party     (:377-378)
//   a'_party = d0.a_party + sum_{p, s} da[p, s] (*) y[p, s] + sum_p db[p] (*) c1[p]                           (:371-376)
//   b'       = d0.b       + sum_{p, s} da[p, s] (*) x[p, s] + sum_p db[p] (*) c0[p]                           (:382-385)
// Three spectrum accumulators are live whatever P is (anyn::mk_blind_rotate_kernel, kernels_anyn.hpp): a'_s of a non-party source is
// fed by its own digits only, so it is finished right after source s.  Built on the any-N blocks, so the kernel is correct for every
// multi-key parameter set a context accepts; the selector spectra are anyn::bk_prepare_kernel's (fft_fwd's order, scaled 1/M).  The
// inputs are read-only and the outputs go to another buffer: nothing is updated in place.  Workgroup barriers only; every loop is
// bounded by a parameter.
#pragma once
#include <hip/hip_runtime.h>

#include "br_core.hpp"
#include "kernels_anyn.hpp"

using namespace tfhe;

namespace leveled {

struct MkArgs {
    const int32_t *in;        // the level's input samples: row r's nodes at in + r * row_words, node m at + m * (P + 1) * N
    const int32_t *row_index; // [B] row g reads input row row_index[g] (level 0 of a tree: its table), or NULL: row g
    const int32_t *sel;       // [B][depth] which selector row g uses at each level, checked by the host
    const int32_t *party_of;  // [S] the party whose expansion selector s is, checked by the host
    const cplx *tgsw;         // [S][2 L P + 2 L][M] selector spectra x[L][P] | y[L][P] | c0[L] | c1[L], fft_fwd's order, scaled 1/M
    int32_t *out;             // [B][nodes_out][P + 1][N] the level's output samples, or NULL when only `ext` is wanted
    int32_t *ext;             // [B][P N + 1] the output extracted at coefficient 0 (mk_internals.jl:88-95; nodes_out = 1), or NULL
    cplx *spec_g;             // [workgroups][3][M] spectrum accumulators when they do not fit LDS, else NULL
    const cplx *wtab;         // [M]  e^{-2 pi i t / M}
    const cplx *twist;        // [M]  e^{-i pi j / N}
    Gadget g;
    int64_t row_words;        // words between two input rows
    int32_t parties, L, log2N;
    int32_t depth, level;     // sel's row length and the column this level reads
    int32_t nodes_out;        // output nodes per row
    int32_t d0_zero;          // 1: the plain external product, d0 = 0 and d1 = input node i (instead of nodes 2 i, 2 i + 1)
};

// LDS: buf [Mp] cplx | self, party, body spectrum accumulators [3][Mp] cplx (only if they fit) | tmp [N] int32
__host__ __device__ inline size_t mk_lds_bytes(int N, bool spec_in_lds) { return anyn::lds_bytes(N, spec_in_lds ? 3 : 0); }

#ifdef TFHE_EMIT_MK_LEVELED_KERNELS       // (defined by engine_mk_leveled.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void mk_cmux_level_kernel(MkArgs P)
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
    const int32_t *row = P.in + (size_t)(P.row_index ? P.row_index[g] : (int64_t)g) * (size_t)P.row_words;
    const int32_t *d0 = P.d0_zero ? nullptr : row + 2 * i * sample;
    const int32_t *d1 = P.d0_zero ? row + i * sample : row + (2 * i + 1) * sample;
    const int si = P.sel[g * (size_t)P.depth + P.level];
    const int party = P.party_of[si];
    const int per = 2 * L * NP + 2 * L;
    const cplx *key = P.tgsw + (size_t)si * per * M;
    const int beta = P.g.log2_base;
    const int32_t xormask = gadget_xor_mask(L, beta);
    int32_t *out = P.out ? P.out + (g * (size_t)P.nodes_out + i) * sample : nullptr;
    int32_t *ext = P.ext ? P.ext + g * ((size_t)NP * N + 1) : nullptr;

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
            const int32_t lo = (int32_t)((d0 ? (uint32_t)d0[e] : 0u) + (uint32_t)round_to_torus32(re));
            const int32_t hi = (int32_t)((d0 ? (uint32_t)d0[e + M] : 0u) + (uint32_t)round_to_torus32(im));
            if (out) { out[e] = lo; out[e + M] = hi; }
            if (ext) {
                // mk_tlwe_extract_sample (mk_internals.jl:88-95): per party a'[0] = p[0], a'[m] = -p[N - m]; b = body[0]
                if (d < NP) {
                    int32_t *a = ext + (size_t)d * N;
                    if (j == 0) a[0] = lo; else a[N - j] = (int32_t)(0u - (uint32_t)lo);
                    a[N - (j + M)] = (int32_t)(0u - (uint32_t)hi);
                } else if (j == 0) {
                    ext[(size_t)NP * N] = lo;
                }
            }
        }
        __syncthreads();
    };

    bool first_pb = true;
#pragma unroll 1
    for (int s = 0; s <= NP; s++) {
        const bool is_body = (s == NP), has_self = (!is_body && s != party);
        // tmp = ((d1 - d0)[s] + offset) ^ xormask: digit2 then reads the signed digits of tgsw.jl:99-117
        for (int j = tid; j < N; j += nt) {
            const uint32_t v = (uint32_t)d1[(size_t)s * N + j] - (d0 ? (uint32_t)d0[(size_t)s * N + j] : 0u);
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
#endif  // TFHE_EMIT_MK_LEVELED_KERNELS

}  // namespace leveled
