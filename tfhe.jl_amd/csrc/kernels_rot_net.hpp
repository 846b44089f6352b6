// kernels_rot_net.hpp — the leveled mode's CMUX networks with a public monomial on every edge: the network of kernels_cmux_net.hpp whose
// node record is (src0, src1, var, rot0, rot1).  Output node i of a level of row g is
//     X^rot0 in[src0] + selector[sel[g][var]] (.) (X^rot1 in[src1] - X^rot0 in[src0])
// with X^r p the reference's mul_by_monomial(p, r) on every polynomial of the sample (bootstrap.jl:21, :54): coefficient j moves to
// j + r mod 2N and changes sign past N.  CMUX(C_b; acc, X^(-2^b) acc) for b = 0 ... r-1 is the blind rotation by TGSW bits, which reads
// a table packed N entries to a sample; X^w on the transitions of an automaton gives weighted automata.  A node with src0 == src1 and
// rot0 == rot1 is a rotated copy: no product, no noise, the exact words of X^rot0 in[src0].
//
// The arithmetic is cmux_net_level_kernel's, statement for statement: the same any-N blocks, the same accumulation order (c outer, p
// inner, the first product initialises), the same rounding — with every rotation 0 the network equals tfhe_cmux_net_batch in every word.
// The only new arithmetic is the rotated read, rot_read below, in the difference, the final + d0 and the copy path.  Workgroup barriers
// only; every loop is bounded by a parameter; inputs are read-only and the outputs go to the other buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "br_core.hpp"
#include "kernels_anyn.hpp"

using namespace tfhe;

namespace leveled {

struct RotNetArgs {
    const int32_t *in;        // the level's input samples: row r's nodes at in + r * row_words, node m at + m * K1 * N
    const int32_t *row_index; // [B] row g reads input row row_index[g] (level 0: its table), or NULL: row g
    const int32_t *nodes;     // [nodes_out][5] this level's records (src0, src1, var, rot0, rot1), checked by the host
    const int32_t *sel;       // [B][V] the selector behind each of row g's variables, checked by the host
    const cplx *tgsw;         // [S][L][K1][K1][M] selector spectra, fft_fwd's order, scaled 1/M
    int32_t *out;             // [B][nodes_out][K1][N] the level's output samples, or NULL when only `ext` is wanted
    int32_t *ext;             // [B][nodes_out][(K1-1) N + 1] every output extracted at coefficient 0 (tlwe.jl:55-59), or NULL
    cplx *spec_g;             // [workgroups][K1][M] spectrum accumulators when they are not in LDS, else NULL
    const cplx *wtab;         // [M]  e^{-2 pi i t / M}
    const cplx *twist;        // [M]  e^{-i pi j / N}
    Gadget g;
    int64_t row_words;        // words between two input rows
    int32_t K1, L, log2N;
    int32_t V;                // sel's row length
    int32_t nodes_out;        // output nodes per row
};

#ifdef TFHE_EMIT_ROT_NET_KERNELS      // (defined by engine_rot_net.hip, the one translation unit that launches it)
// coefficient j of X^r p for 0 <= r < 2N: p[s] for s = (j - r) mod 2N < N, else -p[s - N], negated in uint32 (-2^31 stays -2^31)
__device__ __forceinline__ int32_t rot_read(const int32_t *p, int j, int r, int N)
{
    const int s = (j - r) & (2 * N - 1);
    const int32_t v = p[s & (N - 1)];
    return s < N ? v : (int32_t)(0u - (uint32_t)v);
}

// one pair of output words (coefficients j and j + M of polynomial co) to the sample and / or its extraction at coefficient 0:
// tlwe_extract_sample (tlwe.jl:55-59): a'[0] = p[0], a'[m] = -p[N - m], mask polynomials in order; b = body[0]
__device__ __forceinline__ void rot_net_store(int32_t *out, int32_t *ext, int co, int j, int32_t lo, int32_t hi, int K1, int N, int M)
{
    const size_t e = (size_t)co * N + j;
    if (out) { out[e] = lo; out[e + M] = hi; }
    if (ext) {
        if (co + 1 < K1) {
            int32_t *a = ext + (size_t)co * N;
            if (j == 0) a[0] = lo; else a[N - j] = (int32_t)(0u - (uint32_t)lo);
            a[N - (j + M)] = (int32_t)(0u - (uint32_t)hi);
        } else if (j == 0) {
            ext[(size_t)(K1 - 1) * N] = lo;
        }
    }
}

// blockIdx.x = g * nodes_out + i: the workgroups of a row sit together and share its selector spectra in L2
__global__ __launch_bounds__(512) void rot_net_level_kernel(RotNetArgs P)
{
    using namespace anyn;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = 1 << P.log2N, M = N >> 1, log2M = P.log2N - 1, Mp = padded_len(M);
    const int K1 = P.K1, L = P.L;
    const bool spec_lds = P.spec_g == nullptr;
    cplx *buf = reinterpret_cast<cplx *>(smem);
    cplx *spec = spec_lds ? buf + Mp : P.spec_g + (size_t)blockIdx.x * K1 * M;
    const int spec_stride = spec_lds ? Mp : M;
    int32_t *tmp = reinterpret_cast<int32_t *>(buf + (size_t)(spec_lds ? 1 + K1 : 1) * Mp);
    const size_t g = blockIdx.x / (unsigned)P.nodes_out, i = blockIdx.x % (unsigned)P.nodes_out;
    const size_t sample = (size_t)K1 * N;
    const int32_t *rec = P.nodes + 5 * i;
    const int32_t src0 = rec[0], src1 = rec[1], var = rec[2], rot0 = rec[3], rot1 = rec[4];
    const int32_t *row = P.in + (size_t)(P.row_index ? P.row_index[g] : (int64_t)g) * (size_t)P.row_words;
    const int32_t *d0 = row + (size_t)src0 * sample;
    const int32_t *d1 = row + (size_t)src1 * sample;
    int32_t *out = P.out ? P.out + (size_t)blockIdx.x * sample : nullptr;
    int32_t *ext = P.ext ? P.ext + (size_t)blockIdx.x * ((size_t)(K1 - 1) * N + 1) : nullptr;

    if (src0 == src1 && rot0 == rot1) {       // a rotated copy (uniform over the workgroup: the record depends on blockIdx alone)
#pragma unroll 1
        for (int co = 0; co < K1; co++)
            for (int j = tid; j < M; j += nt)
                rot_net_store(out, ext, co, j, rot_read(d0 + (size_t)co * N, j, rot0, N), rot_read(d0 + (size_t)co * N, j + M, rot0, N), K1, N, M);
        return;
    }

    const cplx *key = P.tgsw + (size_t)P.sel[g * (size_t)P.V + var] * ((size_t)L * K1 * K1 * M);
    const int beta = P.g.log2_base;
    const int32_t xormask = gadget_xor_mask(L, beta);

#pragma unroll 1
    for (int c = 0; c < K1; c++) {
        // tmp = ((X^rot1 d1 - X^rot0 d0)[c] + offset) ^ xormask: digit2 then reads the signed digits of tgsw.jl:99-117
        for (int j = tid; j < N; j += nt) {
            const uint32_t v = (uint32_t)rot_read(d1 + (size_t)c * N, j, rot1, N) - (uint32_t)rot_read(d0 + (size_t)c * N, j, rot0, N);
            tmp[j] = (int32_t)((v + (uint32_t)P.g.offset) ^ (uint32_t)xormask);
        }
        __syncthreads();
#pragma unroll 1
        for (int p = 0; p < L; p++) {
            digits_to_buf(tmp, p + 1, beta, M, P.twist, buf, tid, nt);
            __syncthreads();
            fft_fwd(buf, P.wtab, log2M, tid, nt);
            // out[co] += D[p, c] .* C[p, c].a[co]        tgsw.jl:128
#pragma unroll 1
            for (int co = 0; co < K1; co++)
                mac(buf, key + (size_t)((p * K1 + c) * K1 + co) * M, spec + (size_t)co * spec_stride, spec_lds, c == 0 && p == 0, M, tid, nt);
            __syncthreads();
        }
    }

#pragma unroll 1
    for (int co = 0; co < K1; co++) {
        cplx *y = spec + (size_t)co * spec_stride;
        if (!spec_lds) {
            for (int f = tid; f < M; f += nt) buf[phys(f)] = y[f];
            __syncthreads();
            y = buf;
        }
        fft_inv(y, P.wtab, log2M, tid, nt);
        // conj(y_j) e^{-i pi j/N}: real -> coefficient j, imaginary -> j + M (polynomials.jl:127-129), rounded
        // (polynomials.jl:115-116), plus X^rot0 d0 (bootstrap.jl:22)
        for (int j = tid; j < M; j += nt) {
            const cplx v = y[phys(j)], w = P.twist[j];
            const double re = v.x * w.x + v.y * w.y, im = v.x * w.y - v.y * w.x;
            const int32_t *b = d0 + (size_t)co * N;
            const int32_t lo = (int32_t)((uint32_t)rot_read(b, j, rot0, N) + (uint32_t)round_to_torus32(re));
            const int32_t hi = (int32_t)((uint32_t)rot_read(b, j + M, rot0, N) + (uint32_t)round_to_torus32(im));
            rot_net_store(out, ext, co, j, lo, hi, K1, N, M);
        }
        __syncthreads();
    }
}
#endif  // TFHE_EMIT_ROT_NET_KERNELS

}  // namespace leveled
