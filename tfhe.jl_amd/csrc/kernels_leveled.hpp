// kernels_leveled.hpp — the leveled mode: one CMUX d0 + C (.) (d1 - d0) per workgroup, with a caller's TGSW sample C and a
// caller's TLWE samples d0, d1 (the form of bootstrap.jl:19-23 with tgsw_extern_mul, tgsw.jl:125-129, on operands that are
// not the bootstrapping key and not a rotating accumulator).  A level of a CMUX tree halves a row's table: output node i of
// row g is CMUX(sel[g][level]; in[2 i], in[2 i + 1]); 2^depth - 1 external products fold a 2^depth-entry table down to the
// entry an encrypted address names, with no blind rotation.  A plain external product is the same kernel with d0 = 0.
//
// Built on the any-N blocks (kernels_anyn.hpp): the folded M = N/2-point mixed-radix transform in LDS, digits_to_buf, mac,
// and selector spectra in fft_fwd's order scaled 1/M (anyn::bk_prepare_kernel makes them: tgsw_prepare, engine_keys.hip), so
// the kernel is correct for every parameter set a context accepts: any power-of-two N, any k, any (l, beta).  Rounding is
// the rotation's (round_to_torus32), and so is the exactness domain: (k + 1) l products are summed before the one rounding.
// Workgroup barriers only; every loop is bounded by a parameter.
#pragma once
#include <hip/hip_runtime.h>

#include "br_core.hpp"
#include "kernels_anyn.hpp"

using namespace tfhe;

namespace leveled {

struct Args {
    const int32_t *in;        // the level's input samples: row r's nodes at in + r * row_words, node m at + m * K1 * N
    const int32_t *row_index; // [B] row g reads input row row_index[g] (level 0 of a tree: its table), or NULL: row g
    const int32_t *sel;       // [B][depth] which selector row g uses at each level, checked by the host
    const cplx *tgsw;         // [S][L][K1][K1][M] selector spectra, fft_fwd's order, scaled 1/M
    int32_t *out;             // [B][nodes_out][K1][N] the level's output samples, or NULL when only `ext` is wanted
    int32_t *ext;             // [B][(K1-1) N + 1] the output extracted at coefficient 0 (tlwe.jl:55-59; nodes_out = 1), or NULL
    cplx *spec_g;             // [workgroups][K1][M] spectrum accumulators when they do not fit LDS, else NULL
    const cplx *wtab;         // [M]  e^{-2 pi i t / M}
    const cplx *twist;        // [M]  e^{-i pi j / N}
    Gadget g;
    int64_t row_words;        // words between two input rows
    int32_t K1, L, log2N;
    int32_t depth, level;     // sel's row length and the column this level reads
    int32_t nodes_out;        // output nodes per row
    int32_t d0_zero;          // 1: the plain external product, d0 = 0 and d1 = input node i (instead of nodes 2 i, 2 i + 1)
};

// LDS: buf [Mp] cplx | spectrum accumulators [K1][Mp] cplx (only if they fit) | tmp [N] int32
__host__ __device__ inline size_t lds_bytes(int N, int nspec_in_lds) { return anyn::lds_bytes(N, nspec_in_lds); }

#ifdef TFHE_EMIT_LEVELED_KERNELS       // (defined by engine_leveled.hip, the one translation unit that launches it)
__global__ __launch_bounds__(512) void cmux_level_kernel(Args P)
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
    const int32_t *row = P.in + (size_t)(P.row_index ? P.row_index[g] : (int64_t)g) * (size_t)P.row_words;
    const int32_t *d0 = P.d0_zero ? nullptr : row + 2 * i * sample;
    const int32_t *d1 = P.d0_zero ? row + i * sample : row + (2 * i + 1) * sample;
    const cplx *key = P.tgsw + (size_t)P.sel[g * (size_t)P.depth + P.level] * ((size_t)L * K1 * K1 * M);
    const int beta = P.g.log2_base;
    const int32_t xormask = gadget_xor_mask(L, beta);

#pragma unroll 1
    for (int c = 0; c < K1; c++) {
        // tmp = ((d1 - d0)[c] + offset) ^ xormask: digit2 then reads the signed digits of tgsw.jl:99-117
        for (int j = tid; j < N; j += nt) {
            const uint32_t v = (uint32_t)d1[(size_t)c * N + j] - (d0 ? (uint32_t)d0[(size_t)c * N + j] : 0u);
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

    int32_t *out = P.out ? P.out + (g * (size_t)P.nodes_out + i) * sample : nullptr;
    int32_t *ext = P.ext ? P.ext + g * ((size_t)(K1 - 1) * N + 1) : nullptr;
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
        // (polynomials.jl:115-116), plus d0 (bootstrap.jl:22)
        for (int j = tid; j < M; j += nt) {
            const cplx v = y[phys(j)], w = P.twist[j];
            const double re = v.x * w.x + v.y * w.y, im = v.x * w.y - v.y * w.x;
            const size_t e = (size_t)co * N + j;
            const int32_t lo = (int32_t)((d0 ? (uint32_t)d0[e] : 0u) + (uint32_t)round_to_torus32(re));
            const int32_t hi = (int32_t)((d0 ? (uint32_t)d0[e + M] : 0u) + (uint32_t)round_to_torus32(im));
            if (out) { out[e] = lo; out[e + M] = hi; }
            if (ext) {
                // tlwe_extract_sample (tlwe.jl:55-59): a'[0] = p[0], a'[m] = -p[N - m], mask polynomials in order; b = body[0]
                if (co + 1 < K1) {
                    int32_t *a = ext + (size_t)co * N;
                    if (j == 0) a[0] = lo; else a[N - j] = (int32_t)(0u - (uint32_t)lo);
                    a[N - (j + M)] = (int32_t)(0u - (uint32_t)hi);
                } else if (j == 0) {
                    ext[(size_t)(K1 - 1) * N] = lo;
                }
            }
        }
        __syncthreads();
    }
}
#endif  // TFHE_EMIT_LEVELED_KERNELS

}  // namespace leveled
