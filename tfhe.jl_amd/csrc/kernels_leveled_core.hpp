// kernels_leveled_core.hpp — what the five CMUX level kernels of the leveled mode share, written once: the argument fields, the
// workgroup's frame in LDS, the read of a source sample (plain, absent, or rotated by a public monomial), the store of an output pair
// with its extraction at coefficient 0, the digit / transform / mac pass over one source polynomial, the inverse transform with the
// one rounding, the copy node, and on top of those the single-key and the multi-key CMUX.  The kernels (kernels_leveled.hpp,
// kernels_cmux_net.hpp, kernels_rot_net.hpp, kernels_mk_leveled.hpp, kernels_mk_cmux_net.hpp) decode their own record and call these.
//
// Built on the any-N blocks (kernels_anyn.hpp): the folded M = N/2-point mixed-radix transform in LDS, digits_to_buf, mac, and
// selector spectra in fft_fwd's order scaled 1/M, so a kernel is correct for every parameter set a context accepts.  Rounding is the
// rotation's (round_to_torus32): all products of an output polynomial are summed before the one rounding.  Every function is inlined
// into its kernel and the kind of a source is a compile-time constant: a kernel pays for the source kinds it names and no other.
// Workgroup barriers only; every loop is bounded by a parameter; inputs are read-only and the outputs go to another buffer.
#pragma once
#include <hip/hip_runtime.h>

#include "br_core.hpp"
#include "kernels_anyn.hpp"

using namespace tfhe;

namespace leveled {

// the fields every level kernel's argument struct has; a sample has `polys` polynomials: k + 1 single-key, P + 1 multi-key
struct LevelArgs {
    const int32_t *in;        // the level's input samples: row r's nodes at in + r * row_words, node m at + m * polys * N
    const int32_t *row_index; // [B] row g reads input row row_index[g] (level 0: its table), or NULL: row g
    const int32_t *sel;       // [B][V] the selector behind each of row g's variables (a tree: behind each level), checked by the host
    const cplx *tgsw;         // [S][...][M] selector spectra, fft_fwd's order, scaled 1/M: single-key [L][K1][K1], multi-key
                              // x[L][P] | y[L][P] | c0[L] | c1[L]
    int32_t *out;             // [B][nodes_out][polys][N] the level's output samples, or NULL when only `ext` is wanted
    int32_t *ext;             // [B][nodes_out][(polys-1) N + 1] every output extracted at coefficient 0 (tlwe.jl:55-59,
                              // mk_internals.jl:88-95), or NULL
    cplx *spec_g;             // [workgroups][K1 or 3][M] spectrum accumulators when they are not in LDS, else NULL
    const cplx *wtab;         // [M]  e^{-2 pi i t / M}
    const cplx *twist;        // [M]  e^{-i pi j / N}
    Gadget g;
    int64_t row_words;        // words between two input rows
    int32_t L, log2N;
    int32_t nodes_out;        // output nodes per row
};

// LDS: buf [Mp] cplx | spectrum accumulators [K1][Mp] cplx (only if they fit) | tmp [N] int32
__host__ __device__ inline size_t lds_bytes(int N, int nspec_in_lds) { return anyn::lds_bytes(N, nspec_in_lds); }
// LDS: buf [Mp] cplx | self, party, body spectrum accumulators [3][Mp] cplx (only if they fit) | tmp [N] int32
__host__ __device__ inline size_t mk_lds_bytes(int N, bool spec_in_lds) { return anyn::lds_bytes(N, spec_in_lds ? 3 : 0); }

// ---- the workgroup's frame ------------------------------------------------------------------------------------------------------
// blockIdx.x = g * nodes_out + i: the workgroups of a row sit together and share its selector spectra in L2
struct Frame {
    int tid, nt, N, M, log2M, L;
    bool spec_lds;
    cplx *buf, *spec;         // the transform buffer; the `nspec` spectrum accumulators, `ss` apart
    int ss;
    int32_t *tmp;             // the gadget-offset difference of the source polynomial being decomposed
    size_t g, i;              // the row and the output node of this workgroup
    const int32_t *row;       // the row's input samples
    const cplx *wtab, *twist;
};

__device__ __forceinline__ Frame frame(const LevelArgs &P, char *smem, int nspec)
{
    using namespace anyn;
    Frame f;
    f.tid = threadIdx.x, f.nt = blockDim.x;
    f.N = 1 << P.log2N, f.M = f.N >> 1, f.log2M = P.log2N - 1, f.L = P.L;
    const int Mp = padded_len(f.M);
    f.spec_lds = P.spec_g == nullptr;
    f.buf = reinterpret_cast<cplx *>(smem);
    f.spec = f.spec_lds ? f.buf + Mp : P.spec_g + (size_t)blockIdx.x * nspec * f.M;
    f.ss = f.spec_lds ? Mp : f.M;
    f.tmp = reinterpret_cast<int32_t *>(f.buf + (size_t)(f.spec_lds ? 1 + nspec : 1) * Mp);
    f.g = blockIdx.x / (unsigned)P.nodes_out, f.i = blockIdx.x % (unsigned)P.nodes_out;
    f.row = P.in + (size_t)(P.row_index ? P.row_index[f.g] : (int64_t)f.g) * (size_t)P.row_words;
    f.wtab = P.wtab, f.twist = P.twist;
    return f;
}

// what the decomposition of a polynomial needs; made where a product starts (a copy node leaves before: its workgroup, and the loads
// that depend on a node's record, do not wait for the mask's loop)
struct Decomp { int beta; uint32_t offset, xormask; };
__device__ __forceinline__ Decomp decomp(const Gadget &g, int L) { return {g.log2_base, (uint32_t)g.offset, (uint32_t)gadget_xor_mask(L, g.log2_base)}; }

// this workgroup's output sample and / or its extraction, each NULL when the level does not write it
__device__ __forceinline__ int32_t *node_out(int32_t *base, size_t words) { return base ? base + (size_t)blockIdx.x * words : nullptr; }

// ---- a source sample ------------------------------------------------------------------------------------------------------------
enum SrcKind { SRC_PLAIN, SRC_OR_ZERO, SRC_ROTATED };      // p[j] | p == NULL reads 0 (the plain external product's d0) | (X^rot p)[j]

template <SrcKind KIND>
struct Src { const int32_t *p; int rot; };

// coefficient j of X^r p for 0 <= r < 2N: p[s] for s = (j - r) mod 2N < N, else -p[s - N], negated in uint32 (-2^31 stays -2^31)
__device__ __forceinline__ int32_t rot_read(const int32_t *p, int j, int r, int N)
{
    const int s = (j - r) & (2 * N - 1);
    const int32_t v = p[s & (N - 1)];
    return s < N ? v : (int32_t)(0u - (uint32_t)v);
}

// coefficient j + half of polynomial d of the source (half: 0 or M, added to the 64-bit index as the loop-invariant it is)
template <SrcKind KIND>
__device__ __forceinline__ uint32_t src_read(const Src<KIND> &s, int d, int j, int half, int N)
{
    if constexpr (KIND == SRC_ROTATED) return (uint32_t)rot_read(s.p + (size_t)d * N, j + half, s.rot, N);
    else if constexpr (KIND == SRC_OR_ZERO) return s.p ? (uint32_t)s.p[(size_t)d * N + j + half] : 0u;
    else return (uint32_t)s.p[(size_t)d * N + j + half];
}

// ---- the store ------------------------------------------------------------------------------------------------------------------
// one pair of output words (coefficients j and j + M of polynomial d) to the sample and / or its extraction at coefficient 0, for a
// sample of `masks` mask polynomials and a body: tlwe_extract_sample (tlwe.jl:55-59; per party mk_internals.jl:88-95): a'[0] = p[0],
// a'[m] = -p[N - m], mask polynomials in order; b = body[0]
__device__ __forceinline__ void store_pair(int32_t *out, int32_t *ext, int d, int j, int32_t lo, int32_t hi, int masks, int N, int M)
{
    const size_t e = (size_t)d * N + j;
    if (out) { out[e] = lo; out[e + M] = hi; }
    if (ext) {
        if (d < masks) {
            int32_t *a = ext + (size_t)d * N;
            if (j == 0) a[0] = lo; else a[N - j] = (int32_t)(0u - (uint32_t)lo);
            a[N - (j + M)] = (int32_t)(0u - (uint32_t)hi);
        } else if (j == 0) {
            ext[(size_t)masks * N] = lo;
        }
    }
}

// ---- the product pass -----------------------------------------------------------------------------------------------------------
// polynomial d of d1 - d0, decomposed into L digits; macs(p) multiplies digit p's spectrum (f.buf) into the accumulators it feeds
template <SrcKind K1ND, SrcKind K0ND, class Macs>
__device__ __forceinline__ void product_pass(const Frame &f, const Decomp &g, const Src<K1ND> &d1, const Src<K0ND> &d0, int d, Macs macs)
{
    using namespace anyn;
    // tmp = ((d1 - d0)[d] + offset) ^ xormask: digit2 then reads the signed digits of tgsw.jl:99-117
    for (int j = f.tid; j < f.N; j += f.nt) {
        const uint32_t v = src_read(d1, d, j, 0, f.N) - src_read(d0, d, j, 0, f.N);
        f.tmp[j] = (int32_t)((v + g.offset) ^ g.xormask);
    }
    __syncthreads();
#pragma unroll 1
    for (int p = 0; p < f.L; p++) {
        digits_to_buf(f.tmp, p + 1, g.beta, f.M, f.twist, f.buf, f.tid, f.nt);
        __syncthreads();
        fft_fwd(f.buf, f.wtab, f.log2M, f.tid, f.nt);
        macs(p);
        __syncthreads();
    }
}

// ---- the finish -----------------------------------------------------------------------------------------------------------------
// inverse transform of spectrum accumulator `which`, round, + d0's polynomial d, store as polynomial d
template <SrcKind K0ND>
__device__ __forceinline__ void finish(const Frame &f, int which, const Src<K0ND> &d0, int d, int32_t *out, int32_t *ext, int masks)
{
    using namespace anyn;
    cplx *y = f.spec + (size_t)which * f.ss;
    if (!f.spec_lds) {
        for (int t = f.tid; t < f.M; t += f.nt) f.buf[phys(t)] = y[t];
        __syncthreads();
        y = f.buf;
    }
    fft_inv(y, f.wtab, f.log2M, f.tid, f.nt);
    // conj(y_j) e^{-i pi j/N}: real -> coefficient j, imaginary -> j + M (polynomials.jl:127-129), rounded
    // (polynomials.jl:115-116), plus d0 (bootstrap.jl:22)
    for (int j = f.tid; j < f.M; j += f.nt) {
        const cplx v = y[phys(j)], w = f.twist[j];
        const double re = v.x * w.x + v.y * w.y, im = v.x * w.y - v.y * w.x;
        const int32_t lo = (int32_t)(src_read(d0, d, j, 0, f.N) + (uint32_t)round_to_torus32(re));
        const int32_t hi = (int32_t)(src_read(d0, d, j, f.M, f.N) + (uint32_t)round_to_torus32(im));
        store_pair(out, ext, d, j, lo, hi, masks, f.N, f.M);
    }
    __syncthreads();
}

// ---- the copy node --------------------------------------------------------------------------------------------------------------
// a node whose two edges are the same: no product, no noise, and word for word what the formula gives (the product of the zero
// difference is exactly zero).  Uniform over the workgroup: the record depends on blockIdx alone.
template <SrcKind K0ND>
__device__ __forceinline__ void copy_node(const Frame &f, const Src<K0ND> &d0, int masks, int32_t *out, int32_t *ext)
{
#pragma unroll 1
    for (int d = 0; d <= masks; d++)
        for (int j = f.tid; j < f.M; j += f.nt)
            store_pair(out, ext, d, j, (int32_t)src_read(d0, d, j, 0, f.N), (int32_t)src_read(d0, d, j, f.M, f.N), masks, f.N, f.M);
}

// ---- the single-key CMUX d0 + C (.) (d1 - d0) -----------------------------------------------------------------------------------
// C = selector si, [L][K1][K1][M] (the form of bootstrap.jl:19-23 with tgsw_extern_mul, tgsw.jl:125-129).  Accumulation order: c
// outer, p inner, the first product initialises.
template <SrcKind K1ND, SrcKind K0ND>
__device__ __forceinline__ void cmux(const Frame &f, const Gadget &gadget, const cplx *tgsw, int32_t si, const Src<K1ND> &d1, const Src<K0ND> &d0, int K1, int32_t *out,
                                     int32_t *ext)
{
    using namespace anyn;
    const cplx *key = tgsw + (size_t)si * ((size_t)f.L * K1 * K1 * f.M);
    const Decomp g = decomp(gadget, f.L);
#pragma unroll 1
    for (int c = 0; c < K1; c++)
        product_pass(f, g, d1, d0, c, [&](int p) {
            // out[co] += D[p, c] .* C[p, c].a[co]        tgsw.jl:128
#pragma unroll 1
            for (int co = 0; co < K1; co++)
                mac(f.buf, key + (size_t)((p * K1 + c) * K1 + co) * f.M, f.spec + (size_t)co * f.ss, f.spec_lds, c == 0 && p == 0, f.M, f.tid, f.nt);
        });
#pragma unroll 1
    for (int co = 0; co < K1; co++) finish(f, co, d0, co, out, ext, K1 - 1);
}

// ---- the multi-key CMUX ---------------------------------------------------------------------------------------------------------
// C = expanded RGSW selector si of party `party` (mk_tgsw_extern_mul, mk_internals.jl:348-391).  With digits da[p, s] of mask s of
// d1 - d0 and db[p] of its body (spectrum-domain sums, as every MK kernel here):
//   a'_s     = d0.a_s     + sum_p da[p, s] (*) y[p, party]                          for every s != party     (:377-378)
//   a'_party = d0.a_party + sum_{p, s} da[p, s] (*) y[p, s] + sum_p db[p] (*) c1[p]                           (:371-376)
//   b'       = d0.b       + sum_{p, s} da[p, s] (*) x[p, s] + sum_p db[p] (*) c0[p]                           (:382-385)
// Three spectrum accumulators [self | party | body] are live whatever P is (anyn::mk_blind_rotate_kernel, kernels_anyn.hpp): a'_s of
// a non-party source is fed by its own digits only, so it is finished right after source s.
template <SrcKind K1ND, SrcKind K0ND>
__device__ __forceinline__ void mk_cmux(const Frame &f, const Gadget &gadget, const cplx *tgsw, int32_t si, int party, const Src<K1ND> &d1, const Src<K0ND> &d0, int NP,
                                        int32_t *out, int32_t *ext)
{
    using namespace anyn;
    const int L = f.L, per = 2 * L * NP + 2 * L;
    const cplx *key = tgsw + (size_t)si * per * f.M;
    const Decomp g = decomp(gadget, L);
    bool first_pb = true;
#pragma unroll 1
    for (int s = 0; s <= NP; s++) {
        const bool is_body = (s == NP), has_self = (!is_body && s != party);
        product_pass(f, g, d1, d0, s, [&](int p) {
            const cplx *k_party = key + (size_t)(is_body ? 2 * L * NP + L + p : L * NP + p * NP + s) * f.M;   // c1[p] | y[p, s]
            const cplx *k_body = key + (size_t)(is_body ? 2 * L * NP + p : p * NP + s) * f.M;                 // c0[p] | x[p, s]
            mac(f.buf, k_party, f.spec + (size_t)1 * f.ss, f.spec_lds, first_pb, f.M, f.tid, f.nt);
            mac(f.buf, k_body, f.spec + (size_t)2 * f.ss, f.spec_lds, first_pb, f.M, f.tid, f.nt);
            first_pb = false;
            if (has_self) mac(f.buf, key + (size_t)(L * NP + p * NP + party) * f.M, f.spec, f.spec_lds, p == 0, f.M, f.tid, f.nt);   // y[p, party]
        });
        if (has_self) finish(f, 0, d0, s, out, ext, NP);
    }
    finish(f, 1, d0, party, out, ext, NP);
    finish(f, 2, d0, NP, out, ext, NP);
}

}  // namespace leveled
