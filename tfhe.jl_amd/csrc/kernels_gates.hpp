// kernels_gates.hpp — gate prologue / modulus switch / non-bootstrapped gates (gates.jl, bootstrap.jl:74-75).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/tfhe_mi355x.h"
#include "br_core.hpp"

using namespace tfhe;

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------

// Per-opcode affine prologue  t = (0, cst) + sx*x + sy*y  [* 2 for XOR/XNOR]   (gates.jl)
struct GateForm {
    int32_t cst;   // constant added to b
    int8_t sx, sy; // +-1 coefficients (after the optional doubling)
    int8_t mul2;   // (x + y) * 2 form (gates.jl:52,64)
    int8_t use_z;  // second operand comes from in2 (MUX second half)
};

__host__ __device__ inline GateForm gate_form(int kind)
{
    // kind: opcode for plain gates; 100 = MUX first half (AND(x,y)), 101 = MUX second half (ANDNY(x,z))
    const int32_t p8 = (int32_t)(1u << 29), p4 = (int32_t)(1u << 30);
    switch (kind) {
    case TFHE_GATE_NAND:  return {p8, -1, -1, 0, 0};
    case TFHE_GATE_OR:    return {p8, 1, 1, 0, 0};
    case TFHE_GATE_AND:   return {-p8, 1, 1, 0, 0};
    case TFHE_GATE_XOR:   return {p4, 1, 1, 1, 0};
    case TFHE_GATE_XNOR:  return {-p4, -1, -1, 1, 0};
    case TFHE_GATE_NOR:   return {-p8, -1, -1, 0, 0};
    case TFHE_GATE_ANDNY: return {-p8, -1, 1, 0, 0};
    case TFHE_GATE_ANDYN: return {-p8, 1, -1, 0, 0};
    case TFHE_GATE_ORNY:  return {p8, -1, 1, 0, 0};
    case TFHE_GATE_ORYN:  return {p8, 1, -1, 0, 0};
    case 100:             return {-p8, 1, 1, 0, 0};   // gates.jl:166
    case 101:             return {-p8, -1, 1, 0, 1};  // gates.jl:170
    default:              return {0, 0, 0, 0, 0};
    }
}

// rot_a[w] / rot_b[w] = rows of the two operands of rotation w (batch mode: the gate index; level mode: wire
// indices), rot_kind[w] = kind (see gate_form); writes bara[w][0..n] (barb last).
__global__ void prologue_kernel(const int32_t *in0, const int32_t *in1, const int32_t *in2,
                                const int32_t *__restrict__ rot_a, const int32_t *__restrict__ rot_b,
                                const uint8_t *__restrict__ rot_kind, int32_t *__restrict__ bara, int n,
                                int log2_2N)
{
    const int w = blockIdx.x;
    const GateForm f = gate_form(rot_kind[w]);
    const int32_t *x = in0 + (size_t)rot_a[w] * (n + 1);
    const int32_t *y = (f.use_z ? in2 : in1) + (size_t)rot_b[w] * (n + 1);
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        uint32_t v;
        if (f.mul2) {
            v = ((uint32_t)x[i] + (uint32_t)y[i]) * 2u;
            if (f.sx < 0) v = 0u - v;
        } else {
            const uint32_t xv = f.sx > 0 ? (uint32_t)x[i] : 0u - (uint32_t)x[i];
            const uint32_t yv = f.sy > 0 ? (uint32_t)y[i] : 0u - (uint32_t)y[i];
            v = xv + yv;
        }
        if (i == n) v += (uint32_t)f.cst;
        // decode_message(v, 2N): numeric-functions.jl:31-34
        const int32_t r = (int32_t)(v + (1u << (32 - log2_2N - 1))) >> (32 - log2_2N);
        bara[(size_t)w * (n + 1) + i] = r;
    }
}

// modulus switch only (tfhe_bootstrap_batch): bara[w][i] = decode_message(in[w][i], 2N)
__global__ void modswitch_kernel(const int32_t *__restrict__ in, int32_t *__restrict__ bara, int n, int log2_2N)
{
    const size_t w = blockIdx.x;
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        const uint32_t v = (uint32_t)in[w * (n + 1) + i];
        bara[w * (n + 1) + i] = (int32_t)(v + (1u << (32 - log2_2N - 1))) >> (32 - log2_2N);
    }
}

// Integer linear combination of wire-table rows (tfhe_lut_level / tfhe_linear_level): row g is
//   x_g = sum over t in [term_start[g], term_start[g+1]) of term_coef[t] * wires[term_wire[t]], plus cst[g] on the body (cst NULL: 0)
// in uint32_t wrap-around, exactly LweSampleArray's +, integer scale and add_constant.  kLut: decode_message(x_g, 2N) into
// dst[g] (the modulus switch of modswitch_kernel, the rotation's input in bara); otherwise x_g itself into dst[out[g]] (the wire
// table: no row of a level reads a row it writes, tfhe_lut_level's validation).  One workgroup per row, consecutive threads on
// consecutive words of each term row; the term list is uniform over the workgroup.
template <bool kLut>
__global__ __launch_bounds__(256) void linear_prologue_kernel(const int32_t *wires, const int32_t *__restrict__ term_start,
                                                              const int32_t *__restrict__ term_wire, const int32_t *__restrict__ term_coef,
                                                              const int32_t *__restrict__ cst, const int32_t *__restrict__ out, int32_t *dst,
                                                              int n, int log2_2N)
{
    const size_t g = blockIdx.x;
    const int t0 = term_start[g], t1 = term_start[g + 1];
    const size_t n1 = (size_t)n + 1;
    int32_t *row = dst + (kLut ? g : (size_t)out[g]) * n1;
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        uint32_t v = 0;
        for (int t = t0; t < t1; t++) v += (uint32_t)term_coef[t] * (uint32_t)wires[(size_t)term_wire[t] * n1 + i];
        if (i == n && cst) v += (uint32_t)cst[g];
        if (kLut) row[i] = (int32_t)(v + (1u << (32 - log2_2N - 1))) >> (32 - log2_2N);      // numeric-functions.jl:31-34
        else row[i] = (int32_t)v;
    }
}

// gate_not / gate_constant / copy (gates.jl:76-93)
__global__ void trivial_gates_kernel(const int32_t *in0, const int32_t *__restrict__ src_rows,
                                     const int32_t *__restrict__ dst_rows, const uint8_t *__restrict__ ops,
                                     int32_t *out, int n)
{
    const size_t gs = (size_t)src_rows[blockIdx.x], gd = (size_t)dst_rows[blockIdx.x];
    const int op = ops[blockIdx.x];
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        uint32_t v;
        if (op == TFHE_GATE_NOT) v = 0u - (uint32_t)in0[gs * (n + 1) + i];
        else if (op == TFHE_GATE_COPY) v = (uint32_t)in0[gs * (n + 1) + i];
        else v = (i == n) ? (op == TFHE_GATE_CONST1 ? (1u << 29) : 0u - (1u << 29)) : 0u;
        out[gd * (n + 1) + i] = (int32_t)v;
    }
}


// Multi-output programmable bootstrapping (tfhe_bootstrap_tv_multi_batch): sample j of row g is the extraction of row g's final
// accumulator at coefficient c_j = j N / K instead of 0 (tlwe.jl:55-59 generalised), made from the index-0 extraction ext[g] and the
// body coefficients bodies[g][j] the TV kernel wrote.  Mask polynomial i of out[g][j] = X^{c_j} (mask polynomial i of ext[g]):
// a[u] = e[u - c_j] for u >= c_j, -e[N + u - c_j] for u < c_j; its body = bodies[g][j].  ext: [B][W], bodies: [B][K] = [B K],
// out: [B][K][W] = [B K][W], W = k N + 1.  out is one flat array of `total` = B K W words: thread t writes words 4t .. 4t + 3 with one
// 16-byte store (out is 256-byte aligned; the last, partial group word by word) and reads its source words with dword loads,
// consecutive threads reading consecutive words of a row.  A row spans at least N + 1 > 4 words, so four words cross at most one row end.
__global__ __launch_bounds__(256) void extract_shift_kernel(const int32_t *__restrict__ ext, const int32_t *__restrict__ bodies,
                                                            int32_t *__restrict__ out, size_t total, int W, int log2N, int log2K)
{
    const size_t f0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (f0 >= total) return;
    size_t r = f0 / (size_t)W;                    // output row g K + j
    int p = (int)(f0 - r * (size_t)W);            // word within the row
    const int Nm = (1 << log2N) - 1;
    int32_t v[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int32_t x = 0;
        if (f0 + q < total) {
            if (p == W - 1) {
                x = bodies[r];
            } else {
                const int c = (int)(r & ((1u << log2K) - 1)) << (log2N - log2K);
                const int u = p & Nm, s = u - c;
                const uint32_t e = (uint32_t)ext[(r >> log2K) * (size_t)W + (p - u) + (s & Nm)];
                x = (int32_t)(s >= 0 ? e : 0u - e);
            }
        }
        v[q] = x;
        if (++p == W) { p = 0; r++; }
    }
    if (f0 + 4 <= total) {
        *reinterpret_cast<int4 *>(out + f0) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (f0 + q < total) out[f0 + q] = v[q];
    }
}
