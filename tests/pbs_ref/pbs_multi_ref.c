/* pbs_multi_ref.c — test-only CPU checker of multi-output programmable bootstrapping (tests/test_pbs_multi.py compiles it into pytest's
 * temporary directory).  The oracle's source is included as it stands; the functions added restate blind_rotate_and_extract(v, bk,
 * barb, bara) (bootstrap.jl:50-59) after the modulus switch of bootstrap_wo_keyswitch (bootstrap.jl:69-82) with an arbitrary test
 * polynomial v, on the oracle's own extern_mul_add, as tests/pbs_ref/pbs_ref.c does, and then extract the final accumulator at each
 * coefficient c_j = j N / n_out: tlwe_extract_sample (tlwe.jl:55-59) generalised from coefficient 0 to c, keyswitched (bootstrap.jl:92-95)
 * if with_keyswitch.  With n_out = 1 it is pbs_ref.c's pbs_bootstrap_batch. */
#include "../../oracle/tfhe_oracle.c"

/* the final accumulator [(k+1)][N] of one row */
static int pbs_rotate(const orc_params *P, const double *bk_re, const double *bk_im, const int32_t *bk_i32, int32_t mode, const int32_t *v /*[N]*/,
                      const int32_t *x /*[n+1]*/, int32_t *acc /*[(k+1)][N]*/)
{
    const int N = P->N, n = P->n, k1 = P->k + 1, l = P->l;
    if (N > ORC_MAX_N || l > ORC_MAX_L || P->k > ORC_MAX_K) return -1;
    if (mode == 0 && !get_plan(N)) return -1;
    const int log2_2N = ilog2(2 * N);
    int32_t temp[(ORC_MAX_K + 1) * ORC_MAX_N];

    const int32_t barb = orc_decode_message(x[n], log2_2N);                 /* bootstrap.jl:75 */
    memset(acc, 0, sizeof(int32_t) * (size_t)(k1 * N));                     /* tlwe.jl:77-81   */
    orc_mul_by_monomial(v, N, -barb, acc + (k1 - 1) * N);                   /* bootstrap.jl:54 */

    const size_t per_i = (size_t)l * k1 * k1;
    for (int i = 0; i < n; i++) {                                           /* bootstrap.jl:33 */
        const int32_t bara = orc_decode_message(x[i], log2_2N);             /* bootstrap.jl:74 */
        if (bara == 0) continue;                                            /* bootstrap.jl:34 */
        for (int c = 0; c < k1; c++) {                                      /* bootstrap.jl:21 */
            orc_mul_by_monomial(acc + c * N, N, bara, temp + c * N);
            for (int j = 0; j < N; j++) temp[c * N + j] = wsub(temp[c * N + j], acc[c * N + j]);
        }
        const size_t off = (size_t)i * per_i;
        extern_mul_add(P, temp,
                       bk_re ? bk_re + off * (N / 2) : NULL, bk_im ? bk_im + off * (N / 2) : NULL,
                       bk_i32 ? bk_i32 + off * N : NULL, mode, acc, NULL);   /* bootstrap.jl:22 */
    }
    return 0;
}

/* tlwe_extract_sample at coefficient c (tlwe.jl:55-59 with 0 -> c): coefficient c of body - sum_i a_i s_i is
 * body[c] - sum_i sum_u a'_i[u] s_i[u] with a'_i[u] = p_i[c - u] for u <= c and -p_i[N + c - u] for u > c; b = body[c].
 * c = 0 is the oracle's extract_sample. */
static void extract_at(const int32_t *acc, int k, int N, int c, int32_t *out /*[kN+1]*/)
{
    for (int i = 0; i < k; i++)
        for (int u = 0; u < N; u++)
            out[i * N + u] = u <= c ? acc[i * N + c - u] : (int32_t)(0u - (uint32_t)acc[i * N + N + c - u]);
    out[k * N] = acc[k * N + c];
}

/* rows [B][n+1] -> [B][n_out][n+1] (keyswitched) or [B][n_out][kN+1]; row g uses tv[tv_index[g]] (tv_index NULL: table 0) and its
 * output j is extracted at j N / n_out (n_out a power of two dividing N) */
int pbs_multi_batch(const orc_params *P, const double *bk_re, const double *bk_im, const int32_t *bk_i32, const int32_t *ks, int32_t mode,
                    const int32_t *tv, const int32_t *tv_index, int32_t n_out, const int32_t *in, int32_t *out, int64_t B, int32_t with_keyswitch)
{
    const int n1 = P->n + 1, ext = P->k * P->N + 1, wo = with_keyswitch ? n1 : ext;
    int rc = 0;
    if (n_out < 1 || P->N % n_out) return -1;
    if (mode == 0 && !get_plan(P->N)) return -1;
#pragma omp parallel for schedule(dynamic) reduction(| : rc)
    for (int64_t g = 0; g < B; g++) {
        int32_t acc[(ORC_MAX_K + 1) * ORC_MAX_N], e[ORC_MAX_K * ORC_MAX_N + 1];
        const int32_t *v = tv + (size_t)(tv_index ? tv_index[g] : 0) * P->N;
        rc |= pbs_rotate(P, bk_re, bk_im, bk_i32, mode, v, in + g * n1, acc);
        for (int j = 0; j < n_out; j++) {
            int32_t *o = out + ((size_t)g * n_out + j) * wo;
            extract_at(acc, P->k, P->N, j * (P->N / n_out), e);
            if (with_keyswitch) orc_keyswitch(P, ks, e, o);
            else memcpy(o, e, sizeof(int32_t) * (size_t)ext);
        }
    }
    return rc;
}

/* the shift rule the engine applies (extract_shift_kernel): X^c times each of the k mask polynomials of an index-0 extraction e,
 * and the body `body`: [kN+1] -> [kN+1] */
void pbs_shift_extraction(const int32_t *e, int k, int N, int c, int32_t body, int32_t *out)
{
    for (int i = 0; i < k; i++)
        for (int u = 0; u < N; u++)
            out[i * N + u] = u >= c ? e[i * N + u - c] : (int32_t)(0u - (uint32_t)e[i * N + N + u - c]);
    out[k * N] = body;
}

/* extract_at on a caller's accumulator [(k+1)][N] (the CPU test of the shift rule) */
void pbs_extract_at(const int32_t *acc, int k, int N, int c, int32_t *out)
{
    extract_at(acc, k, N, c, out);
}
