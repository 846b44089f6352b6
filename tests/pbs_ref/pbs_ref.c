/* pbs_ref.c — test-only CPU checker of programmable bootstrapping (tests/test_pbs.py compiles it into pytest's temporary directory).
 * The oracle's source is included as it stands; the one function added restates blind_rotate_and_extract(v, bk, barb, bara)
 * (bootstrap.jl:50-59) after the modulus switch of bootstrap_wo_keyswitch (bootstrap.jl:69-82) with an arbitrary test polynomial
 * v instead of repeat([mu], N), keyswitched (bootstrap.jl:92-95) if with_keyswitch, on the oracle's own extern_mul_add and
 * extract_sample.  With v = (mu, ..., mu) it is orc_bootstrap_wo_keyswitch. */
#include "../../oracle/tfhe_oracle.c"

static int pbs_one(const orc_params *P, const double *bk_re, const double *bk_im, const int32_t *bk_i32, int32_t mode,
                   const int32_t *v /*[N]*/, const int32_t *x /*[n+1]*/, int32_t *out /*[kN+1]*/)
{
    const int N = P->N, n = P->n, k1 = P->k + 1, l = P->l;
    if (N > ORC_MAX_N || l > ORC_MAX_L || P->k > ORC_MAX_K) return -1;
    if (mode == 0 && !get_plan(N)) return -1;
    const int log2_2N = ilog2(2 * N);
    int32_t acc[(ORC_MAX_K + 1) * ORC_MAX_N], temp[(ORC_MAX_K + 1) * ORC_MAX_N];

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
    extract_sample(acc, P->k, N, out);                                      /* bootstrap.jl:58 */
    return 0;
}

/* rows [B][n+1] -> [B][n+1] (keyswitched) or [B][kN+1]; row g uses tv[tv_index[g]] (tv_index NULL: table 0) */
int pbs_bootstrap_batch(const orc_params *P, const double *bk_re, const double *bk_im, const int32_t *bk_i32, const int32_t *ks,
                        int32_t mode, const int32_t *tv, const int32_t *tv_index, const int32_t *in, int32_t *out, int64_t B,
                        int32_t with_keyswitch)
{
    const int n1 = P->n + 1, ext = P->k * P->N + 1;
    int rc = 0;
    if (mode == 0 && !get_plan(P->N)) return -1;
#pragma omp parallel for schedule(dynamic) reduction(| : rc)
    for (int64_t g = 0; g < B; g++) {
        int32_t e[ORC_MAX_K * ORC_MAX_N + 1];
        const int32_t *v = tv + (size_t)(tv_index ? tv_index[g] : 0) * P->N;
        rc |= pbs_one(P, bk_re, bk_im, bk_i32, mode, v, in + g * n1, e);
        if (with_keyswitch) orc_keyswitch(P, ks, e, out + g * n1);
        else memcpy(out + g * ext, e, sizeof(int32_t) * (size_t)ext);
    }
    return rc;
}
