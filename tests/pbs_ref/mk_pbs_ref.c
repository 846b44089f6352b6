/* mk_pbs_ref.c — test-only CPU checker of multi-key programmable bootstrapping (tests/test_mk_pbs.py compiles it into pytest's temporary
 * directory).  The oracle's source is included as it stands; mk_pbs_rotate restates orc_mk_bootstrap_wo_keyswitch (mk_internals.jl:464-509)
 * with an arbitrary test polynomial v for the body instead of (mu, ..., mu), on the oracle's own mk_extern_mul_add; the final accumulator
 * is then extracted at each coefficient c_j = j N / n_out (mk_tlwe_extract_sample, mk_internals.jl:88-95, generalised from coefficient 0
 * to c, one extracted mask column per party) and keyswitched with orc_mk_keyswitch (mk_internals.jl:397-411) if with_keyswitch. */
#include "../../oracle/tfhe_oracle.c"

/* the final accumulator [(Pn+1)][N] of one row x [Pn n + 1] */
static int mk_pbs_rotate(const orc_params *P, int32_t Pn, const double *bk_re, const double *bk_im, const int32_t *bk_i32, int32_t mode,
                         const int32_t *v /*[N]*/, const int32_t *x, int32_t *acc)
{
    const int N = P->N, n = P->n, l = P->l;
    if (Pn > ORC_MAX_PARTIES || N > ORC_MAX_N || l > ORC_MAX_L_MK) return -1;
    if (mode == 0 && !get_plan(N)) return -1;
    const int log2_2N = ilog2(2 * N);
    int32_t *temp = malloc(sizeof(int32_t) * (size_t)(Pn + 1) * N);
    if (!temp) return -1;
    const int32_t barb = orc_decode_message(x[(size_t)Pn * n], log2_2N);      /* :502 */
    memset(acc, 0, sizeof(int32_t) * (size_t)(Pn + 1) * N);                    /* :72-79 */
    orc_mul_by_monomial(v, N, -barb, acc + (size_t)Pn * N);                    /* :491 with testvect = v */
    const size_t ppk = mk_polys_per_key(l, Pn);
    for (int i = 0; i < Pn; i++) {                                             /* :475 */
        for (int j = 0; j < n; j++) {                                          /* :476 */
            const int32_t bara = orc_decode_message(x[(size_t)i * n + j], log2_2N);
            if (bara == 0) continue;
            for (int c = 0; c <= Pn; c++) {
                orc_mul_by_monomial(acc + (size_t)c * N, N, bara, temp + (size_t)c * N);
                for (int q = 0; q < N; q++) temp[(size_t)c * N + q] = wsub(temp[(size_t)c * N + q], acc[(size_t)c * N + q]);
            }
            const size_t koff = ((size_t)i * n + j) * ppk;
            mk_extern_mul_add(P, Pn, i, temp, bk_re ? bk_re + koff * (N / 2) : NULL, bk_im ? bk_im + koff * (N / 2) : NULL,
                              bk_i32 ? bk_i32 + koff * N : NULL, mode, acc, NULL);
        }
    }
    free(temp);
    return 0;
}

/* mk_tlwe_extract_sample at coefficient c: per party a'[u] = p[c - u] for u <= c, -p[N + c - u] for u > c; b = body[c] */
static void mk_extract_at(const int32_t *acc, int Pn, int N, int c, int32_t *out /*[Pn N + 1]*/)
{
    for (int i = 0; i < Pn; i++)
        for (int u = 0; u < N; u++)
            out[(size_t)i * N + u] = u <= c ? acc[(size_t)i * N + c - u] : (int32_t)(0u - (uint32_t)acc[(size_t)i * N + N + c - u]);
    out[(size_t)Pn * N] = acc[(size_t)Pn * N + c];
}

/* rows [B][Pn n + 1] -> [B][n_out][Pn n + 1] (keyswitched) or [B][n_out][Pn N + 1]; row g uses tv[tv_index[g]] (NULL: table 0) */
int mk_pbs_multi_batch(const orc_params *P, int32_t Pn, const double *bk_re, const double *bk_im, const int32_t *bk_i32, const int32_t *ks,
                       int32_t mode, const int32_t *tv, const int32_t *tv_index, int32_t n_out, const int32_t *in, int32_t *out, int64_t B,
                       int32_t with_keyswitch)
{
    const size_t wi = (size_t)Pn * P->n + 1, we = (size_t)Pn * P->N + 1, wo = with_keyswitch ? wi : we;
    if (n_out < 1 || P->N % n_out) return -1;
    int32_t *acc = malloc(sizeof(int32_t) * (size_t)(Pn + 1) * P->N), *e = malloc(sizeof(int32_t) * we);
    int rc = (acc && e) ? 0 : -1;
    for (int64_t g = 0; g < B && !rc; g++) {
        const int32_t *v = tv + (size_t)(tv_index ? tv_index[g] : 0) * P->N;
        rc = mk_pbs_rotate(P, Pn, bk_re, bk_im, bk_i32, mode, v, in + (size_t)g * wi, acc);
        for (int j = 0; j < n_out && !rc; j++) {
            int32_t *o = out + ((size_t)g * n_out + j) * wo;
            mk_extract_at(acc, Pn, P->N, j * (P->N / n_out), e);
            if (with_keyswitch) orc_mk_keyswitch(P, Pn, ks, e, o);
            else memcpy(o, e, sizeof(int32_t) * we);
        }
    }
    free(acc);
    free(e);
    return rc;
}
