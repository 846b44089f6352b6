/* mk_rotate_ref.c — test-only CPU checker of the multi-key blind rotation of the caller's accumulators (tests/test_mk_blind_rotate.py
 * compiles it into pytest's temporary directory).  The oracle's source is included as it stands, as mk_pbs_ref.c does; mk_rotate_full
 * restates mk_blind_rotate (mk_internals.jl:473-485) from a FULL accumulator: all Pn + 1 polynomials of acc are multiplied by X^-barb
 * (mk_mul_by_monomial, :79-85), the masks included, and every live step is mk_mux_rotate (:464-470) on the oracle's own
 * mk_extern_mul_add with the (party, bit) entry of the bootstrapping key.  The final accumulator is returned as it is (out_form 0),
 * extracted at each coefficient c_j = j N / n_out (mk_tlwe_extract_sample, :88-95, generalised from coefficient 0 to c; out_form 1) or
 * those through orc_mk_keyswitch (:397-411; out_form 2). */
#include "../../oracle/tfhe_oracle.c"

/* acc [(Pn+1)][N] rotated in place by one row x [Pn n + 1] */
static int mk_rotate_full(const orc_params *P, int32_t Pn, const double *bk_re, const double *bk_im, const int32_t *bk_i32, int32_t mode,
                          const int32_t *x, int32_t *acc)
{
    const int N = P->N, n = P->n, l = P->l;
    if (Pn > ORC_MAX_PARTIES || N > ORC_MAX_N || l > ORC_MAX_L_MK) return -1;
    if (mode == 0 && !get_plan(N)) return -1;
    const int log2_2N = ilog2(2 * N);
    int32_t *temp = malloc(sizeof(int32_t) * (size_t)(Pn + 1) * N);
    if (!temp) return -1;
    const int32_t barb = orc_decode_message(x[(size_t)Pn * n], log2_2N);      /* :502 */
    for (int c = 0; c <= Pn; c++) {                                            /* :79-85, on every polynomial */
        orc_mul_by_monomial(acc + (size_t)c * N, N, -barb, temp + (size_t)c * N);
        memcpy(acc + (size_t)c * N, temp + (size_t)c * N, sizeof(int32_t) * N);
    }
    const size_t ppk = mk_polys_per_key(l, Pn);
    for (int i = 0; i < Pn; i++) {                                             /* :475 */
        for (int j = 0; j < n; j++) {                                          /* :476 */
            const int32_t bara = orc_decode_message(x[(size_t)i * n + j], log2_2N);
            if (bara == 0) continue;                                           /* :478-480 */
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
static void mk_rot_extract_at(const int32_t *acc, int Pn, int N, int c, int32_t *out /*[Pn N + 1]*/)
{
    for (int i = 0; i < Pn; i++)
        for (int u = 0; u < N; u++)
            out[(size_t)i * N + u] = u <= c ? acc[(size_t)i * N + c - u] : (int32_t)(0u - (uint32_t)acc[(size_t)i * N + N + c - u]);
    out[(size_t)Pn * N] = acc[(size_t)Pn * N + c];
}

/* rows [B][Pn n + 1], accs [T][Pn+1][N], row g rotates accs[acc_index[g]] (NULL: accumulator 0) -> out_form 0: [B][Pn+1][N] (n_out 1);
 * 1: [B][n_out][Pn N + 1]; 2: [B][n_out][Pn n + 1] */
int mk_rotate_batch(const orc_params *P, int32_t Pn, const double *bk_re, const double *bk_im, const int32_t *bk_i32, const int32_t *ks,
                    int32_t mode, const int32_t *accs, const int32_t *acc_index, int32_t n_out, const int32_t *in, int32_t *out, int64_t B,
                    int32_t out_form)
{
    const size_t wi = (size_t)Pn * P->n + 1, we = (size_t)Pn * P->N + 1, ws = (size_t)(Pn + 1) * P->N;
    if (n_out < 1 || P->N % n_out || out_form < 0 || out_form > 2 || (out_form == 0 && n_out != 1)) return -1;
    const size_t wo = out_form == 2 ? wi : we;
    int32_t *acc = malloc(sizeof(int32_t) * ws), *e = malloc(sizeof(int32_t) * we);
    int rc = (acc && e) ? 0 : -1;
    for (int64_t g = 0; g < B && !rc; g++) {
        memcpy(acc, accs + (size_t)(acc_index ? acc_index[g] : 0) * ws, sizeof(int32_t) * ws);
        rc = mk_rotate_full(P, Pn, bk_re, bk_im, bk_i32, mode, in + (size_t)g * wi, acc);
        if (!rc && out_form == 0) memcpy(out + (size_t)g * ws, acc, sizeof(int32_t) * ws);
        for (int j = 0; out_form != 0 && j < n_out && !rc; j++) {
            int32_t *o = out + ((size_t)g * n_out + j) * wo;
            mk_rot_extract_at(acc, Pn, P->N, j * (P->N / n_out), e);
            if (out_form == 2) orc_mk_keyswitch(P, Pn, ks, e, o);
            else memcpy(o, e, sizeof(int32_t) * we);
        }
    }
    free(acc);
    free(e);
    return rc;
}
