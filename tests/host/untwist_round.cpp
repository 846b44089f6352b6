// Host-side check of the rounding-only untwist (tfhe.jl_amd/csrc/br_core.hpp compiles for the host as well): untwist_round2, whose
// words blind_rotate_kernel_v3 adds into its LDS image by ds_add_u32, against untwist_add2 applied to a zero accumulator, in the
// fused and the unfused form, with the rounding margin both track.  Prints the number of words compared and the number that
// differ; tests/test_untwist_round.py asserts on both.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <random>
#include "br_core.hpp"
using namespace tfhe;

int main()
{
    std::mt19937_64 rng(2027);
    long words = 0, diff = 0, margin_diff = 0;
    for (int it = 0; it < 20000; it++) {
        // spectra of the size the inverse transform delivers (tests/host/twist_forms.cpp): integers up to 2^48 plus a small error
        cplx y[8];
        for (int i = 0; i < 8; i++) {
            const double re = (double)((int64_t)(rng() >> 16) - ((int64_t)1 << 47)) + 0.05 * ((double)(rng() % 2001) / 1000.0 - 1.0);
            const double im = (double)((int64_t)(rng() >> 16) - ((int64_t)1 << 47)) + 0.05 * ((double)(rng() % 2001) / 1000.0 - 1.0);
            const double c = twc(i), s = tws(i);
            y[i].x = re * c - im * s; y[i].y = -(re * s + im * c);
        }
        int32_t acc_f[16] = {0}, acc_u[16] = {0}, w_f[16], w_u[16];
        double worst_a = 0.0, worst_r = 0.0;
        untwist_add2<true, true>(y, acc_f, &worst_a);
        untwist_round2<true, true>(y, w_f, &worst_r);
        untwist_add2<false, false>(y, acc_u);
        untwist_round2<false, false>(y, w_u);
        for (int i = 0; i < 16; i++) {
            words += 2;
            diff += (w_f[i] != acc_f[i]) + (w_u[i] != acc_u[i]);
        }
        margin_diff += worst_a != worst_r;
    }
    printf("untwist_words %ld untwist_diff %ld margin_diff %ld\n", words, diff, margin_diff);
    return 0;
}
