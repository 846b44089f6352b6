// Host-side check of the consumer-side pass-B twiddles in tan form (tfhe.jl_amd/csrc/br_core.hpp: fill_tan2, tan2_apply,
// dft8_scaled — the lane code of blind_rotate_kernel_v3, which compiles for the host as well).
//   stage: tan2_apply<INV> + dft8_scaled<INV> and the plain form (x[v] * tw2[v][s], conjugated for the inverse, + dft8<INV>) against a
//          long-double evaluation with long-double twiddles, for every lane group s = lane & 7 and both directions, on random inputs of the
//          magnitudes the kernel sees (forward: |x| up to 2^19; inverse: up to 2^52).  Error of one trial: the largest |difference| of
//          the eight outputs over the largest |reference output|.
//   chain: the 512-point forward transform of a random digit polynomial (|d| <= 512) as the kernel runs it, lane by lane, times the
//          prepared spectrum of a random Int32 polynomial, through the kernel's inverse transform, untwist and rounding: every coefficient
//          must be the integer negacyclic product mod 2^32.
// tests/test_tan2_pass_b.py asserts on the printed lines.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "br_core.hpp"
using namespace tfhe;

typedef cplx Regs[64][8];
static const long double kPi = 3.14159265358979323846264338327950288L;

static double urand(std::mt19937_64 &rng, double mag) { return mag * (2.0 * ((double)(rng() >> 11) / 9007199254740992.0) - 1.0); }

// one direction of the stage test for lane group s; returns the worst errors of the (tan, plain) forms
template <bool INV>
static void stage(int s, const double *tan2, const cplx *tw2, std::mt19937_64 &rng, double &worst_tan, double &worst_plain)
{
    LaneTan2 k;
    load_lane_tan2(s, tan2, k);
    const double mag = INV ? 4503599627370496.0 : 524288.0;
    worst_tan = worst_plain = 0.0;
    for (int it = 0; it < 300; it++) {
        cplx a[8], b[8];
        long double xr[8], xi[8];
        for (int v = 0; v < 8; v++) {
            a[v] = b[v] = mk(urand(rng, mag), urand(rng, mag));
            // x[v] * e^{-+ 2 pi i v s/64} in long double
            const long double ang = (INV ? 2 : -2) * kPi * (long double)(v * s) / 64.0L, c = cosl(ang), sn = sinl(ang);
            xr[v] = (long double)a[v].x * c - (long double)a[v].y * sn;
            xi[v] = (long double)a[v].x * sn + (long double)a[v].y * c;
        }
        long double rr[8], ri[8], ref_mag = 0.0L;
        for (int q = 0; q < 8; q++) {
            rr[q] = ri[q] = 0.0L;
            for (int v = 0; v < 8; v++) {
                const long double ang = (INV ? 2 : -2) * kPi * (long double)((v * q) & 7) / 8.0L, c = cosl(ang), sn = sinl(ang);
                rr[q] += xr[v] * c - xi[v] * sn;
                ri[q] += xr[v] * sn + xi[v] * c;
            }
            ref_mag = fmaxl(ref_mag, fmaxl(fabsl(rr[q]), fabsl(ri[q])));
        }
        tan2_apply<INV>(a, k);
        dft8_scaled<INV>(a, k);
        for (int v = 1; v < 8; v++) b[v] = INV ? cmulc(b[v], tw2[v * 8 + s]) : cmul(b[v], tw2[v * 8 + s]);
        dft8<INV>(b);
        for (int q = 0; q < 8; q++) {
            const long double et = fmaxl(fabsl((long double)a[q].x - rr[q]), fabsl((long double)a[q].y - ri[q]));
            const long double ep = fmaxl(fabsl((long double)b[q].x - rr[q]), fabsl((long double)b[q].y - ri[q]));
            worst_tan = fmax(worst_tan, (double)(et / ref_mag));
            worst_plain = fmax(worst_plain, (double)(ep / ref_mag));
        }
    }
}

// the plain forward transform (key preparation)
static void forward_plain(Regs &x, const Tables &T, cplx *xch)
{
    for (int l = 0; l < 64; l++) { fwd_pass_a(l, x[l], T); x1_store_a(l, x[l], xch); }
    for (int l = 0; l < 64; l++) x1_load_b(l, x[l], xch);
    for (int l = 0; l < 64; l++) { fwd_pass_b(l, x[l], T); x2_store(l, x[l], xch); }
    for (int l = 0; l < 64; l++) x2_load(l, x[l], xch);
    for (int l = 0; l < 64; l++) fwd_pass_c(x[l]);
}

int main()
{
    std::vector<cplx> tab(kTableElems);
    fill_tables<long double>(tab.data(), [](long double a) { return cosl(a); }, [](long double a) { return sinl(a); });
    const Tables T = tables_from(tab.data());
    std::vector<double> tan2(2 * kTan2Elems);
    fill_tan2<long double>(tan2.data(), [](long double a) { return cosl(a); }, [](long double a) { return sinl(a); });

    std::mt19937_64 rng(20261018);
    for (int inv = 0; inv < 2; inv++)
        for (int s = 0; s < 8; s++) {
            double wt, wp;
            if (inv) stage<true>(s, tan2.data(), T.tw2, rng, wt, wp); else stage<false>(s, tan2.data(), T.tw2, rng, wt, wp);
            printf("stage dir %s group %d tan %.3e plain %.3e\n", inv ? "inv" : "fwd", s, wt, wp);
        }

    // ---- the chain ----
    static LaneTan2 tk[64];
    static cplx tw1f[64][8];
    for (int l = 0; l < 64; l++) {
        load_lane_tan2(l, tan2.data(), tk[l]);
        for (int q = 0; q < 8; q++) tw1f[l][q] = T.tw1f[q * 64 + l];
    }
    std::vector<cplx> xch(kXchElems);
    long wrong = 0;
    double worst = 0.0;
    for (int trial = 0; trial < 8; trial++) {
        std::vector<int32_t> d(kN), key(kN);
        for (int j = 0; j < kN; j++) {
            d[j] = (int32_t)(rng() % 1024) - 512;          // a 10-bit signed digit
            key[j] = (int32_t)(uint32_t)rng();
        }
        // key spectrum, scaled 1/M (bk_prepare_kernel)
        static Regs ks, x;
        for (int l = 0; l < 64; l++) load_poly(l, key.data(), T, ks[l]);
        forward_plain(ks, T, xch.data());
        // the digit polynomial through blind_rotate_kernel_v3's forward transform
        for (int l = 0; l < 64; l++) {
            int32_t temp[16];
            for (int m = 0; m < 16; m++) temp[m] = (int32_t)(((uint32_t)d[l + 64 * m] & 1023u) << 22);       // digit 1 of 10 bits
            load_digits2t(temp, 1, 10, x[l]);
            dft8_fwd_tw(x[l]);
            for (int q = 0; q < 8; q++) x[l][q] = cmul(x[l][q], tw1f[l][q]);
            x1_store_a(l, x[l], xch.data());
        }
        for (int l = 0; l < 64; l++) x1_load_b(l, x[l], xch.data());
        for (int l = 0; l < 64; l++) { dft8<false>(x[l]); x2_store(l, x[l], xch.data()); }
        for (int l = 0; l < 64; l++) x2_load(l, x[l], xch.data());
        for (int l = 0; l < 64; l++) {
            tan2_apply<false>(x[l], tk[l]);
            dft8_scaled<false>(x[l], tk[l]);
            for (int k2 = 0; k2 < 8; k2++) x[l][k2] = cmul(x[l][k2], mk(ks[l][k2].x / kM, ks[l][k2].y / kM));
        }
        // ... and its inverse
        for (int l = 0; l < 64; l++) { dft8<true>(x[l]); x2_store(l, x[l], xch.data()); }
        for (int l = 0; l < 64; l++) x2_load(l, x[l], xch.data());
        for (int l = 0; l < 64; l++) {
            tan2_apply<true>(x[l], tk[l]);
            dft8_scaled<true>(x[l], tk[l]);
            x1_store_b(l, x[l], xch.data());
        }
        for (int l = 0; l < 64; l++) x1_load_a(l, x[l], xch.data());
        std::vector<int32_t> got(kN);
        for (int l = 0; l < 64; l++) {
            for (int q = 0; q < 8; q++) x[l][q] = cmulc(x[l][q], tw1f[l][q]);
            dft8<true>(x[l]);
            int32_t acc[16] = {0};
            untwist_add2<true>(x[l], acc, &worst);
            for (int m = 0; m < 16; m++) got[l + 64 * m] = acc[m];
        }
        // integer negacyclic schoolbook mod 2^32
        for (int j = 0; j < kN; j++) {
            uint32_t sum = 0;
            for (int i = 0; i < kN; i++) {
                const uint32_t p = (uint32_t)d[i] * (uint32_t)key[(j - i) & (kN - 1)];
                sum += (i <= j) ? p : 0u - p;
            }
            wrong += (uint32_t)got[j] != sum;
        }
    }
    printf("chain wrong_words %ld of %d max_dist_from_integer %.4f\n", wrong, 8 * kN, worst);
    return 0;
}
