// engine_tv.hip — programmable bootstrapping: the TV kernels and their launches.  This unit compiles every single-key blind-rotation
// kernel with TFHE_TV_KERNELS (kernels_common.hpp): blind_rotate_kernel_*_tv starts rotation w from X^{-barb} tv[tv_index[w]] instead
// of X^{-barb} (mu, ..., mu) (bootstrap.jl:50-59); everything after the accumulator's initial value is the kernel it was compiled from.
// launch_blind_rotate_part (engine_dispatch.hip) decides kernel, geometry and LDS exactly as for a mu batch and calls the launcher of
// the family here.  No DIAG instantiation exists: tfhe_bootstrap_tv_batch refuses measure_margin.  The unit's compiler report is
// build/resource_usage_tv.txt (tests/test_tv_kernels.py applies the rules of tests/test_resource_usage.py to it).
#define TFHE_TV_KERNELS
#include "engine.hpp"

template <class A>
static WithTv<A> with_tv(const A &a, const TvPtrs &tv)
{
    WithTv<A> t;
    static_cast<A &>(t) = a;
    t.tv = tv.tv;
    t.tv_index = tv.index;
    return t;
}

// L = 2 / 3: the tuned instantiations, 0: the run-time-l one (launch_blind_rotate_part has picked which)
#define TV_L_CASES(LAUNCH)                                                                                         \
    switch (L) {                                                                                                   \
    case 2: LAUNCH(2); break;                                                                                      \
    case 3: LAUNCH(3); break;                                                                                      \
    case 0: LAUNCH(0); break;                                                                                      \
    default: return c->set_err(TFHE_ERR_STATE, "bootstrap_tv: no TV kernel for l = %d", L);                       \
    }
#define TV_L23_CASES(LAUNCH)                                                                                       \
    switch (L) {                                                                                                   \
    case 2: LAUNCH(2); break;                                                                                      \
    case 3: LAUNCH(3); break;                                                                                      \
    default: return c->set_err(TFHE_ERR_STATE, "bootstrap_tv: no TV kernel for l = %d", L);                       \
    }

int32_t tv_launch_anyn(tfhe_ctx *c, const anyn::Args &g, const TvPtrs &tv, size_t R, unsigned nt, size_t lds, hipStream_t s)
{
    if (lds > 64 * 1024) LDS_TRY(c, lds, anyn::blind_rotate_kernel_tv<false>);
    hipLaunchKernelGGL((anyn::blind_rotate_kernel_tv<false>), dim3((unsigned)R), dim3(nt), lds, s, with_tv(g, tv));
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_n512w2(tfhe_ctx *c, const N512Args &b, const TvPtrs &tv, int L, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<N512Args> t = with_tv(b, tv);
#define LAUNCH(LL) hipLaunchKernelGGL((blind_rotate_kernel_n512w2_tv<LL, false>), dim3((unsigned)R), dim3(128), lds, s, t)
    TV_L_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_n512(tfhe_ctx *c, const N512Args &b, const TvPtrs &tv, int L, bool group, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<N512Args> t = with_tv(b, tv);
#define LAUNCH(LL)                                                                                                 \
    if (group) hipLaunchKernelGGL((blind_rotate_kernel_n512_tv<LL, false, 4>), dim3((unsigned)((R + 3) / 4)), dim3(256), lds, s, t); \
    else hipLaunchKernelGGL((blind_rotate_kernel_n512_tv<LL, false, 1>), dim3((unsigned)R), dim3(64), lds, s, t)
    TV_L_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_general(tfhe_ctx *c, const BrGenArgs &g, const TvPtrs &tv, bool n2048, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<BrGenArgs> t = with_tv(g, tv);
    if (n2048) {
        if (lds > 64 * 1024) LDS_TRY(c, lds, blind_rotate_kernel_general_tv<32, false>);
        hipLaunchKernelGGL((blind_rotate_kernel_general_tv<32, false>), dim3((unsigned)R), dim3(64), lds, s, t);
    } else {
        if (lds > 64 * 1024) LDS_TRY(c, lds, blind_rotate_kernel_general_tv<16, false>);
        hipLaunchKernelGGL((blind_rotate_kernel_general_tv<16, false>), dim3((unsigned)R), dim3(64), lds, s, t);
    }
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_n2048(tfhe_ctx *c, const Br2048Args &b, const TvPtrs &tv, int rw, unsigned nblk, size_t lds, hipStream_t s)
{
    const WithTv<Br2048Args> t = with_tv(b, tv);
    if (rw == 2) {
        if (lds > 64 * 1024) LDS_TRY(c, lds, blind_rotate_kernel_n2048x_tv<3, false, 2>);
        hipLaunchKernelGGL((blind_rotate_kernel_n2048x_tv<3, false, 2>), dim3(nblk), dim3(256), lds, s, t);
    } else {
        if (lds > 64 * 1024) LDS_TRY(c, lds, blind_rotate_kernel_n2048x_tv<3, false, 1>);
        hipLaunchKernelGGL((blind_rotate_kernel_n2048x_tv<3, false, 1>), dim3(nblk), dim3(128), lds, s, t);
    }
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_k2w3(tfhe_ctx *c, const BrArgs &a, const TvPtrs &tv, int L, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<BrArgs> t = with_tv(a, tv);
#define LAUNCH(LL)                                                                                                 \
    do {                                                                                                           \
        LDS_TRY(c, lds, blind_rotate_kernel_k2w3_tv<LL, false>);                                                   \
        hipLaunchKernelGGL((blind_rotate_kernel_k2w3_tv<LL, false>), dim3((unsigned)R), dim3(192), lds, s, t);      \
    } while (0)
    TV_L23_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

// grouped: `blocks` workgroups of seven rotation slots (a.grp_q / grp_big set), else one rotation per workgroup
int32_t tv_launch_k2(tfhe_ctx *c, const BrArgs &a, const TvPtrs &tv, int L, bool grouped, size_t blocks, size_t lds, hipStream_t s)
{
    const WithTv<BrArgs> t = with_tv(a, tv);
#define LAUNCH(LL)                                                                                                 \
    if (grouped) {                                                                                                 \
        LDS_TRY(c, (7 * lds), blind_rotate_kernel_k2_tv<LL, false, 7>);                                            \
        hipLaunchKernelGGL((blind_rotate_kernel_k2_tv<LL, false, 7>), dim3((unsigned)blocks), dim3(448), 7 * lds, s, t); \
    } else hipLaunchKernelGGL((blind_rotate_kernel_k2_tv<LL, false, 1>), dim3((unsigned)blocks), dim3(64), lds, s, t)
    TV_L23_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_h2(tfhe_ctx *c, const BrArgs &a, const H2Tables &ht, const TvPtrs &tv, int L, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<BrArgs> t = with_tv(a, tv);
#define LAUNCH(LL)                                                                                                 \
    do {                                                                                                           \
        LDS_TRY(c, lds, blind_rotate_kernel_h2_tv<LL, false>);                                                     \
        hipLaunchKernelGGL((blind_rotate_kernel_h2_tv<LL, false>), dim3((unsigned)R), dim3(256 * LL), lds, s, t, ht); \
    } while (0)
    TV_L23_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_w2(tfhe_ctx *c, const BrArgs &a, const TvPtrs &tv, int L, bool pairs, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<BrArgs> t = with_tv(a, tv);
#define LAUNCH(LL)                                                                                                 \
    if (pairs) hipLaunchKernelGGL((blind_rotate_kernel_w2_tv<LL, false, 2>), dim3((unsigned)((R + 1) / 2)), dim3(256), 2 * lds, s, t); \
    else hipLaunchKernelGGL((blind_rotate_kernel_w2_tv<LL, false, 1>), dim3((unsigned)R), dim3(128), lds, s, t)
    TV_L_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t tv_launch_v3(tfhe_ctx *c, const BrArgs &a, const TvPtrs &tv, int L, bool group, size_t R, size_t lds, hipStream_t s)
{
    const WithTv<BrArgs> t = with_tv(a, tv);
#define LAUNCH(LL)                                                                                                 \
    if (group) {                                                                                                   \
        LDS_TRY(c, (4 * lds), blind_rotate_kernel_v3_tv<LL, 8, true, false, 4>);                                   \
        hipLaunchKernelGGL((blind_rotate_kernel_v3_tv<LL, 8, true, false, 4>), dim3((unsigned)((R + 3) / 4)), dim3(256), 4 * lds, s, t); \
    } else hipLaunchKernelGGL((blind_rotate_kernel_v3_tv<LL, 8, true, false>), dim3((unsigned)R), dim3(64), lds, s, t)
    TV_L_CASES(LAUNCH)
#undef LAUNCH
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}
