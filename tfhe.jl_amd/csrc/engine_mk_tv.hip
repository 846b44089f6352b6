// engine_mk_tv.hip — multi-key programmable bootstrapping: the multi-key TV kernels.  This unit compiles the multi-key blind-rotation
// families (mk_w2, mk_general, the any-N kernel) with TFHE_TV_KERNELS (kernels_common.hpp): mk_blind_rotate_kernel_*_tv starts the
// body polynomial of rotation w from X^{-barb} tv[tv_index[w]] instead of X^{-barb} (mu, ..., mu); the masks start at zero and
// everything after the accumulator's initial value is the kernel it was compiled from.  launch_mk_blind_rotate (engine_multikey.hip)
// decides kernel, geometry and LDS exactly as for a mu batch and calls the launchers below (the many-party two-wave kernel's TV forms
// are mk_g2_inst.hip with -DG2_TV=1).  No DIAG instantiation exists: the multi-key TV entry points refuse measure_margin.  The unit's
// compiler report is build/resource_usage_mk_tv.txt, together with the mk_g2_tv_* objects.
#define TFHE_TV_KERNELS
#include "engine.hpp"

template <class K, class A>
static int32_t mk_tv_run(tfhe_ctx *c, K *kernel, unsigned nblk, unsigned nt, size_t lds, hipStream_t s, const A &a)
{
    if (lds > 64 * 1024) {
        const int32_t rl = ensure_dyn_lds(c, (const void *)kernel, lds, "multi-key TV kernel");
        if (rl) return rl;
    }
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(nt), lds, s, a);
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

int32_t mk_tv_launch_anyn(tfhe_ctx *c, const WithTv<anyn::Args> &a, unsigned nblk, unsigned nt, size_t lds, hipStream_t s)
{
    return mk_tv_run(c, anyn::mk_blind_rotate_kernel_tv<false>, nblk, nt, lds, s, a);
}

// (the two-party kernel has l = 4 only: launch_mk_blind_rotate's `special`)
int32_t mk_tv_launch_w2(tfhe_ctx *c, const WithTv<MkBrArgs> &a, int rw, unsigned nblk, size_t lds, hipStream_t s)
{
    if (rw == 2) return mk_tv_run(c, mk_blind_rotate_kernel_w2_tv<4, false, 2>, nblk, 128 * 2, lds, s, a);
    return mk_tv_run(c, mk_blind_rotate_kernel_w2_tv<4, false, 1>, nblk, 128, lds, s, a);
}

int32_t mk_tv_launch_general(tfhe_ctx *c, const WithTv<MkGenArgs> &a, int rw, bool accg, unsigned nblk, size_t lds, hipStream_t s)
{
    if (rw == 2)
        return accg ? mk_tv_run(c, mk_blind_rotate_kernel_general_tv<false, 2, true>, nblk, 64 * 2, lds, s, a)
                    : mk_tv_run(c, mk_blind_rotate_kernel_general_tv<false, 2, false>, nblk, 64 * 2, lds, s, a);
    return accg ? mk_tv_run(c, mk_blind_rotate_kernel_general_tv<false, 1, true>, nblk, 64, lds, s, a)
                : mk_tv_run(c, mk_blind_rotate_kernel_general_tv<false, 1, false>, nblk, 64, lds, s, a);
}
