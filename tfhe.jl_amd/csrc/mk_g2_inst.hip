// One instantiation of mk_blind_rotate_kernel_g2 and its launcher: -DG2_P=<parties> -DG2_L=<l> -DG2_DG=<0|1> -DG2_RW=<2|4> -DG2_AL=<0|1> (Makefile).
// With -DG2_TV=1 the unit compiles the instantiation's TV form instead (mk_blind_rotate_kernel_g2_tv, multi-key programmable
// bootstrapping; no DIAG form) and its launcher TFHE_G2_TV_LAUNCHER: the objects mk_g2_tv_*.o, reported in resource_usage_mk_tv.txt.
#if G2_TV
#define TFHE_TV_KERNELS
#endif
#include "mk_g2_launch.hpp"

#define G2_PASTE_(P, L, DG, RW, AL) TFHE_G2_LAUNCHER(P, L, DG, RW, AL)
#define G2_PASTE(P, L, DG, RW, AL) G2_PASTE_(P, L, DG, RW, AL)
#define G2_TV_PASTE_(P, L, RW, AL) TFHE_G2_TV_LAUNCHER(P, L, RW, AL)
#define G2_TV_PASTE(P, L, RW, AL) G2_TV_PASTE_(P, L, RW, AL)

#if G2_TV
static_assert(G2_DG == 0, "the TV kernels have no DIAG form");
hipError_t G2_TV_PASTE(G2_P, G2_L, G2_RW, G2_AL)(unsigned nblk, size_t lds_bytes, hipStream_t s, const WithTv<MkGenArgs> &ga)
{
    constexpr bool AL = G2_AL != 0;
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)mk_blind_rotate_kernel_g2_tv<G2_P, G2_L, false, G2_RW, AL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mk_blind_rotate_kernel_g2_tv<G2_P, G2_L, false, G2_RW, AL>), dim3(nblk), dim3(128 * G2_RW), lds_bytes, s, ga);
    return hipGetLastError();
}
#else
hipError_t G2_PASTE(G2_P, G2_L, G2_DG, G2_RW, G2_AL)(unsigned nblk, size_t lds_bytes, hipStream_t s, const MkGenArgs &ga)
{
    constexpr bool DG = G2_DG != 0, AL = G2_AL != 0;
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)mk_blind_rotate_kernel_g2<G2_P, G2_L, DG, G2_RW, AL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mk_blind_rotate_kernel_g2<G2_P, G2_L, DG, G2_RW, AL>), dim3(nblk), dim3(128 * G2_RW), lds_bytes, s, ga);
    return hipGetLastError();
}
#endif
