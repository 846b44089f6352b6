// br_launch.hpp — the launch of each single-key blind-rotation family, written once and compiled twice, as the kernels themselves are
// (kernels_common.hpp: TV_KERNEL, TV_ARGS, kTV): engine_dispatch.hip compiles br_launch_<family>(c, <family's arguments>, ...) for the
// mu / DIAG kernels, engine_tv.hip (TFHE_TV_KERNELS) br_launch_<family>(c, WithTv<family's arguments>, ...) for the TV kernels.
// launch_blind_rotate_part decides family, instantiation and geometry (BrLaunch) and calls either form; a launcher maps (L, rotations
// per workgroup, DIAG) to the kernel and launches it.  It names only the instantiations the dispatcher selects: no DIAG form of the TV
// kernels, nor of the grouped geometries (n512 rw4, w2 rw2, k2 rw7, n2048x rw2: the dispatcher groups only without DIAG).
#pragma once
#include "engine.hpp"

#include <type_traits>

// (with_tv, engine.hpp: a TV batch's arguments)
// One launch.  Dynamic LDS beyond the default 64 KB is granted first (ensure_dyn_lds: once per device and kernel).
template <class K, class... A>
static int32_t br_run(tfhe_ctx *c, K *kernel, const BrLaunch &g, hipStream_t s, const A &...args)
{
    if (g.lds > 64 * 1024) {
        const int32_t rl = ensure_dyn_lds(c, (const void *)kernel, g.lds, "blind-rotation kernel");
        if (rl) return rl;
    }
    hipLaunchKernelGGL(kernel, g.grid, g.block, g.lds, s, args...);
    HIP_TRY(c, hipGetLastError());
    return TFHE_OK;
}

// f(DG) with DG = g.dg as a compile-time constant (std::bool_constant); always false in the TV unit, whose kernels have no DIAG form
// (tfhe_bootstrap_tv_batch refuses measure_margin)
template <class F>
static int32_t br_dg(const BrLaunch &g, F &&f)
{
    if constexpr (!kTV)
        if (g.dg) return f(std::true_type());
    return f(std::false_type());
}

// f(L, DG) with L = g.L as a compile-time constant (std::integral_constant) among the family's instantiations: 2 and 3, and 0 (run-time
// l) where RT_L
template <bool RT_L, class F>
static int32_t br_inst(tfhe_ctx *c, const BrLaunch &g, F &&f)
{
    auto at = [&](auto L) { return br_dg(g, [&](auto DG) { return f(L, DG); }); };
    switch (g.L) {
    case 2: return at(std::integral_constant<int, 2>());
    case 3: return at(std::integral_constant<int, 3>());
    case 0:
        if constexpr (RT_L) return at(std::integral_constant<int, 0>());
        break;
    }
    return c->set_err(TFHE_ERR_STATE, "blind rotate: no tuned kernel for bs_l = %d", c->P.bs_l);
}

int32_t br_launch_anyn(tfhe_ctx *c, const TV_ARGS(anyn::Args) &a, const BrLaunch &g, hipStream_t s)
{
    return br_dg(g, [&](auto DG) { return br_run(c, anyn::TV_KERNEL(blind_rotate_kernel)<DG>, g, s, a); });
}

int32_t br_launch_n512w2(tfhe_ctx *c, const TV_ARGS(N512Args) &a, const BrLaunch &g, hipStream_t s)
{
    return br_inst<true>(c, g, [&](auto L, auto DG) { return br_run(c, TV_KERNEL(blind_rotate_kernel_n512w2)<L, DG>, g, s, a); });
}

int32_t br_launch_n512(tfhe_ctx *c, const TV_ARGS(N512Args) &a, const BrLaunch &g, hipStream_t s)
{
    return br_inst<true>(c, g, [&](auto L, auto DG) {
        if constexpr (!DG)
            if (g.rw == 4) return br_run(c, TV_KERNEL(blind_rotate_kernel_n512)<L, false, 4>, g, s, a);
        return br_run(c, TV_KERNEL(blind_rotate_kernel_n512)<L, DG, 1>, g, s, a);
    });
}

int32_t br_launch_general(tfhe_ctx *c, const TV_ARGS(BrGenArgs) &a, bool n2048, const BrLaunch &g, hipStream_t s)
{
    return br_dg(g, [&](auto DG) {
        if (n2048) return br_run(c, TV_KERNEL(blind_rotate_kernel_general)<32, DG>, g, s, a);
        return br_run(c, TV_KERNEL(blind_rotate_kernel_general)<16, DG>, g, s, a);
    });
}

int32_t br_launch_n2048x(tfhe_ctx *c, const TV_ARGS(Br2048Args) &a, const BrLaunch &g, hipStream_t s)
{
    return br_dg(g, [&](auto DG) {
        if constexpr (!DG)
            if (g.rw == 2) return br_run(c, TV_KERNEL(blind_rotate_kernel_n2048x)<3, false, 2>, g, s, a);
        return br_run(c, TV_KERNEL(blind_rotate_kernel_n2048x)<3, DG, 1>, g, s, a);
    });
}

int32_t br_launch_k2w3(tfhe_ctx *c, const TV_ARGS(BrArgs) &a, const BrLaunch &g, hipStream_t s)
{
    return br_inst<false>(c, g, [&](auto L, auto DG) { return br_run(c, TV_KERNEL(blind_rotate_kernel_k2w3)<L, DG>, g, s, a); });
}

int32_t br_launch_k2(tfhe_ctx *c, const TV_ARGS(BrArgs) &a, const BrLaunch &g, hipStream_t s)
{
    return br_inst<false>(c, g, [&](auto L, auto DG) {
        if constexpr (!DG)
            if (g.rw == 7) return br_run(c, TV_KERNEL(blind_rotate_kernel_k2)<L, false, 7>, g, s, a);
        return br_run(c, TV_KERNEL(blind_rotate_kernel_k2)<L, DG, 1>, g, s, a);
    });
}

int32_t br_launch_h2(tfhe_ctx *c, const TV_ARGS(BrArgs) &a, const H2Tables &ht, const BrLaunch &g, hipStream_t s)
{
    return br_inst<false>(c, g, [&](auto L, auto DG) { return br_run(c, TV_KERNEL(blind_rotate_kernel_h2)<L, DG>, g, s, a, ht); });
}

int32_t br_launch_w2(tfhe_ctx *c, const TV_ARGS(BrArgs) &a, const BrLaunch &g, hipStream_t s)
{
    return br_inst<true>(c, g, [&](auto L, auto DG) {
        if constexpr (!DG)
            if (g.rw == 2) return br_run(c, TV_KERNEL(blind_rotate_kernel_w2)<L, false, 2>, g, s, a);
        return br_run(c, TV_KERNEL(blind_rotate_kernel_w2)<L, DG, 1>, g, s, a);
    });
}

int32_t br_launch_v3(tfhe_ctx *c, const TV_ARGS(BrArgs) &a, const BrLaunch &g, hipStream_t s)
{
    return br_inst<true>(c, g, [&](auto L, auto DG) {
        if (g.rw == 4) return br_run(c, TV_KERNEL(blind_rotate_kernel_v3)<L, 8, true, DG, 4>, g, s, a);
        return br_run(c, TV_KERNEL(blind_rotate_kernel_v3)<L, 8, true, DG, 1>, g, s, a);
    });
}
