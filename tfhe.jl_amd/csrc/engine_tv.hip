// engine_tv.hip — programmable bootstrapping: the TV kernels.  This unit compiles every single-key blind-rotation kernel and the launcher
// of its family (br_launch.hpp) with TFHE_TV_KERNELS (kernels_common.hpp): blind_rotate_kernel_*_tv starts rotation w from
// X^{-barb} tv[tv_index[w]] instead of X^{-barb} (mu, ..., mu) (bootstrap.jl:50-59); everything after the accumulator's initial value is
// the kernel it was compiled from.  launch_blind_rotate_part (engine_dispatch.hip) decides kernel, geometry and LDS exactly as for a mu
// batch and calls the TV form of the family's launcher.  No DIAG instantiation exists: tfhe_bootstrap_tv_batch refuses measure_margin.
// The unit's compiler report is build/resource_usage_tv.txt (tests/test_tv_kernels.py applies the rules of tests/test_resource_usage.py
// to it).
#define TFHE_TV_KERNELS
#include "engine.hpp"
#include "br_launch.hpp"
