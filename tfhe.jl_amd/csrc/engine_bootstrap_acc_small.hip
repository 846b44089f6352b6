// engine_bootstrap_acc_small.hip — the ACC forms of the two multi-wave gate kernels, for the small batches of tfhe_bootstrap_acc_batch and
// tfhe_bootstrap_acc_level under option acc_dispatch (engine_bootstrap_acc.hip has the entry points, the dispatcher and the one-wave
// form).  This unit compiles blind_rotate_kernel_w2 and blind_rotate_kernel_h2 with TFHE_ACC_KERNELS (kernels_common.hpp): between
// init_acc before the first barrier and store_acc after the last they are the kernels they were compiled from — two waves per row,
// wave c owning polynomial c, and 4 l waves per row with every transform split over two.  Exactly the forms br_launch_w2 and
// br_launch_h2 name without DIAG are instantiated: blind_rotate_kernel_w2_acc<2 | 3 | 0, no DIAG, 1 | 2> and
// blind_rotate_kernel_h2_acc<2 | 3, no DIAG>, eight kernels.  The unit's compiler report is
// build/resource_usage_bootstrap_acc_small.txt (tests/test_bootstrap_acc_small_resources.py); the v3 form keeps its own unit and
// report.  Nothing else is here: the dispatcher takes the kernels as launch handles.
#define TFHE_ACC_KERNELS
#include "engine.hpp"

const void *acc_kernel_w2(int L, int rw)
{
    if (rw != 1 && rw != 2) return nullptr;
    switch (L) {
    case 2: return rw == 2 ? (const void *)blind_rotate_kernel_w2_acc<2, false, 2> : (const void *)blind_rotate_kernel_w2_acc<2, false, 1>;
    case 3: return rw == 2 ? (const void *)blind_rotate_kernel_w2_acc<3, false, 2> : (const void *)blind_rotate_kernel_w2_acc<3, false, 1>;
    case 0: return rw == 2 ? (const void *)blind_rotate_kernel_w2_acc<0, false, 2> : (const void *)blind_rotate_kernel_w2_acc<0, false, 1>;
    }
    return nullptr;
}

const void *acc_kernel_h2(int L)
{
    switch (L) {
    case 2: return (const void *)blind_rotate_kernel_h2_acc<2, false>;
    case 3: return (const void *)blind_rotate_kernel_h2_acc<3, false>;
    }
    return nullptr;
}
