// kern_sgd.hip -- the kernels of the path-guided SGD node order (sgd_lds_kernel, sgd_term_kernel, sgd_apply_kernel:
// poa_sgd.hip.h) and their launchers.  A translation unit of its own because it is the one built with -ffp-contract=off
// (build.py): decree Y5 rounds every double operation once, so a multiply must never fuse with the add after it.
#define SXG_SGD_IMPL
#include "poa_sgd.hip.h"
