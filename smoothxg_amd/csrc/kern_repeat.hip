// kern_repeat.hip -- the kernels of the tandem-repeat scan (repeat_count_kernel, repeat_stats_kernel: poa_repeat.hip.h on the
// arithmetic of poa_repeat.h) and their launchers.  A translation unit of its own, built with -ffp-contract=off (build.py) as
// kern_sgd.hip is: decree R3 rounds every double operation once, so (r - mean) * (r - mean) must never fuse with the add after it.
#define SXG_REPEAT_IMPL
#include "poa_repeat.hip.h"
