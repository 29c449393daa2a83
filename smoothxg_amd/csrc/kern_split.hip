// kern_split.hip -- the kernels of the identity split (pair_identity_kernel, split_kernel: poa_split.hip.h; mash_sketch_kernel,
// mash_pair_kernel, split_mash_kernel: poa_mash.hip.h), of the identity estimate of the adaptive scores (identity_pairs_kernel,
// identity_select_kernel: poa_identity.hip.h, on the sets and the intersection of poa_mash.hip.h) and their launchers, a
// translation unit of its own beside the kernel classes of kern_part.hip.
#define SXG_SPLIT_IMPL
#include "poa_split.hip.h"
#include "poa_mash.hip.h"
#include "poa_identity.hip.h"
