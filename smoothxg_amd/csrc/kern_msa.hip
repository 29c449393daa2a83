// kern_msa.hip -- the kernels of the trimmed MSA (msa_cols_kernel, msa_rows_kernel: poa_msa.hip.h) and their launchers, a
// translation unit of its own beside the kernel classes of kern_part.hip.
#define SXG_MSA_IMPL
#include "poa_msa.hip.h"
