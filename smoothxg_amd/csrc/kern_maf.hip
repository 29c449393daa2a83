// kern_maf.hip -- the kernels of the MAF text (maf_text_kernel, msa_row_letters_kernel: poa_maf_text.hip.h on the arithmetic of
// poa_maf_text.h) and their launchers.  A translation unit of its own; no special flags.
#define SXG_MAF_IMPL
#include "poa_maf_text.hip.h"
