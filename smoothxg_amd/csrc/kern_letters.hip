// kern_letters.hip -- the kernel of the range gather (range_gather_kernel<CODED>: poa_letters.hip.h on the arithmetic of
// poa_letters.h) and its launcher.  A translation unit of its own; no special flags.
#define SXG_LETTERS_IMPL
#include "poa_letters.hip.h"
