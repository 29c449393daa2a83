// kern_part.hip -- instantiates one part of the engine's kernel classes (the rows of kClasses, poa_classes.h, whose part is
// SXG_KERN_PART; see poa_kern_tables.hip.h).  smoothxg_amd/build.py compiles it once per part, side by side, and links the
// objects into libsxgpoa.so.
#ifndef SXG_KERN_PART
#error "compile with -DSXG_KERN_PART=<1..9>"
#endif
#include "poa_kern_tables.hip.h"
