// poa_kern_tables.hip.h -- from a launch geometry to its kernel.
//
// The engine has ~560 kernel instantiations (strip width x workgroup size x gap model x alignment mode x plane cell
// format, block and align-only kernels): compiled in ONE translation unit they cost minutes of hipcc.  The list of classes,
// kClasses in poa_classes.h, therefore assigns every class to a PART; kern_part.hip, compiled once per part with
// -DSXG_KERN_PART=<k> by smoothxg_amd/build.py (in parallel), instantiates the rows of its part and defines that part's
// entry points, sxg_part_kernel<BlockArgs / AlignArgs, k>; sxg_poa.hip only sees their declaration.  What a class is compiled
// for (thread count, plane read-back, launch bounds) is class_traits in poa_classes.h.
// Development builds of a single packed class (-DSXG_DEV_ONLY_W=<w> -DSXG_DEV_ONLY_TMAX=<t>, -DSXG_DEV_CB4: its 4-byte cells
// too; seconds) compile sxg_poa.hip alone: the same list, filtered, with every part in that one translation unit.
#pragma once
#include <type_traits>
#include <utility>

#include "poa_kernels.hip.h"

template <class Args> using KernelFn = void (*)(const Args);
template <class Args> constexpr ClassKind kind_of = std::is_same_v<Args, AlignArgs> ? CLASS_ALIGN : CLASS_BLOCK;

// the kernel of part PART for geometry v (nullptr: not a class of this part)
template <class Args, int PART> KernelFn<Args> sxg_part_kernel(const Variant& v, bool cvx, bool sw);

#if defined(SXG_KERN_PART) || defined(SXG_DEV_ONLY_W)
// is the class <row R, width W, row mode RM> instantiated in this translation unit's part PART?
template <class Args, int PART, int R, int W, int RM> constexpr bool class_here() {
    constexpr ClassRow c = kClasses[R];
#ifdef SXG_DEV_ONLY_W
#ifdef SXG_DEV_CB4
    constexpr bool dev = c.kind == CLASS_BLOCK && RM == 2 && c.tmax == SXG_DEV_ONLY_TMAX && W == SXG_DEV_ONLY_W;
#else
    constexpr bool dev = c.kind == CLASS_BLOCK && RM == 2 && c.cb == 2 && c.tmax == SXG_DEV_ONLY_TMAX && W == SXG_DEV_ONLY_W;
#endif
#else
    constexpr bool dev = true;
#endif
    return dev && c.part == PART && c.kind == kind_of<Args> && (c.widths & cw(W)) != 0 && (c.rms & cw(RM)) != 0;
}
template <class Args, int R, int W, int RM, bool CVX, bool SW, bool DS> static KernelFn<Args> class_kernel() {
    constexpr ClassRow c = kClasses[R];
    if constexpr (std::is_same_v<Args, AlignArgs>) return poa_align_kernel<c.tmax, W, CVX, RM, SW>;
    else return poa_block_kernel<c.tmax, W, CVX, RM, SW, c.cb, DS, (c.widths2 & cw(W)) != 0 ? W - 1 : 0>;   // (the second width: class_w2)
}
// the kernel of a class for (cvx, sw, ds): only the modes its row lists are instantiated
template <class Args, int R, int W, int RM> static KernelFn<Args> pick_mode(bool cvx, bool sw, bool ds) {
    constexpr unsigned m = kClasses[R].modes;
    if constexpr ((m & CLS_DS) != 0) {
        if (cvx && ds) {
            if constexpr ((m & CLS_LOCAL) != 0) if (sw) return class_kernel<Args, R, W, RM, true, true, true>();
            if constexpr ((m & CLS_GLOBAL) != 0) if (!sw) return class_kernel<Args, R, W, RM, true, false, true>();
        }
    }
    if (cvx) {
        if constexpr ((m & CLS_LOCAL) != 0) if (sw) return class_kernel<Args, R, W, RM, true, true, false>();
        if constexpr ((m & CLS_GLOBAL) != 0) if (!sw) return class_kernel<Args, R, W, RM, true, false, false>();
    } else {
        if constexpr ((m & CLS_LOCAL) != 0) if (sw) return class_kernel<Args, R, W, RM, false, true, false>();
        if constexpr ((m & CLS_GLOBAL) != 0) if (!sw) return class_kernel<Args, R, W, RM, false, false, false>();
    }
    return nullptr;
}
// One selector: rows x widths x row modes, folded at compile time.  (Each level is folded from its LAST element to its first: the
// compiler emits the kernels of a translation unit in the reverse order of these references, and the order of kernels inside a code
// object is kept as it was when the classes were spelled out one by one -- inlining and register allocation of the shared
// out-of-line functions depend on it.)
template <int N, int... I> using rev_seq = std::integer_sequence<int, (N - 1 - I)...>;
template <int N, int... I> constexpr rev_seq<N, I...> rev_of(std::integer_sequence<int, I...>) { return {}; }
template <int N> constexpr auto rev_range() { return rev_of<N>(std::make_integer_sequence<int, N>()); }
template <class Args, int PART, int R, int W, int... RM> static void pick_rm(KernelFn<Args>& k, int row, const Variant& v, bool cvx, bool sw, std::integer_sequence<int, RM...>) {
    ((void)([&] { if constexpr (class_here<Args, PART, R, W, RM>()) if (row == R && v.W == W && v.RM == RM) k = pick_mode<Args, R, W, RM>(cvx, sw, v.DS); }()), ...);
}
template <class Args, int PART, int R, int... Wo> static void pick_width(KernelFn<Args>& k, int row, const Variant& v, bool cvx, bool sw, std::integer_sequence<int, Wo...>) {
    (pick_rm<Args, PART, R, CLASS_W_MIN + Wo>(k, row, v, cvx, sw, rev_range<CLASS_RM_MAX + 1>()), ...);
}
template <class Args, int PART, int... R> static KernelFn<Args> pick_class(const Variant& v, bool cvx, bool sw, std::integer_sequence<int, R...>) {
    KernelFn<Args> k = nullptr;
    const int row = class_row(kind_of<Args>, v, sw);
    (pick_width<Args, PART, R>(k, row, v, cvx, sw, rev_range<CLASS_W_MAX - CLASS_W_MIN + 1>()), ...);
    return k;
}
template <class Args, int PART> KernelFn<Args> sxg_part_kernel(const Variant& v, bool cvx, bool sw) {
    return pick_class<Args, PART>(v, cvx, sw, rev_range<kNumClasses>());
}
#endif
#ifdef SXG_KERN_PART
template KernelFn<BlockArgs> sxg_part_kernel<BlockArgs, SXG_KERN_PART>(const Variant&, bool, bool);
template KernelFn<AlignArgs> sxg_part_kernel<AlignArgs, SXG_KERN_PART>(const Variant&, bool, bool);
#endif

#ifndef SXG_KERN_PART
// host side: the kernel class of a geometry, exactly the class v names (nullptr: none built)
// (kept out of the parts' translation units: there it would instantiate every part's entry point, and with it every class)
template <class Args, int... P> static KernelFn<Args> kernel_of(const Variant& v, bool cvx, bool sw, std::integer_sequence<int, P...>) {
    const int row = class_row(kind_of<Args>, v, sw);
    KernelFn<Args> k = nullptr;
    if (row >= 0) ((void)(kClasses[row].part == P + 1 ? (k = sxg_part_kernel<Args, P + 1>(v, cvx, sw), 0) : 0), ...);
    return k;
}
static inline KernelFn<BlockArgs> block_kernel(const Variant& v, bool cvx, bool sw) { return kernel_of<BlockArgs>(v, cvx, sw, std::make_integer_sequence<int, CLASS_PARTS>()); }
static inline KernelFn<AlignArgs> align_kernel(const Variant& v, bool cvx, bool sw) { return kernel_of<AlignArgs>(v, cvx, sw, std::make_integer_sequence<int, CLASS_PARTS>()); }
#endif
