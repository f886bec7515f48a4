// launch.h -- the host side of a fused-GEMM launch, ONE definition: how a PNPP_* switch is read, when a kernel is granted dynamic LDS, how
// many persistent workers a launch gets, how a failed launch is reported, how a runtime (A, E) mode pair picks a kernel instantiation,
// and how the in-kernel stamps are read out.  A new try_launch_* includes this header; it does not paste from another kernel file.
//
// Host code only: nothing here reaches a code object.  Everything is internal to the translation unit that includes it.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "kernels.h"

namespace pnpp {
namespace {

// ---- switches ----------------------------------------------------------------------------------------------------------------------
// The one parser of the PNPP_* integer switches (the table: tests/test_gpu_switch_forms.py).  Unset gives dflt; anything atoi() does not
// read as a number gives 0.  A site keeps the result in a `static const`: a switch is read once per process.  The senses in use:
//     a PNPP_NO_* switch (1 = off):       env_int(name, 0) == 0 is "on"
//     a switch that is on by default:     env_int(name, 1) != 0 is "on"
//     a switch that names a form:         env_int(name, 1) == 2 selects form 2
// (Written with the name as a literal at the call: tests/test_switch_coverage.py finds the switches by that spelling.)
static inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}

// ---- dynamic LDS -------------------------------------------------------------------------------------------------------------------
// A launch may ask for 48 KB of dynamic LDS unasked; beyond that the kernel has to be allowed once.  The state is per KERNEL (the kernel is
// the template argument: kernels of one signature share a pointer type, not this), and it is a high-water mark, so a launcher whose
// size depends on the shape asks again only when it grows.  (Process-wide, not per device: one process drives one GPU.)
template <auto KFN>
static inline void grant_lds(size_t bytes) {
    static size_t granted = 48 * 1024;
    if (bytes > granted) {
        (void)hipFuncSetAttribute((const void *)KFN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        granted = bytes;
    }
}

// ---- persistent workers ------------------------------------------------------------------------------------------------------------
// `target` workers (what fills the chip), but no more than the `units` of work (strips, tiles) can give `per` units each, and never more
// than kMaxStatBlocks: every worker writes one statistics slab (and one dW partial), and the workspaces are sized for that many.
static inline int worker_count(int target, int units, int per) {
    int w = target < kMaxStatBlocks ? target : kMaxStatBlocks;
    const int busy = (units + per - 1) / per;
    if (w > busy) w = busy;
    return w < 1 ? 1 : w;
}

// ---- launch check ------------------------------------------------------------------------------------------------------------------
// The tail of a try_launch_* (which returns "taken", not a status): the status goes to *rc.  Functions that return the status use
// PNPP_CHECK_LAUNCH (common.h).
static inline void check_launch(const char *what, int *rc) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        *rc = PNPP_ERR_LAUNCH;
    }
}

// ---- mode fan ----------------------------------------------------------------------------------------------------------------------
// A runtime mode -> a template argument: f is a generic lambda and is called with a std::integral_constant, so `m()` is a constant
// expression in its body.  dispatch_mode<V0, V1> tells two values apart (V1 stands for "not V0": the *_applies predicates admit no
// third) and instantiates f for V0 first -- the kernels appear in the code object in that order.  dispatch_ae is the usual pair, the
// operand loader (A_BNRELU | A_PLAIN) outside and the epilogue (E_STORE_STATS | E_STORE) inside; f is instantiated for all four, so
// fan by hand with dispatch_mode where fewer kernels exist.
template <int V>
using mode_c = std::integral_constant<int, V>;

template <int V0, int V1, typename F>
static inline void dispatch_mode(int mode, F &&f) {
    if (mode == V0) f(mode_c<V0>{});
    else f(mode_c<V1>{});
}
template <typename F>
static inline void dispatch_ae(int amode, int emode, F &&f) {
    dispatch_mode<A_BNRELU, A_PLAIN>(amode, [&](auto am) { dispatch_mode<E_STORE_STATS, E_STORE>(emode, [&](auto em) { f(am, em); }); });
}

// ---- in-kernel stamps (builds with PNPP_STAMPS=1 only) -----------------------------------------------------------------------------
#ifdef PNPP_STAMPS
constexpr unsigned stamps_bit() { return 64u; }   // bit 6 of pnpp_build_flags(): a library with stamps compiled in does not ship
#else
constexpr unsigned stamps_bit() { return 0u; }
#endif
#if defined(PNPP_STAMPS) || defined(MID3_STAMPS)
// reset != 0: zero the N counters of a __device__ array; reset == 0: wait for the device and copy them to out
template <size_t N>
static inline int stamps_io(const void *symbol, unsigned long long *out, int reset) {
    if (reset) {
        const unsigned long long z[N] = {0};
        (void)hipMemcpyToSymbol(symbol, z, sizeof(z));
    } else {
        (void)hipDeviceSynchronize();
        (void)hipMemcpyFromSymbol(out, symbol, N * sizeof(unsigned long long));
    }
    return 0;
}
#endif

}  // namespace
}  // namespace pnpp
