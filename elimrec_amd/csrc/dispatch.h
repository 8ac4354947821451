// Run-time value -> template argument, for the host side of a launch: f is a generic lambda called with a std::integral_constant,
// so each launch is an ordinary statement and the set of values IS the set of instantiations in the code object. Host code only.
#pragma once
#include <cstddef>
#include <type_traits>
#include "../../include/elimrec_hip.h"

#ifndef ELIMREC_RAISE_LDS_LIMIT   // the header's one HIP call (tools/dispatch_check.cpp defines a counting stand-in and needs no HIP)
#include <hip/hip_runtime.h>
#define ELIMREC_RAISE_LDS_LIMIT(kernel, bytes) \
    (void)hipFuncSetAttribute((const void *)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))
#endif

namespace elimrec {

void set_error(const char *fmt, ...);

template <int V> using int_c = std::integral_constant<int, V>;

template <class F> auto with_fast(bool fast, F f) {
    if (fast) return f(std::true_type{});
    return f(std::false_type{});
}

// v must be a power of two in [MIN, 64]: f(int_c<v>{}) and its result (0 or an error code) is returned; anything else: set_error +
// ELIMREC_E_BADARG, f not called. Values below MIN are not instantiated.
template <int MIN, class F> int with_pow2(const char *who, int v, F f) {
    static_assert(MIN >= 1 && MIN <= 64 && (MIN & (MIN - 1)) == 0, "MIN: a power of two in [1, 64]");
    if constexpr (MIN <= 1) { if (v == 1) return f(int_c<1>{}); }
    if constexpr (MIN <= 2) { if (v == 2) return f(int_c<2>{}); }
    if constexpr (MIN <= 4) { if (v == 4) return f(int_c<4>{}); }
    if constexpr (MIN <= 8) { if (v == 8) return f(int_c<8>{}); }
    if constexpr (MIN <= 16) { if (v == 16) return f(int_c<16>{}); }
    if constexpr (MIN <= 32) { if (v == 32) return f(int_c<32>{}); }
    if (v == 64) return f(int_c<64>{});
    set_error("%s: %d is not a power of two in [%d, 64]", who, v, MIN);
    return ELIMREC_E_BADARG;
}

// The 16-lane group kernels' width (cosine.h): f(int_c<NQ>{}) for NQ = ceil(d / 64) float4s per lane, 1 <= NQ <= 4 (4 <= d <= 256).
// Any other d: set_error + ELIMREC_E_BADARG, f not called -- the entry points check d first (table_dims), so that arm is not reached.
template <class F> int with_quads(const char *who, int d, F f) {
    switch (d >= 4 ? (d + 63) / 64 : 0) {
    case 1: return f(int_c<1>{});
    case 2: return f(int_c<2>{});
    case 3: return f(int_c<3>{});
    case 4: return f(int_c<4>{});
    }
    set_error("%s: d = %d is outside [4, 256]", who, d);
    return ELIMREC_E_BADARG;
}

template <auto KERNEL> void allow_lds(size_t bytes) {      // beyond 64 KiB of dynamic LDS: once per kernel instantiation
    static bool done = false;
    if (!done) { ELIMREC_RAISE_LDS_LIMIT(KERNEL, bytes); done = true; }
}

}  // namespace elimrec
