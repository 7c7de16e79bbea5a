// dispatch.h -- host side only: how a launcher turns run-time values into template arguments.
//
// A launcher writes its launch line ONCE, inside a generic lambda, and these helpers call the lambda with the value as a
// type: a typed index pointer, a std::integral_constant, a std::bool_constant.  The rule of the launch layer:
//   * a value with a documented fallback (an unknown store policy, a k-step count that is rounded up) is mapped to that
//     fallback in plain code BEFORE the dispatch, which then runs over the closed list of instantiations;
//   * a value outside the list launches nothing: dispatch_int returns false and the launcher returns dispatch_miss().
// Only what a lambda names is instantiated, so nesting the dispatches decides the set of kernels in the library.
#pragma once
#include <type_traits>

#include "tgn_common.h"

namespace tgn {

// element type of a typed index pointer (int / long long), for the kernel's template argument
template <typename P>
using idx_elem_t = std::remove_cv_t<std::remove_pointer_t<P>>;

// f(const int *) or f(const long long *); the non-const overload serves index buffers that a kernel writes
template <typename F>
inline auto dispatch_idx(const void *idx, int is64, F &&f) {
    return is64 ? f((const long long *)idx) : f((const int *)idx);
}
template <typename F>
inline auto dispatch_idx(void *idx, int is64, F &&f) {
    return is64 ? f((long long *)idx) : f((int *)idx);
}

template <typename F>
inline auto dispatch_bool(bool v, F &&f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}

// f(std::integral_constant<int, Vi>{}) for the Vi equal to v; false (and no call) if there is none
template <int... Vs, typename F>
inline bool dispatch_int(int v, F &&f) {
    return ((v == Vs ? ((void)f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// what a launcher returns when dispatch_int matched nothing
inline int dispatch_miss(const char *who, const char *what, int v) {
    set_error("%s: no kernel for %s = %d", who, what, v);
    return TGN_ERR_UNSUPPORTED;
}

// Lets `kernel` be launched with more dynamic LDS than the runtime's default allows: called before a launch that asks for
// `request` bytes, it raises the kernel's limit to `limit` (>= request; a site that launches one kernel with several sizes
// passes its largest) when the request is past the 48 KiB that need no attribute.  The attribute belongs to the (function,
// device) pair, so it is set on every such launch (a host-side table look-up; a once-per-process flag would leave a second
// GPU of the process without it).
template <typename K>
inline int raise_dynamic_lds(K kernel, const char *name, size_t request, size_t limit) {
    if (request <= 48 * 1024) return TGN_OK;
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) != hipSuccess) {
        (void)hipGetLastError();   // the failure is reported here, not by the next check_launch
        set_error("%s: cannot raise the dynamic LDS limit to %zu bytes", name, limit);
        return TGN_ERR_LAUNCH;
    }
    return TGN_OK;
}

}  // namespace tgn
