// dispatch.hpp -- run-time value -> template argument, for the kernel launchers.  Host only, no HIP.
#pragma once

#include <cstdint>
#include <type_traits>
#include <utility>

namespace msvs
{

/// f(std::integral_constant<int, Vi>{}) for the first Vi == v; any other v (negative ones too) takes the LAST value, as the
/// `default:` of a switch did.  f runs exactly once and is instantiated for the listed values only: the list IS the set of
/// kernel instantiations, so a launcher without T = 1 says with_int<2, 4, 8>.
template <int V0, int... Rest, typename F>
inline void with_int(int v, F && f)
{
    if constexpr (sizeof...(Rest) == 0)
        f(std::integral_constant<int, V0>{});
    else if (v == V0)
        f(std::integral_constant<int, V0>{});
    else
        with_int<Rest...>(v, std::forward<F>(f));
}

template <typename F>
inline void with_bool(bool b, F && f)
{
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}

/// top-k registers per lane of the scan / merge kernels: with_int<1, 2, 4>(r_for_k(k), ...)
inline int r_for_k(uint32_t k) { return k <= 64 ? 1 : (k <= 128 ? 2 : 4); }

}
