// gelu_math.h — the device functions of the GELU layer kernel (include/cnngp.h "The GELU
// nonlinearity"), GeluMap's arithmetic (nonlin_walk.h): one function per stream,
// shared by the layer-path, the variance and the position-pair walks, so the overridden K' of
// a pair and the variance entry point's output are the same bits.
//
// phi(x) = x·Phi(x), the exact GELU.  For (u1, u2) ~ N(0, [[v1, c], [c, v2]]), with
// P = v1 v2, P1 = (1 + v1)(1 + v2), D2 = P1 - c², D = sqrt(D2), t = c/D, a = atan(t)
// (Tsuchida, Pearce et al. 2021):
//   K'   = E[phi(u1) phi(u2)]   = ((c² + P·D2)/(P1·D) + c·a)/2π + c/4
//   kdot = E[phi'(u1) phi'(u2)] = (1/D2 + (1 - P)/P1 + 1)·t/2π + 1/4 + a/2π = dK'/dc
// D2 >= 1 + v1 + v2 >= 1 for a valid covariance: no singularity at rho = ±1, so one
// evaluation mode and no polynomial tables.  Correctly rounded division and square root, the
// device library's atan, every op rounded in T (the unit is compiled with -ffp-contract=off).
// The /2π of the formulas is a product with the constant 1/2π and c/4 one with 1/4 (exact):
// the forward map costs two divisions of its own (t and the quotient), κ̇ two more.
#pragma once

#include "cgp_common.h"

namespace cgp {

template <typename T> struct KGelu {
    static constexpr T inv_two_pi = T(0.15915494309189533577);   // 1/2π: a product, no division
};

// the map of one pixel; kdot is dead code where the caller drops it
template <typename T>
__device__ __forceinline__ T gelu_map(T c, T v1, T v2, T& kdot) {
    const T p = v1 * v2;
    const T p1 = (T(1) + v1) * (T(1) + v2);
    T d2 = p1 - c * c;
    d2 = d2 < T(1) ? T(1) : d2;                              // NaN kept
    const T d = sqrt_t(d2);
    const T t = c / d;
    const T a = atan_t(t);
    kdot = ((T(1) / d2 + (T(1) - p) / p1 + T(1)) * t) * KGelu<T>::inv_two_pi + T(0.25) +
           a * KGelu<T>::inv_two_pi;
    return ((c * c + p * d2) / (p1 * d) + c * a) * KGelu<T>::inv_two_pi + c / T(4);
}

// per-image variance: the pair map at c = v1 = v2 = v, where D2 = 1 + 2v; kdot is the NTK
// factor of a pair the reference overrides with its own variance (the partial derivative
// at fixed variances, not dv'/dv)
template <typename T>
__device__ __forceinline__ T gelu_var(T v, T& kdot) {
    const T s = sqrt_t(T(1) + T(2) * v);
    const T t = v / s;
    const T a = atan_t(t);
    kdot = ((T(1) / (T(1) + T(2) * v) + (T(1) - v) / (T(1) + v) + T(1)) * t) *
               KGelu<T>::inv_two_pi + T(0.25) + a * KGelu<T>::inv_two_pi;
    return ((T(2) * (v * v)) / ((T(1) + v) * s) + v * a) * KGelu<T>::inv_two_pi + v / T(4);
}
template <typename T>
__device__ __forceinline__ T gelu_var(T v) {
    T kdot;
    return gelu_var(v, kdot);
}

// the pixel whose variances are *vx and *vy; `self`: both arguments are one pre-activation
// (the reference's override, kernels.py:155-162), K' = v' and vy is not read
template <typename T>
__device__ __forceinline__ T gelu_pair(T c, const T* __restrict__ vx, const T* __restrict__ vy,
                                       bool self, T& kdot) {
    const T v1 = *vx;
    if (self) return gelu_var(v1, kdot);
    return gelu_map(c, v1, *vy, kdot);
}

}  // namespace cgp
