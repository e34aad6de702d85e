// nonlin_walk.h — the one element walk of every nonlinearity kernel.
//
// A nonlinearity is a map type F with two members,
//   template <bool NTK> T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const
//   T var(T v) const
// pair: K' of one pixel with covariance c and variances *vx, *vy, and with NTK its
// κ̇ = dK'/dc at fixed variances (kdot is not written without NTK).  `self`: the two arguments
// are one pre-activation (the reference's override, kernels.py:155-162): K' is var(*vx) and
// vy is not read, so it may be any address.  var: the per-image variance map.
//
// Three kernels walk the elements and call the map:
//   pair_walk_kernel  the layer path: pair maps [nmaps][hw], whole maps per workgroup
//   cov_walk_kernel   position-pair maps [pair][p_row][q_row][p_col][q_col], one chunk per
//                     workgroup, which may straddle pairs
//   var_walk_kernel   the per-image variances, grid-stride
// A workgroup takes at most 2048 elements, 8 per thread, and all of a thread's loads of K and
// of Θ are issued before its math; the small variance maps are read through L2.  Every
// element is read and written by one thread, so the outputs may alias the inputs and Θ may
// alias K: no __restrict__ on the maps for that reason.  An addend is added after the map, a
// rounding of its own.  nonlin.hip holds the entry points; covpool.hip and covntk.hip use
// cov_nonlin() below for the post-stages of their conv kernels.
#pragma once

#include "cgp_common.h"
#include "gelu_math.h"

namespace cgp {

constexpr int kWalkBlock = 256;                        // 4 waves of 64
constexpr int kWalkChunk = 2048;                       // elements of one workgroup
constexpr int kWalkE = kWalkChunk / kWalkBlock;        // loads in flight per thread and stream (8)

// ----------------------------------------------------------------------------------
// the maps
// ----------------------------------------------------------------------------------

// the ReLU map R and its κ̇ of two distinct pre-activations (cgp_common.h's functions)
template <typename T, bool NTK>
__device__ __forceinline__ T relu_elem(T c, T v1, T v2, int exact, T& kdot) {
    const T r = exact ? relu_exact(c, v1, v2) : relu_fast(c, v1, v2);
    if constexpr (NTK) kdot = relu_kdot(c, v1, v2, exact);
    return r;
}

template <typename T>
struct ReluMap {
    int exact;   // CGP_FLAG_EXACT_RELU
    template <bool NTK>
    __device__ __forceinline__ T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const {
        const T v1 = *vx;
        if (self) {
            if constexpr (NTK) kdot = T(0.5);                // kdot at rho = 1
            return var(v1);                                  // xy' = xx' = xx/2
        }
        return relu_elem<T, NTK>(c, v1, *vy, exact, kdot);
    }
    __device__ __forceinline__ T var(T v) const { return v / T(2); }
};

// erf: one evaluation mode, kdot from the square root K' already paid for
template <typename T>
struct ErfMap {
    template <bool NTK>
    __device__ __forceinline__ T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const {
        const T v1 = *vx;
        if (self) return erf_var(v1, kdot);                  // xy' = xx'
        const T v2 = *vy;
        T d = T(1) + T(2) * (v1 + v2) + T(4) * (v1 * v2 - c * c);
        d = d < T(1) ? T(1) : d;                             // NaN kept
        const T s = sqrt_t(d);
        kdot = KErf<T>::four_over_pi / s;                    // dead code without NTK
        return KErf<T>::two_over_pi * atan_t((T(2) * c) / s);
    }
    __device__ __forceinline__ T var(T v) const { return erf_var(v); }
};

// GELU (gelu_math.h)
template <typename T>
struct GeluMap {
    template <bool NTK>
    __device__ __forceinline__ T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const {
        return gelu_pair(c, vx, vy, self, kdot);             // kdot: dead code without NTK
    }
    __device__ __forceinline__ T var(T v) const { return gelu_var(v); }
};

// The two-slope ReLU φ(x) = a·min(x, 0) + b·max(x, 0) is affine in the ReLU's
// two maps: with the host's s = (a − b)², m = a·b, h = (a² + b²)/2,
//   K' = fma(s, R, m·c)      κ̇ = fma(s, k, m)      v' = h·v
// and h·v, κ̇ = h where the ReLU overrides, so (a, b) = (0, 1) gives the ReLU's bits.
template <typename T>
struct ABReluMap {
    T s, m, h;
    int exact;
    template <bool NTK>
    __device__ __forceinline__ T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const {
        const T v1 = *vx;
        if (self) {
            if constexpr (NTK) kdot = h;
            return var(v1);
        }
        T k;
        const T r = relu_elem<T, NTK>(c, v1, *vy, exact, k);
        if constexpr (NTK) kdot = fma_t(s, k, m);
        const T t = m * c;
        return fma_t(s, r, t);
    }
    __device__ __forceinline__ T var(T v) const { return h * v; }
};

// The sinusoid φ(x) = a·sin(b·x + θ) is a function of the distance
// d = v1 + v2 − 2c and of s = v1 + v2 + 2c: with the host's A = a²/2, B = b²/2, C = cos 2θ,
// D = a²b²/2,
//   K' = A·(e_d − C·e_s)     κ̇ = D·(e_d + C·e_s)     e_d = exp(−B·d), e_s = exp(−B·s)
// and v' = A·(1 − C·exp(−4B·v)), κ̇ = D·(1 + C·exp(−4B·v)) where the ReLU overrides.  d and s
// are raised to 0 where rounding made them negative, so e_d <= 1.  At C == 0 (Rbf: K' =
// exp(−γ·d)) the second exponential is skipped, a launch-uniform branch; for finite inputs the
// bits are those of the full form.  double: the library's exp; float: expf.
__device__ __forceinline__ double exp_t(double x) { return exp(x); }
__device__ __forceinline__ float exp_t(float x) { return expf(x); }

template <typename T>
struct SinMap {
    T A, B, C, D;
    // C·exp(−B·s), s raised to 0 (NaN kept)
    __device__ __forceinline__ T ces(T s) const {
        if (C == T(0)) return T(0);
        s = s < T(0) ? T(0) : s;
        return C * exp_t(-B * s);
    }
    template <bool NTK>
    __device__ __forceinline__ T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const {
        const T v1 = *vx;
        if (self) {
            if constexpr (NTK) kdot = D * (T(1) + ces(T(4) * v1));
            return var(v1);                                  // xy' = xx'
        }
        const T sum = v1 + *vy, c2 = T(2) * c;
        T d = sum - c2;
        d = d < T(0) ? T(0) : d;                             // NaN kept
        const T ed = exp_t(-B * d);
        const T ce = ces(sum + c2);
        if constexpr (NTK) kdot = D * (ed + ce);
        return A * (ed - ce);
    }
    __device__ __forceinline__ T var(T v) const { return A * (T(1) - ces(T(4) * v)); }
};

// Any smooth φ by its Hermite (Mehler) series: with ρ = c/√(v1·v2) and the
// coefficients a_n(v) = E_z[φ(√v·z)·h_n(z)], h_n = He_n/√n!, of each image pixel,
//   K' = Σ_{n<=N} a_n(v1)·a_n(v2)·ρⁿ     κ̇ = Σ_{n<=N} a'_n(v1)·a'_n(v2)·ρⁿ     (a' of φ')
// and v' = Σ a_n(v)², κ̇ = Σ a'_n(v)² where the ReLU overrides: the series at ρ = 1, so the
// diagonal is the kernel's own.  The coefficients come from hermite_coef_kernel as tables
// [n][image·hw + pixel] over the variance buffer: a pixel's offset into a table is its
// variance's offset from the buffer's base, no division, and a wave's loads for one n are
// contiguous in the pixel.  ρ is 0 where v1·v2 is not positive (a zero-variance pixel has
// a_n = 0 for n >= 1: the series is a_0·a_0, exact) and is clamped to [−1, 1], NaN kept.  The
// series is summed by Horner from n = N down, one fma per term on the rounded product, so
// pair(x, y) and pair(y, x) are the same bits.  There is no var(): the variances need the
// coefficients (cgp_var_hermite_*).
template <typename T>
struct HermiteMap {
    const T *ax, *ay, *dax, *day;   // tables of a and a' of xx and of yy; a' read with NTK
    const T *xb, *yb;               // the variance buffers the walk's vx / vy point into
    long long sx, sy;               // elements between two n of the x and of the y tables
    int N;
    // Σ a_n², n = N down to 0
    __device__ __forceinline__ T sumsq(const T* a, long long s) const {
        T acc = T(0);
        for (int n = N; n >= 0; --n) {
            const T t = a[n * s];
            acc = fma_t(t, t, acc);
        }
        return acc;
    }
    __device__ __forceinline__ T series(const T* a, long long s, const T* b, long long sb,
                                        T rho) const {
        T acc = T(0);
        for (int n = N; n >= 0; --n) {
            const T t = a[n * s] * b[n * sb];
            acc = fma_t(acc, rho, t);
        }
        return acc;
    }
    template <bool NTK>
    __device__ __forceinline__ T pair(T c, const T* vx, const T* vy, bool self, T& kdot) const {
        const long long ox = vx - xb;
        if (self) {
            if constexpr (NTK) kdot = sumsq(dax + ox, sx);
            return sumsq(ax + ox, sx);                       // xy' = xx'
        }
        const long long oy = vy - yb;
        const T t = *vx * *vy;
        T rho = t > T(0) ? c / sqrt_t(t) : T(0);
        rho = rho > T(1) ? T(1) : rho;                       // NaN kept
        rho = rho < T(-1) ? T(-1) : rho;
        if constexpr (NTK) kdot = series(dax + ox, sx, day + oy, sy, rho);
        return series(ax + ox, sx, ay + oy, sy, rho);
    }
};

// φ and φ' of the series, chosen by a launch-uniform id (CGP_HERMITE_*: cnngp.h), in double.
// σ(x) is evaluated on the side where exp does not overflow; 1 − σ(x) is σ(−x).
__device__ __forceinline__ double hermite_sigmoid(double x) {
    const double e = exp(-fabs_t(x));
    const double s = 1.0 / (1.0 + e);
    return x >= 0 ? s : e * s;
}
__device__ __forceinline__ double hermite_phi(int id, bool deriv, double x) {
    constexpr double kS2pi = 0.79788456080286535588;         // √(2/π)
    constexpr double kRs2 = 0.70710678118654752440;          // 1/√2
    constexpr double kRs2pi = 0.39894228040143267794;        // 1/√(2π)
    switch (id) {
        case 0: {                                            // tanh
            const double t = tanh(x);
            return deriv ? 1.0 - t * t : t;
        }
        case 1: {                                            // sigmoid
            const double s = hermite_sigmoid(x);
            return deriv ? s * hermite_sigmoid(-x) : s;
        }
        case 2:                                              // softplus log(1 + eˣ)
            return deriv ? hermite_sigmoid(x)
                         : log1p(exp(-fabs_t(x))) + (x > 0 ? x : 0.0);
        case 3: {                                            // SiLU x·σ(x)
            const double s = hermite_sigmoid(x);
            return deriv ? s * (1.0 + x * hermite_sigmoid(-x)) : x * s;
        }
        case 4: {                                            // GELU's tanh approximation
            const double x2 = x * x;
            const double t = tanh(kS2pi * x * (1.0 + 0.044715 * x2));
            return deriv ? 0.5 * (1.0 + t) +
                               0.5 * x * (1.0 - t * t) * kS2pi * (1.0 + 3.0 * 0.044715 * x2)
                         : 0.5 * x * (1.0 + t);
        }
        case 5:                                              // erf
            return deriv ? 2.0 * kS2pi * kRs2 * exp(-x * x) : erf(x);
        default: {                                           // GELU x·Φ(x)
            const double cdf = 0.5 * (1.0 + erf(x * kRs2));
            return deriv ? cdf + x * kRs2pi * exp(-0.5 * x * x) : x * cdf;
        }
    }
}

// The coefficients of `count` variances (image pixels): a Q-node Gauss–Hermite rule per pixel
// with the N + 1 accumulators in registers (NMAX: the order's bucket, so the array is indexed
// at compile time), in double whatever T is.  nodes: [2][nq], z_q then w_q, Σ w_q = 1.  h_n by
// h_{n+1} = (z·h_n − √n·h_{n−1})/√(n+1).  blockIdx.y = 1 is the table of φ'.  With var_out
// (grid y = 1) no table is written: var_out = Σ a_n² of the coefficients rounded to T, the
// bits HermiteMap's override returns.
template <typename T>
struct HermiteCoefP {
    const T* var;
    T* a;
    T* da;
    T* var_out;
    const double* nodes;
    long long count;
    int phi, order, nq;
};

template <typename T, int NMAX>
__global__ __launch_bounds__(kWalkBlock) void hermite_coef_kernel(const HermiteCoefP<T> p) {
    const long long e = (long long)blockIdx.x * kWalkBlock + threadIdx.x;
    if (e >= p.count) return;
    const bool deriv = blockIdx.y != 0;
    double v = (double)p.var[e];
    v = v < 0.0 ? 0.0 : v;                                   // NaN kept
    const double s = __builtin_sqrt(v);
    double acc[NMAX + 1];
#pragma unroll
    for (int n = 0; n <= NMAX; ++n) acc[n] = 0.0;
    for (int q = 0; q < p.nq; ++q) {
        const double z = p.nodes[q];
        const double f = p.nodes[p.nq + q] * hermite_phi(p.phi, deriv, s * z);
        double h0 = 1.0, h1 = z;
        acc[0] += f;
        acc[1] = fma_t(f, h1, acc[1]);
#pragma unroll
        for (int n = 1; n < NMAX; ++n) {
            // √n and 1/√(n+1) fold to constants in the unrolled loop: no division per node
            const double h2 = (z * h1 - __builtin_sqrt((double)n) * h0) *
                              (1.0 / __builtin_sqrt((double)(n + 1)));
            acc[n + 1] = fma_t(f, h2, acc[n + 1]);
            h0 = h1;
            h1 = h2;
        }
    }
    if (p.var_out) {
        T sum = T(0);
#pragma unroll
        for (int n = NMAX; n >= 0; --n) {
            if (n <= p.order) {
                const T t = (T)acc[n];
                sum = fma_t(t, t, sum);
            }
        }
        p.var_out[e] = sum;
        return;
    }
    T* tab = deriv ? p.da : p.a;
#pragma unroll
    for (int n = 0; n <= NMAX; ++n)
        if (n <= p.order) tab[n * p.count + e] = (T)acc[n];
}

// The post-stage of the conv kernels on position-pair maps (covpool.hip, covntk.hip): the map
// of run-time `kind` at (c, v1, v2) = (S[p, q], xx_i[p], yy_j[q]).  The override applies where
// same, i == j and p == q.  The forward conv has no GELU post-stage (cgp_cov_conv_* rejects
// it), so without NTK every kind but the ReLU is erf.
template <typename T, bool NTK>
__device__ __forceinline__ T cov_nonlin(T c, int kind, const T* xx, const T* yy, int i, int j,
                                        int hw, int p, int q, int same, int exact, T& kdot) {
    const T* vx = xx + (size_t)i * hw + p;
    const T* vy = yy + (size_t)j * hw + q;
    const bool self = same && i == j && p == q;
    if (kind == CGP_COV_RELU)
        return ReluMap<T>{exact}.template pair<NTK>(c, vx, vy, self, kdot);
    if (!NTK || kind == CGP_COV_ERF) return ErfMap<T>{}.template pair<NTK>(c, vx, vy, self, kdot);
    return GeluMap<T>{}.template pair<NTK>(c, vx, vy, self, kdot);
}

// ----------------------------------------------------------------------------------
// the layer path: pair map m = i·n2 + j (or i = j = m with diag) of hw pixels; a workgroup
// takes mpb whole maps, at most kWalkChunk elements.  theta / out_theta are read with NTK,
// addend with ADD.
// ----------------------------------------------------------------------------------
template <typename T, class F>
struct PairWalkP {
    const T* xy;
    const T* theta;
    T* out_xy;
    T* out_theta;
    const T* addend;
    const T* xx;
    const T* yy;       // may be NULL when same && diag: every element is `self`
    long long nmaps;
    FastDiv n2, dhw;
    int hw, same, diag, mpb;
    F f;
};

template <typename T, class F, bool NTK, bool ADD>
__global__ __launch_bounds__(kWalkBlock) void pair_walk_kernel(const PairWalkP<T, F> p) {
    const long long m0 = (long long)blockIdx.x * p.mpb;
    const long long rem = p.nmaps - m0;
    const int mb = rem < p.mpb ? (int)rem : p.mpb;
    const int n = mb * p.hw;
    const T* src = p.xy + m0 * p.hw;
    const T* tsrc = NTK ? p.theta + m0 * p.hw : nullptr;
    T* dst = p.out_xy + m0 * p.hw;
    T* tdst = NTK ? p.out_theta + m0 * p.hw : nullptr;
    const T* add = ADD ? p.addend + m0 * p.hw : nullptr;
    T v[kWalkE], th[NTK ? kWalkE : 1];
#pragma unroll
    for (int k = 0; k < kWalkE; ++k) {
        const int e = threadIdx.x + k * kWalkBlock;
        v[k] = e < n ? src[e] : T(0);
        if constexpr (NTK) th[k] = e < n ? tsrc[e] : T(0);
    }
#pragma unroll
    for (int k = 0; k < kWalkE; ++k) {
        const int e = threadIdx.x + k * kWalkBlock;
        if (e < n) {
            const unsigned ml = fdiv((unsigned)e, p.dhw);
            const int px = e - (int)ml * p.hw;
            unsigned i, j;
            pair_of((unsigned)(m0 + ml), p.n2, p.diag, i, j);
            const bool self = p.same && (p.diag || i == j);
            T kd;
            T r = p.f.template pair<NTK>(v[k], p.xx + (size_t)i * p.hw + px,
                                         p.yy + (size_t)j * p.hw + px, self, kd);
            if constexpr (ADD) r = r + add[e];
            dst[e] = r;
            if constexpr (NTK) tdst[e] = th[k] * kd;
        }
    }
}

// ----------------------------------------------------------------------------------
// position-pair maps: element -> pixels p = p_row·w + p_col, q = q_row·w + q_col (CovIdx,
// cov_decode: cgp_common.h); one kWalkChunk-element chunk per workgroup.  ADD: the forward
// kernel has its addend; the two-stream kernel an addend on either stream, each pointer
// tested on its own.
// ----------------------------------------------------------------------------------
template <typename T, class F>
struct CovWalkP {
    const T* in;
    const T* theta;
    T* out;
    T* out_theta;
    const T* addend;
    const T* addend_theta;
    const T* xx;
    const T* yy;
    const int* pi;
    const int* pj;
    long long total;
    CovIdx g;
    int hw, same;
    F f;
};

template <typename T, class F, bool NTK, bool ADD>
__global__ __launch_bounds__(kWalkBlock) void cov_walk_kernel(const CovWalkP<T, F> p) {
    const long long base = (long long)blockIdx.x * kWalkChunk;
    const long long rem = p.total - base;
    const int n = rem < kWalkChunk ? (int)rem : kWalkChunk;
    const long long m0 = base / p.g.dn.d;
    const unsigned r0 = (unsigned)(base - m0 * p.g.dn.d);
    const T* src = p.in + base;
    const T* tsrc = NTK ? p.theta + base : nullptr;
    T* dst = p.out + base;
    T* tdst = NTK ? p.out_theta + base : nullptr;
    T v[kWalkE], th[NTK ? kWalkE : 1];
#pragma unroll
    for (int k = 0; k < kWalkE; ++k) {
        const int e = threadIdx.x + k * kWalkBlock;
        v[k] = e < n ? src[e] : T(0);
        if constexpr (NTK) th[k] = e < n ? tsrc[e] : T(0);
    }
#pragma unroll
    for (int k = 0; k < kWalkE; ++k) {
        const int e = threadIdx.x + k * kWalkBlock;
        if (e < n) {
            const unsigned rt = r0 + (unsigned)e;
            const unsigned mm = fdiv(rt, p.g.dn);
            const long long m = m0 + mm;
            int px, qx;
            cov_decode(p.g, rt - mm * p.g.dn.d, px, qx);
            const int i = p.pi[m], j = p.pj[m];
            // the override applies where both arguments are one pre-activation
            const bool self = p.same && i == j && px == qx;
            T kd;
            T r = p.f.template pair<NTK>(v[k], p.xx + (size_t)i * p.hw + px,
                                         p.yy + (size_t)j * p.hw + qx, self, kd);
            if constexpr (ADD) {
                if (!NTK || p.addend) r = r + p.addend[base + e];
            }
            dst[e] = r;
            if constexpr (NTK) {
                T t = th[k] * kd;
                if constexpr (ADD) {
                    if (p.addend_theta) t = t + p.addend_theta[base + e];
                }
                tdst[e] = t;
            }
        }
    }
}

// ----------------------------------------------------------------------------------
// the per-image variances (kernels.py:154-164): xo = var(xx), yo = var(same ? xx : yy)
// ----------------------------------------------------------------------------------
template <typename T, class F>
struct VarWalkP {
    const T* xx;
    const T* yy;
    T* xo;
    T* yo;
    long long n_xx, n_yy;
    int same;
    F f;
};

template <typename T, class F>
__global__ __launch_bounds__(kWalkBlock) void var_walk_kernel(const VarWalkP<T, F> p) {
    const T* __restrict__ xx = p.xx;
    const T* __restrict__ yy = p.yy;
    const long long stride = (long long)gridDim.x * kWalkBlock;
    for (long long e = (long long)blockIdx.x * kWalkBlock + threadIdx.x; e < p.n_xx + p.n_yy;
         e += stride) {
        if (e < p.n_xx) {
            p.xo[e] = p.f.var(xx[e]);
        } else {
            const long long f = e - p.n_xx;
            p.yo[f] = p.f.var(p.same ? xx[f] : yy[f]);
        }
    }
}

}  // namespace cgp
