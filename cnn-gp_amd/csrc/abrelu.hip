// abrelu.hip — the two-slope ReLU φ(x) = a·min(x, 0) + b·max(x, 0) (LeakyReLU, |x|, a damped
// identity) on pair maps, per-image variances and position-pair maps (include/cnngp.h "The
// two-slope ReLU").
//
// Its layer kernel is affine in two maps the ReLU kernels already evaluate: with R the ReLU
// map (relu_fast / relu_exact) and k = relu_kdot, and the host's s = (a − b)², m = a·b,
// h = (a² + b²)/2,
//   K' = fma(s, R, m·c)      κ̇ = fma(s, k, m)      v' = h·v
// and h·v, Θ·h where the ReLU entry points override.  R and k are cgp_common.h's functions,
// called with the ReLU kernels' arguments, so (a, b) = (0, 1) gives the ReLU entry points' bits.
//
// Three entry-point families:
//   cgp_abrelu_*      the layer path: K' (+ addend) and, with theta, Θ' = Θ·κ̇ in the same pass
//   cgp_var_abrelu_*  the per-image variances
//   cgp_abrelu_cov_*  position-pair maps S[p, q] (covpool.hip's layout), with and without Θ
// The kernels have the shapes of their erf twins (erf_pair_kernel, var_erf_kernel,
// cov_nonlin_kernel / cov_nonlin_ntk_kernel): whole 2048-element chunks per workgroup, all of
// a thread's loads issued before its math, the small variance maps read through L2.  Every
// element is read and written by one thread, so outputs may alias inputs; no __restrict__ on
// the maps for that reason.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cnngp.h"
#include "cgp_common.h"

using namespace cgp;

namespace {

constexpr int kBlock = 256;                   // 4 waves of 64
constexpr int kChunk = 2048;                  // elements of one workgroup
constexpr int kE = kChunk / kBlock;           // loads in flight per thread and stream (8)
constexpr long long kMaxPairElems = 1LL << 30;   // (h·w)² of one pair: 32-bit index math

// s = (a − b)², m = a·b, h = (a² + b²)/2 in the map's type
template <typename T>
struct Slopes {
    T s, m, h;
};

// One element of both streams.  self: the two arguments are one pre-activation (the ReLU
// entry points' override).  kdot is written only with NTK.
template <typename T, bool NTK>
__device__ __forceinline__ T abrelu_elem(T c, const T* vx, const T* vy, bool self, int exact,
                                         const Slopes<T>& k, T& kdot) {
    const T v1 = *vx;
    if (self) {
        if constexpr (NTK) kdot = k.h;
        return k.h * v1;                                     // the variance kernel's bits
    }
    const T v2 = *vy;
    const T r = exact ? relu_exact(c, v1, v2) : relu_fast(c, v1, v2);
    if constexpr (NTK) kdot = fma_t(k.s, relu_kdot(c, v1, v2, exact), k.m);
    const T t = k.m * c;
    return fma_t(k.s, r, t);
}

// ----------------------------------------------------------------------------------
// the layer path: pair map m = i·n2 + j (or i = j = m with diag) of hw pixels; a workgroup
// takes mpb whole maps, at most kChunk elements
// ----------------------------------------------------------------------------------
template <typename T>
struct ABReluP {
    const T* xy;
    const T* theta;
    T* out_xy;
    T* out_theta;
    const T* addend;
    const T* xx;
    const T* yy;
    long long nmaps;
    FastDiv n2, dhw;
    int hw, same, diag, exact, mpb;
    Slopes<T> k;
};

template <typename T, bool NTK, bool ADD>
__global__ __launch_bounds__(kBlock) void abrelu_pair_kernel(const ABReluP<T> p) {
    const long long m0 = (long long)blockIdx.x * p.mpb;
    const long long rem = p.nmaps - m0;
    const int mb = rem < p.mpb ? (int)rem : p.mpb;
    const int n = mb * p.hw;
    const T* src = p.xy + m0 * p.hw;
    const T* tsrc = NTK ? p.theta + m0 * p.hw : nullptr;
    T* dst = p.out_xy + m0 * p.hw;
    T* tdst = NTK ? p.out_theta + m0 * p.hw : nullptr;
    const T* add = ADD ? p.addend + m0 * p.hw : nullptr;
    T v[kE], th[NTK ? kE : 1];
#pragma unroll
    for (int k = 0; k < kE; ++k) {
        const int e = threadIdx.x + k * kBlock;
        v[k] = e < n ? src[e] : T(0);
        if constexpr (NTK) th[k] = e < n ? tsrc[e] : T(0);
    }
#pragma unroll
    for (int k = 0; k < kE; ++k) {
        const int e = threadIdx.x + k * kBlock;
        if (e < n) {
            const unsigned ml = fdiv((unsigned)e, p.dhw);
            const int px = e - (int)ml * p.hw;
            unsigned i, j;
            pair_of((unsigned)(m0 + ml), p.n2, p.diag, i, j);
            const bool self = p.same && (p.diag || i == j);
            const T* vx = p.xx + (size_t)i * p.hw + px;
            T kd;
            T r = abrelu_elem<T, NTK>(v[k], vx, self ? vx : p.yy + (size_t)j * p.hw + px, self,
                                      p.exact, p.k, kd);
            if constexpr (ADD) r = r + add[e];
            dst[e] = r;
            if constexpr (NTK) tdst[e] = th[k] * kd;
        }
    }
}

// the per-image variances: v' = h·v
template <typename T>
__global__ __launch_bounds__(kBlock) void var_abrelu_kernel(const T* __restrict__ xx,
                                                            const T* __restrict__ yy,
                                                            long long n_xx, long long n_yy,
                                                            int same, T h, T* xo, T* yo) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < n_xx + n_yy;
         e += stride) {
        if (e < n_xx) {
            xo[e] = h * xx[e];
        } else {
            const long long f = e - n_xx;
            yo[f] = h * (same ? xx[f] : yy[f]);
        }
    }
}

// ----------------------------------------------------------------------------------
// position-pair maps [pair][p_row][q_row][p_col][q_col]: element -> pixels
// p = p_row·w + p_col, q = q_row·w + q_col; one kChunk-element chunk per workgroup, which
// may straddle pairs (CovIdx, cov_decode: cgp_common.h).  ADD: an addend on either stream,
// each tested at run time as in cov_nonlin_ntk_kernel.
// ----------------------------------------------------------------------------------
template <typename T>
struct ABReluCovP {
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
    int hw, same, exact;
    Slopes<T> k;
};

template <typename T, bool NTK, bool ADD>
__global__ __launch_bounds__(kBlock) void abrelu_cov_kernel(const ABReluCovP<T> p) {
    const long long base = (long long)blockIdx.x * kChunk;
    const long long rem = p.total - base;
    const int n = rem < kChunk ? (int)rem : kChunk;
    const long long m0 = base / p.g.dn.d;
    const unsigned r0 = (unsigned)(base - m0 * p.g.dn.d);
    const T* src = p.in + base;
    const T* tsrc = NTK ? p.theta + base : nullptr;
    T* dst = p.out + base;
    T* tdst = NTK ? p.out_theta + base : nullptr;
    T v[kE], th[NTK ? kE : 1];
#pragma unroll
    for (int k = 0; k < kE; ++k) {
        const int e = threadIdx.x + k * kBlock;
        v[k] = e < n ? src[e] : T(0);
        if constexpr (NTK) th[k] = e < n ? tsrc[e] : T(0);
    }
#pragma unroll
    for (int k = 0; k < kE; ++k) {
        const int e = threadIdx.x + k * kBlock;
        if (e < n) {
            const unsigned rt = r0 + (unsigned)e;
            const unsigned mm = fdiv(rt, p.g.dn);
            const long long m = m0 + mm;
            int px, qx;
            cov_decode(p.g, rt - mm * p.g.dn.d, px, qx);
            const int i = p.pi[m], j = p.pj[m];
            // the override applies where both arguments are one pre-activation
            const bool self = p.same && i == j && px == qx;
            const T* vx = p.xx + (size_t)i * p.hw + px;
            T kd;
            T r = abrelu_elem<T, NTK>(v[k], vx, self ? vx : p.yy + (size_t)j * p.hw + qx, self,
                                      p.exact, p.k, kd);
            if constexpr (ADD) {
                if (p.addend) r = r + p.addend[base + e];
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
// host side: every check returns CGP_EINVAL before any HIP call
// ----------------------------------------------------------------------------------
inline unsigned grid_for(long long n) {
    long long g = (n + kBlock - 1) / kBlock;
    if (g > 256 * 8 * 4) g = 256 * 8 * 4;   // ≈4 rounds of 8 blocks per CU, grid-stride rest
    return (unsigned)(g < 1 ? 1 : g);
}

inline bool finite3(double s, double m, double h) {
    return std::isfinite(s) && std::isfinite(m) && std::isfinite(h);
}

template <typename T>
Slopes<T> slopes(double s, double m, double h) {
    Slopes<T> k;
    k.s = (T)s, k.m = (T)m, k.h = (T)h;
    return k;
}

template <typename T, bool NTK>
int launch_abrelu(const ABReluP<T>& p, long long blocks, hipStream_t s) {
    if (p.addend)
        hipLaunchKernelGGL((abrelu_pair_kernel<T, NTK, true>), dim3((unsigned)blocks),
                           dim3(kBlock), 0, s, p);
    else
        hipLaunchKernelGGL((abrelu_pair_kernel<T, NTK, false>), dim3((unsigned)blocks),
                           dim3(kBlock), 0, s, p);
    return check_launch("abrelu_pair_kernel");
}

template <typename T>
int abrelu_impl(const cgp_abrelu_args* a, void* stream) {
    // cgp_erf_*'s checks; theta == NULL is the forward-only form
    if (!a || !a->xy || !a->out_xy || !a->xx || (a->theta && !a->out_theta))
        return fail(CGP_EINVAL, "abrelu: NULL argument");
    if (a->hw <= 0 || a->nmaps <= 0 || a->nmaps >= (1LL << 31))
        return fail(CGP_EINVAL, "abrelu: bad sizes");
    if (a->n1 <= 0 || a->n2 <= 0 || (a->diag ? a->n1 : a->n1 * a->n2) != a->nmaps)
        return fail(CGP_EINVAL, "abrelu: nmaps inconsistent with n1/n2/diag");
    if ((a->same || a->diag) && a->n1 != a->n2)
        return fail(CGP_EINVAL, "abrelu: same / diag need n1 == n2");
    if (!(a->same && a->diag) && !a->yy) return fail(CGP_EINVAL, "abrelu: yy is NULL");
    if (a->hw > kChunk) return fail(CGP_EINVAL, "abrelu: map of %d pixels too large", a->hw);
    if (!finite3(a->s, a->m, a->h)) return fail(CGP_EINVAL, "abrelu: s, m or h is not finite");
    ABReluP<T> p;
    p.xy = static_cast<const T*>(a->xy);
    p.theta = static_cast<const T*>(a->theta);
    p.out_xy = static_cast<T*>(a->out_xy);
    p.out_theta = static_cast<T*>(a->out_theta);
    p.addend = static_cast<const T*>(a->addend);
    p.xx = static_cast<const T*>(a->xx);
    p.yy = static_cast<const T*>(a->yy);
    p.nmaps = a->nmaps;
    p.n2 = make_fastdiv((unsigned)a->n2);
    p.dhw = make_fastdiv((unsigned)a->hw);
    p.hw = a->hw;
    p.same = a->same;
    p.diag = a->diag;
    p.exact = (a->flags & CGP_FLAG_EXACT_RELU) != 0;
    p.k = slopes<T>(a->s, a->m, a->h);
    // whole maps per workgroup, at most kE elements per thread
    p.mpb = std::max(1, kChunk / a->hw);
    const long long blocks = (a->nmaps + p.mpb - 1) / p.mpb;
    hipStream_t s = as_stream(stream);
    return a->theta ? launch_abrelu<T, true>(p, blocks, s)
                    : launch_abrelu<T, false>(p, blocks, s);
}

template <typename T>
int var_abrelu_impl(const T* xx, const T* yy, int64_t n1, int64_t n2, int32_t hw, int32_t same,
                    double h, T* xo, T* yo, void* stream) {
    if (!xx || !yy || !xo || !yo) return fail(CGP_EINVAL, "var_abrelu: NULL argument");
    if (n1 <= 0 || n2 <= 0 || hw <= 0) return fail(CGP_EINVAL, "var_abrelu: bad sizes");
    if (same && n1 != n2) return fail(CGP_EINVAL, "var_abrelu: same needs n1 == n2");
    if (!std::isfinite(h)) return fail(CGP_EINVAL, "var_abrelu: h is not finite");
    const long long nx = n1 * hw, ny = n2 * hw;
    hipLaunchKernelGGL((var_abrelu_kernel<T>), dim3(grid_for(nx + ny)), dim3(kBlock), 0,
                       as_stream(stream), xx, yy, nx, ny, same, (T)h, xo, yo);
    return check_launch("var_abrelu_kernel");
}

template <typename T, bool NTK>
int launch_abrelu_cov(const ABReluCovP<T>& p, long long blocks, hipStream_t s) {
    if (p.addend || (NTK && p.addend_theta))
        hipLaunchKernelGGL((abrelu_cov_kernel<T, NTK, true>), dim3((unsigned)blocks),
                           dim3(kBlock), 0, s, p);
    else
        hipLaunchKernelGGL((abrelu_cov_kernel<T, NTK, false>), dim3((unsigned)blocks),
                           dim3(kBlock), 0, s, p);
    return check_launch("abrelu_cov_kernel");
}

template <typename T>
int abrelu_cov_impl(const cgp_abrelu_cov_args* a, void* stream) {
    // cgp_cov_nonlin_*'s checks, and cgp_covntk_nonlin_*'s for the second stream
    if (!a || !a->in || !a->out || !a->xx || !a->yy || !a->pair_i || !a->pair_j ||
        (a->theta && !a->out_theta))
        return fail(CGP_EINVAL, "abrelu_cov: NULL argument");
    if (a->theta && a->out == a->out_theta)
        return fail(CGP_EINVAL, "abrelu_cov: out and out_theta are one buffer");
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || a->h <= 0 || a->w <= 0 ||
        (long long)a->h * a->w * a->h * a->w > kMaxPairElems)
        return fail(CGP_EINVAL, "abrelu_cov: bad sizes");
    if (!finite3(a->s, a->m, a->hh))
        return fail(CGP_EINVAL, "abrelu_cov: s, m or hh is not finite");
    ABReluCovP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.theta = static_cast<const T*>(a->theta);
    p.out = static_cast<T*>(a->out);
    p.out_theta = static_cast<T*>(a->out_theta);
    p.addend = static_cast<const T*>(a->addend);
    p.addend_theta = static_cast<const T*>(a->addend_theta);
    p.xx = static_cast<const T*>(a->xx);
    p.yy = static_cast<const T*>(a->yy);
    p.pi = a->pair_i;
    p.pj = a->pair_j;
    p.total = (long long)a->npairs * a->h * a->w * a->h * a->w;
    p.g = make_idx(a->h, a->w);
    p.hw = a->h * a->w;
    p.same = a->same != 0;
    p.exact = (a->flags & CGP_FLAG_EXACT_RELU) != 0;
    p.k = slopes<T>(a->s, a->m, a->hh);
    const long long blocks = (p.total + kChunk - 1) / kChunk;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "abrelu_cov: %lld elements", p.total);
    hipStream_t s = as_stream(stream);
    return a->theta ? launch_abrelu_cov<T, true>(p, blocks, s)
                    : launch_abrelu_cov<T, false>(p, blocks, s);
}

}  // namespace

extern "C" {

size_t cgp_abrelu_args_size(void) { return sizeof(cgp_abrelu_args); }
size_t cgp_abrelu_cov_args_size(void) { return sizeof(cgp_abrelu_cov_args); }

int cgp_abrelu_f64(const cgp_abrelu_args* args, void* stream) {
    return abrelu_impl<double>(args, stream);
}
int cgp_abrelu_f32(const cgp_abrelu_args* args, void* stream) {
    return abrelu_impl<float>(args, stream);
}
int cgp_var_abrelu_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                       int32_t same, double h, double* xx_out, double* yy_out, void* stream) {
    return var_abrelu_impl<double>(xx, yy, n1, n2, hw, same, h, xx_out, yy_out, stream);
}
int cgp_var_abrelu_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                       int32_t same, double h, float* xx_out, float* yy_out, void* stream) {
    return var_abrelu_impl<float>(xx, yy, n1, n2, hw, same, h, xx_out, yy_out, stream);
}
int cgp_abrelu_cov_f64(const cgp_abrelu_cov_args* args, void* stream) {
    return abrelu_cov_impl<double>(args, stream);
}
int cgp_abrelu_cov_f32(const cgp_abrelu_cov_args* args, void* stream) {
    return abrelu_cov_impl<float>(args, stream);
}

}  // extern "C"
