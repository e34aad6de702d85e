// gelu.hip — the GELU nonlinearity on pair maps, per-image variances and position-pair maps
// (include/cnngp.h "The GELU nonlinearity").
//
// Three entry-point families, one device function per stream (gelu_math.h):
//   cgp_gelu_*      the layer path: K' (+ addend) and, with theta, Θ' = Θ·κ̇ in the same pass
//   cgp_var_gelu_*  the per-image variances
//   cgp_gelu_cov_*  position-pair maps S[p, q] (covpool.hip's layout)
// The kernels have the shapes of their erf twins (erf_pair_kernel, var_erf_kernel,
// cov_nonlin_kernel): whole 2048-element chunks per workgroup, all of a thread's loads issued
// before its math, the small variance maps read through L2.  Every element is read and
// written by one thread, so outputs may alias inputs; no __restrict__ on the maps for that
// reason.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "cnngp.h"
#include "cgp_common.h"
#include "gelu_math.h"

using namespace cgp;

namespace {

constexpr int kBlock = 256;                   // 4 waves of 64
constexpr int kChunk = 2048;                  // elements of one workgroup
constexpr int kE = kChunk / kBlock;           // loads in flight per thread (8)
constexpr long long kMaxPairElems = 1LL << 30;   // (h·w)² of one pair: 32-bit index math

// ----------------------------------------------------------------------------------
// the layer path: pair map m = i·n2 + j (or i = j = m with diag) of hw pixels; a workgroup
// takes mpb whole maps, at most kChunk elements
// ----------------------------------------------------------------------------------
template <typename T>
struct GeluP {
    const T* xy;
    const T* theta;
    T* out_xy;
    T* out_theta;
    const T* addend;
    const T* xx;
    const T* yy;
    long long nmaps;
    FastDiv n2, dhw;
    int hw, same, diag, mpb;
};

template <typename T, bool NTK, bool ADD>
__global__ __launch_bounds__(kBlock) void gelu_pair_kernel(const GeluP<T> p) {
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
            T r = gelu_pair(v[k], vx, self ? vx : p.yy + (size_t)j * p.hw + px, self, kd);
            if constexpr (ADD) r = r + add[e];
            dst[e] = r;
            if constexpr (NTK) tdst[e] = th[k] * kd;
        }
    }
}

// GELU on the per-image variances
template <typename T>
__global__ __launch_bounds__(kBlock) void var_gelu_kernel(const T* __restrict__ xx,
                                                          const T* __restrict__ yy,
                                                          long long n_xx, long long n_yy,
                                                          int same, T* xo, T* yo) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < n_xx + n_yy;
         e += stride) {
        if (e < n_xx) {
            xo[e] = gelu_var(xx[e]);
        } else {
            const long long f = e - n_xx;
            yo[f] = gelu_var(same ? xx[f] : yy[f]);
        }
    }
}

// ----------------------------------------------------------------------------------
// position-pair maps [pair][p_row][q_row][p_col][q_col]: element -> pixels
// p = p_row·w + p_col, q = q_row·w + q_col; one kChunk-element chunk per workgroup, which
// may straddle pairs (CovIdx, cov_decode: cgp_common.h)
// ----------------------------------------------------------------------------------
template <typename T>
struct GeluCovP {
    const T* in;
    T* out;
    const T* addend;
    const T* xx;
    const T* yy;
    const int* pi;
    const int* pj;
    long long total;
    CovIdx g;
    int hw, same;
};

template <typename T, bool ADD>
__global__ __launch_bounds__(kBlock) void gelu_cov_kernel(const GeluCovP<T> p) {
    const long long base = (long long)blockIdx.x * kChunk;
    const long long rem = p.total - base;
    const int n = rem < kChunk ? (int)rem : kChunk;
    const long long m0 = base / p.g.dn.d;
    const unsigned r0 = (unsigned)(base - m0 * p.g.dn.d);
    const T* src = p.in + base;
    const T* add = ADD ? p.addend + base : nullptr;
    T* dst = p.out + base;
    T v[kE];
#pragma unroll
    for (int k = 0; k < kE; ++k) {
        const int e = threadIdx.x + k * kBlock;
        v[k] = e < n ? src[e] : T(0);
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
            T r = gelu_pair(v[k], vx, self ? vx : p.yy + (size_t)j * p.hw + qx, self, kd);
            if constexpr (ADD) r = r + add[e];
            dst[e] = r;
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

template <typename T, bool NTK>
int launch_gelu(const GeluP<T>& p, long long blocks, hipStream_t s) {
    if (p.addend)
        hipLaunchKernelGGL((gelu_pair_kernel<T, NTK, true>), dim3((unsigned)blocks),
                           dim3(kBlock), 0, s, p);
    else
        hipLaunchKernelGGL((gelu_pair_kernel<T, NTK, false>), dim3((unsigned)blocks),
                           dim3(kBlock), 0, s, p);
    return check_launch("gelu_pair_kernel");
}

template <typename T>
int gelu_impl(const cgp_gelu_args* a, void* stream) {
    // cgp_erf_*'s checks; theta == NULL is the forward-only form
    if (!a || !a->xy || !a->out_xy || !a->xx || (a->theta && !a->out_theta))
        return fail(CGP_EINVAL, "gelu: NULL argument");
    if (a->hw <= 0 || a->nmaps <= 0 || a->nmaps >= (1LL << 31))
        return fail(CGP_EINVAL, "gelu: bad sizes");
    if (a->n1 <= 0 || a->n2 <= 0 || (a->diag ? a->n1 : a->n1 * a->n2) != a->nmaps)
        return fail(CGP_EINVAL, "gelu: nmaps inconsistent with n1/n2/diag");
    if ((a->same || a->diag) && a->n1 != a->n2)
        return fail(CGP_EINVAL, "gelu: same / diag need n1 == n2");
    if (!(a->same && a->diag) && !a->yy) return fail(CGP_EINVAL, "gelu: yy is NULL");
    if (a->hw > kChunk) return fail(CGP_EINVAL, "gelu: map of %d pixels too large", a->hw);
    GeluP<T> p;
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
    // whole maps per workgroup, at most kE elements per thread
    p.mpb = std::max(1, kChunk / a->hw);
    const long long blocks = (a->nmaps + p.mpb - 1) / p.mpb;
    hipStream_t s = as_stream(stream);
    return a->theta ? launch_gelu<T, true>(p, blocks, s) : launch_gelu<T, false>(p, blocks, s);
}

template <typename T>
int var_gelu_impl(const T* xx, const T* yy, int64_t n1, int64_t n2, int32_t hw, int32_t same,
                  T* xo, T* yo, void* stream) {
    if (!xx || !yy || !xo || !yo) return fail(CGP_EINVAL, "var_gelu: NULL argument");
    if (n1 <= 0 || n2 <= 0 || hw <= 0) return fail(CGP_EINVAL, "var_gelu: bad sizes");
    if (same && n1 != n2) return fail(CGP_EINVAL, "var_gelu: same needs n1 == n2");
    const long long nx = n1 * hw, ny = n2 * hw;
    hipLaunchKernelGGL((var_gelu_kernel<T>), dim3(grid_for(nx + ny)), dim3(kBlock), 0,
                       as_stream(stream), xx, yy, nx, ny, same, xo, yo);
    return check_launch("var_gelu_kernel");
}

template <typename T>
int gelu_cov_impl(const cgp_gelu_cov_args* a, void* stream) {
    // cgp_cov_nonlin_*'s checks
    if (!a || !a->in || !a->out || !a->xx || !a->yy || !a->pair_i || !a->pair_j)
        return fail(CGP_EINVAL, "gelu_cov: NULL argument");
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || a->h <= 0 || a->w <= 0 ||
        (long long)a->h * a->w * a->h * a->w > kMaxPairElems)
        return fail(CGP_EINVAL, "gelu_cov: bad sizes");
    GeluCovP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.out = static_cast<T*>(a->out);
    p.addend = static_cast<const T*>(a->addend);
    p.xx = static_cast<const T*>(a->xx);
    p.yy = static_cast<const T*>(a->yy);
    p.pi = a->pair_i;
    p.pj = a->pair_j;
    p.total = (long long)a->npairs * a->h * a->w * a->h * a->w;
    p.g = make_idx(a->h, a->w);
    p.hw = a->h * a->w;
    p.same = a->same != 0;
    const long long blocks = (p.total + kChunk - 1) / kChunk;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "gelu_cov: %lld elements", p.total);
    hipStream_t s = as_stream(stream);
    if (a->addend)
        hipLaunchKernelGGL((gelu_cov_kernel<T, true>), dim3((unsigned)blocks), dim3(kBlock), 0,
                           s, p);
    else
        hipLaunchKernelGGL((gelu_cov_kernel<T, false>), dim3((unsigned)blocks), dim3(kBlock), 0,
                           s, p);
    return check_launch("gelu_cov_kernel");
}

}  // namespace

extern "C" {

size_t cgp_gelu_args_size(void) { return sizeof(cgp_gelu_args); }
size_t cgp_gelu_cov_args_size(void) { return sizeof(cgp_gelu_cov_args); }

int cgp_gelu_f64(const cgp_gelu_args* args, void* stream) {
    return gelu_impl<double>(args, stream);
}
int cgp_gelu_f32(const cgp_gelu_args* args, void* stream) {
    return gelu_impl<float>(args, stream);
}
int cgp_var_gelu_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                     int32_t same, double* xx_out, double* yy_out, void* stream) {
    return var_gelu_impl<double>(xx, yy, n1, n2, hw, same, xx_out, yy_out, stream);
}
int cgp_var_gelu_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                     int32_t same, float* xx_out, float* yy_out, void* stream) {
    return var_gelu_impl<float>(xx, yy, n1, n2, hw, same, xx_out, yy_out, stream);
}
int cgp_gelu_cov_f64(const cgp_gelu_cov_args* args, void* stream) {
    return gelu_cov_impl<double>(args, stream);
}
int cgp_gelu_cov_f32(const cgp_gelu_cov_args* args, void* stream) {
    return gelu_cov_impl<float>(args, stream);
}

}  // extern "C"
