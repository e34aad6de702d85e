// covpool.hip — position-pair covariance maps for networks that end in global average
// pooling (include/cnngp.h "Position-pair maps").
//
// A dense readout needs, per image pair, the covariance of a pixel of x with the SAME pixel
// of y: one [H][W] map.  A pooled head averages the covariance of EVERY pixel p of x_i with
// EVERY pixel q of y_j, so the recursion carries S[p, q]: (H·W)² values per pair, stored as
//
//     [pair][p_row][q_row][p_col][q_col]
//
// so that the W×W block of one row pair is contiguous.  A conv shifts p and q by the same
// tap, i.e. it is a stencil along the diagonal of the row pair index and, inside a block,
// along the diagonal of the column pair index.  Pairs are given as two device index arrays
// (pair_i[m], pair_j[m]); every kernel is a pure function of one pair's data with a fixed
// summation order, so a result does not depend on how the host chunks the pair list.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "cnngp.h"
#include "nonlin_walk.h"

using namespace cgp;

namespace {

constexpr int kBlock = 256;                   // 4 waves of 64
constexpr int kChunk = 2048;                  // elements of one elementwise workgroup
constexpr int kE = kChunk / kBlock;           // loads in flight per thread (8)
constexpr int kMaxUnits = 256;                // row pairs one conv workgroup may hold
constexpr int kMaxBlocks = 1024;              // blocks (row pairs x taps) it may stage
constexpr int kPoolBlock = 1024;              // threads of a pool workgroup (one per pair)
constexpr int kMaxLds = 64 * 1024;            // bytes of LDS one conv workgroup may take

// ----------------------------------------------------------------------------------
// input moments: S[m][p, q] = mean_c x_i[c, p]·y_j[c, q], summed like moments_var_kernel
// (the i == j, p == q entries are the per-image variances bit for bit)
// ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void cov_moments_kernel(const T* __restrict__ x,
                                                             const T* __restrict__ y,
                                                             const int* __restrict__ pi,
                                                             const int* __restrict__ pj,
                                                             long long total, CovIdx g, int c,
                                                             int hw, T* __restrict__ out) {
    const long long base = (long long)blockIdx.x * kChunk;
    const long long rem = total - base;
    const int n = rem < kChunk ? (int)rem : kChunk;
    const long long m0 = base / g.dn.d;
    const unsigned r0 = (unsigned)(base - m0 * g.dn.d);
    for (int e = threadIdx.x; e < n; e += kBlock) {
        const unsigned rt = r0 + (unsigned)e;
        const unsigned mm = fdiv(rt, g.dn);
        const long long m = m0 + mm;
        int p, q;
        cov_decode(g, rt - mm * g.dn.d, p, q);
        const T* xi = x + (size_t)pi[m] * c * hw + p;
        const T* yj = y + (size_t)pj[m] * c * hw + q;
        T acc = xi[0] * yj[0];
        for (int k = 1; k < c; ++k) acc += xi[(size_t)k * hw] * yj[(size_t)k * hw];
        out[base + e] = acc / T(c);
    }
}

// ----------------------------------------------------------------------------------
// Conv2d on position-pair maps:
//   S'[p, q] = weight · Σ_a Σ_b S[(p_row·s + off + a·d, p_col·s + off + b·d),
//                                 (q_row·s + off + a·d, q_col·s + off + b·d)] + bias
// A workgroup owns `upb` output row pairs (p_row, q_row) of consecutive pairs.  It stages
// the `taps` input blocks (p_row·s + off + a·d, q_row·s + off + a·d) of each, contiguous
// w×w ranges, in LDS (zeros where a row leaves the map), then every output takes its
// `taps` diagonal window sums from LDS: the column taps first, then the row taps, left to
// right -- the order of conv_cov_kernel, so the p == q entries of a self pair equal the
// layer path's variance maps bit for bit.  The output of a row pair is one contiguous
// wo×wo range.  An input block is read by up to `taps` workgroups, ho + 1 row pairs apart
// in launch order (DESIGN §3.3 has the measurements and what was tried).
// ----------------------------------------------------------------------------------
template <typename T>
struct CovConvP {
    const T* in;
    T* out;
    const T* addend;
    const T* xx;
    const T* yy;
    const int* pi;
    const int* pj;
    long long units;           // npairs·ho·ho row pairs
    FastDiv dww, dwowo, dwo;
    int h, w, ho, wo, taps, off, stride, dil, upb, post, same, exact;
    int tab_offset;            // byte offset of the index tables in LDS
    T weight, bias;
};

template <typename T, bool ADD>
__global__ __launch_bounds__(kBlock) void cov_conv_kernel(const CovConvP<T> p) {
    // dynamic LDS: the staged blocks [upb][taps][w·w], then each block's element offset in
    // `in` (-1: a row outside the map) and each row pair's (pair, p_row, q_row)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds = reinterpret_cast<T*>(smem);
    long long* s_base = reinterpret_cast<long long*>(smem + p.tab_offset);
    int* s_m = reinterpret_cast<int*>(s_base + p.upb * p.taps);
    int* s_pr = s_m + p.upb;
    int* s_qr = s_pr + p.upb;
    const int tid = threadIdx.x;
    const long long u0 = (long long)blockIdx.x * p.upb;
    const long long urem = p.units - u0;
    const int nu = urem < p.upb ? (int)urem : p.upb;
    const int ww = p.w * p.w, wowo = p.wo * p.wo, hoho = p.ho * p.ho;
    const int per = p.taps * ww;
    for (int b = tid; b < nu * p.taps; b += kBlock) {
        const int ul = b / p.taps, a = b - ul * p.taps;
        const long long u = u0 + ul;
        const long long m = u / hoho;
        const int r = (int)(u - m * hoho);
        const int pr = r / p.ho, qr = r - pr * p.ho;
        const int ir = pr * p.stride + p.off + a * p.dil;
        const int jr = qr * p.stride + p.off + a * p.dil;
        const bool in = (unsigned)ir < (unsigned)p.h && (unsigned)jr < (unsigned)p.h;
        s_base[b] = in ? ((m * p.h + ir) * p.h + jr) * ww : -1;
        if (a == 0) {
            s_m[ul] = (int)m;
            s_pr[ul] = pr;
            s_qr[ul] = qr;
        }
    }
    __syncthreads();

    // ---- stage: the taps input blocks of every row pair, kE loads in flight per thread ----
    const int total = nu * per;
    for (int e0 = tid; e0 < total; e0 += kE * kBlock) {
        T v[kE];
#pragma unroll
        for (int k = 0; k < kE; ++k) {
            const int e = e0 + k * kBlock;
            v[k] = T(0);
            if (e < total) {
                const unsigned blk = fdiv((unsigned)e, p.dww);
                const long long base = s_base[blk];
                if (base >= 0) v[k] = p.in[base + (e - (int)blk * ww)];
            }
        }
#pragma unroll
        for (int k = 0; k < kE; ++k) {
            const int e = e0 + k * kBlock;
            if (e < total) lds[e] = v[k];
        }
    }
    __syncthreads();

    // ---- window sums, affine, nonlinearity, addend, store ----
    for (int e = tid; e < nu * wowo; e += kBlock) {
        const unsigned ul = fdiv((unsigned)e, p.dwowo);
        const int o = e - (int)ul * wowo;
        const unsigned pc = fdiv((unsigned)o, p.dwo);
        const int qc = o - (int)pc * p.wo;
        const int c0 = (int)pc * p.stride + p.off, d0 = qc * p.stride + p.off;
        const T* blk = lds + (int)ul * per;
        T acc = T(0);
        for (int a = 0; a < p.taps; ++a) {
            T rs = T(0);
            for (int b = 0; b < p.taps; ++b) {
                const int ic = c0 + b * p.dil, jc = d0 + b * p.dil;
                T t = T(0);
                if ((unsigned)ic < (unsigned)p.w && (unsigned)jc < (unsigned)p.w)
                    t = blk[a * ww + ic * p.w + jc];
                rs = b == 0 ? t : rs + t;
            }
            acc = a == 0 ? rs : acc + rs;
        }
        T val = p.weight * acc + p.bias;
        const int m = s_m[ul];
        if (p.post != CGP_COV_NONE) {
            T kd;
            val = cov_nonlin<T, false>(val, p.post, p.xx, p.yy, p.pi[m], p.pj[m], p.ho * p.wo,
                                       s_pr[ul] * p.wo + (int)pc, s_qr[ul] * p.wo + qc, p.same,
                                       p.exact, kd);
        }
        const long long oe = (u0 + ul) * wowo + o;
        if constexpr (ADD) val = val + p.addend[oe];
        p.out[oe] = val;
    }
}

// ----------------------------------------------------------------------------------
// out[m] = mean of pair m's n elements.  One workgroup of 1024 threads per pair (a tile
// has fewer pairs than the device has wave slots): four running sums per
// thread over a fixed stride pattern, then a fixed tree over the workgroup, all in double.
// No atomics: the bits depend on (n, the data) only.
// ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kPoolBlock) void cov_pool_kernel(const T* __restrict__ in, long long n,
                                                          T* __restrict__ out) {
    __shared__ double part[kPoolBlock];
    const T* src = in + (long long)blockIdx.x * n;
    const int tid = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long long e = tid;
    for (; e + 3 * kPoolBlock < n; e += 4 * kPoolBlock) {
        const T t0 = src[e], t1 = src[e + kPoolBlock], t2 = src[e + 2 * kPoolBlock],
                t3 = src[e + 3 * kPoolBlock];
        a0 += (double)t0;
        a1 += (double)t1;
        a2 += (double)t2;
        a3 += (double)t3;
    }
    for (; e < n; e += kPoolBlock) a0 += (double)src[e];
    part[tid] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int s = kPoolBlock / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = (T)(part[0] / (double)n);
}

// ----------------------------------------------------------------------------------
// AvgPool2d on position-pair maps: p and q move independently,
//   S'[P, Q][U, V] = k⁻⁴ · Σ_{a,a'<k} Σ_{b,b'<k} S[P·s + a, Q·s + a'][U·s + b, V·s + b']
// (a conv moves both by one tap).  A workgroup owns `upb` output row pairs
// (P, Q) of consecutive pairs.  It streams the k² input blocks (P·s + a, Q·s + a') of each,
// contiguous w×w ranges, one element per lane per block with a thread's loads issued before
// its adds, sums them elementwise in registers and stores the w×w sums to LDS.  Then every
// output takes its k×k window of the sums from LDS, is divided once by k⁴ and stored: one
// contiguous wo×wo range per row pair.  With s >= k every input element is fetched at most
// once.  All sums are held in T and their order depends on k alone.  Both sums run over the
// offset pairs in the order  t(0,0), t(0,1) + t(1,0), ..., t(1,1), t(1,2) + t(2,1), ...:
// an offset pair and its mirror are added to each other first (a + b == b + a in IEEE), so
// a self pair's map, symmetric bit for bit under p <-> q coming in, is so going out.
// ----------------------------------------------------------------------------------
template <typename T>
struct CovAvgP {
    const T* in;
    T* out;
    long long units;           // npairs·ho·ho row pairs
    FastDiv dww, dwowo, dwo;
    int h, w, ho, wo, k, stride, upb;
    int tab_offset;            // byte offset of the row pairs' base offsets in LDS
    T k4;
};

// K: the window edge at compile time (every block's loads of a pass in flight at once), or
// 0 for p.k at run time (one block's loads in flight at a time)
template <typename T, int K>
__global__ __launch_bounds__(kBlock) void cov_avgpool_kernel(const CovAvgP<T> p) {
    // dynamic LDS: the summed blocks [upb][w·w], then each row pair's element offset in
    // `in` of its block (P·s, Q·s)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds = reinterpret_cast<T*>(smem);
    long long* s_base = reinterpret_cast<long long*>(smem + p.tab_offset);
    const int tid = threadIdx.x;
    const int k = K ? K : p.k;
    const long long u0 = (long long)blockIdx.x * p.upb;
    const long long urem = p.units - u0;
    const int nu = urem < p.upb ? (int)urem : p.upb;
    const int ww = p.w * p.w, wowo = p.wo * p.wo, hoho = p.ho * p.ho;
    for (int ul = tid; ul < nu; ul += kBlock) {
        const long long u = u0 + ul;
        const long long m = u / hoho;
        const int r = (int)(u - m * hoho);
        const int pr = r / p.ho, qr = r - pr * p.ho;
        s_base[ul] = ((m * p.h + pr * p.stride) * p.h + qr * p.stride) * ww;
    }
    __syncthreads();

    // ---- stream: the k² blocks of every row pair, summed elementwise into LDS ----
    const int total = nu * ww;
    const long long rowstep = (long long)p.h * ww;     // from block (a, a') to (a + 1, a')
    for (int e0 = tid; e0 < total; e0 += kE * kBlock) {
        const T* src[kE];
        T acc[kE];
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            const int e = e0 + j * kBlock;
            src[j] = p.in;
            if (e < total) {
                const unsigned ul = fdiv((unsigned)e, p.dww);
                src[j] = p.in + s_base[ul] + (e - (int)ul * ww);
            }
        }
        if constexpr (K == 2) {
            T v[4][kE];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int j = 0; j < kE; ++j)
                    v[b][j] = e0 + j * kBlock < total ? src[j][(b >> 1) * rowstep + (b & 1) * ww]
                                                      : T(0);
#pragma unroll
            for (int j = 0; j < kE; ++j) acc[j] = (v[0][j] + (v[1][j] + v[2][j])) + v[3][j];
        } else {
            for (int a = 0; a < k; ++a) {
                const long long o = a * rowstep + (long long)a * ww;
                T v[kE];
#pragma unroll
                for (int j = 0; j < kE; ++j) v[j] = e0 + j * kBlock < total ? src[j][o] : T(0);
#pragma unroll
                for (int j = 0; j < kE; ++j) acc[j] = a == 0 ? v[j] : acc[j] + v[j];
                for (int a2 = a + 1; a2 < k; ++a2) {
                    const long long o1 = a * rowstep + (long long)a2 * ww;
                    const long long o2 = a2 * rowstep + (long long)a * ww;
                    T v1[kE], v2[kE];
#pragma unroll
                    for (int j = 0; j < kE; ++j) {
                        const bool in = e0 + j * kBlock < total;
                        v1[j] = in ? src[j][o1] : T(0);
                        v2[j] = in ? src[j][o2] : T(0);
                    }
#pragma unroll
                    for (int j = 0; j < kE; ++j) acc[j] = acc[j] + (v1[j] + v2[j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            const int e = e0 + j * kBlock;
            if (e < total) lds[e] = acc[j];
        }
    }
    __syncthreads();

    // ---- window sums over the columns, the one scale, store ----
    for (int e = tid; e < nu * wowo; e += kBlock) {
        const unsigned ul = fdiv((unsigned)e, p.dwowo);
        const int o = e - (int)ul * wowo;
        const unsigned pc = fdiv((unsigned)o, p.dwo);
        const int qc = o - (int)pc * p.wo;
        const T* blk = lds + (int)ul * ww + (int)pc * p.stride * p.w + qc * p.stride;
        T acc = T(0);
        for (int b = 0; b < k; ++b) {
            const T t = blk[b * p.w + b];
            acc = b == 0 ? t : acc + t;
            for (int b2 = b + 1; b2 < k; ++b2) acc = acc + (blk[b * p.w + b2] + blk[b2 * p.w + b]);
        }
        p.out[(u0 + ul) * wowo + o] = acc / p.k4;
    }
}

// ----------------------------------------------------------------------------------
// out[pi[m]][r][c] = in[m][r][r][c][c]: the p = q diagonal of pair m's map, the variance map
// of image pi[m] when pair m is (i, i).  A gather of h·w elements per pair.
// ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void cov_diag_kernel(const T* __restrict__ in,
                                                          const int* __restrict__ pi,
                                                          long long total, int h, int w,
                                                          T* __restrict__ out) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= total) return;
    const int hw = h * w;
    const long long m = t / hw;
    const int rc = (int)(t - m * hw);
    const int r = rc / w, c = rc - r * w;
    const long long n = (long long)hw * hw;
    out[(long long)pi[m] * hw + rc] = in[m * n + ((long long)(r * h + r) * w + c) * w + c];
}

// ----------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------
template <typename T>
int cov_moments_impl(const T* x, const T* y, const int32_t* pi, const int32_t* pj,
                     int64_t npairs, int32_t c, int32_t h, int32_t w, T* out, void* stream) {
    if (!x || !y || !pi || !pj || !out) return fail(CGP_EINVAL, "cov_moments: NULL argument");
    if (npairs <= 0 || npairs >= (1LL << 31) || c <= 0 || bad_map(h, w))
        return fail(CGP_EINVAL, "cov_moments: bad sizes");
    const long long total = (long long)npairs * h * w * h * w;
    const long long blocks = (total + kChunk - 1) / kChunk;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "cov_moments: %lld elements", total);
    hipLaunchKernelGGL((cov_moments_kernel<T>), dim3((unsigned)blocks), dim3(kBlock), 0,
                       as_stream(stream), x, y, pi, pj, total, make_idx(h, w), c, h * w, out);
    return check_launch("cov_moments_kernel");
}

template <typename T>
int cov_conv_impl(const cgp_cov_conv_args* a, void* stream) {
    if (!a || !a->in || !a->out) return fail(CGP_EINVAL, "cov_conv: NULL argument");
    if (a->in == a->out) return fail(CGP_EINVAL, "cov_conv: out must not be in");
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || bad_map(a->h, a->w) ||
        bad_map(a->ho, a->wo))
        return fail(CGP_EINVAL, "cov_conv: bad sizes");
    if (a->taps <= 0 || a->stride <= 0 || a->dilation <= 0)
        return fail(CGP_EINVAL, "cov_conv: bad geometry");
    if (a->post != CGP_COV_NONE && a->post != CGP_COV_RELU && a->post != CGP_COV_ERF)
        return fail(CGP_EINVAL, "cov_conv: post %d is not a nonlinearity", a->post);
    if (a->post != CGP_COV_NONE && (!a->xx || !a->yy || !a->pair_i || !a->pair_j))
        return fail(CGP_EINVAL, "cov_conv: a post-nonlinearity needs xx, yy and the pair lists");
    const long long per = (long long)a->taps * a->w * a->w;
    // one row pair's blocks and its index entries (a block offset per tap, three ints)
    const long long unit_bytes = per * (long long)sizeof(T) + 8LL * a->taps + 12;
    if (unit_bytes + 8 > kMaxLds || a->taps > kMaxBlocks)
        return fail(CGP_EINVAL,
                    "cov_conv: %d taps of a %dx%d block are %lld bytes, more than the %d of LDS "
                    "a workgroup stages", a->taps, a->w, a->w, per * (long long)sizeof(T),
                    kMaxLds);
    CovConvP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.out = static_cast<T*>(a->out);
    p.addend = static_cast<const T*>(a->addend);
    p.xx = static_cast<const T*>(a->xx);
    p.yy = static_cast<const T*>(a->yy);
    p.pi = a->pair_i;
    p.pj = a->pair_j;
    p.units = (long long)a->npairs * a->ho * a->ho;
    p.h = a->h, p.w = a->w, p.ho = a->ho, p.wo = a->wo;
    p.taps = a->taps, p.off = a->offset, p.stride = a->stride, p.dil = a->dilation;
    p.post = a->post;
    p.same = a->same != 0;
    p.exact = (a->flags & CGP_FLAG_EXACT_RELU) != 0;
    p.weight = (T)a->weight;
    p.bias = (T)a->bias;
    // small maps: several row pairs per workgroup, about 1024 staged or written elements
    const long long big = std::max<long long>((long long)a->w * a->w, (long long)a->wo * a->wo);
    long long upb = std::max<long long>(1, 1024 / big);
    upb = std::min<long long>(upb, kMaxUnits);
    upb = std::min<long long>(upb, kMaxBlocks / a->taps);
    upb = std::min<long long>(upb, (kMaxLds - 8) / unit_bytes);
    p.upb = (int)upb;
    p.tab_offset = (int)((upb * per * (long long)sizeof(T) + 7) / 8 * 8);
    p.dww = make_fastdiv((unsigned)(a->w * a->w));
    p.dwowo = make_fastdiv((unsigned)(a->wo * a->wo));
    p.dwo = make_fastdiv((unsigned)a->wo);
    const long long blocks = (p.units + upb - 1) / upb;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "cov_conv: %lld row pairs", p.units);
    const size_t lds = (size_t)p.tab_offset + (size_t)upb * (8 * a->taps + 12);
    hipStream_t s = as_stream(stream);
    if (a->addend)
        hipLaunchKernelGGL((cov_conv_kernel<T, true>), dim3((unsigned)blocks), dim3(kBlock), lds,
                           s, p);
    else
        hipLaunchKernelGGL((cov_conv_kernel<T, false>), dim3((unsigned)blocks), dim3(kBlock),
                           lds, s, p);
    return check_launch("cov_conv_kernel");
}

template <typename T>
int cov_pool_impl(const T* in, int64_t npairs, int64_t n, T* out, void* stream) {
    if (!in || !out) return fail(CGP_EINVAL, "cov_pool: NULL argument");
    if (npairs <= 0 || npairs >= (1LL << 31) || n <= 0)
        return fail(CGP_EINVAL, "cov_pool: bad sizes");
    hipLaunchKernelGGL((cov_pool_kernel<T>), dim3((unsigned)npairs), dim3(kPoolBlock), 0,
                       as_stream(stream), in, (long long)n, out);
    return check_launch("cov_pool_kernel");
}

template <typename T>
int cov_avgpool_impl(const cgp_covmap_avgpool_args* a, void* stream) {
    if (!a || !a->in || !a->out) return fail(CGP_EINVAL, "covmap_avgpool: NULL argument");
    if (a->in == a->out) return fail(CGP_EINVAL, "covmap_avgpool: out must not be in");
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || bad_map(a->h, a->w) ||
        bad_map(a->ho, a->wo))
        return fail(CGP_EINVAL, "covmap_avgpool: bad sizes");
    if (a->k < 1 || a->stride < 1)
        return fail(CGP_EINVAL, "covmap_avgpool: bad geometry (kernel_size %d, stride %d)", a->k,
                    a->stride);
    if (a->k > a->h || a->k > a->w)
        return fail(CGP_EINVAL, "covmap_avgpool: a %dx%d window does not fit a %dx%d map", a->k,
                    a->k, a->h, a->w);
    if (a->ho != (a->h - a->k) / a->stride + 1 || a->wo != (a->w - a->k) / a->stride + 1)
        return fail(CGP_EINVAL,
                    "covmap_avgpool: output size %dx%d is not floor((%dx%d - %d)/%d) + 1", a->ho,
                    a->wo, a->h, a->w, a->k, a->stride);
    const long long ww = (long long)a->w * a->w;
    // one row pair's summed block and its base offset
    const long long unit_bytes = ww * (long long)sizeof(T) + 8;
    if (unit_bytes + 8 > kMaxLds)
        return fail(CGP_EINVAL,
                    "covmap_avgpool: a %dx%d block is %lld bytes, more than the %d of LDS a "
                    "workgroup holds", a->w, a->w, ww * (long long)sizeof(T), kMaxLds);
    CovAvgP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.out = static_cast<T*>(a->out);
    p.units = (long long)a->npairs * a->ho * a->ho;
    p.h = a->h, p.w = a->w, p.ho = a->ho, p.wo = a->wo;
    p.k = a->k, p.stride = a->stride;
    p.k4 = (T)((double)a->k * a->k * a->k * a->k);
    // small maps: several row pairs per workgroup, one full pass of kE loads per thread
    long long upb = std::max<long long>(1, kChunk / ww);
    upb = std::min<long long>(upb, kMaxUnits);
    upb = std::min<long long>(upb, (kMaxLds - 8) / unit_bytes);
    p.upb = (int)upb;
    p.tab_offset = (int)((upb * ww * (long long)sizeof(T) + 7) / 8 * 8);
    p.dww = make_fastdiv((unsigned)ww);
    p.dwowo = make_fastdiv((unsigned)(a->wo * a->wo));
    p.dwo = make_fastdiv((unsigned)a->wo);
    const long long blocks = (p.units + upb - 1) / upb;
    if (blocks >= (1LL << 31))
        return fail(CGP_EINVAL, "covmap_avgpool: %lld row pairs", p.units);
    const size_t lds = (size_t)p.tab_offset + (size_t)upb * 8;
    hipStream_t s = as_stream(stream);
    if (a->k == 2)
        hipLaunchKernelGGL((cov_avgpool_kernel<T, 2>), dim3((unsigned)blocks), dim3(kBlock), lds,
                           s, p);
    else
        hipLaunchKernelGGL((cov_avgpool_kernel<T, 0>), dim3((unsigned)blocks), dim3(kBlock), lds,
                           s, p);
    return check_launch("cov_avgpool_kernel");
}

template <typename T>
int cov_diag_impl(const T* in, const int32_t* pi, int64_t npairs, int32_t h, int32_t w, T* out,
                  void* stream) {
    if (!in || !pi || !out) return fail(CGP_EINVAL, "covmap_diag: NULL argument");
    if (npairs <= 0 || npairs >= (1LL << 31) || bad_map(h, w))
        return fail(CGP_EINVAL, "covmap_diag: bad sizes");
    const long long total = (long long)npairs * h * w;
    const long long blocks = (total + kBlock - 1) / kBlock;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "covmap_diag: %lld elements", total);
    hipLaunchKernelGGL((cov_diag_kernel<T>), dim3((unsigned)blocks), dim3(kBlock), 0,
                       as_stream(stream), in, pi, total, h, w, out);
    return check_launch("cov_diag_kernel");
}

}  // namespace

extern "C" {

size_t cgp_cov_conv_args_size(void) { return sizeof(cgp_cov_conv_args); }

int cgp_cov_moments_f64(const double* x, const double* y, const int32_t* pair_i,
                        const int32_t* pair_j, int64_t npairs, int32_t c, int32_t h, int32_t w,
                        double* out, void* stream) {
    return cov_moments_impl<double>(x, y, pair_i, pair_j, npairs, c, h, w, out, stream);
}
int cgp_cov_moments_f32(const float* x, const float* y, const int32_t* pair_i,
                        const int32_t* pair_j, int64_t npairs, int32_t c, int32_t h, int32_t w,
                        float* out, void* stream) {
    return cov_moments_impl<float>(x, y, pair_i, pair_j, npairs, c, h, w, out, stream);
}
int cgp_cov_conv_f64(const cgp_cov_conv_args* args, void* stream) {
    return cov_conv_impl<double>(args, stream);
}
int cgp_cov_conv_f32(const cgp_cov_conv_args* args, void* stream) {
    return cov_conv_impl<float>(args, stream);
}
int cgp_cov_pool_f64(const double* in, int64_t npairs, int64_t n, double* out, void* stream) {
    return cov_pool_impl<double>(in, npairs, n, out, stream);
}
int cgp_cov_pool_f32(const float* in, int64_t npairs, int64_t n, float* out, void* stream) {
    return cov_pool_impl<float>(in, npairs, n, out, stream);
}

size_t cgp_covmap_avgpool_args_size(void) { return sizeof(cgp_covmap_avgpool_args); }
int cgp_covmap_avgpool_f64(const cgp_covmap_avgpool_args* args, void* stream) {
    return cov_avgpool_impl<double>(args, stream);
}
int cgp_covmap_avgpool_f32(const cgp_covmap_avgpool_args* args, void* stream) {
    return cov_avgpool_impl<float>(args, stream);
}
int cgp_covmap_diag_f64(const double* in, const int32_t* pair_i, int64_t npairs, int32_t h,
                        int32_t w, double* out, void* stream) {
    return cov_diag_impl<double>(in, pair_i, npairs, h, w, out, stream);
}
int cgp_covmap_diag_f32(const float* in, const int32_t* pair_i, int64_t npairs, int32_t h,
                        int32_t w, float* out, void* stream) {
    return cov_diag_impl<float>(in, pair_i, npairs, h, w, out, stream);
}

}  // extern "C"
