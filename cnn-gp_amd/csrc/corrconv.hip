// corrconv.hip — convs and readouts with correlated weights on position-pair maps
// (include/cnngp.h "cgp_corrconv_*").
//
// A conv whose taps δ and δ' of one filter have the correlation R[δ, δ'] mixes different
// positions of x and y:
//
//   S'[p, q] = weight · Σ_{δ, δ'} R[δ, δ'] · S[p·s + off + δ·d, q·s + off + δ'·d] + bias
//
// with R separable, R[(a, b), (a', b')] = Rr[a, a']·Rc[b, b'].  R = I is cov_conv_kernel's
// diagonal stencil, R = ones cov_avgpool_kernel's window sum (with padding and dilation) and,
// at taps = h, cov_pool_kernel's mean.  The layout is covpool.hip's
// [pair][p_row][q_row][p_col][q_col]: the w×w block of one row pair is contiguous.
//
// The shape is cov_avgpool_kernel's.  A workgroup owns `upb` consecutive output row pairs
// (P, Q).  It streams the contributing input blocks (P·s + off + a·d, Q·s + off + a'·d), one
// element per lane per block, accumulates the Rr-weighted sums in registers and stores the
// w×w sums to LDS; after a barrier every output takes its Rc-weighted window from LDS.
// Both sums run over the offset pairs a <= a' in row-major order, an offset pair taken with
// its mirror first, Rr[a, a']·(t(a, a') + t(a', a)) (R is symmetric; x + y == y + x in IEEE):
// a self pair's map that comes in symmetric bit for bit under p <-> q goes out so.  Offset
// pairs whose weight is exactly zero are dropped from the walk by the workgroup's first wave
// before anything is fetched (the lists below), so the walk is uniform over the workgroup:
// R = I fetches taps blocks per output row pair, a band of half-width c (2c + 1)·taps.
// Every choice the host makes (row pairs per workgroup, the instantiation, the lanes that
// share an output) is a function of the geometry alone, and an element's arithmetic is the
// same in every instantiation: a result does not depend on the grid, the pair count or how
// the caller chunks the pairs.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "cnngp.h"
#include "cgp_common.h"

using namespace cgp;

namespace {

constexpr int kMaxUnits = 256;                // row pairs one workgroup may hold
constexpr int kMaxLds = 64 * 1024;            // bytes of LDS one workgroup may take

// offset pairs the 1024-thread instantiation carries at a time (their block offsets and
// weights stay in scalar registers: 16 pairs spill them, and measured no faster)
constexpr int kWideTaps = 8;

template <typename T>
struct CorrP {
    const T* in;
    T* out;
    const T* rr;               // [taps][taps] row correlations
    const T* rc;               // [taps][taps] column correlations
    long long units;           // npairs·ho·ho row pairs
    FastDiv dww, dwowo, dwo;
    int h, w, ho, wo, taps, off, stride, dil, upb;
    int lshift;                // log2 of the lanes that share one output's window sum
    int tab_offset;            // byte offset of the tables behind the sums in LDS
    T weight, bias;
};

// LDS behind the upb·w·w sums: Rr, Rc [taps²] of T, the row pairs' base offsets (8 bytes
// each), their first input rows (2 ints each), the two lists of offset pairs with a non-zero
// weight (taps·(taps + 1)/2 ints each) and the lists' lengths
template <typename T>
long long corr_lds_bytes(long long upb, long long ww, long long taps) {
    const long long sums = (upb * ww * (long long)sizeof(T) + 7) / 8 * 8;
    const long long tables = (2 * taps * taps * (long long)sizeof(T) + 7) / 8 * 8;
    return sums + tables + upb * 16 + taps * (taps + 1) * 4 + 8;
}

// A value every lane of the wave holds, moved to scalar registers: what is derived from it
// (a tap's block offset in 64 bits, the zero tests) then runs on the scalar unit
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uniform(float v) {
    return __builtin_bit_cast(float, uniform(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double uniform(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)uniform((int)(unsigned)u), hi = (unsigned)uniform((int)(u >> 32));
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// V consecutive elements as one load (V = 1: the element itself)
template <typename T, int V>
struct Vec {
    typedef T type __attribute__((ext_vector_type(V)));
};
template <typename T>
struct Vec<T, 1> {
    typedef T type;
};

// BLOCK threads; a thread carries E groups of V consecutive elements of the row pairs' blocks
// through B offset pairs at a time: 2·E·B loads of V elements are issued before the first
// add.  V > 1 needs w·w to be a multiple of V and `in` aligned to V elements; the arithmetic
// of an element is the same for every V
template <typename T, int BLOCK, int E, int B, int V>
__global__ __launch_bounds__(BLOCK) void cov_corrconv_kernel(const CorrP<T> p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int k = p.taps, kk = k * k, ntri = k * (k + 1) / 2;
    const int ww = p.w * p.w, wowo = p.wo * p.wo, hoho = p.ho * p.ho;
    T* lds = reinterpret_cast<T*>(smem);
    T* s_rr = reinterpret_cast<T*>(smem + p.tab_offset);
    T* s_rc = s_rr + kk;
    long long* s_base = reinterpret_cast<long long*>(
        smem + p.tab_offset + (2 * kk * (int)sizeof(T) + 7) / 8 * 8);
    int* s_row = reinterpret_cast<int*>(s_base + p.upb);
    int* s_tap = s_row + 2 * p.upb;
    int* s_ctap = s_tap + ntri;
    int* s_cnt = s_ctap + ntri;
    const long long u0 = (long long)blockIdx.x * p.upb;
    const long long urem = p.units - u0;
    const int nu = urem < p.upb ? (int)urem : p.upb;

    for (int i = tid; i < kk; i += BLOCK) {
        s_rr[i] = p.rr[i];
        s_rc[i] = p.rc[i];
    }
    for (int ul = tid; ul < nu; ul += BLOCK) {
        const long long u = u0 + ul;
        const long long m = u / hoho;
        const int r = (int)(u - m * hoho);
        const int pr = r / p.ho, qr = r - pr * p.ho;
        const int rp0 = pr * p.stride + p.off, rq0 = qr * p.stride + p.off;
        // the element offset of block (rp0, rq0): outside the pair's map where a row is
        // padding, and only ever dereferenced with a tap that leads back inside
        s_base[ul] = m * p.h * p.h * ww + ((long long)rp0 * p.h + rq0) * ww;
        s_row[2 * ul] = rp0;
        s_row[2 * ul + 1] = rq0;
    }
    __syncthreads();

    // ---- the offset pairs a <= a' with a non-zero weight, in row-major order ----
    if (tid < 64) {
        int nr = 0, nc = 0;
        const unsigned long long below = (1ull << tid) - 1;
        for (int i0 = 0; i0 < kk; i0 += 64) {
            const int i = i0 + tid;
            const int a = i / k, a2 = i - a * k;
            const bool upper = i < kk && a2 >= a;
            const bool zr = upper && s_rr[i] != T(0);
            const bool zc = upper && s_rc[i] != T(0);
            const unsigned long long mr = __ballot(zr), mc = __ballot(zc);
            if (zr) s_tap[nr + __popcll(mr & below)] = (a << 16) | a2;
            if (zc) s_ctap[nc + __popcll(mc & below)] = (a << 16) | a2;
            nr += __popcll(mr);
            nc += __popcll(mc);
        }
        if (tid == 0) {
            s_cnt[0] = nr;
            s_cnt[1] = nc;
        }
    }
    __syncthreads();
    const int nrow = uniform(s_cnt[0]), ncol = uniform(s_cnt[1]);

    // ---- stream: the Rr-weighted sum of every row pair's blocks, elementwise into LDS ----
    typedef typename Vec<T, V>::type VT;
    const int total = nu * ww;
    for (int e0 = tid * V; e0 < total; e0 += E * BLOCK * V) {
        long long base[E];
        int rp0[E], rq0[E];
        bool live[E];
        VT acc[E];
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int e = e0 + j * BLOCK * V;
            live[j] = e < total;
            base[j] = 0;
            rp0[j] = rq0[j] = 0;
            acc[j] = (VT)(T(0));
            if (live[j]) {
                const unsigned ul = fdiv((unsigned)e, p.dww);
                base[j] = s_base[ul] + (e - (int)ul * ww);
                rp0[j] = s_row[2 * ul];
                rq0[j] = s_row[2 * ul + 1];
            }
        }
        for (int t0 = 0; t0 < nrow; t0 += B) {
            VT v1[B][E], v2[B][E];
            T wg[B];
#pragma unroll
            for (int i = 0; i < B; ++i) {
                const bool on = t0 + i < nrow;
                const int tap = on ? uniform(s_tap[t0 + i]) : 0;
                const int a = tap >> 16, a2 = tap & 0xffff;
                wg[i] = on ? uniform(s_rr[a * k + a2]) : T(0);
                const int da = a * p.dil, da2 = a2 * p.dil;
                const long long o1 = ((long long)da * p.h + da2) * ww;     // block (a, a')
                const long long o2 = ((long long)da2 * p.h + da) * ww;     // its mirror
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const bool ok1 = on && live[j] && (unsigned)(rp0[j] + da) < (unsigned)p.h &&
                                     (unsigned)(rq0[j] + da2) < (unsigned)p.h;
                    const bool ok2 = on && live[j] && a != a2 &&
                                     (unsigned)(rp0[j] + da2) < (unsigned)p.h &&
                                     (unsigned)(rq0[j] + da) < (unsigned)p.h;
                    v1[i][j] = ok1 ? *reinterpret_cast<const VT*>(p.in + base[j] + o1)
                                   : (VT)(T(0));
                    v2[i][j] = ok2 ? *reinterpret_cast<const VT*>(p.in + base[j] + o2)
                                   : (VT)(T(0));
                }
            }
#pragma unroll
            for (int i = 0; i < B; ++i) {
                if (t0 + i < nrow) {
#pragma unroll
                    for (int j = 0; j < E; ++j) acc[j] = acc[j] + wg[i] * (v1[i][j] + v2[i][j]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int e = e0 + j * BLOCK * V;
            if (live[j]) *reinterpret_cast<VT*>(lds + e) = acc[j];
        }
    }
    __syncthreads();

    // ---- every output's Rc-weighted window of the sums, weight, bias, store ----
    // 1 << lshift lanes of one wave share an output: lane l takes the offset pairs l,
    // l + lanes, ... of the list, then a fixed xor tree (both sides of every add hold the
    // same two values, so every lane ends with the same bits)
    const int lanes = 1 << p.lshift;
    const int sub = tid & (lanes - 1);
    const int items = (nu * wowo) << p.lshift;
    for (int it0 = tid & ~63; it0 < items; it0 += BLOCK) {
        const int it = it0 + (tid & 63);
        const bool live = it < items;
        unsigned ul = 0;
        int o = 0;
        T acc = T(0);
        if (live) {
            const int e = it >> p.lshift;
            ul = fdiv((unsigned)e, p.dwowo);
            o = e - (int)ul * wowo;
            const unsigned pc = fdiv((unsigned)o, p.dwo);
            const int qc = o - (int)pc * p.wo;
            const int c0 = (int)pc * p.stride + p.off, d0 = qc * p.stride + p.off;
            const T* blk = lds + (int)ul * ww;
            for (int t = sub; t < ncol; t += lanes) {
                const int tap = s_ctap[t];
                const int b = tap >> 16, b2 = tap & 0xffff;
                const T wgt = s_rc[b * k + b2];
                const int c1 = c0 + b * p.dil, d1 = d0 + b2 * p.dil;
                const int c2 = c0 + b2 * p.dil, d2 = d0 + b * p.dil;
                const bool ok1 = (unsigned)c1 < (unsigned)p.w && (unsigned)d1 < (unsigned)p.w;
                const bool ok2 = b != b2 && (unsigned)c2 < (unsigned)p.w &&
                                 (unsigned)d2 < (unsigned)p.w;
                const T x = ok1 ? blk[c1 * p.w + d1] : T(0);
                const T y = ok2 ? blk[c2 * p.w + d2] : T(0);
                acc = acc + wgt * (x + y);
            }
        }
        for (int s = lanes >> 1; s > 0; s >>= 1) acc = acc + __shfl_xor(acc, s, 64);
        if (live && sub == 0) p.out[(u0 + ul) * wowo + o] = p.weight * acc + p.bias;
    }
}

template <typename T>
int corrconv_impl(const cgp_corrconv_args* a, void* stream) {
    if (!a || !a->in || !a->out || !a->corr_rows || !a->corr_cols)
        return fail(CGP_EINVAL, "corrconv: NULL argument");
    if (a->in == a->out) return fail(CGP_EINVAL, "corrconv: out must not be in");
    const auto bad_map = [](int h, int w) {
        return h <= 0 || w <= 0 || (long long)h * w * h * w > kMaxPairElems;
    };
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || bad_map(a->h, a->w) ||
        bad_map(a->ho, a->wo))
        return fail(CGP_EINVAL, "corrconv: bad sizes");
    // 32-bit row and column arithmetic: offset, stride and the taps' span stay below 2^24
    constexpr long long kMaxSpan = 1LL << 24;
    if (a->taps < 1 || a->stride < 1 || a->dilation < 1 || a->stride >= kMaxSpan ||
        (long long)(a->taps - 1) * a->dilation >= kMaxSpan || a->offset <= -kMaxSpan ||
        a->offset >= kMaxSpan)
        return fail(CGP_EINVAL,
                    "corrconv: bad geometry (taps %d, offset %d, stride %d, dilation %d)",
                    a->taps, a->offset, a->stride, a->dilation);
    // every output row and column has a tap inside the map: the first output's last tap is
    // not before it, the last output's first tap not behind it
    const long long reach = (long long)a->offset + (long long)(a->taps - 1) * a->dilation;
    const long long last_r = (long long)(a->ho - 1) * a->stride + a->offset;
    const long long last_c = (long long)(a->wo - 1) * a->stride + a->offset;
    if (reach < 0 || last_r > a->h - 1 || last_c > a->w - 1)
        return fail(CGP_EINVAL,
                    "corrconv: output size %dx%d has rows or columns whose taps (%d from offset "
                    "%d, stride %d, dilation %d) all miss the %dx%d map", a->ho, a->wo, a->taps,
                    a->offset, a->stride, a->dilation, a->h, a->w);
    const long long ww = (long long)a->w * a->w;
    if (a->taps > 0x7fff || corr_lds_bytes<T>(1, ww, a->taps) > kMaxLds)
        return fail(CGP_EINVAL,
                    "corrconv: a %dx%d block of sums and two %dx%d tables are more than the %d "
                    "bytes of LDS a workgroup holds", a->w, a->w, a->taps, a->taps, kMaxLds);
    // many taps (a readout over the map): 1024 threads and kWideTaps offset pairs in flight
    // per element, as few row pairs exist; else 256 threads with 8 elements each
    const bool wide = a->taps >= 8;
    const int block = wide ? 1024 : 256;
    CorrP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.out = static_cast<T*>(a->out);
    p.rr = static_cast<const T*>(a->corr_rows);
    p.rc = static_cast<const T*>(a->corr_cols);
    p.units = (long long)a->npairs * a->ho * a->ho;
    p.h = a->h, p.w = a->w, p.ho = a->ho, p.wo = a->wo;
    p.taps = a->taps, p.off = a->offset, p.stride = a->stride, p.dil = a->dilation;
    p.weight = (T)a->weight;
    p.bias = (T)a->bias;
    // small maps: several row pairs per workgroup, one pass of the threads' elements
    long long upb = std::max<long long>(1, (wide ? 1024 : 2048) / ww);
    upb = std::min<long long>(upb, kMaxUnits);
    // (32-bit counts of a workgroup's outputs)
    upb = std::min<long long>(upb,
                              std::max<long long>(1, (1LL << 24) / ((long long)a->wo * a->wo)));
    while (upb > 1 && corr_lds_bytes<T>(upb, ww, a->taps) > kMaxLds) --upb;
    p.upb = (int)upb;
    p.tab_offset = (int)((upb * ww * (long long)sizeof(T) + 7) / 8 * 8);
    // few outputs per workgroup (a readout's one per row pair): the lanes of a wave share
    // an output's window.  A function of the geometry alone, like everything above
    const long long outs = upb * a->wo * a->wo, ntri = (long long)a->taps * (a->taps + 1) / 2;
    p.lshift = 0;
    while ((2 << p.lshift) <= 64 && outs * (2 << p.lshift) <= block &&
           (4LL << p.lshift) <= ntri)
        ++p.lshift;
    p.dww = make_fastdiv((unsigned)ww);
    p.dwowo = make_fastdiv((unsigned)(a->wo * a->wo));
    p.dwo = make_fastdiv((unsigned)a->wo);
    const long long blocks = (p.units + upb - 1) / upb;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "corrconv: %lld row pairs", p.units);
    const size_t lds = (size_t)corr_lds_bytes<T>(upb, ww, a->taps);
    hipStream_t s = as_stream(stream);
    // 16-byte loads where every block starts on a 16-byte boundary
    constexpr int kVec = 16 / (int)sizeof(T);
    if (wide && ww % kVec == 0 && reinterpret_cast<uintptr_t>(a->in) % 16 == 0)
        hipLaunchKernelGGL((cov_corrconv_kernel<T, 1024, 1, kWideTaps, kVec>),
                           dim3((unsigned)blocks), dim3(1024), lds, s, p);
    else if (wide)
        hipLaunchKernelGGL((cov_corrconv_kernel<T, 1024, 1, kWideTaps, 1>),
                           dim3((unsigned)blocks), dim3(1024), lds, s, p);
    else
        hipLaunchKernelGGL((cov_corrconv_kernel<T, 256, 8, 1, 1>), dim3((unsigned)blocks),
                           dim3(256), lds, s, p);
    return check_launch("cov_corrconv_kernel");
}

}  // namespace

extern "C" {

size_t cgp_corrconv_args_size(void) { return sizeof(cgp_corrconv_args); }
int cgp_corrconv_f64(const cgp_corrconv_args* args, void* stream) {
    return corrconv_impl<double>(args, stream);
}
int cgp_corrconv_f32(const cgp_corrconv_args* args, void* stream) {
    return corrconv_impl<float>(args, stream);
}

}  // extern "C"
