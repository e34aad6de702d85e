// tapconv.hip — a conv whose taps carry individual weights (include/cnngp.h "cgp_tapconv_*",
// DESIGN.md §3.10): Conv2d.propagate with a kernel buffer that is not the constant box.
//
//   out[m][oh][ow] = ( Σ_a p_a ) + bias [+ addend],
//   p_a = Σ_b table[a][b] · in[m][oh·s + off + a·d][ow·s + off + b·d]
//
// on the layer path's maps (tapconv_kernel) and, with p and q moved by the same tap, on
// position-pair maps (tapconv_cov_kernel).  Unlike the box stencil it has no separable window
// sums: an output costs extent² multiply-adds.  The order of an output's arithmetic is the
// header's and depends on the geometry alone: every product rounded, p_a summed left to
// right, the p_a added top to bottom, then bias, then the addend.  A sum that starts from
// T(0) equals the one that starts from its first term (0 + x == x), and taps whose weights are
// exactly zero may be skipped: for finite inputs neither changes a value.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "cnngp.h"
#include "cgp_common.h"

using namespace cgp;

namespace {

constexpr int kBlock = 256;                   // 4 waves of 64
constexpr int kE = 8;                         // loads in flight per thread while staging
constexpr int kMaxLds = 64 * 1024;            // bytes of LDS one workgroup may take
constexpr int kStage = 4096;                  // elements a layer-path workgroup aims to stage
constexpr int kMaxMaps = 64;                  // whole maps of one chunk
constexpr int kMaxGrid = 1 << 16;             // workgroups of the default grid
constexpr int kMaxUnits = 256;                // row pairs one position-pair workgroup may hold
constexpr int kMaxBlocks = 1024;              // blocks (row pairs x taps) it may stage

// ----------------------------------------------------------------------------------
// Layer path.  A workgroup walks chunks of `mpb` whole maps (chunk c, c + grid, ...).  It
// stages each map with the zero border its taps reach, hp x wp elements from row and column
// `off` of the map, so no tap is tested against the map's edge: an output reads
// lds[(oh·s + a·d)·wp + ow·s + b·d].  Where a map has at least a wave of outputs a thread
// owns an output; below that 1 << lshift lanes share one, lane l taking the tap rows l,
// l + lanes, ..., and after a barrier one lane adds the p_a top to bottom.  The table is read
// through wave-uniform loads (tap_row).
// ----------------------------------------------------------------------------------
template <typename T>
struct TapP {
    const T* in;
    T* out;
    const T* addend;
    long long nmaps, chunks;
    FastDiv dpad, dwp, dhowo, dwo;
    int h, w, ho, wo, ke, off, stride, dil, hp, wp, mpb, lshift;
    int pa_offset;             // byte offset of the split rows' p_a behind the maps in LDS
    T bias;
};

// p_a of tap row `trow` over the staged row `row`.  The weights (wave-uniform loads) and the
// staged values of up to kGroup taps are fetched before the first multiply, so their
// latencies overlap; a group whose weights are all zero is skipped (the zero first row of an
// even "same" kernel), a single zero weight inside a group is multiplied like any other.
// KE > 0: the extent at compile time, one group per row, fully unrolled; KE = 0: p.ke at run
// time in groups of kGroup (a slot behind the row's end reads the row's last tap and counts as
// 0 · 0).  Either way the products are added left to right.
constexpr int kGroup = 8;
constexpr int kMaxFixed = 7;                  // extents with an instantiation of their own

template <typename T, int KE>
__device__ __forceinline__ T tap_row(const T* __restrict__ trow, const T* row, int ke, int dil) {
    T pa = T(0);
    if constexpr (KE > 0) {
        T wv[KE], t[KE];
        bool any = false;
#pragma unroll
        for (int i = 0; i < KE; ++i) {
            wv[i] = trow[i];
            any |= wv[i] != T(0);
        }
        if (any) {
#pragma unroll
            for (int i = 0; i < KE; ++i) t[i] = row[i * dil];
#pragma unroll
            for (int i = 0; i < KE; ++i) pa = pa + wv[i] * t[i];
        }
    } else {
        for (int b0 = 0; b0 < ke; b0 += kGroup) {
            T wv[kGroup], t[kGroup];
            bool any = false;
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const bool on = b0 + i < ke;
                wv[i] = on ? trow[on ? b0 + i : 0] : T(0);
                any |= wv[i] != T(0);
            }
            if (any) {
#pragma unroll
                for (int i = 0; i < kGroup; ++i) {
                    const bool on = b0 + i < ke;
                    const T v = row[(on ? b0 + i : ke - 1) * dil];
                    t[i] = on ? v : T(0);
                }
#pragma unroll
                for (int i = 0; i < kGroup; ++i)
                    if (b0 + i < ke) pa = pa + wv[i] * t[i];
            }
        }
    }
    return pa;
}

template <typename T, bool ADD, int KE>
__global__ __launch_bounds__(kBlock) void tapconv_kernel(const TapP<T> p,
                                                         const T* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds = reinterpret_cast<T*>(smem);
    T* s_pa = reinterpret_cast<T*>(smem + p.pa_offset);
    const int tid = threadIdx.x;
    const int pad = p.hp * p.wp, hw = p.h * p.w, howo = p.ho * p.wo;
    for (long long c = blockIdx.x; c < p.chunks; c += gridDim.x) {
        const long long m0 = c * p.mpb;
        const long long mrem = p.nmaps - m0;
        const int nm = mrem < p.mpb ? (int)mrem : p.mpb;
        const T* src = p.in + m0 * hw;

        // ---- stage: nm maps with their zero border, kE loads in flight per thread ----
        const int total = nm * pad;
        for (int e0 = tid; e0 < total; e0 += kE * kBlock) {
            T v[kE];
#pragma unroll
            for (int k = 0; k < kE; ++k) {
                const int e = e0 + k * kBlock;
                v[k] = T(0);
                if (e < total) {
                    const unsigned ml = fdiv((unsigned)e, p.dpad);
                    const unsigned r = (unsigned)e - ml * (unsigned)pad;
                    const unsigned rr = fdiv(r, p.dwp);
                    const int ir = (int)rr + p.off, ic = (int)(r - rr * (unsigned)p.wp) + p.off;
                    if ((unsigned)ir < (unsigned)p.h && (unsigned)ic < (unsigned)p.w)
                        v[k] = src[(long long)ml * hw + ir * p.w + ic];
                }
            }
#pragma unroll
            for (int k = 0; k < kE; ++k) {
                const int e = e0 + k * kBlock;
                if (e < total) lds[e] = v[k];
            }
        }
        __syncthreads();

        const int nout = nm * howo;
        if (p.lshift == 0) {
            // ---- one thread per output ----
            for (int e = tid; e < nout; e += kBlock) {
                const unsigned ml = fdiv((unsigned)e, p.dhowo);
                const unsigned o = (unsigned)e - ml * (unsigned)howo;
                const unsigned oh = fdiv(o, p.dwo);
                const int ow = (int)(o - oh * (unsigned)p.wo);
                const T* base = lds + (int)ml * pad + (int)oh * p.stride * p.wp + ow * p.stride;
                T acc = T(0);
                if constexpr (KE > 0) {
#pragma unroll
                    for (int a = 0; a < KE; ++a)
                        acc = acc +
                              tap_row<T, KE>(tab + a * KE, base + a * p.dil * p.wp, KE, p.dil);
                } else {
                    for (int a = 0; a < p.ke; ++a)
                        acc = acc + tap_row<T, 0>(tab + a * p.ke, base + a * p.dil * p.wp, p.ke,
                                                  p.dil);
                }
                T val = acc + p.bias;
                const long long oe = m0 * howo + e;
                if constexpr (ADD) val = val + p.addend[oe];
                p.out[oe] = val;
            }
        } else {
            // ---- the tap rows of an output over 1 << lshift lanes, then top to bottom ----
            const int lanes = 1 << p.lshift;
            const int sub = tid & (lanes - 1);
            const int items = nout << p.lshift;
            for (int it = tid; it < items; it += kBlock) {
                const int e = it >> p.lshift;
                const unsigned ml = fdiv((unsigned)e, p.dhowo);
                const unsigned o = (unsigned)e - ml * (unsigned)howo;
                const unsigned oh = fdiv(o, p.dwo);
                const int ow = (int)(o - oh * (unsigned)p.wo);
                const T* base = lds + (int)ml * pad + (int)oh * p.stride * p.wp + ow * p.stride;
                for (int a = sub; a < p.ke; a += lanes)
                    s_pa[e * p.ke + a] =
                        tap_row<T, KE>(tab + a * p.ke, base + a * p.dil * p.wp, p.ke, p.dil);
            }
            __syncthreads();
            for (int e = tid; e < nout; e += kBlock) {
                T acc = T(0);
                for (int a = 0; a < p.ke; ++a) acc = acc + s_pa[e * p.ke + a];
                T val = acc + p.bias;
                const long long oe = m0 * howo + e;
                if constexpr (ADD) val = val + p.addend[oe];
                p.out[oe] = val;
            }
        }
        __syncthreads();       // the next chunk's staging overwrites the maps
    }
}

// the checks both entry points share; 0 or the code fail() returned
int check_geometry(const char* who, int h, int w, int ho, int wo, int extent, int offset,
                   int stride, int dilation) {
    // 32-bit row and column arithmetic: offset, stride and the taps' span stay below 2^24
    constexpr long long kMaxSpan = 1LL << 24;
    if (extent < 1 || stride < 1 || dilation < 1 || stride >= kMaxSpan ||
        (long long)(extent - 1) * dilation >= kMaxSpan || offset <= -kMaxSpan ||
        offset >= kMaxSpan)
        return fail(CGP_EINVAL, "%s: bad geometry (extent %d, offset %d, stride %d, dilation %d)",
                    who, extent, offset, stride, dilation);
    // F.conv2d's output size with padding = -offset
    const long long span = (long long)(extent - 1) * dilation;
    const long long nh = (long long)h - 2LL * offset - span - 1;
    const long long nw = (long long)w - 2LL * offset - span - 1;
    if (nh < 0 || nw < 0 || ho != nh / stride + 1 || wo != nw / stride + 1)
        return fail(CGP_EINVAL,
                    "%s: output size %dx%d is inconsistent with a %dx%d map (extent %d, offset "
                    "%d, stride %d, dilation %d)", who, ho, wo, h, w, extent, offset, stride,
                    dilation);
    // every output row and column has a tap inside the map: the first output's last tap is
    // not before it, the last output's first tap not behind it
    const long long reach = (long long)offset + span;
    const long long last_r = (long long)(ho - 1) * stride + offset;
    const long long last_c = (long long)(wo - 1) * stride + offset;
    if (reach < 0 || last_r > h - 1 || last_c > w - 1)
        return fail(CGP_EINVAL,
                    "%s: output size %dx%d has rows or columns whose taps (%d from offset %d, "
                    "stride %d, dilation %d) all miss the %dx%d map", who, ho, wo, extent, offset,
                    stride, dilation, h, w);
    return 0;
}

// bytes of LDS for `mpb` staged maps of `pad` elements and, with split rows, their p_a
template <typename T>
long long tap_lds_bytes(long long mpb, long long pad, long long howo, long long ke, bool split) {
    const long long maps = (mpb * pad * (long long)sizeof(T) + 7) / 8 * 8;
    return maps + (split ? mpb * howo * ke * (long long)sizeof(T) : 0);
}

template <typename T>
int tapconv_impl(const cgp_tapconv_args* a, void* stream) {
    if (!a || !a->in || !a->out || !a->table) return fail(CGP_EINVAL, "tapconv: NULL argument");
    if (a->in == a->out) return fail(CGP_EINVAL, "tapconv: out must not be in");
    constexpr long long kMaxMapElems = 1LL << 24;
    if (a->nmaps <= 0 || a->nmaps >= (1LL << 40) || a->h <= 0 || a->w <= 0 || a->ho <= 0 ||
        a->wo <= 0 || (long long)a->h * a->w > kMaxMapElems ||
        (long long)a->ho * a->wo > kMaxMapElems)
        return fail(CGP_EINVAL, "tapconv: bad sizes");
    if (a->max_groups < 0)
        return fail(CGP_EINVAL, "tapconv: max_groups %d is negative", a->max_groups);
    if (const int rc = check_geometry("tapconv", a->h, a->w, a->ho, a->wo, a->extent, a->offset,
                                      a->stride, a->dilation))
        return rc;
    const long long span = (long long)(a->extent - 1) * a->dilation;
    const long long hp = (long long)(a->ho - 1) * a->stride + span + 1;
    const long long wp = (long long)(a->wo - 1) * a->stride + span + 1;
    const long long pad = hp * wp, howo = (long long)a->ho * a->wo;
    // fewer than a wave of outputs per map: the lanes of a wave share an output's tap rows.
    // A function of the geometry alone, like everything below
    int lshift = 0;
    while (howo * (2 << lshift) <= 64 && (1 << lshift) < a->extent) ++lshift;
    const bool split = lshift > 0;
    if (hp > kMaxMapElems || wp > kMaxMapElems || a->extent > 0x7fff ||
        tap_lds_bytes<T>(1, pad, howo, a->extent, split) > kMaxLds)
        return fail(CGP_EINVAL,
                    "tapconv: a %dx%d map staged with its border (%lldx%lld elements, %d taps a "
                    "side) is more than the %d bytes of LDS a workgroup holds", a->h, a->w, hp, wp,
                    a->extent, kMaxLds);
    long long mpb = std::max<long long>(1, kStage / pad);
    mpb = std::min<long long>(mpb, kMaxMaps);
    while (mpb > 1 && tap_lds_bytes<T>(mpb, pad, howo, a->extent, split) > kMaxLds) --mpb;
    TapP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.out = static_cast<T*>(a->out);
    p.addend = static_cast<const T*>(a->addend);
    p.nmaps = a->nmaps;
    p.chunks = (a->nmaps + mpb - 1) / mpb;
    p.h = a->h, p.w = a->w, p.ho = a->ho, p.wo = a->wo;
    p.ke = a->extent, p.off = a->offset, p.stride = a->stride, p.dil = a->dilation;
    p.hp = (int)hp, p.wp = (int)wp, p.mpb = (int)mpb, p.lshift = lshift;
    p.pa_offset = (int)((mpb * pad * (long long)sizeof(T) + 7) / 8 * 8);
    p.bias = (T)a->bias;
    p.dpad = make_fastdiv((unsigned)pad);
    p.dwp = make_fastdiv((unsigned)wp);
    p.dhowo = make_fastdiv((unsigned)howo);
    p.dwo = make_fastdiv((unsigned)a->wo);
    long long grid = std::min<long long>(p.chunks, kMaxGrid);
    if (a->max_groups > 0) grid = std::min<long long>(grid, a->max_groups);
    const size_t lds = (size_t)tap_lds_bytes<T>(mpb, pad, howo, a->extent, split);
    const T* tab = static_cast<const T*>(a->table);
    hipStream_t s = as_stream(stream);
    const dim3 g((unsigned)grid), b(kBlock);
    const bool add = a->addend != nullptr;
#define CGP_TAP_LAUNCH(KE)                                                          \
    if (add)                                                                        \
        hipLaunchKernelGGL((tapconv_kernel<T, true, KE>), g, b, lds, s, p, tab);    \
    else                                                                            \
        hipLaunchKernelGGL((tapconv_kernel<T, false, KE>), g, b, lds, s, p, tab)
    // the extent at compile time up to kMaxFixed; the arithmetic of an output is the same
    // in every instantiation
    static_assert(kMaxFixed == 7, "one case per fixed extent");
    switch (a->extent) {
        case 1: CGP_TAP_LAUNCH(1); break;
        case 2: CGP_TAP_LAUNCH(2); break;
        case 3: CGP_TAP_LAUNCH(3); break;
        case 4: CGP_TAP_LAUNCH(4); break;
        case 5: CGP_TAP_LAUNCH(5); break;
        case 6: CGP_TAP_LAUNCH(6); break;
        case 7: CGP_TAP_LAUNCH(7); break;
        default: CGP_TAP_LAUNCH(0); break;
    }
#undef CGP_TAP_LAUNCH
    return check_launch("tapconv_kernel");
}

// ----------------------------------------------------------------------------------
// Position-pair maps: cov_conv_kernel's shape (covpool.hip).  A workgroup owns `upb` output
// row pairs (P, Q) of consecutive pairs, stages the `extent` input blocks
// (P·s + off + a·d, Q·s + off + a·d) of each, contiguous w×w ranges, in LDS (zeros where a row
// leaves the map), then every output takes its weighted diagonal windows from LDS in the
// layer kernel's order.
// ----------------------------------------------------------------------------------
template <typename T>
struct TapCovP {
    const T* in;
    T* out;
    const T* addend;
    long long units;           // npairs·ho·ho row pairs
    FastDiv dww, dwowo, dwo;
    int h, w, ho, wo, ke, off, stride, dil, upb;
    int tab_offset;            // byte offset of the blocks' element offsets in LDS
    T bias;
};

template <typename T, bool ADD>
__global__ __launch_bounds__(kBlock) void tapconv_cov_kernel(const TapCovP<T> p,
                                                             const T* __restrict__ tab) {
    // dynamic LDS: the staged blocks [upb][extent][w·w], then each block's element offset in
    // `in` (-1: a row outside the map)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* lds = reinterpret_cast<T*>(smem);
    long long* s_base = reinterpret_cast<long long*>(smem + p.tab_offset);
    const int tid = threadIdx.x;
    const long long u0 = (long long)blockIdx.x * p.upb;
    const long long urem = p.units - u0;
    const int nu = urem < p.upb ? (int)urem : p.upb;
    const int ww = p.w * p.w, wowo = p.wo * p.wo, hoho = p.ho * p.ho;
    const int per = p.ke * ww;
    for (int b = tid; b < nu * p.ke; b += kBlock) {
        const int ul = b / p.ke, a = b - ul * p.ke;
        const long long u = u0 + ul;
        const long long m = u / hoho;
        const int r = (int)(u - m * hoho);
        const int pr = r / p.ho, qr = r - pr * p.ho;
        const int ir = pr * p.stride + p.off + a * p.dil;
        const int jr = qr * p.stride + p.off + a * p.dil;
        const bool in = (unsigned)ir < (unsigned)p.h && (unsigned)jr < (unsigned)p.h;
        s_base[b] = in ? ((m * p.h + ir) * p.h + jr) * ww : -1;
    }
    __syncthreads();

    // ---- stage: the blocks of every row pair, kE loads in flight per thread ----
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

    // ---- weighted windows, bias, addend, store ----
    for (int e = tid; e < nu * wowo; e += kBlock) {
        const unsigned ul = fdiv((unsigned)e, p.dwowo);
        const int o = e - (int)ul * wowo;
        const unsigned pc = fdiv((unsigned)o, p.dwo);
        const int qc = o - (int)pc * p.wo;
        const int c0 = (int)pc * p.stride + p.off, d0 = qc * p.stride + p.off;
        const T* blk = lds + (int)ul * per;
        T acc = T(0);
        for (int a = 0; a < p.ke; ++a) {
            const T* trow = tab + a * p.ke;
            T pa = T(0);
            for (int b = 0; b < p.ke; ++b) {
                const T wv = trow[b];
                if (wv == T(0)) continue;
                const int ic = c0 + b * p.dil, jc = d0 + b * p.dil;
                T t = T(0);
                if ((unsigned)ic < (unsigned)p.w && (unsigned)jc < (unsigned)p.w)
                    t = blk[a * ww + ic * p.w + jc];
                pa = pa + wv * t;
            }
            acc = acc + pa;
        }
        T val = acc + p.bias;
        const long long oe = (u0 + ul) * wowo + o;
        if constexpr (ADD) val = val + p.addend[oe];
        p.out[oe] = val;
    }
}

template <typename T>
int tapconv_cov_impl(const cgp_tapconv_cov_args* a, void* stream) {
    if (!a || !a->in || !a->out || !a->table)
        return fail(CGP_EINVAL, "tapconv_cov: NULL argument");
    if (a->in == a->out) return fail(CGP_EINVAL, "tapconv_cov: out must not be in");
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || bad_map(a->h, a->w) ||
        bad_map(a->ho, a->wo))
        return fail(CGP_EINVAL, "tapconv_cov: bad sizes");
    if (const int rc = check_geometry("tapconv_cov", a->h, a->w, a->ho, a->wo, a->extent,
                                      a->offset, a->stride, a->dilation))
        return rc;
    const long long per = (long long)a->extent * a->w * a->w;
    // one row pair's blocks and their element offsets
    const long long unit_bytes = per * (long long)sizeof(T) + 8LL * a->extent;
    if (unit_bytes + 8 > kMaxLds || a->extent > kMaxBlocks)
        return fail(CGP_EINVAL,
                    "tapconv_cov: %d taps of a %dx%d block are %lld bytes, more than the %d of "
                    "LDS a workgroup stages", a->extent, a->w, a->w,
                    per * (long long)sizeof(T), kMaxLds);
    TapCovP<T> p;
    p.in = static_cast<const T*>(a->in);
    p.out = static_cast<T*>(a->out);
    p.addend = static_cast<const T*>(a->addend);
    p.units = (long long)a->npairs * a->ho * a->ho;
    p.h = a->h, p.w = a->w, p.ho = a->ho, p.wo = a->wo;
    p.ke = a->extent, p.off = a->offset, p.stride = a->stride, p.dil = a->dilation;
    p.bias = (T)a->bias;
    // small maps: several row pairs per workgroup, about 1024 staged or written elements
    const long long big = std::max<long long>((long long)a->w * a->w, (long long)a->wo * a->wo);
    long long upb = std::max<long long>(1, 1024 / big);
    upb = std::min<long long>(upb, kMaxUnits);
    upb = std::min<long long>(upb, kMaxBlocks / a->extent);
    upb = std::min<long long>(upb, (kMaxLds - 8) / unit_bytes);
    p.upb = (int)upb;
    p.tab_offset = (int)((upb * per * (long long)sizeof(T) + 7) / 8 * 8);
    p.dww = make_fastdiv((unsigned)(a->w * a->w));
    p.dwowo = make_fastdiv((unsigned)(a->wo * a->wo));
    p.dwo = make_fastdiv((unsigned)a->wo);
    const long long blocks = (p.units + upb - 1) / upb;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "tapconv_cov: %lld row pairs", p.units);
    const size_t lds = (size_t)p.tab_offset + (size_t)upb * 8 * a->extent;
    const T* tab = static_cast<const T*>(a->table);
    hipStream_t s = as_stream(stream);
    if (a->addend)
        hipLaunchKernelGGL((tapconv_cov_kernel<T, true>), dim3((unsigned)blocks), dim3(kBlock),
                           lds, s, p, tab);
    else
        hipLaunchKernelGGL((tapconv_cov_kernel<T, false>), dim3((unsigned)blocks), dim3(kBlock),
                           lds, s, p, tab);
    return check_launch("tapconv_cov_kernel");
}

}  // namespace

extern "C" {

size_t cgp_tapconv_args_size(void) { return sizeof(cgp_tapconv_args); }
int cgp_tapconv_f64(const cgp_tapconv_args* args, void* stream) {
    return tapconv_impl<double>(args, stream);
}
int cgp_tapconv_f32(const cgp_tapconv_args* args, void* stream) {
    return tapconv_impl<float>(args, stream);
}
size_t cgp_tapconv_cov_args_size(void) { return sizeof(cgp_tapconv_cov_args); }
int cgp_tapconv_cov_f64(const cgp_tapconv_cov_args* args, void* stream) {
    return tapconv_cov_impl<double>(args, stream);
}
int cgp_tapconv_cov_f32(const cgp_tapconv_cov_args* args, void* stream) {
    return tapconv_cov_impl<float>(args, stream);
}

}  // extern "C"
