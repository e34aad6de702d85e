// covntk.hip — the neural tangent kernel on position-pair maps (include/cnngp.h "The NTK on
// position-pair maps"): a second map Θ[p, q] beside S[p, q] of covpool.hip,
// in the same layout [pair][p_row][q_row][p_col][q_col] and with the same conventions (pairs
// as device index arrays, a fixed summation order, no atomics, a pair's result a function of
// that pair's data alone).
//
// Every linear op of the forward run serves Θ unchanged.  The two steps that do not are here:
//   cgp_covntk_nonlin_*   K' = map(K) [+ addend] and Θ' = Θ·κ̇ [+ addend] in one pass
//   cgp_covntk_conv_*     K' = A(K) + b and Θ' = A(Θ) + K' from one staging of both streams,
//                          optionally followed by the nonlinearity step on (K', Θ')
// The forward values are the bits of cgp_cov_nonlin_* / cgp_gelu_cov_* / cgp_cov_conv_*: the
// same device functions in the same order.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "cnngp.h"
#include "nonlin_walk.h"

using namespace cgp;

namespace {

constexpr int kBlock = 256;                   // 4 waves of 64
constexpr int kChunk = 2048;                  // elements of one elementwise workgroup
constexpr int kE = kChunk / kBlock;           // loads in flight per thread and stream (8)
constexpr int kMaxUnits = 256;                // row pairs one conv workgroup may hold
constexpr int kMaxBlocks = 1024;              // blocks (row pairs x taps) of one stream it may stage
constexpr int kMaxLds = 64 * 1024;            // bytes of LDS one conv workgroup may take

bool is_nonlin(int kind) {
    return kind == CGP_COV_RELU || kind == CGP_COV_ERF || kind == CGP_COV_GELU;
}

// ----------------------------------------------------------------------------------
// the two-stream conv: cov_conv_kernel with the `taps` blocks of K and, with TH, of Θ staged
// for the workgroup's row pairs (the Θ blocks after all K blocks), both streams' loads of a
// pass in flight together.  Per output, in cov_conv_kernel's order (column taps, then row
// taps, left to right):
//     k' = weight·A(K) + bias
//     t' = (weight·A(Θ) + 0) + k'      cgp_cov_conv_* on Θ with bias 0 and addend k', its
//                                      roundings one by one; without TH (Θ = 0): t' = k'
// then the nonlinearity step on (k', t') with a post-stage, then the addends.
// ----------------------------------------------------------------------------------
template <typename T>
struct CovConvNtkP {
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
    long long units;           // npairs·ho·ho row pairs
    FastDiv dww, dwowo, dwo;
    int h, w, ho, wo, taps, off, stride, dil, upb, post, same, exact;
    int tab_offset;            // byte offset of the index tables in LDS
    T weight, bias;
};

template <typename T, bool TH>
__global__ __launch_bounds__(kBlock) void cov_conv_ntk_kernel(const CovConvNtkP<T> p) {
    // dynamic LDS: K's staged blocks [upb][taps][w·w], with TH Θ's likewise, then each
    // block's element offset in `in` / `theta` (-1: a row outside the map) and each row
    // pair's (pair, p_row, q_row)
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
    T* ldt = lds + p.upb * per;
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

    // ---- stage: the taps input blocks of every row pair, kE loads in flight per thread
    // and stream ----
    const int total = nu * per;
    for (int e0 = tid; e0 < total; e0 += kE * kBlock) {
        T v[kE], t[TH ? kE : 1];
#pragma unroll
        for (int k = 0; k < kE; ++k) {
            const int e = e0 + k * kBlock;
            v[k] = T(0);
            if constexpr (TH) t[k] = T(0);
            if (e < total) {
                const unsigned blk = fdiv((unsigned)e, p.dww);
                const long long base = s_base[blk];
                if (base >= 0) {
                    const long long o = base + (e - (int)blk * ww);
                    v[k] = p.in[o];
                    if constexpr (TH) t[k] = p.theta[o];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kE; ++k) {
            const int e = e0 + k * kBlock;
            if (e < total) {
                lds[e] = v[k];
                if constexpr (TH) ldt[e] = t[k];
            }
        }
    }
    __syncthreads();

    // ---- window sums of both streams, affine, nonlinearity step, addends, store ----
    for (int e = tid; e < nu * wowo; e += kBlock) {
        const unsigned ul = fdiv((unsigned)e, p.dwowo);
        const int o = e - (int)ul * wowo;
        const unsigned pc = fdiv((unsigned)o, p.dwo);
        const int qc = o - (int)pc * p.wo;
        const int c0 = (int)pc * p.stride + p.off, d0 = qc * p.stride + p.off;
        const T* blk = lds + (int)ul * per;
        const T* blt = ldt + (int)ul * per;
        T acc = T(0), tacc = T(0);
        for (int a = 0; a < p.taps; ++a) {
            T rs = T(0), ts = T(0);
            for (int b = 0; b < p.taps; ++b) {
                const int ic = c0 + b * p.dil, jc = d0 + b * p.dil;
                T x = T(0), y = T(0);
                if ((unsigned)ic < (unsigned)p.w && (unsigned)jc < (unsigned)p.w) {
                    x = blk[a * ww + ic * p.w + jc];
                    if constexpr (TH) y = blt[a * ww + ic * p.w + jc];
                }
                rs = b == 0 ? x : rs + x;
                if constexpr (TH) ts = b == 0 ? y : ts + y;
            }
            acc = a == 0 ? rs : acc + rs;
            if constexpr (TH) tacc = a == 0 ? ts : tacc + ts;
        }
        T val = p.weight * acc + p.bias;
        T tval = val;
        if constexpr (TH) tval = (p.weight * tacc + T(0)) + val;
        if (p.post != CGP_COV_NONE) {
            const int m = s_m[ul];
            T kd;
            val = cov_nonlin<T, true>(val, p.post, p.xx, p.yy, p.pi[m], p.pj[m], p.ho * p.wo,
                                      s_pr[ul] * p.wo + (int)pc, s_qr[ul] * p.wo + qc, p.same,
                                      p.exact, kd);
            tval = tval * kd;
        }
        const long long oe = (u0 + ul) * wowo + o;
        if (p.addend) val = val + p.addend[oe];
        if (p.addend_theta) tval = tval + p.addend_theta[oe];
        p.out[oe] = val;
        p.out_theta[oe] = tval;
    }
}

// ----------------------------------------------------------------------------------
// host side: every check returns CGP_EINVAL before any launch
// ----------------------------------------------------------------------------------
template <typename T>
int cov_conv_ntk_impl(const cgp_covntk_conv_args* a, void* stream) {
    if (!a || !a->in || !a->out || !a->out_theta)
        return fail(CGP_EINVAL, "cov_conv_ntk: NULL argument");
    if (a->out == a->in || a->out == a->theta || a->out_theta == a->in ||
        a->out_theta == a->theta || a->out == a->out_theta)
        return fail(CGP_EINVAL, "cov_conv_ntk: out / out_theta must not be in / theta, nor "
                                "each other");
    if (a->npairs <= 0 || a->npairs >= (1LL << 31) || bad_map(a->h, a->w) ||
        bad_map(a->ho, a->wo))
        return fail(CGP_EINVAL, "cov_conv_ntk: bad sizes");
    if (a->taps <= 0 || a->stride <= 0 || a->dilation <= 0)
        return fail(CGP_EINVAL, "cov_conv_ntk: bad geometry");
    if (a->post != CGP_COV_NONE && !is_nonlin(a->post))
        return fail(CGP_EINVAL, "cov_conv_ntk: post %d is not a nonlinearity", a->post);
    if (a->post != CGP_COV_NONE && (!a->xx || !a->yy || !a->pair_i || !a->pair_j))
        return fail(CGP_EINVAL,
                    "cov_conv_ntk: a post-nonlinearity needs xx, yy and the pair lists");
    const int streams = a->theta ? 2 : 1;
    const long long per = (long long)a->taps * a->w * a->w;
    // one row pair's blocks of every staged stream and its index entries (a block offset per
    // tap, three ints)
    const long long unit_bytes = streams * per * (long long)sizeof(T) + 8LL * a->taps + 12;
    if (unit_bytes + 8 > kMaxLds || a->taps > kMaxBlocks)
        return fail(CGP_EINVAL,
                    "cov_conv_ntk: %d taps of a %dx%d block of %d stream(s) are %lld bytes, "
                    "more than the %d of LDS a workgroup stages", a->taps, a->w, a->w, streams,
                    streams * per * (long long)sizeof(T), kMaxLds);
    CovConvNtkP<T> p;
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
    p.units = (long long)a->npairs * a->ho * a->ho;
    p.h = a->h, p.w = a->w, p.ho = a->ho, p.wo = a->wo;
    p.taps = a->taps, p.off = a->offset, p.stride = a->stride, p.dil = a->dilation;
    p.post = a->post;
    p.same = a->same != 0;
    p.exact = (a->flags & CGP_FLAG_EXACT_RELU) != 0;
    p.weight = (T)a->weight;
    p.bias = (T)a->bias;
    // small maps: several row pairs per workgroup, about 1024 staged (per stream) or written
    // elements, as cgp_cov_conv_*
    const long long big = std::max<long long>((long long)a->w * a->w, (long long)a->wo * a->wo);
    long long upb = std::max<long long>(1, 1024 / big);
    upb = std::min<long long>(upb, kMaxUnits);
    upb = std::min<long long>(upb, kMaxBlocks / a->taps);
    upb = std::min<long long>(upb, (kMaxLds - 8) / unit_bytes);
    p.upb = (int)upb;
    p.tab_offset = (int)((streams * upb * per * (long long)sizeof(T) + 7) / 8 * 8);
    p.dww = make_fastdiv((unsigned)(a->w * a->w));
    p.dwowo = make_fastdiv((unsigned)(a->wo * a->wo));
    p.dwo = make_fastdiv((unsigned)a->wo);
    const long long blocks = (p.units + upb - 1) / upb;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "cov_conv_ntk: %lld row pairs", p.units);
    const size_t lds = (size_t)p.tab_offset + (size_t)upb * (8 * a->taps + 12);
    hipStream_t s = as_stream(stream);
    if (a->theta)
        hipLaunchKernelGGL((cov_conv_ntk_kernel<T, true>), dim3((unsigned)blocks), dim3(kBlock),
                           lds, s, p);
    else
        hipLaunchKernelGGL((cov_conv_ntk_kernel<T, false>), dim3((unsigned)blocks),
                           dim3(kBlock), lds, s, p);
    return check_launch("cov_conv_ntk_kernel");
}

}  // namespace

extern "C" {

size_t cgp_covntk_conv_args_size(void) { return sizeof(cgp_covntk_conv_args); }

int cgp_covntk_conv_f64(const cgp_covntk_conv_args* args, void* stream) {
    return cov_conv_ntk_impl<double>(args, stream);
}
int cgp_covntk_conv_f32(const cgp_covntk_conv_args* args, void* stream) {
    return cov_conv_ntk_impl<float>(args, stream);
}

}  // extern "C"
