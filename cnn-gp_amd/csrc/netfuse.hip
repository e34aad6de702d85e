// netfuse.hip — the whole pair program of a network in ONE kernel (cgp_net_*).
//
// The layer-by-layer path (cnngp.hip) streams every pair map through HBM once per fused
// op: ~100-500 KB of traffic per pair, so it is HBM-bound.  Here one workgroup (two
// waves) owns one (i, j) pair at a time and runs every op of the network on LDS-resident
// planes; the only global traffic per pair is the two input images and the per-image
// variance maps the ReLUs read (both shared by many pairs, so L2/MALL-resident) plus
// the one K[i, j] it writes.  The kernel is fp64-VALU bound.
//
// Reference semantics: moments kernels.py:44-47, Conv2d.propagate kernels.py:92-98,
// ReLU.propagate kernels.py:134-165, Sequential kernels.py:184-187, Sum/Mixture
// kernels.py:220-254.  The host (cnn_gp/netplan.py) lowers the module tree into a list
// of cgp_net_op over LDS slots; this file only executes the list.
//
// Per pair, per conv: a row pass writes horizontal window sums of every input row into
// the row-sum scratch `hs` ([HSR][WO]; rows outside the input are zero), then a column
// pass finishes the windows for R3 output rows per item, applies w·Σ + b, the ReLU (with
// variances prefetched before the row pass) and the residual add, and writes the output
// slot.  Geometry is compile time (one instantiation per conv shape the reference
// configs use), so every LDS offset inside a pass is an immediate.

#include "cgp_common.h"


#include <map>
#include <mutex>
#include <utility>
#include <algorithm>
#include <climits>

using namespace cgp;

namespace {

constexpr int kNT = 128;  // threads per workgroup (one pair): two waves
// threads of a workgroup carrying NP pairs: NP == 2 is two one-pair halves on four waves
// (units u and u + 1, the same image i: the i-side variance loads of the halves meet in
// L1 and each barrier serves both pairs; net_kernel); the small-map stages pack 4 / 16
// pairs on two waves.  Ops only ever run on one half (NP = 1) or on NP = 4 / 16.  (Four
// one-pair slices on 512 threads measured -15% fp64: LDS then admits 2 workgroups per CU.)
constexpr int kSplit = 2;
template <int NP>
constexpr int kNTof = NP == 2 ? kSplit * kNT : kNT;
// pair units a workgroup takes per step of the walk
template <int NP>
constexpr int kUnitsOf = NP == 2 ? kSplit : NP;
constexpr int kSTL = 3;             // log2(kST) (16² / 32² supertiles measured ±0.7%)
constexpr int kST = 1 << kSTL;      // supertile edge: pairs are walked in 8x8 (i, j) blocks
constexpr int kEw = 4;          // elementwise ops: pixels per thread per pass

// R | len outputs per item, chosen to minimise rounds·(per-item cost) with ≤ 8 outputs
// (register budget); ties go to the larger R (fewer LDS reads per output).
constexpr int pick_r(int lines, int len, int taps, int s, int epi, int nt) {
    int best = 1;
    long long best_cost = LLONG_MAX;
    for (int r = 1; r <= 8 && r <= len; ++r) {
        if (len % r) continue;
        const int items = lines * (len / r);
        const int rounds = (items + nt - 1) / nt;
        const long long cost = (long long)rounds * (epi * r + (r - 1) * s + taps);
        if (cost < best_cost || (cost == best_cost && r > best)) {
            best = r;
            best_cost = cost;
        }
    }
    return best;
}

// NP_: pairs per workgroup (their items share the passes; per-pair counts below)
template <int H_, int W_, int HO_, int WO_, int TAPS_, int S_, int OFF_, int NP_ = 1>
struct NG {
    static constexpr int H = H_, W = W_, HO = HO_, WO = WO_, TAPS = TAPS_, S = S_, OFF = OFF_;
    static constexpr int NP = NP_;
    static constexpr int NT = kNT;
    static_assert(NP_ != 2, "two-pair workgroups run their ops as one-pair halves");
    static constexpr int HW = H * W, HOWO = HO * WO;
    static constexpr bool POINT = TAPS == 1 && OFF == 0;
    static constexpr bool REDUCE = HO == 1 && WO == 1 && OFF == 0 && TAPS == H && TAPS == W;
    static constexpr int HSR = (HO - 1) * S + TAPS;           // hs rows; row q <-> input q+OFF
    static constexpr int Q0 = OFF < 0 ? -OFF : 0;              // first hs row backed by input
    static constexpr int Q1 = HSR < H - OFF ? HSR : H - OFF;   // one past the last
    static constexpr int NVR = Q1 - Q0;                        // input rows the row pass reads
    static constexpr int R2 = pick_r(NVR * NP, WO, TAPS, S, 2, NT);
    static constexpr int R3 = pick_r(WO * NP, HO, TAPS, S, 8, NT);
    static constexpr int WIN2 = (R2 - 1) * S + TAPS, WIN3 = (R3 - 1) * S + TAPS;
    static constexpr int NG2 = WO / R2, NH = NVR * NG2, KH = (NP * NH + NT - 1) / NT;
    static constexpr int NG3 = HO / R3, NV = NG3 * WO, KV = (NP * NV + NT - 1) / NT;
    static constexpr int NZ = (HSR - NVR) * WO;                // zero cells of hs
    // windows of at most 3 taps (the ResNets' 3x3 convs) run in one pass straight from the
    // source slot: no row-sum scratch, so a smaller arena
    static constexpr bool DIRECT = !POINT && !REDUCE && TAPS <= 3;
    static constexpr int HS_ELEMS = (POINT || REDUCE || DIRECT) ? 2 : HSR * WO;
};

// The fused kernel's conv shapes: (H, W, HO, WO, taps, stride, offset) — every conv of the
// reference configs plus their CIFAR-size analogues.
#define CGP_NET_GEOMETRIES(X)          \
    X(28, 28, 28, 28, 7, 1, -3)        \
    X(28, 28, 28, 28, 4, 1, -1)        \
    X(28, 28, 28, 28, 3, 1, -1)        \
    X(28, 28, 28, 28, 1, 1, 0)         \
    X(28, 28, 14, 14, 3, 2, -1)        \
    X(28, 28, 14, 14, 1, 2, 0)         \
    X(28, 28, 1, 1, 28, 1, 0)          \
    X(14, 14, 14, 14, 3, 1, -1)        \
    X(14, 14, 7, 7, 3, 2, -1)          \
    X(14, 14, 7, 7, 1, 2, 0)           \
    X(7, 7, 7, 7, 3, 1, -1)            \
    X(7, 7, 1, 1, 7, 1, 0)             \
    X(1, 1, 1, 1, 1, 1, 0)             \
    X(32, 32, 32, 32, 3, 1, -1)        \
    X(32, 32, 32, 32, 1, 1, 0)         \
    X(32, 32, 16, 16, 3, 2, -1)        \
    X(32, 32, 16, 16, 1, 2, 0)         \
    X(16, 16, 16, 16, 3, 1, -1)        \
    X(16, 16, 8, 8, 3, 2, -1)          \
    X(16, 16, 8, 8, 1, 2, 0)           \
    X(8, 8, 8, 8, 3, 1, -1)            \
    X(8, 8, 1, 1, 8, 1, 0)             \
    X(14, 14, 1, 1, 14, 1, 0)          \
    X(16, 16, 1, 1, 16, 1, 0)          \
    X(32, 32, 1, 1, 32, 1, 0)

struct GeoRow {
    int h, w, ho, wo, taps, s, off, hs_elems;
};
#define CGP_NET_ROW(h, w, ho, wo, k, s, o) {h, w, ho, wo, k, s, o, NG<h, w, ho, wo, k, s, o>::HS_ELEMS},
constexpr GeoRow kGeoTable[] = {CGP_NET_GEOMETRIES(CGP_NET_ROW)};
#undef CGP_NET_ROW
constexpr int kNumGeo = sizeof(kGeoTable) / sizeof(kGeoTable[0]);

// out[o] = Σ_{t<TAPS} w[o·S + t], o < R.  Stride 1 with TAPS ≥ 4: outputs in groups of
// g ≤ TAPS share the common core of their windows; the suffix sums of the first window run
// through the core and the taps after it are prefix sums, so a group costs TAPS + 2g - 4
// adds instead of g(TAPS-1) (7x7: 17 per pass instead of 42).  The round-3 form kept the
// core apart (TAPS + 3g - 6: 22) and measured 2.5% slower on ConvNet GP
// (profiles/r4/ab_r4l_window_sums.log).
template <typename T, int TAPS, int O0, int G, int N, int R>
__device__ __forceinline__ void win_group(const T (&w)[N], T (&out)[R]) {
    T core = w[O0 + G - 1];
#pragma unroll
    for (int t = O0 + G; t < O0 + TAPS; ++t) core += w[t];
    if constexpr (G == 1) {
        out[O0] = core;
    } else {
        // suffix sums of the first window that end in the core, prefix sums of the taps
        // after it (van Herk / Gil-Werman): TAPS + 2G - 4 adds
        T suf[G], right[G];
        suf[G - 1] = core;
#pragma unroll
        for (int o = G - 2; o >= 0; --o) suf[o] = w[O0 + o] + suf[o + 1];
        right[1] = w[O0 + TAPS];
#pragma unroll
        for (int o = 2; o < G; ++o) right[o] = right[o - 1] + w[O0 + TAPS + o - 1];
        out[O0] = suf[0];
#pragma unroll
        for (int o = 1; o < G; ++o) out[O0 + o] = suf[o] + right[o];
    }
}

template <typename T, int TAPS, int O0, int N, int R>
__device__ __forceinline__ void win_groups(const T (&w)[N], T (&out)[R]) {
    if constexpr (O0 < R) {
        constexpr int G = (R - O0) < TAPS ? (R - O0) : TAPS;
        win_group<T, TAPS, O0, G, N, R>(w, out);
        win_groups<T, TAPS, O0 + TAPS, N, R>(w, out);
    }
}

template <typename T, int TAPS, int S, int R>
__device__ __forceinline__ void win_sums(const T (&w)[(R - 1) * S + TAPS], T (&out)[R]) {
    if constexpr (S == 1 && TAPS >= 4 && R > 1) {
        win_groups<T, TAPS, 0, (R - 1) * S + TAPS, R>(w, out);
    } else {
#pragma unroll
        for (int o = 0; o < R; ++o) {
            T acc = w[o * S];
#pragma unroll
            for (int t = 1; t < TAPS; ++t) acc += w[o * S + t];
            out[o] = acc;
        }
    }
}

// threadIdx.x through an opaque move: per-thread index math of one op is then recomputed
// inside the op instead of being hoisted out of the pair loop, where it would hold
// registers for every geometry at once (hoisted: -1% fp64, scratch spills in the head
// programs)
// (thread index within its 128-thread half: a two-pair workgroup runs one pair per half)
__device__ __forceinline__ int opaque_tid() {
    static_assert(kNT == 128, "opaque_tid masks to 128-thread halves");
    int t;
    asm volatile("v_and_b32 %0, 0x7f, %1" : "=v"(t) : "v"((int)threadIdx.x));
    return t;
}

// a / d for a >= 0 as an unsigned division (a constant d costs a mul-hi and a shift; the
// signed form needs three more fix-up ops)
__device__ __forceinline__ int udiv(int a, int d) { return (int)((unsigned)a / (unsigned)d); }

// the op table through a generic pointer: per-lane vector loads (the constant address
// space's scalar loads measured -7% on ConvNet: SMEM returns count in lgkmcnt, so every
// LDS wait also drains them)
typedef const cgp_net_op* OpsC;
__device__ __forceinline__ OpsC ops_c(const cgp_net_op* p) { return (OpsC)p; }
__device__ __forceinline__ cgp_net_op load_op(OpsC r) {
    cgp_net_op o;
    o.kind = r->kind;
    o.code = r->code;
    o.src = r->src;
    o.dst = r->dst;
    o.add = r->add;
    o.ws_in = r->ws_in;
    o.ws_out = r->ws_out;
    o.relu = r->relu;
    o.h = r->h;
    o.w = r->w;
    o.div_m = r->div_m;
    o.div_s = r->div_s;
    o.dst2 = r->dst2;
    o.zero_halo = r->zero_halo;
    o.weight = r->weight;
    o.bias = r->bias;
    o.var_x = r->var_x;
    o.var_y = r->var_y;
    o.var2_x = r->var2_x;
    o.var2_y = r->var2_y;
    return o;
}

// global-address-space views: pointers read from the op table are generic, and flat
// loads would also count in lgkmcnt, so every LDS wait would drain them
template <typename T>
using GP = const __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ GP<T> gptr(const void* p) {
    return (GP<T>)(const T*)p;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <typename T>
struct NetP {
    const T* __restrict__ x;
    const T* __restrict__ y;
    T* __restrict__ out;
    const T* __restrict__ kdiag;
    const cgp_net_op* __restrict__ ops;
    unsigned long long* work;   // per-XCD unit counters, zeroed per launch
    long long ldo, units, ubeg, uend;
    unsigned n1, n2, nbi, nbj;
    int nops, channels, hw_in, same, final_slot, hs, lds_elems, exact, final_stage, part;
};

// The pairs an op works on.  NP == 1: (i, j), uniform.  NP > 1: pair q of the group is
// (tab[q], tab[kMaxNP + q]) from the workgroup's pair table in LDS, unit u0 + q.
constexpr int kMaxNP = 16;
// LDS the kernel declares statically (pair table, SUM partials, program records, the
// work-counter slots) on top of the dynamic arenas: every LDS check (net_impl, net_wpe,
// cgp_net_static_lds for the host's planner) counts this reserve
constexpr long long kStaticLds = 1536;
struct Pairs {
    unsigned i, j;
    const unsigned* tab;
    long long u0;
    void* red;   // one-pair code: the pair's two wave partial sums (CGP_NET_CODE_SUM)
};
template <int NP>
__device__ __forceinline__ void pair_q(const Pairs& pr, int q, unsigned& iq, unsigned& jq) {
    if constexpr (NP == 1) {
        iq = pr.i;
        jq = pr.j;
    } else {
        iq = pr.tab[q];
        jq = pr.tab[kMaxNP + q];
    }
}

// EXACT (CGP_FLAG_EXACT_RELU) is a separate instantiation: a call to the out-of-line
// relu_exact would make every register live across it caller-saved
template <bool EXACT, typename T>
__device__ __forceinline__ T relu_of(T c, T v1, T v2, const PolyTab& tab) {
    if constexpr (EXACT)
        return relu_exact_inl(c, v1, v2);
    else
        return relu_fast(c, v1, v2, tab);
}
// The fp64 closed form (relu_q_n, f64 launches without CGP_FLAG_EXACT_RELU) reads the maps
// cgp_net_var_form() names in place of plain variances: 1/sqrt(v/8) on both sides (the
// one-root form, default), or v × cgp_net_xvar_scale() = v/16 on the x side and v on the y
// side (CGP_RELU_ONE_ROOT=0); and, when the producing conv scaled its weight and bias by
// 1/4 (QIN), a quartered input.  u1 / u2 below are those maps' pixels, whatever the form.
template <typename T, bool EX>
constexpr bool kQuarter = !EX && sizeof(T) == 8;

// R ReLUs in place: v[k] = relu(v[k], u1[k], u2[k]) (QIN: v holds c/4; AD: the fp64 form
// may take the range-adaptive polynomial, see relu_q_n).  The fp32 closed form keeps its
// full polynomial: its adaptive form measured neutral (the fp32 kernel is bound by its
// per-op latency chain, not by issue; profiles/r3/ab_r3f_relu_adapt_f32.log)
// NC / HF: the fp64 form's lean variants (relu_q_n NOCAP / HALF; HF needs the half-scaled
// tables in `tab`), picked per ReLU site by a compiled program (ProgLean below)
template <bool EXACT, bool QIN, typename T, int R, int AD = 0, bool NC = false, bool HF = false>
__device__ __forceinline__ void relu_n(T (&v)[R], const T (&u1)[R], const T (&u2)[R],
                                       const PolyTab& tab, unsigned long long seg = ~0ull) {
    static_assert(!(NC || HF) || (!EXACT && sizeof(T) == 8), "lean ReLU forms: fp64 closed form");
    if constexpr (EXACT) {
#pragma unroll
        for (int k = 0; k < R; ++k) v[k] = relu_exact_inl(v[k], u1[k], u2[k]);
    } else if constexpr (sizeof(T) == 8) {
        relu_q_n<R, QIN, AD, NC, HF>(v, u1, u2, tab, seg);
    } else {
        relu_fast_n<R>(v, u1, u2, tab);
    }
}

// Elementwise-op map sizes with a compile-time instantiation (cgp_net_resolution); any
// other size runs the generic runtime-size path.
#define CGP_NET_RESOLUTIONS(X) X(28, 28) X(14, 14) X(7, 7) X(32, 32) X(16, 16) X(8, 8) X(1, 1)

struct ResRow {
    int h, w;
};
#define CGP_NET_RES_ROW(h, w) {h, w},
constexpr ResRow kResTable[] = {CGP_NET_RESOLUTIONS(CGP_NET_RES_ROW)};
#undef CGP_NET_RES_ROW
constexpr int kNumRes = sizeof(kResTable) / sizeof(kResTable[0]);
constexpr int res_index(int h, int w) {
    for (int n = 0; n < kNumRes; ++n)
        if (kResTable[n].h == h && kResTable[n].w == w) return n;
    return -1;
}

// Output stage shared by every op: v (R results at LDS offsets at[k] of the dst/add
// class, variance-map pixels px[k]) -> [ReLU] -> [+ add] -> dst, and optionally
// relu(result) -> dst2 (the next block's ReLU branch input, saving a separate op).
// An op has the ReLU or dst2, never both, so one set of prefetched variances (u1, u2)
// serves either.
// NC / HF: the lean forms of the op's own ReLU (an HF op has no dst2, so the half-scaled
// tables in `tab` never reach the dst2 ReLU).
template <typename T, bool EX, bool DU, int R, int AD = 0, bool NC = false, bool HF = false>
__device__ __forceinline__ void net_out(T* __restrict__ lds, const cgp_net_op& op, T (&v)[R],
                                        const int (&at)[R], const bool (&ok)[R],
                                        const T (&u1)[R], const T (&u2)[R],
                                        const PolyTab& tab, unsigned long long seg = ~0ull) {
    if (op.relu) relu_n<EX, kQuarter<T, EX>, T, R, AD, NC, HF>(v, u1, u2, tab, seg);
    if (op.add >= 0) {
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (ok[k]) v[k] += lds[op.add + at[k]];
    }
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (ok[k]) lds[op.dst + at[k]] = v[k];
    if (DU && op.dst2 >= 0) {
        relu_n<EX, false, T, R, AD>(v, u1, u2, tab, seg);
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (ok[k]) lds[op.dst2 + at[k]] = v[k];
    }
}

// A pointer every lane holds the same value of (an op-record field) as a scalar: loads
// through it take the SGPR-base form (global_load … vOFF, s[BASE] offset:IMM), so a
// variance load costs no 64-bit VALU address arithmetic
__device__ __forceinline__ GP<char> ubase(const void* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (GP<char>)(const char*)(((unsigned long long)hi << 32) | lo);
}

// variances for the op's ReLU (var_x/var_y) or its dst2 ReLU (var2_x/var2_y).  x / y are
// uniform bases; xo / yo the byte offsets of the pair's maps when they differ per lane
// (multi-pair stages), else 0 with the image offset folded into the base.  ldx(px, k)
// reads pixel px + k of the x-side map: px is the per-lane part (one 32-bit offset
// register shared by both sides when the offsets are folded), k a compile-time step
// that lands in the instruction's immediate offset.  Per-lane offsets are 32-bit: the
// multi-pair maps are at most 32x32, and net_impl bounds n1, n2 so they cannot wrap.
template <typename T>
struct VarSrc {
    GP<char> x, y;
    unsigned xo, yo;
    bool on;
    __device__ __forceinline__ T ldx(unsigned px, int k = 0) const {
        return *(GP<T>)(x + (size_t)(xo + px * (unsigned)sizeof(T)) + k * (int)sizeof(T));
    }
    __device__ __forceinline__ T ldy(unsigned px, int k = 0) const {
        return *(GP<T>)(y + (size_t)(yo + px * (unsigned)sizeof(T)) + k * (int)sizeof(T));
    }
    // the same with the per-lane part in bytes (ConvHoist::px)
    __device__ __forceinline__ T ldxb(unsigned pb, int k) const {
        return *(GP<T>)(x + (size_t)(xo + pb) + k * (int)sizeof(T));
    }
    __device__ __forceinline__ T ldyb(unsigned pb, int k) const {
        return *(GP<T>)(y + (size_t)(yo + pb) + k * (int)sizeof(T));
    }
};
// UNI: i and j are the same in every lane (one pair per workgroup), so their offsets fold
// into the scalar bases
template <typename T, bool UNI>
__device__ __forceinline__ VarSrc<T> var_maps(const void* vx, const void* vy, bool on,
                                              unsigned i, unsigned j, int hw) {
    VarSrc<T> r;
    r.on = on;
    r.x = ubase(vx);
    r.y = ubase(vy);
    if constexpr (UNI) {
        r.x += (size_t)i * (size_t)hw * sizeof(T);   // scalar 64-bit arithmetic
        r.y += (size_t)j * (size_t)hw * sizeof(T);
        r.xo = r.yo = 0;
    } else {
        r.xo = i * (unsigned)hw * (unsigned)sizeof(T);
        r.yo = j * (unsigned)hw * (unsigned)sizeof(T);
    }
    return r;
}
template <typename T, bool UNI>
__device__ __forceinline__ VarSrc<T> var_src(const cgp_net_op& op, unsigned i, unsigned j,
                                             int hw) {
    const bool two = op.dst2 >= 0;
    return var_maps<T, UNI>(two ? op.var2_x : op.var_x, two ? op.var2_y : op.var_y,
                            op.relu != 0 || two, i, j, hw);
}

// ---- CGP_NET_CONV -------------------------------------------------------------------
// G::NP pairs: item it of a pass belongs to pair q = it / (items per pair) and works on
// that pair's LDS arena (q · lds_elems) and variance maps.
// Range-adaptive ReLU in a conv epilogue (relu_q_n): one-pair code votes over the wave
// (AD 1: both waves of a pair hold the same items of it in every workgroup); multi-pair
// stages vote per vote group (AD 2, below).
template <int NP>
constexpr int kAdaptOf = NP == 1 ? 1 : 2;
// Wave priority: a conv raises its waves' issue priority (s_setprio 2) while it sends its
// variance loads and window reads and drops it for the arithmetic epilogue, so the memory
// requests of a wave entering an op go out ahead of the other waves' long ALU runs and
// their latency overlaps that work.  Measured (one B = 1024 Kxz tile,
// profiles/r3/ab_r3u_prio.log): ConvNet +4.5-5%, Residual +4-5%, mnist_as_tf +3% (its 28x28
// head; the multi-pair stages do not move), but the cifar10 head (32x32 maps, four waves
// per SIMD) -3%: applied to maps of at most 28x28 pixels.  Priority 1 / 2 / 3 measure the
// same; raised over the variance loads only, or the window reads only, it loses half or
// more of the gain (profiles/r3/ab_r3x_prio_span.log); around the elementwise ops' loads
// it adds nothing.
constexpr int kPrio = 2;
constexpr int kPrioMaxHW = 28 * 28;
template <int NP, int HW>
constexpr bool kPrioOn = HW <= kPrioMaxHW;
template <int NP, int HW>
__device__ __forceinline__ void prio_mem() {
    if constexpr (kPrioOn<NP, HW>) __builtin_amdgcn_s_setprio(kPrio);
}
template <int NP, int HW>
__device__ __forceinline__ void prio_alu() {
    if constexpr (kPrioOn<NP, HW>) __builtin_amdgcn_s_setprio(0);
}
// Vote groups of a multi-pair stage (AD 2).  Items of pair q are [q·PER, (q+1)·PER) and
// item it runs on lane it % 64 of wave it / 64, so which items of a pair share a wave
// depends on the pair's slot q in the workgroup — a vote over "this pair's lanes of this
// wave" would make a pair's polynomial choice depend on its slot, i.e. on its place in the
// tile (1-ulp differences between a tile and a single-pair forward, found at round 4).
// Instead every pair's items are cut at the same local offsets: every offset at which a
// wave boundary can fall for SOME slot, {64k mod PER}.  A group then never straddles a
// wave, and it is the same set of the pair's pixels in every slot, so a pair's result
// depends on its own pixels only.
template <int PER, int NPR>
struct VoteCuts {
    int n = 0;
    int at[64] = {};
    constexpr VoteCuts() {
        for (int off = 1; off < PER && n < 64; ++off) {
            bool cut = false;
            for (int k = 1; 64 * k < NPR * PER; ++k) cut = cut || (64 * k) % PER == off;
            if (cut) at[n++] = off;
        }
    }
};
// the lanes of this wave in item it's vote group (a mask over the wave's 64 lanes)
template <int PER, int NPR>
__device__ __forceinline__ unsigned long long vote_lanes(int it) {
    constexpr VoteCuts<PER, NPR> cuts{};
    const int wb = it & ~63, q = udiv(it, PER), l = it - q * PER;
    int lo = 0, hi = PER;
#pragma unroll
    for (int k = 0; k < cuts.n; ++k) {
        if (cuts.at[k] <= l) lo = cuts.at[k];
        if (cuts.at[k] > l && cuts.at[k] < hi) hi = cuts.at[k];
    }
    int a = q * PER + lo - wb, b = q * PER + hi - wb;
    a = a < 0 ? 0 : a;
    b = b > 64 ? 64 : b;
    const unsigned long long top = b >= 64 ? ~0ull : ((1ull << b) - 1ull);
    return top & ~((1ull << a) - 1ull);
}
#ifndef CGP_NET_RES_UNDEF
#define CGP_NET_RES_UNDEF 1
#endif
// CGP_NET_HOIST=1 (default, round 9): a compiled one-pair fp64 program whose separable convs
// all share one geometry and one pair of pitches (kHoistProg: the ConvNet's seven 7x7 convs,
// the Residual net's nine 4x4 ones; the ResNets' 3x3 convs take the one-pass path)
// decodes a thread's items once per kernel instead of once per op and pair.  The item of a
// thread in the row pass and in the column pass, and so every address below, depends on the
// thread, the geometry, the pitches and the launch's scratch offset only: the pointers carry
// the workgroup half's arena and p.hs, the op's src / dst are immediates of the program and
// land in the instruction offsets.  Five registers held across the walk against about 29
// integer VALU instructions per op (opaque_tid() keeps the per-op decode of every other
// kernel out of the pair loop's registers).  0: the per-op decode everywhere.
#ifndef CGP_NET_HOIST
#define CGP_NET_HOIST 1
#endif
template <typename T>
using LP = __attribute__((address_space(3))) T*;   // an LDS address: one 32-bit register
template <typename T>
struct ConvHoist {
    LP<T> row;         // row pass: the item's first window cell for an op with src == src0
    LP<T> hrow;        // row pass: its first row-sum cell
    LP<T> col;         // column pass: the item's first row-sum cell
    LP<T> at;          // output 0 of the item for an op with dst == dst0
    unsigned px;       // byte offset of output 0 in a variance map (item 0's for an idle thread)
    bool row_on, col_on;   // the thread has an item in the pass
    // the slots of the program's first separable conv (immediates): an op adds src - src0 /
    // dst - dst0, zero where the convs share their slots, so the offsets of a window's cells
    // stay within the reach of the paired LDS reads
    int src0, dst0;
};
template <typename T, class G>
__device__ __forceinline__ ConvHoist<T> conv_hoist(T* lds, const NetP<T>& p, int tid, int wsi,
                                                   int wso, int src0, int dst0) {
    static_assert(G::NP == 1 && G::KH == 1 && G::KV == 1 && !G::POINT && !G::REDUCE && !G::DIRECT,
                  "hoisted decode: one item per thread and pass of a separable conv");
    ConvHoist<T> h;
    h.src0 = src0;
    h.dst0 = dst0;
    h.row_on = G::NH % G::NT == 0 || tid < G::NH;
    h.col_on = G::NV % G::NT == 0 || tid < G::NV;
    const LP<T> base = (LP<T>)lds;
    const int qi = udiv(tid, G::NG2), g2 = tid - qi * G::NG2;
    h.row = base + (src0 + (G::Q0 + qi + G::OFF) * wsi + g2 * G::R2 * G::S + G::OFF);
    h.hrow = base + p.hs + ((G::Q0 + qi) * G::WO + g2 * G::R2);
    const int g3 = udiv(tid, G::WO), c = tid - g3 * G::WO;
    h.col = base + p.hs + (g3 * G::R3 * G::S * G::WO + c);
    h.at = base + (dst0 + g3 * G::R3 * wso + c);
    // each address as one opaque register: left visible, the compiler splits the slots'
    // constants off again and keeps a register per pair of window cells instead
    asm volatile("" : "+v"(h.row), "+v"(h.hrow), "+v"(h.col), "+v"(h.at));
    const int itc = h.col_on ? tid : 0;
    const int g3c = udiv(itc, G::WO), cc = itc - g3c * G::WO;
    h.px = (unsigned)(g3c * G::R3 * G::WO + cc) * (unsigned)sizeof(T);
    return h;
}
// PRE: weight and bias arrive already scaled (a compiled program's records, prog_recs)
// NC / HF: the op's ReLU runs cap-free / on a non-negative input with a halved output
// (relu_q_n NOCAP / HALF; a compiled program's lean chain, ProgLean)
// HO: the separable path takes its item decode from hx (ConvHoist)
template <typename T, bool EX, bool DU, class G, bool PRE = false, bool NC = false,
          bool HF = false, bool HO = false>
__device__ __forceinline__ void net_conv(T* __restrict__ lds, const cgp_net_op& op,
                                         const NetP<T>& p, const Pairs& pr,
                                         const ConvHoist<T>* hx = nullptr) {
    constexpr int NP = G::NP;
    static_assert(!HO || (NP == 1 && !G::POINT && !G::REDUCE && !G::DIRECT && G::KH == 1 &&
                          G::KV == 1),
                  "hoisted decode: separable one-pair convs");
    const int tid = opaque_tid();
    const PolyTab tab = poly_table<HF>();
    // a conv feeding the fp64 closed-form ReLU produces c/4 (exact: w/4, b/4) for relu_q_n
    const T qs = !PRE && kQuarter<T, EX> && op.relu ? T(0.25) : T(1);
    const T w = T(op.weight) * qs, b = T(op.bias) * qs;
    const int arena = NP == 1 ? 0 : p.lds_elems;
    prio_mem<NP, G::HW>();
    const VarSrc<T> vs0 = var_src<T, NP == 1>(op, pr.i, pr.j, G::HOWO);   // NP == 1
    auto vs_of = [&](int q) {
        if constexpr (NP == 1) {
            return vs0;
        } else {
            unsigned iq, jq;
            pair_q<NP>(pr, q, iq, jq);
            return var_src<T, false>(op, iq, jq, G::HOWO);
        }
    };
    const T* __restrict__ src = lds + op.src;
    const int wsi = op.ws_in, wso = op.ws_out;

    if constexpr (G::REDUCE && NP == 1) {
        prio_alu<NP, G::HW>();
        // 1x1 output from a full-plane window: a block reduction — or, after a conv marked
        // CGP_NET_CODE_SUM, the wave partial sums that conv left (the map was never stored)
        const bool from_sum = (op.code & CGP_NET_CODE_FROM_SUM) != 0;
        T* part = from_sum ? static_cast<T*>(pr.red)
                           : lds + p.part;   // off the scratch's zero rows (cgp_net_args.part)
        if (!from_sum) {
            T acc = T(0);
#pragma unroll
            for (int k = 0; k < (G::HW + G::NT - 1) / G::NT; ++k) {
                const int px = tid + k * G::NT;
                if (G::HW % G::NT == 0 || px < G::HW) {
                    const int r = udiv(px, G::W), c = px - r * G::W;
                    acc += src[r * wsi + c];
                }
            }
            acc = wave_sum(acc);
            if ((tid & 63) == 0) part[tid >> 6] = acc;
            lds_barrier();
        }
        if (tid == 0) {
            T tot = part[0];
#pragma unroll
            for (int k = 1; k < G::NT / 64; ++k) tot += part[k];
            T v[1] = {fma_t(w, tot, b)};
            const int at[1] = {0};
            const bool ok[1] = {true};
            T u1[1] = {T(1)}, u2[1] = {T(1)};
            if (vs0.on) {
                u1[0] = vs0.ldx(0);
                u2[0] = vs0.ldy(0);
            }
            net_out<T, EX, DU, 1, 0, NC, HF>(lds, op, v, at, ok, u1, u2, tab);
        }
    } else if constexpr (G::REDUCE) {
        prio_alu<NP, G::HW>();
        // NP pairs: G::NT / NP lanes per pair (within one wave) sum its map, then a
        // segmented butterfly; the group's first lane finishes the pair
        constexpr int TPP = G::NT / NP;
        static_assert(TPP <= 64 && G::NT % NP == 0, "reduce groups must not straddle waves");
        const int q = udiv(tid, TPP), lane = tid - q * TPP;
        const T* srcq = src + q * arena;
        T acc = T(0);
#pragma unroll
        for (int k = 0; k < (G::HW + TPP - 1) / TPP; ++k) {
            const int px = lane + k * TPP;
            if (G::HW % TPP == 0 || px < G::HW) {
                const int r = udiv(px, G::W), c = px - r * G::W;
                acc += srcq[r * wsi + c];
            }
        }
#pragma unroll
        for (int m = TPP / 2; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0) {
            const VarSrc<T> vs = vs_of(q);
            T v[1] = {fma_t(w, acc, b)};
            const int at[1] = {q * arena};
            const bool ok[1] = {true};
            T u1[1] = {T(1)}, u2[1] = {T(1)};
            if (vs.on) {
                u1[0] = vs.ldx(0);
                u2[0] = vs.ldy(0);
            }
            net_out<T, EX, DU, 1, 0, NC, HF>(lds, op, v, at, ok, u1, u2, tab);
        }
    } else if constexpr (G::POINT) {
        prio_alu<NP, G::HW>();
        constexpr int N = NP * G::HOWO;
        constexpr int KP = (N + G::NT - 1) / G::NT;
        T u1[KP], u2[KP], v[KP];
        int at[KP];
        bool ok[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const int e = tid + k * G::NT;
            ok[k] = N % G::NT == 0 || e < N;
            const int ec = ok[k] ? e : 0;
            const int q = NP == 1 ? 0 : udiv(ec, G::HOWO), pc = ec - q * G::HOWO;
            const int r = udiv(pc, G::WO), c = pc - r * G::WO;
            const VarSrc<T> vs = vs_of(q);
            at[k] = q * arena + r * wso + c;
            u1[k] = (vs.on && ok[k]) ? vs.ldx((unsigned)pc) : T(1);
            u2[k] = (vs.on && ok[k]) ? vs.ldy((unsigned)pc) : T(1);
            v[k] = fma_t(w, src[q * arena + (r * G::S) * wsi + c * G::S], b);
        }
        net_out<T, EX, DU, KP, NP == 1 ? 1 : 0, NC, HF>(lds, op, v, at, ok, u1, u2, tab);
    } else if constexpr (G::DIRECT) {
        // one pass: item (q, g3, c) sums its WIN3 x TAPS input window straight from the
        // source slot (row sums, then column sums: the separable path's order, so the
        // same bits); rows outside the map read as zero, columns outside are the slot's
        // zero halo
        constexpr int NVT = NP * G::NV;
        T u1[G::KV][G::R3], u2[G::KV][G::R3];
#pragma unroll
        for (int kv = 0; kv < G::KV; ++kv) {
            const int it = tid + kv * G::NT;
            const int itc = (NVT % G::NT == 0 || it < NVT) ? it : 0;
            const int q = NP == 1 ? 0 : udiv(itc, G::NV), l = itc - q * G::NV;
            const int g3 = udiv(l, G::WO), c = l - g3 * G::WO;
            const VarSrc<T> vs = vs_of(q);
#pragma unroll
            for (int k = 0; k < G::R3; ++k) {
                const unsigned px0 = (unsigned)(g3 * G::R3 * G::WO + c);
                u1[kv][k] = vs.on ? vs.ldx(px0, k * G::WO) : T(1);
                u2[kv][k] = vs.on ? vs.ldy(px0, k * G::WO) : T(1);
            }
        }
        // outputs that land on the source (in place, or dst2 on the source) are stored
        // after every item has read its window
        const int s_lo = op.src - wsi, s_hi = op.src + G::H * wsi;
        auto hits = [&](int d) {
            return d >= 0 && d - wso < s_hi && d + G::HO * wso > s_lo;
        };
        const bool hazard = hits(op.dst) || (DU && hits(op.dst2));
        T res[G::KV][G::R3];
#if CGP_NET_RES_UNDEF
        // an idle item's outputs are never stored: defined by an empty asm, not by 7 zero
        // moves per item and op
#pragma unroll
        for (int kv = 0; kv < G::KV; ++kv)
#pragma unroll
            for (int k = 0; k < G::R3; ++k) asm volatile("" : "=v"(res[kv][k]));
#endif
#pragma unroll
        for (int kv = 0; kv < G::KV; ++kv) {
            const int it = tid + kv * G::NT;
            if (NVT % G::NT == 0 || it < NVT) {
                const int q = NP == 1 ? 0 : udiv(it, G::NV), l = it - q * G::NV;
                const int g3 = udiv(l, G::WO), c = l - g3 * G::WO;
                const T* base = src + q * arena + c * G::S + G::OFF;
                const int r0 = g3 * G::R3 * G::S + G::OFF;
                T rs[G::WIN3];
#pragma unroll
                for (int t = 0; t < G::WIN3; ++t) {
                    const bool lo = G::OFF + t < 0, hi = (G::NG3 - 1) * G::R3 * G::S + G::OFF + t >= G::H;
                    const int r = r0 + t;
                    const bool in = (!lo || r >= 0) && (!hi || r < G::H);
                    const T* row = base + (in ? r : 0) * wsi;
                    T a = row[0];
#pragma unroll
                    for (int dx = 1; dx < G::TAPS; ++dx) a += row[dx];
                    rs[t] = in ? a : T(0);
                }
                T o[G::R3];
                win_sums<T, G::TAPS, G::S, G::R3>(rs, o);
#pragma unroll
                for (int k = 0; k < G::R3; ++k) res[kv][k] = fma_t(w, o[k], b);
#pragma unroll
                for (int k = 0; k < G::R3; ++k)
                    asm volatile("" : "+v"(u1[kv][k]), "+v"(u2[kv][k]));
            }
        }
        prio_alu<NP, G::HW>();
        if (hazard) lds_barrier();
#pragma unroll
        for (int kv = 0; kv < G::KV; ++kv) {
            const int it = tid + kv * G::NT;
            if (NVT % G::NT == 0 || it < NVT) {
                const int q = NP == 1 ? 0 : udiv(it, G::NV), l = it - q * G::NV;
                const int g3 = udiv(l, G::WO), c = l - g3 * G::WO;
                int at[G::R3];
                bool ok[G::R3];
#pragma unroll
                for (int k = 0; k < G::R3; ++k) {
                    at[k] = q * arena + (g3 * G::R3 + k) * wso + c;
                    ok[k] = true;
                }
                net_out<T, EX, DU, G::R3, kAdaptOf<NP>, NC, HF>(
                    lds, op, res[kv], at, ok, u1[kv], u2[kv], tab,
                    NP == 1 ? ~0ull : vote_lanes<G::NV, NP>(it));
            }
        }
    } else {
        T* __restrict__ hs = lds + p.hs;
        constexpr int NHT = NP * G::NH, NVT = NP * G::NV, NZT = NP * G::NZ;
        // variances of this thread's outputs, in flight during the row pass
        T u1[G::KV][G::R3], u2[G::KV][G::R3];
        if constexpr (HO) {
            if (vs0.on) {
                // through an opaque move: the offset's zero extension then stays in this block,
                // where it folds into the loads' SGPR-base form (hoisted with the offset, it
                // costs a register pair and a 64-bit VALU add per side and op)
                unsigned pb = hx->px;
                asm volatile("" : "+v"(pb));
#pragma unroll
                for (int k = 0; k < G::R3; ++k) {
                    u1[0][k] = vs0.ldxb(pb, k * G::WO);
                    u2[0][k] = vs0.ldyb(pb, k * G::WO);
                }
            } else {
#pragma unroll
                for (int k = 0; k < G::R3; ++k) u1[0][k] = u2[0][k] = T(1);
            }
        } else if (vs0.on) {
#pragma unroll
            for (int kv = 0; kv < G::KV; ++kv) {
                const int it = tid + kv * G::NT;
                const int itc = (NVT % G::NT == 0 || it < NVT) ? it : 0;
                const int q = NP == 1 ? 0 : udiv(itc, G::NV), l = itc - q * G::NV;
                const int g3 = udiv(l, G::WO), c = l - g3 * G::WO;
                const VarSrc<T> vs = vs_of(q);
#pragma unroll
                for (int k = 0; k < G::R3; ++k) {
                    const unsigned px0 = (unsigned)(g3 * G::R3 * G::WO + c);
                    u1[kv][k] = vs.ldx(px0, k * G::WO);
                    u2[kv][k] = vs.ldy(px0, k * G::WO);
                }
            }
        } else {
#pragma unroll
            for (int kv = 0; kv < G::KV; ++kv)
#pragma unroll
                for (int k = 0; k < G::R3; ++k) u1[kv][k] = u2[kv][k] = T(1);
        }
        // row pass: hs[q][c] = Σ_t in[q + OFF][c·S + OFF + t]
        if constexpr (HO) {
            if (hx->row_on) {
                const LP<T> row = hx->row + (op.src - hx->src0);
                T win[G::WIN2];
#pragma unroll
                for (int t = 0; t < G::WIN2; ++t) win[t] = row[t];
                T o[G::R2];
                win_sums<T, G::TAPS, G::S, G::R2>(win, o);
#pragma unroll
                for (int t = 0; t < G::R2; ++t) hx->hrow[t] = o[t];
            }
        } else {
#pragma unroll
            for (int kh = 0; kh < G::KH; ++kh) {
                const int it = tid + kh * G::NT;
                if (NHT % G::NT == 0 || it < NHT) {
                    const int q = NP == 1 ? 0 : udiv(it, G::NH), l = it - q * G::NH;
                    const int qi = udiv(l, G::NG2), g2 = l - qi * G::NG2;
                    const T* row = lds + (op.src + q * arena + (G::Q0 + qi + G::OFF) * wsi +
                                          g2 * G::R2 * G::S + G::OFF);
                    T win[G::WIN2];
#pragma unroll
                    for (int t = 0; t < G::WIN2; ++t) win[t] = row[t];
                    T o[G::R2];
                    win_sums<T, G::TAPS, G::S, G::R2>(win, o);
                    T* h = hs + q * arena + (G::Q0 + qi) * G::WO + g2 * G::R2;
#pragma unroll
                    for (int t = 0; t < G::R2; ++t) h[t] = o[t];
                }
            }
        }
        // hs rows outside the input are zero (the scratch is shared by every conv); skipped
        // when the host proved they still are (CGP_NET_CODE_HS_CLEAN)
        if constexpr (G::NZ > 0) {
            if (!(op.code & CGP_NET_CODE_HS_CLEAN)) {
#pragma unroll
                for (int z0 = 0; z0 < NZT; z0 += G::NT) {
                    const int z = z0 + tid;
                    if (NZT % G::NT == 0 || z < NZT) {
                        const int q = NP == 1 ? 0 : udiv(z, G::NZ), zl = z - q * G::NZ;
                        hs[q * arena + (zl < G::Q0 * G::WO ? zl : zl + G::NVR * G::WO)] = T(0);
                    }
                }
            }
        }
        lds_barrier();
        // column pass + output stage (uniform branches outside the per-pixel loops: each
        // stage is one basic block, so the R3 independent ReLUs interleave).  A conv marked
        // CGP_NET_CODE_SUM (one pair) keeps its outputs in registers and leaves only their
        // wave sums for the reduction that follows
        const bool to_sum = NP == 1 && (op.code & CGP_NET_CODE_SUM) != 0;
        T sacc = T(0);
#pragma unroll
        for (int kv = 0; kv < G::KV; ++kv) {
            const int it = tid + kv * G::NT;
            if (HO ? hx->col_on : (NVT % G::NT == 0 || it < NVT)) {
                // (HO: q, g3 and c are dead; the item's cells come from hx)
                const int q = NP == 1 ? 0 : udiv(it, G::NV), l = it - q * G::NV;
                const int g3 = udiv(l, G::WO), c = l - g3 * G::WO;
                const T* col = HO ? (const T*)hx->col
                                  : lds + (p.hs + q * arena + g3 * G::R3 * G::S * G::WO + c);
                T win[G::WIN3];
#pragma unroll
                for (int t = 0; t < G::WIN3; ++t) win[t] = col[t * G::WO];
                // the variances are first needed here: without this fence the compiler
                // folds u1·u2 (the ReLU's t) into the load block at the op start and
                // waits for the loads there, before the row pass
#pragma unroll
                for (int k = 0; k < G::R3; ++k) asm volatile("" : "+v"(u1[kv][k]), "+v"(u2[kv][k]));
                T o[G::R3], v[G::R3];
                win_sums<T, G::TAPS, G::S, G::R3>(win, o);
                prio_alu<NP, G::HW>();
                int at[G::R3];
                bool ok[G::R3];
#pragma unroll
                for (int k = 0; k < G::R3; ++k) {
                    v[k] = fma_t(w, o[k], b);
                    at[k] = HO ? k * wso - hx->dst0 : q * arena + (g3 * G::R3 + k) * wso + c;
                    ok[k] = true;
                }
                if (to_sum) {
                    if (op.relu)
                        relu_n<EX, kQuarter<T, EX>, T, G::R3, 1, NC, HF>(v, u1[kv], u2[kv], tab);
#pragma unroll
                    for (int k = 0; k < G::R3; ++k) sacc += v[k];
                } else {
                    net_out<T, EX, DU, G::R3, kAdaptOf<NP>, NC, HF>(
                        HO ? (T*)hx->at : lds, op, v, at, ok, u1[kv], u2[kv], tab,
                        NP == 1 ? ~0ull : vote_lanes<G::NV, NP>(it));
                }
            }
        }
        if constexpr (NP == 1) {
            if (to_sum) {
                sacc = wave_sum(sacc);
                if ((tid & 63) == 0) static_cast<T*>(pr.red)[tid >> 6] = sacc;
            }
        }
    }
}

// ---- elementwise ops: RELU, LINEAR, MOMENTS -------------------------------------------
// One pass: KE pixels per thread at e = base + k·NT + tid over the NP pairs' maps
// (pair q = e / hw; NP > 1 needs the compile-time size W_).
template <typename T, bool EX, bool DU, int KIND, int KE, int W_, int NP>
__device__ __forceinline__ void elem_pass(T* __restrict__ lds, const cgp_net_op& op,
                                          const NetP<T>& p, const Pairs& pr, int tid,
                                          int base, int hw, const PolyTab& tab) {
    static_assert(NP == 1 || W_ > 0, "multi-pair elementwise ops need a compile-time size");
    const int wd = W_ ? W_ : op.w, ws = op.ws_out;
    const int arena = NP == 1 ? 0 : p.lds_elems;
    const FastDiv fw{op.div_m, op.div_s, (unsigned)op.w};
    // RELU reads (var_x, var_y) = variances of src (an elementwise ReLU has no dst2);
    // LINEAR may carry a dst2 ReLU with (var2_x, var2_y)
    auto vs_of = [&](unsigned iq, unsigned jq) {
        return KIND == CGP_NET_RELU
                   ? var_maps<T, NP == 1>(op.var_x, op.var_y, true, iq, jq, hw)
                   : var_src<T, NP == 1>(op, iq, jq, hw);
    };
    const VarSrc<T> vs0 = vs_of(pr.i, pr.j);
    // the pair's images (MOMENTS, one pair per half: i, j uniform) as scalar byte bases;
    // pixel offsets stay 32-bit unsigned, so every load is SGPR base + VGPR offset with no
    // 64-bit VALU address arithmetic (an image is at most C·hw·8 bytes)
    const GP<char> xi = ubase(p.x) + (size_t)pr.i * p.channels * hw * sizeof(T);
    const GP<char> yj = ubase(p.y) + (size_t)pr.j * p.channels * hw * sizeof(T);
    auto img = [](GP<char> b, unsigned e) {
        return *(GP<T>)(b + (size_t)(e * (unsigned)sizeof(T)));
    };
    const int n = NP * hw;
    // waves with no pixel in this pass skip the ReLUs (uniform per wave)
    const bool live = base + (tid & ~63) < n;
    T a[KE], u1[KE], u2[KE];
    int at[KE];
    bool ok[KE];
#pragma unroll
    for (int k = 0; k < KE; ++k) {
        const int e = base + k * kNT + tid;
        ok[k] = e < n;
        const int ec = ok[k] ? e : 0;
        const int q = NP == 1 ? 0 : ec / hw, pc = ec - q * hw;
        const int r = W_ ? udiv(pc, W_) : (int)fdiv((unsigned)pc, fw);
        at[k] = q * arena + r * ws + (pc - r * wd);
        VarSrc<T> vs = vs0;
        if constexpr (NP > 1) {
            unsigned iq, jq;
            pair_q<NP>(pr, q, iq, jq);
            vs = vs_of(iq, jq);
        }
        u1[k] = (vs.on && ok[k]) ? vs.ldx((unsigned)pc) : T(1);
        u2[k] = (vs.on && ok[k]) ? vs.ldy((unsigned)pc) : T(1);
        if constexpr (KIND == CGP_NET_RELU) {
            a[k] = lds[op.src + at[k]];
        } else if constexpr (KIND == CGP_NET_MOMENTS) {
            static_assert(NP == 1, "moments run one pair per workgroup (half)");
            T acc = img(xi, (unsigned)pc) * img(yj, (unsigned)pc);
            for (int ch = 1; ch < p.channels; ++ch) {
                const unsigned e = (unsigned)(ch * hw + pc);
                acc += img(xi, e) * img(yj, e);
            }
            a[k] = acc;
        } else {
            a[k] = T(op.weight) * lds[op.src + at[k]] + T(op.bias) * lds[op.add + at[k]];
        }
    }
    if constexpr (KIND == CGP_NET_MOMENTS) {
        // the channel mean (x / 1 == x: a uniform branch, so one-channel inputs run no
        // division at all)
        if (p.channels != 1) {
#pragma unroll
            for (int k = 0; k < KE; ++k) a[k] = a[k] / T(p.channels);
        }
    }
    if constexpr (KIND == CGP_NET_RELU) {
        if (live) relu_n<EX, false, T, KE, NP == 1 ? 1 : 0>(a, u1, u2, tab);
        if (op.add >= 0) {
#pragma unroll
            for (int k = 0; k < KE; ++k)
                if (ok[k]) a[k] += lds[op.add + at[k]];
        }
    }
#pragma unroll
    for (int k = 0; k < KE; ++k)
        if (ok[k]) lds[op.dst + at[k]] = a[k];
    if constexpr (KIND == CGP_NET_LINEAR && DU) {
        if (op.dst2 >= 0) {
            if (live) relu_n<EX, false, T, KE, NP == 1 ? 1 : 0>(a, u1, u2, tab);
#pragma unroll
            for (int k = 0; k < KE; ++k)
                if (ok[k]) lds[op.dst2 + at[k]] = a[k];
        }
    }
}

// compile-time map size: passes of at most kEw pixels per thread, the last one sized to
// what is left (28x28: 4 + 3)
template <typename T, bool EX, bool DU, int KIND, int H_, int W_, int NP, int PI>
__device__ __forceinline__ void elem_passes(T* __restrict__ lds, const cgp_net_op& op,
                                            const NetP<T>& p, const Pairs& pr, int tid,
                                            const PolyTab& tab) {
    constexpr int KF = (NP * H_ * W_ + kNT - 1) / kNT;
    if constexpr (PI * kEw < KF) {
        constexpr int KE = KF - PI * kEw < kEw ? KF - PI * kEw : kEw;
        elem_pass<T, EX, DU, KIND, KE, W_, NP>(lds, op, p, pr, tid, PI * kEw * kNT, H_ * W_,
                                               tab);
        elem_passes<T, EX, DU, KIND, H_, W_, NP, PI + 1>(lds, op, p, pr, tid, tab);
    }
}

// H_ = W_ = 0: runtime map size (generic path, one pair per workgroup).
template <typename T, bool EX, bool DU, int KIND, int H_, int W_, int NP>
__device__ __forceinline__ void net_elem(T* __restrict__ lds, const cgp_net_op& op,
                                         const NetP<T>& p, const Pairs& pr) {
    const int tid = opaque_tid();
    const PolyTab tab = poly_table();
    if constexpr (H_ == 0) {
        const int hw = op.h * op.w;
        for (int base = 0; base < hw; base += kEw * kNT)
            elem_pass<T, EX, DU, KIND, kEw, 0, 1>(lds, op, p, pr, tid, base, hw, tab);
    } else {
        elem_passes<T, EX, DU, KIND, H_, W_, NP, 0>(lds, op, p, pr, tid, tab);
    }
}

// ---- MOMENTS of a compiled program: batched image loads (round 10) ---------------------
// elem_pass keeps the runtime channel loop between a thread's consecutive pixels, so a wave
// entering a pair pays one dependent global round trip per pixel (7 at 28x28) before its
// first conv.  With the channel count a compile-time CH the x and y loads of all of a
// thread's pixels of one channel go out as one block and are waited for once (1 channel: 14
// loads, one wait; 3 channels: three blocks of 14).  Each pixel still computes x0·y0, then
// += x_ch·y_ch in channel order, then the same division when channels != 1: bit for bit
// what elem_pass stores.  CGP_NET_MOMENTS_BATCH=0: elem_pass everywhere (the A/B switch).
// HO (CGP_NET_MOMENTS_ITEMS, kHoistProg programs whose MOMENTS map has the hoisted conv's
// output size and pitch): the thread's pixels are those of its column item (rows g3·R3 + k
// of column c), so pixel k's image offset is hx.px + k·WO·sizeof(T) and its LDS cell
// hx.at + (DST − dst0) + k·WS: immediates on one register each, one predicate (col_on).
// Measured (bench.py, ConvNet Kxx 4096², three alternating rounds, profiles/r10): the batch
// alone -1.9% ms per step, with the column items -3.9%; the wave priority raised around the
// block (prio_mem / prio_alu) cost 0.9 ms of that and is not applied.
#ifndef CGP_NET_MOMENTS_BATCH
#define CGP_NET_MOMENTS_BATCH 1
#endif
#ifndef CGP_NET_MOMENTS_ITEMS
#define CGP_NET_MOMENTS_ITEMS 1
#endif
// maps of at most 28x28 pixels: with the 32x32 head's 8 pixels per thread (16 loads a block)
// the cifar10 head kernel goes from 93 to 101 VGPRs, past the 96 of five waves per SIMD, so
// that program keeps elem_pass
#ifndef CGP_NET_MOMENTS_MAXHW
#define CGP_NET_MOMENTS_MAXHW (28 * 28)
#endif
// the values of one block of loads, all present from here on: one wait for the block
template <typename T, int N>
__device__ __forceinline__ void loads_fence(T (&v)[N]) {
    static_assert(N >= 1 && N <= 8, "loads_fence: at most 8 values a side");
    if constexpr (N == 1) asm volatile("" : "+v"(v[0]));
    if constexpr (N == 2) asm volatile("" : "+v"(v[0]), "+v"(v[1]));
    if constexpr (N == 3) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
    if constexpr (N == 4) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
    if constexpr (N == 5)
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]));
    if constexpr (N == 6)
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
    if constexpr (N == 7)
        asm volatile(""
                     : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]),
                       "+v"(v[6]));
    if constexpr (N == 8)
        asm volatile(""
                     : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]),
                       "+v"(v[6]), "+v"(v[7]));
}
// G: the hoisted conv's geometry (HO), unused otherwise
template <typename T, int CH, int H_, int W_, int WS, int DST, bool HO, class G>
__device__ __forceinline__ void moments_batch(T* __restrict__ lds, const NetP<T>& p,
                                              const Pairs& pr, const ConvHoist<T>& hx) {
    constexpr int HW = H_ * W_;
    constexpr int KF = HO ? G::R3 : (HW + kNT - 1) / kNT;   // pixels per thread
    static_assert(KF <= 8, "moments_batch: at most 8 pixels per thread");
    const int tid = opaque_tid();
    // the pair's images as scalar byte bases (elem_pass), one per channel
    const GP<char> xi = ubase(p.x) + (size_t)pr.i * CH * HW * sizeof(T);
    const GP<char> yj = ubase(p.y) + (size_t)pr.j * CH * HW * sizeof(T);
    // pixel k of the thread in a channel plane: byte offset pb plus an immediate step; on the
    // elementwise layout the ragged last pass has its own, `last` (pixel 0 for an idle thread)
    unsigned pb, last = 0;
    bool ok_last = true;
    if constexpr (HO) {
        pb = hx.px;
        asm volatile("" : "+v"(pb));   // the zero extension stays here (net_conv)
    } else {
        pb = (unsigned)tid * (unsigned)sizeof(T);
        if constexpr (HW % kNT != 0) {
            const int e = (KF - 1) * kNT + tid;
            ok_last = e < HW;
            last = (unsigned)(ok_last ? e : 0) * (unsigned)sizeof(T);
        }
    }
    auto ld = [&](GP<char> b, int k) -> T {
        if constexpr (HO) {
            return *(GP<T>)(b + (size_t)pb + k * G::WO * (int)sizeof(T));
        } else {
            if (HW % kNT != 0 && k == KF - 1) return *(GP<T>)(b + (size_t)last);
            return *(GP<T>)(b + (size_t)pb + k * kNT * (int)sizeof(T));
        }
    };
    T a[KF];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const GP<char> xc = xi + (size_t)ch * HW * sizeof(T);
        const GP<char> yc = yj + (size_t)ch * HW * sizeof(T);
        T xv[KF], yv[KF];
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            xv[k] = ld(xc, k);
            yv[k] = ld(yc, k);
        }
        loads_fence(xv);
        loads_fence(yv);
#pragma unroll
        for (int k = 0; k < KF; ++k) a[k] = ch == 0 ? xv[k] * yv[k] : a[k] + xv[k] * yv[k];
        // the next channel's block goes out after this one is consumed (register budget):
        // nothing is scheduled across
        if (ch + 1 < CH) {
            loads_fence(a);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (CH != 1) {   // the channel mean: T(p.channels) as a constant
#pragma unroll
        for (int k = 0; k < KF; ++k) a[k] = a[k] / T(CH);
    }
    if constexpr (HO) {
        if (hx.col_on) {
            const LP<T> at = hx.at + (DST - hx.dst0);
#pragma unroll
            for (int k = 0; k < KF; ++k) at[k * WS] = a[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < KF; ++k) {
            const bool ok = HW % kNT == 0 || k < KF - 1 || ok_last;
            const int e = ok ? k * kNT + tid : 0;
            const int r = udiv(e, W_);
            if (ok) lds[DST + r * WS + (e - r * W_)] = a[k];
        }
    }
}
// the workgroup-uniform choice of the channel count: 1 and 3 are compiled, any other count
// runs elem_pass's runtime loop
template <typename T, bool DU, int H_, int W_, int WS, int DST, bool HO, class G>
__device__ __forceinline__ void net_moments(T* __restrict__ lds, const cgp_net_op& op,
                                            const NetP<T>& p, const Pairs& pr,
                                            const ConvHoist<T>& hx) {
    if (p.channels == 1)
        moments_batch<T, 1, H_, W_, WS, DST, HO, G>(lds, p, pr, hx);
    else if (p.channels == 3)
        moments_batch<T, 3, H_, W_, WS, DST, HO, G>(lds, p, pr, hx);
    else
        net_elem<T, false, DU, CGP_NET_MOMENTS, H_, W_, 1>(lds, op, p, pr);
}

// Stage boundary (CGP_NET_LOAD / CGP_NET_STORE): the map of each of the NP pairs moves
// between its slot and the unit's state record, state[(u - ubeg) · code + add + pixel].
template <typename T, int KIND, int NP>
__device__ __forceinline__ void net_move(T* __restrict__ lds, const cgp_net_op& op,
                                         const NetP<T>& p, const Pairs& pr) {
    const int tid = opaque_tid();
    const int hw = op.h * op.w, n = NP * hw;
    const int arena = NP == 1 ? 0 : p.lds_elems;
    T* state = const_cast<T*>(static_cast<const T*>(op.var_x));
    for (int e = tid; e < n; e += kNT) {
        const int q = NP == 1 ? 0 : e / hw, l = e - q * hw;
        const int r = l / op.w, c = l - r * op.w;
        // the state buffer holds the units of this launch, [ubeg, uend)
        const size_t g = (size_t)(pr.u0 + q - p.ubeg) * (size_t)op.code + (size_t)op.add +
                         (size_t)l;
        if constexpr (KIND == CGP_NET_LOAD)
            lds[op.dst + q * arena + r * op.ws_out + c] = state[g];
        else
            state[g] = lds[op.src + q * arena + r * op.ws_in + c];
    }
}

// The same move for a compiled program (geometry, slot and pitches compile-time): pass k
// covers elements e = k·kNT + tid of the NP pairs' H×W maps, all passes unrolled.  The
// launch's state base (u0 − ubeg)·code + add is scalar (u0 is uniform), so an element's
// global address is that SGPR base plus a 32-bit lane offset q·code + l, and its LDS cell
// q·arena + r·ws + c comes from compile-time divisions: about 12 VALU per element where
// the generic loop above spent about 25 (64-bit address math, signed divisions by runtime
// sizes; ISA count, tools/isa_attrib.py).  CGP_NET_MOVE_C=0 keeps the generic loop.
#ifndef CGP_NET_MOVE_C
#define CGP_NET_MOVE_C 1
#endif
template <typename T, int KIND, int NP, int H_, int W_, int SLOT, int WS>
__device__ __forceinline__ void net_move_c(T* __restrict__ lds, const cgp_net_op& op,
                                           const NetP<T>& p, const Pairs& pr) {
    const int tid = opaque_tid();
    constexpr int HW = H_ * W_, N = NP * HW, KP = (N + kNT - 1) / kNT;
    const int arena = NP == 1 ? 0 : p.lds_elems;
    const unsigned long long u0 =
        ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)pr.u0 >> 32)) << 32) |
        __builtin_amdgcn_readfirstlane((unsigned)pr.u0);
    const unsigned code = (unsigned)__builtin_amdgcn_readfirstlane(op.code);
    const GP<char> base = ubase(op.var_x) +
                          ((size_t)(u0 - (unsigned long long)p.ubeg) * code + (size_t)op.add) *
                              sizeof(T);
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const int e = k * kNT + tid;
        if (N % kNT == 0 || e < N) {
            const unsigned q = NP == 1 ? 0u : (unsigned)udiv(e, HW);
            const unsigned l = (unsigned)e - q * (unsigned)HW;
            const unsigned r = (unsigned)udiv((int)l, W_), c = l - r * (unsigned)W_;
            T* cell = lds + (SLOT + (int)q * arena + (int)(r * (unsigned)WS + c));
            typedef __attribute__((address_space(1))) T* GW;   // the state record, writable
            GW g = (GW)(base + (size_t)((q * code + l) * (unsigned)sizeof(T)));
            if constexpr (KIND == CGP_NET_LOAD)
                *cell = *g;
            else
                *g = *cell;
        }
    }
}

// Zero the halo cells of the slot whose pixel (0, 0) is at `origin` (code = (HL << 8) |
// gap, see cgp_net_op.zero_halo): HL cells before it and `gap` after each of the h rows.
// Disjoint from every data cell, so it needs no barrier against the op's own writes.
template <typename T, int NT>
__device__ __forceinline__ void zero_halos(T* lds, int origin, int code, int h, int w, int ws,
                                           int tid) {
    if (!code) return;
    const int hl = code >> 8, gap = code & 0xff;
    for (int e = tid; e < hl + h * gap; e += NT) {
        int cell;
        if (e < hl) {
            cell = origin - hl + e;
        } else {
            const int r = (e - hl) / gap;
            cell = origin + r * ws + w + (e - hl - r * gap);
        }
        lds[cell] = T(0);
    }
}

// pair walk: supertile s (kST x kST pairs) -> (bi, bj); same tiles enumerate the upper
// triangle (bi <= bj) row-major
__device__ __forceinline__ void tri_decode(unsigned s, unsigned nb, unsigned& bi,
                                           unsigned& bj) {
    const double a = 2.0 * nb + 1.0;
    long long r = (long long)((a - sqrt(a * a - 8.0 * (double)s)) * 0.5);
    auto off = [nb](long long q) { return q * (long long)nb - q * (q - 1) / 2; };
    if (r < 0) r = 0;
    while (r > 0 && off(r) > (long long)s) --r;
    while (off(r + 1) <= (long long)s) ++r;
    bi = (unsigned)r;
    bj = (unsigned)(r + ((long long)s - off(r)));
}

// tile unit u (supertile, pair within it) -> (i, j); false if outside the tile
template <typename T>
__device__ __forceinline__ bool unit_pair(const NetP<T>& p, long long u, unsigned& i,
                                          unsigned& j) {
    const unsigned s = (unsigned)(u >> (2 * kSTL)), q = (unsigned)u & (kST * kST - 1u);
    unsigned bi, bj;
    if (p.same) {
        tri_decode(s, p.nbi, bi, bj);
    } else {
        bi = s / p.nbj;
        bj = s - bi * p.nbj;
    }
    i = bi * kST + (q >> kSTL);
    j = bj * kST + (q & (kST - 1u));
    return u < p.units && i < p.n1 && j < p.n2;
}

constexpr int geo_index(int h, int w, int ho, int wo, int k, int s, int o) {
    for (int n = 0; n < kNumGeo; ++n) {
        const GeoRow& g = kGeoTable[n];
        if (g.h == h && g.w == w && g.ho == ho && g.wo == wo && g.taps == k && g.s == s &&
            g.off == o)
            return n;
    }
    return -1;
}

// a geometry / map size is instantiated for NP pairs when the NP maps fit the passes
// (NP·h·w <= 1024: 4 pairs at <= 16x16, 16 at <= 8x8); the host stages networks to match
#define CGP_NET_FITS(h, w) (NP == 1 || (h) * (w) * NP <= 1024)

#define CGP_NET_CASE(h, w, ho, wo, k, s, o)                                          \
    case geo_index(h, w, ho, wo, k, s, o):                                           \
        if constexpr (CGP_NET_FITS(h, w))                                            \
            net_conv<T, EX, DU, NG<h, w, ho, wo, k, s, o, NP>>(lds, op, p, pr);      \
        break;

#define CGP_NET_RES_CASE(h, w)                                                        \
    case res_index(h, w):                                                             \
        if constexpr (CGP_NET_FITS(h, w)) net_elem<T, EX, DU, KIND, h, w, NP>(lds, op, p, pr); \
        break;

// only the ReLU is worth a per-size instantiation (MOMENTS runs once per pair, LINEAR
// only for Mixture / multi-term Sum); fewer cases also keep the SGPR budget.  Multi-pair
// stages run compile-time sizes only (the host keeps moments and other sizes at NP = 1).
template <typename T, bool EX, bool DU, int KIND, int NP>
__device__ __forceinline__ void net_elem_dispatch(T* __restrict__ lds, const cgp_net_op& op,
                                                  const NetP<T>& p, const Pairs& pr) {
    if constexpr (KIND == CGP_NET_RELU || (KIND == CGP_NET_LINEAR && NP > 1)) {
        switch (op.code) {
            CGP_NET_RESOLUTIONS(CGP_NET_RES_CASE)
        default:
            if constexpr (NP == 1) net_elem<T, EX, DU, KIND, 0, 0, 1>(lds, op, p, pr);
            break;
        }
    } else if constexpr (NP == 1) {
        net_elem<T, EX, DU, KIND, 0, 0, 1>(lds, op, p, pr);
    }
}

template <typename T, bool EX, bool DU, int NP>
__device__ __forceinline__ void net_op(T* __restrict__ lds, const cgp_net_op& op,
                                       const NetP<T>& p, const Pairs& pr, int tid) {
    if (op.zero_halo) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int qa = NP == 1 ? 0 : q * p.lds_elems;
            zero_halos<T, kNT>(lds + qa, op.dst, op.zero_halo & 0xffff, op.h, op.w,
                                     op.ws_out, tid);
            zero_halos<T, kNT>(lds + qa, op.dst2, (unsigned)op.zero_halo >> 16, op.h, op.w,
                       op.ws_out, tid);
        }
    }
    switch (op.kind) {
    case CGP_NET_CONV:
        switch (op.code & CGP_NET_CODE_GEOMETRY) {
            CGP_NET_GEOMETRIES(CGP_NET_CASE)
        default:
            break;
        }
        break;
    case CGP_NET_RELU:
        net_elem_dispatch<T, EX, DU, CGP_NET_RELU, NP>(lds, op, p, pr);
        break;
    case CGP_NET_MOMENTS:
        net_elem_dispatch<T, EX, DU, CGP_NET_MOMENTS, NP>(lds, op, p, pr);
        break;
    case CGP_NET_LINEAR:
        net_elem_dispatch<T, EX, DU, CGP_NET_LINEAR, NP>(lds, op, p, pr);
        break;
    case CGP_NET_LOAD:
        net_move<T, CGP_NET_LOAD, NP>(lds, op, p, pr);
        break;
    case CGP_NET_STORE:
        net_move<T, CGP_NET_STORE, NP>(lds, op, p, pr);
        break;
    default:
        break;
    }
}

// ---- compiled programs ------------------------------------------------------------
// The lowered op lists of the reference configs (tools/gen_net_programs.py ->
// net_programs.h).  A program kernel runs its ops as straight-line code: kind, geometry,
// LDS offsets and strides are immediates, only weight / bias / variance pointers are read
// from the launch's op records.  The host picks it with cgp_net_program().
// compiled programs take their convs' ReLU scaling (w/4, b/4) from prog_recs, applied once
// per workgroup (two VALU ops less per conv and pair); CGP_NET_PRESCALE=0: per op as before
#ifndef CGP_NET_PRESCALE
#define CGP_NET_PRESCALE 1
#endif
constexpr bool kNetPrescale = CGP_NET_PRESCALE != 0;
struct ProgOp {
    int kind, code, src, dst, add, ws_in, ws_out, relu, h, w, dst2, zero_halo;
};
struct ProgInfo {
    int first, nops, pairs, dual, lds_elems, sizes;
};
#include "net_programs.h"
constexpr int kNumProgs = sizeof(kProgs) / sizeof(kProgs[0]);

// The runtime fields of a compiled program's op records (weight, bias, variance / state
// pointers), copied into LDS once per workgroup: an op then starts with an LDS read of its
// pointers instead of a dependent global load of its record (round 4, one B = 1024 Kxz tile,
// two rounds in one call, profiles/r4/ab_r4d_rec_pre.log: ConvNet +1.2%, mnist_as_tf +1.8%,
// cifar10 +2.7%).  Issuing op k + 1's variance loads at the end of op k instead measured
// -2.8% on ConvNet and neutral elsewhere (same log): the wave priority already overlaps them.
struct ProgRec {
    double weight, bias;
    const void* var_x;
    const void* var_y;
    const void* var2_x;
    const void* var2_y;
};
template <int PID>
constexpr int kRecsOf = PID >= 0 ? kProgs[PID < 0 ? 0 : PID].nops : 1;

// op K of program PID as a record: compile-time fields from the program, runtime ones
// (weight, bias, variance / state pointers) from the launch's op records
template <int PID, int K>
__device__ __forceinline__ cgp_net_op prog_op(const ProgRec* recs) {
    constexpr ProgOp o = kProgOps[kProgs[PID].first + K];
    const ProgRec& rt = recs[K];
    cgp_net_op op;
    op.kind = o.kind;
    op.code = o.code;
    op.src = o.src;
    op.dst = o.dst;
    op.add = o.add;
    op.ws_in = o.ws_in;
    op.ws_out = o.ws_out;
    op.relu = o.relu;
    op.h = o.h;
    op.w = o.w;
    op.div_m = 0;
    op.div_s = 0;
    op.dst2 = o.dst2;
    op.zero_halo = o.zero_halo;
    op.weight = rt.weight;
    op.bias = rt.bias;
    op.var_x = rt.var_x;
    op.var_y = rt.var_y;
    op.var2_x = rt.var2_x;
    op.var2_y = rt.var2_y;
    return op;
}
// the conv geometry of a program op
template <int PID, int K, int NP>
struct ProgGeo {
    static constexpr ProgOp o = kProgOps[kProgs[PID].first + K];
    static constexpr GeoRow g = kGeoTable[o.code & CGP_NET_CODE_GEOMETRY];
    using G = NG<g.h, g.w, g.ho, g.wo, g.taps, g.s, g.off, NP>;
};
// ---- the lean chain of a program (round 8) -------------------------------
// Two operations of the one-root ReLU (relu_q_n) are idle at most conv+ReLU sites when every
// CONV record of the launch passes lean_rec_ok: the cap of Y (NOCAP: both variances are at
// least b) and the c + |c| of the output (HALF: the input is non-negative; the site stores
// out/2 and the convs that read it take 2w).  prog_lean walks a program's ops once and keeps
// two facts per slot — an LDS interval [lo, hi) written by one op:
//   nonneg: written by a ReLU (conv epilogue, dst2 or standalone; plus a non-negative
//           addend, if any) or by a conv of a non-negative slot (plus the same);
//   halved: holds out/2.
// Slots written by CGP_NET_LOAD, MOMENTS (signed images) or LINEAR (its coefficients are not
// part of the predicate) have no facts.  A conv+ReLU stores halved only if it has no addend
// and no dst2 and, until its interval is overwritten whole, every op that touches it is a
// CONV reading it as `src` from its origin (never `add`, never RELU / LINEAR / STORE, no
// partial overwrite).  A CGP_NET_CODE_SUM conv never stores its map: its one reader is the
// FROM_SUM reduction that follows.  A halved map still live when the program ends can only
// be read as the launch's final slot, which net_impl checks (lean_final_clash).
// Standalone RELU ops and dst2 ReLUs keep the default form.
__host__ __device__ inline bool lean_rec_ok(double w, double b) {
    // finite 0 <= w <= 2^60, 2^-60 <= b <= 2^60 (every comparison is false on NaN)
    return w >= 0.0 && w <= 0x1p60 && b >= 0x1p-60 && b <= 0x1p60;
}
constexpr int kMaxProgOps = 24;   // at most 32: ProgLean::dbl_mask
struct LeanOp {
    bool nocap = false, half = false, dbl = false;   // dbl: the conv's source is halved (2w)
};
struct ProgLean {
    LeanOp op[kMaxProgOps] = {};
    unsigned dbl_mask = 0;   // bit k: op[k].dbl
    int capfree = 0, addfree = 0;
    int nend = 0, end_lo[4] = {}, end_hi[4] = {};   // halved maps live at the program's end
    bool bad = false;                                // an op list the walk does not cover
};
struct LeanFact {
    int lo = 0, hi = 0;
    bool nonneg = false, halved = false;
};
constexpr bool lean_overlap(int lo, int hi, int lo2, int hi2) { return lo < hi2 && lo2 < hi; }
constexpr bool op_is_sum(const ProgOp& o) {
    return o.kind == CGP_NET_CONV && (o.code & CGP_NET_CODE_SUM) != 0;
}
// the interval op o reads through src / add and writes through dst / dst2 (hi == lo: none)
constexpr int op_src_hi(const ProgOp& o) {
    if (o.kind == CGP_NET_CONV) return o.src + kGeoTable[o.code & CGP_NET_CODE_GEOMETRY].h * o.ws_in;
    if (o.kind == CGP_NET_RELU || o.kind == CGP_NET_LINEAR || o.kind == CGP_NET_STORE)
        return o.src + o.h * o.ws_in;
    return o.src;
}
constexpr bool op_reads_add(const ProgOp& o) {
    return (o.kind == CGP_NET_CONV || o.kind == CGP_NET_RELU) ? o.add >= 0
                                                              : o.kind == CGP_NET_LINEAR;
}
constexpr bool op_writes_dst(const ProgOp& o) { return o.kind != CGP_NET_STORE; }
constexpr int op_ext(const ProgOp& o) { return o.h * o.ws_out; }
// may the conv+ReLU op k of [ops, ops + n) store out/2 at [lo, hi)?  (*end: live at the end)
constexpr bool lean_can_halve(const ProgOp* ops, int n, int k, int lo, int hi, bool* end) {
    *end = false;
    for (int m = k + 1; m < n; ++m) {
        const ProgOp& r = ops[m];
        if (op_reads_add(r) && lean_overlap(lo, hi, r.add, r.add + op_ext(r))) return false;
        if (lean_overlap(lo, hi, r.src, op_src_hi(r)) &&
            !(r.kind == CGP_NET_CONV && r.src == lo && op_src_hi(r) <= hi))
            return false;
        if (op_is_sum(r)) continue;   // no store
        if (op_writes_dst(r) && lean_overlap(lo, hi, r.dst, r.dst + op_ext(r))) {
            if (r.dst <= lo && r.dst + op_ext(r) >= hi) return true;
            return false;
        }
        if (r.dst2 >= 0 && lean_overlap(lo, hi, r.dst2, r.dst2 + op_ext(r))) {
            if (r.dst2 <= lo && r.dst2 + op_ext(r) >= hi) return true;
            return false;
        }
    }
    if (op_is_sum(ops[k]))   // never stored: read by the FROM_SUM reduction alone
        return k + 1 < n && ops[k + 1].kind == CGP_NET_CONV &&
               (ops[k + 1].code & CGP_NET_CODE_FROM_SUM) != 0 && ops[k + 1].src == lo;
    *end = true;
    return true;
}
constexpr ProgLean prog_lean(int pid) {
    ProgLean L{};
    const ProgInfo I = kProgs[pid];
    const ProgOp* ops = kProgOps + I.first;
    if (I.nops > kMaxProgOps) {
        L.bad = true;
        return L;
    }
    // one-pair code without dual outputs only (one pair per workgroup, or the two-pair
    // head's halves).  The 4- and 16-pair stages gain registers with a second chain; the
    // dual-output heads (the ResNets') measured 0.3-1% slower on their default chain with a
    // lean one beside it (profiles/r8/ab_r8a_heads.txt), and the reference ResNets, whose
    // convs have no bias, never take it
    if (I.pairs > 2 || I.dual) return L;
    constexpr int kMaxFacts = 8;
    LeanFact f[kMaxFacts] = {};
    int nf = 0;
    auto find = [&](int lo, int hi) -> const LeanFact* {   // the fact a read of [lo, hi) sees
        for (int n = 0; n < nf; ++n)
            if (f[n].lo == lo && hi <= f[n].hi) return &f[n];
        return nullptr;
    };
    auto touches_halved = [&](int lo, int hi) {
        for (int n = 0; n < nf; ++n)
            if (f[n].halved && lean_overlap(lo, hi, f[n].lo, f[n].hi)) return true;
        return false;
    };
    auto write = [&](int lo, int hi, bool nonneg, bool halved) {
        int m = 0;
        for (int n = 0; n < nf; ++n)
            if (!lean_overlap(lo, hi, f[n].lo, f[n].hi)) f[m++] = f[n];
        nf = m;
        if (!nonneg) return;        // no facts: not kept
        if (nf == kMaxFacts) {      // table full: forget the fact (halved ones must stay)
            if (halved) L.bad = true;
            return;
        }
        f[nf].lo = lo;
        f[nf].hi = hi;
        f[nf].nonneg = nonneg;
        f[nf].halved = halved;
        ++nf;
    };
    for (int k = 0; k < I.nops; ++k) {
        const ProgOp& o = ops[k];
        const int ext = op_ext(o);
        const LeanFact* fs = find(o.src, op_src_hi(o));
        const LeanFact* fa = op_reads_add(o) ? find(o.add, o.add + ext) : nullptr;
        const bool add_nn = !op_reads_add(o) || (fa && fa->nonneg);
        // a halved map is read by convs through src from its origin only (lean_can_halve)
        if (op_reads_add(o) && touches_halved(o.add, o.add + ext)) L.bad = true;
        if (o.kind != CGP_NET_CONV && op_src_hi(o) > o.src && touches_halved(o.src, op_src_hi(o)))
            L.bad = true;
        if (o.kind == CGP_NET_CONV) {
            if (touches_halved(o.src, op_src_hi(o)) && !(fs && fs->halved)) L.bad = true;
            const bool src_nn = fs && fs->nonneg;
            L.op[k].dbl = fs && fs->halved;
            if (L.op[k].dbl) L.dbl_mask |= 1u << k;
            bool half = false;
            if (o.relu) {
                L.op[k].nocap = true;
                ++L.capfree;
                bool end = false;
                half = src_nn && o.add < 0 && o.dst2 < 0 &&
                       lean_can_halve(ops, I.nops, k, o.dst, o.dst + ext, &end);
                if (half && end) {
                    if (L.nend == 4) {
                        half = false;
                    } else {
                        L.end_lo[L.nend] = o.dst;
                        L.end_hi[L.nend++] = o.dst + ext;
                    }
                }
                L.op[k].half = half;
                L.addfree += half;
            }
            write(o.dst, o.dst + ext, (o.relu || src_nn) && add_nn, half);
            if (o.dst2 >= 0) write(o.dst2, o.dst2 + ext, true, false);
        } else if (o.kind == CGP_NET_RELU) {
            write(o.dst, o.dst + ext, add_nn, false);
        } else if (o.kind == CGP_NET_LINEAR) {
            write(o.dst, o.dst + ext, false, false);
            if (o.dst2 >= 0) write(o.dst2, o.dst2 + ext, true, false);
        } else if (o.kind == CGP_NET_MOMENTS || o.kind == CGP_NET_LOAD) {
            write(o.dst, o.dst + ext, false, false);
        }
    }
    return L;
}
template <int PID>
struct LeanOf {
    static constexpr ProgLean L = prog_lean(PID < 0 ? 0 : PID);
    static_assert(!L.bad, "prog_lean: a program the slot walk does not cover");
};
// the same walks for the host (cgp_net_program_lean, net_impl)
#define CGP_LEAN_ROW(k) LeanOf<k>::L,
constexpr ProgLean kLeanTab[] = {CGP_NET_PROGRAMS(CGP_LEAN_ROW)};
#undef CGP_LEAN_ROW
// would the launch's final slot read a map the lean chain of program pid leaves halved?
bool lean_final_clash(int pid, int final_slot) {
    const ProgLean& L = kLeanTab[pid];
    for (int n = 0; n < L.nend; ++n)
        if (final_slot >= L.end_lo[n] && final_slot < L.end_hi[n]) return true;
    return false;
}
// a program kernel carries the lean chain beside the default one: fp64, with a site to gain
template <typename T, int PID>
constexpr bool kLeanProg = PID >= 0 && kReluLean && sizeof(T) == 8 &&
                           LeanOf<PID>::L.capfree + LeanOf<PID>::L.addfree > 0;

// ---- one item decode per walk (CGP_NET_HOIST, ConvHoist) -------------------------------
// is op o a separable conv (row pass + column pass through the row-sum scratch)?
constexpr bool op_separable(const ProgOp& o) {
    if (o.kind != CGP_NET_CONV) return false;
    const GeoRow& g = kGeoTable[o.code & CGP_NET_CODE_GEOMETRY];
    const bool point = g.taps == 1 && g.off == 0;
    const bool reduce = g.ho == 1 && g.wo == 1 && g.off == 0 && g.taps == g.h && g.taps == g.w;
    return !point && !reduce && g.taps > 3;
}
// the first separable conv of program pid if every separable conv of it has that one's
// geometry and pitches and the program runs one pair per workgroup (half), else -1
constexpr int prog_hoist_op(int pid) {
    const ProgInfo I = kProgs[pid];
    if (I.pairs > 2) return -1;
    int first = -1;
    for (int k = 0; k < I.nops; ++k) {
        const ProgOp& o = kProgOps[I.first + k];
        if (!op_separable(o)) continue;
        if (first < 0) first = k;
        const ProgOp& f = kProgOps[I.first + first];
        if ((o.code & CGP_NET_CODE_GEOMETRY) != (f.code & CGP_NET_CODE_GEOMETRY) ||
            o.ws_in != f.ws_in || o.ws_out != f.ws_out)
            return -1;
    }
    return first;
}
// fp64 closed-form program kernels only (fp32 is bound by latency, not by issue)
template <typename T, int PID>
constexpr bool kHoistProg = CGP_NET_HOIST != 0 && PID >= 0 && sizeof(T) == 8 &&
                            prog_hoist_op(PID < 0 ? 0 : PID) >= 0;

// the geometry of the program's hoisted conv (op HK), or a stand-in where it has none
struct NoGeo {
    enum { HO = 0, WO = 1, R3 = 1, NG3 = 0 };
};
template <int PID, int HK, bool ON>
struct HoistGeo {
    using G = NoGeo;
};
template <int PID, int HK>
struct HoistGeo<PID, HK, true> {
    using G = typename ProgGeo<PID, HK, 1>::G;
};

// LEAN: the lean chain (the workgroup found every CONV record lean_rec_ok; prog_recs then
// holds 2w for the convs that read a halved map)
template <typename T, bool DU, int NP, int PID, int K, bool LEAN = false>
__device__ __forceinline__ void prog_ops(T* __restrict__ lds, const NetP<T>& p, const Pairs& pr,
                                         int tid, const ProgRec* recs,
                                         const ConvHoist<T>& hx) {
    constexpr ProgInfo I = kProgs[PID];
    if constexpr (K < I.nops) {
        constexpr ProgOp o = kProgOps[I.first + K];
        constexpr LeanOp lean = LEAN ? LeanOf<PID>::L.op[K] : LeanOp{};
        const cgp_net_op op = prog_op<PID, K>(recs);
        if constexpr (o.zero_halo != 0) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const int qa = q * I.lds_elems;
                zero_halos<T, kNT>(lds + qa, o.dst, o.zero_halo & 0xffff, o.h, o.w,
                                         o.ws_out, tid);
                zero_halos<T, kNT>(lds + qa, o.dst2, (unsigned)o.zero_halo >> 16, o.h, o.w,
                                         o.ws_out,
                           tid);
            }
        }
        if constexpr (o.kind == CGP_NET_CONV) {
            static_assert(!lean.half || (o.relu && o.add < 0 && o.dst2 < 0), "halved output");
            constexpr bool hoist = kHoistProg<T, PID> && op_separable(o);
            net_conv<T, false, DU, typename ProgGeo<PID, K, NP>::G, kNetPrescale, lean.nocap,
                     lean.half, hoist>(lds, op, p, pr, &hx);
        } else if constexpr (o.kind == CGP_NET_MOMENTS && NP == 1 && CGP_NET_MOMENTS_BATCH != 0 &&
                             o.h * o.w <= CGP_NET_MOMENTS_MAXHW) {
            // on the column items of the hoisted convs where the map has their output's size
            // and pitch (moments_batch)
            constexpr int hk = prog_hoist_op(PID);
            using HG = typename HoistGeo<PID, hk, (hk >= 0)>::G;
            constexpr ProgOp hc = kProgOps[I.first + (hk < 0 ? 0 : hk)];
            constexpr bool items = CGP_NET_MOMENTS_ITEMS != 0 && kHoistProg<T, PID> &&
                                   o.ws_out == hc.ws_out && o.h == HG::HO && o.w == HG::WO &&
                                   HG::NG3 * HG::R3 == HG::HO;
            net_moments<T, DU, o.h, o.w, o.ws_out, o.dst, items, HG>(lds, op, p, pr, hx);
        } else if constexpr (o.kind == CGP_NET_RELU || o.kind == CGP_NET_LINEAR ||
                             o.kind == CGP_NET_MOMENTS) {
            net_elem<T, false, DU, o.kind, o.h, o.w, NP>(lds, op, p, pr);
        } else if constexpr (o.kind == CGP_NET_LOAD || o.kind == CGP_NET_STORE) {
            if constexpr (CGP_NET_MOVE_C)
                net_move_c<T, o.kind, NP, o.h, o.w, o.kind == CGP_NET_LOAD ? o.dst : o.src,
                           o.kind == CGP_NET_LOAD ? o.ws_out : o.ws_in>(lds, op, p, pr);
            else
                net_move<T, o.kind, NP>(lds, op, p, pr);
        }
        lds_barrier();
        prog_ops<T, DU, NP, PID, K + 1, LEAN>(lds, p, pr, tid, recs, hx);
    }
}
// the compiled program whose op list equals ops[0, nops) field by field (host memory), +1;
// 0 if none
int prog_match(const cgp_net_op* ops, int nops, int pairs, int dual, int lds_elems,
               int itemsize) {
    for (int k = 0; k < kNumProgs; ++k) {
        const ProgInfo& I = kProgs[k];
        if (I.nops != nops || I.pairs != pairs || I.dual != dual || I.lds_elems != lds_elems ||
            !(I.sizes & itemsize))
            continue;
        bool eq = true;
        for (int n = 0; n < nops && eq; ++n) {
            const ProgOp& o = kProgOps[I.first + n];
            const cgp_net_op& r = ops[n];
            eq = o.kind == r.kind && o.code == r.code && o.src == r.src && o.dst == r.dst &&
                 o.add == r.add && o.ws_in == r.ws_in && o.ws_out == r.ws_out &&
                 o.relu == r.relu && o.h == r.h && o.w == r.w && o.dst2 == r.dst2 &&
                 o.zero_halo == r.zero_halo;
        }
        if (eq) return k + 1;
    }
    return 0;
}

// WPE: waves per SIMD the register allocation targets (amdgpu_waves_per_eu).  LDS caps
// the resident workgroups per CU (two waves each) at 160 KB / footprint, so allocating
// registers for more waves than that only forces spills; net_launch picks WPE from the
// LDS footprint (net_wpe).  NP: pairs per workgroup (1; 2 on four waves, sharing image i;
// 4 / 16 for small-map stages).
// PID >= 0: compiled program PID instead of the op-record interpreter.
template <typename T, bool EX, bool DU, int WPE, int NP, int PID = -1>
__global__ __launch_bounds__(kNTof<NP>) __attribute__((amdgpu_waves_per_eu(WPE))) void net_kernel(const NetP<T> p) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ unsigned pair_tab[2 * kMaxNP];
    __shared__ T red_part[kUnitsOf<NP> * (kNT / 64)];   // CGP_NET_CODE_SUM partials
    T* lds = reinterpret_cast<T*>(smem_raw);
    const int tid = threadIdx.x;
    constexpr int UN = kUnitsOf<NP>;
    for (int e = tid; e < UN * p.lds_elems; e += kNTof<NP>) lds[e] = T(0);   // halos stay zero
    // a FROM_SUM reduction reads these: zeroed, so an op list that breaks the SUM / FROM_SUM
    // contract (cgp_net_validate) reads zeros, never another launch's LDS
    if (tid < UN * (kNT / 64)) red_part[tid] = T(0);
    __shared__ ProgRec prog_recs[kRecsOf<PID>];
    __shared__ long long next_u[2];
    __shared__ int lean_flag;   // every CONV record of this launch is lean_rec_ok
    static_assert(sizeof(pair_tab) + sizeof(red_part) + sizeof(prog_recs) + sizeof(next_u) +
                      sizeof(lean_flag) <= kStaticLds,
                  "static LDS beyond the reserve the host checks count (kStaticLds)");
    if constexpr (PID >= 0) {
        const ProgOp* po = kProgOps + kProgs[PID < 0 ? 0 : PID].first;
        for (int k = tid; k < kRecsOf<PID>; k += kNTof<NP>) {
            const cgp_net_op& r = p.ops[k];
            // a conv feeding the fp64 closed-form ReLU runs on w/4, b/4 (net_conv): scaled
            // here once per workgroup (exact) instead of per op and pair
            const ProgOp& o = po[k];
            const double qs =
                kNetPrescale && kQuarter<T, false> && o.kind == CGP_NET_CONV && o.relu ? 0.25 : 1.0;
            double ws = qs;
            if constexpr (kLeanProg<T, PID>) {
                // the lean chain's condition, from the records this launch runs on: each
                // filling thread reads every CONV record's weight and bias (a few loads, once
                // per workgroup), so the records it writes and the flag agree
                bool ok = true;
                for (int n = 0; n < kRecsOf<PID>; ++n)
                    if (po[n].kind == CGP_NET_CONV)
                        ok = ok && lean_rec_ok(p.ops[n].weight, p.ops[n].bias);
                // a conv whose source holds out/2 takes 2w (exact: w <= 2^60)
                if (ok && ((LeanOf<PID>::L.dbl_mask >> k) & 1u)) ws *= 2.0;
                if (k == 0) lean_flag = ok;
            }
            prog_recs[k] = ProgRec{r.weight * ws, r.bias * qs, r.var_x, r.var_y, r.var2_x,
                                   r.var2_y};
        }
    }
    lds_barrier();
    // XCD-contiguous work ranges: workgroup b runs on XCD b % 8, so each XCD walks one
    // contiguous run of supertiles and its L2 holds the images/variances they share.
    // Ranges and groups are whole multiples of NP units.
    const unsigned xcd = blockIdx.x % 8;
    const long long span = p.uend - p.ubeg;
    const long long per = ((span + 7) / 8 + UN - 1) / UN * UN;
    const long long beg = p.ubeg + (long long)xcd * per;
    const long long end = beg + per < p.uend ? beg + per : p.uend;
    // the XCD's workgroups take its units in order from one counter, so the pairs in
    // flight on an XCD stay one contiguous window (a few supertiles) whose images and
    // variance maps its L2 holds; a static stride lets workgroups drift apart and the
    // window (and L2 misses) grow.  The next group's index is fetched one pair ahead.
    // two slots used alternately (next_u): a slot is rewritten two advances later, after
    // every thread has passed the barrier of the advance in between, so one barrier suffices
    int adv = 0;
    unsigned long long* ctr = p.work + xcd;
    unsigned long long grab = 0;   // thread 0: the counter value fetched one pair ahead
    if (tid == 0) grab = atomicAdd(ctr, 1ull);
    auto advance = [&]() {
        if (tid == 0) next_u[adv] = beg + (long long)grab * UN;
        lds_barrier();
        const long long v = next_u[adv];
        adv ^= 1;
        return v;
    };
    // the item decode of the program's separable convs, once (ConvHoist): on the arena of this
    // wave's half, as the walk hands it to the ops
    ConvHoist<T> hx{};
    if constexpr (kHoistProg<T, PID>) {
        static_assert(NP <= 2, "hoisted decode: one-pair code");
        constexpr int hk = prog_hoist_op(PID < 0 ? 0 : PID);
        constexpr ProgOp ho = kProgOps[kProgs[PID < 0 ? 0 : PID].first + hk];
        T* lh = lds;
        if constexpr (NP == 2) lh += __builtin_amdgcn_readfirstlane(tid >> 7) * p.lds_elems;
        hx = conv_hoist<T, typename ProgGeo<PID < 0 ? 0 : PID, hk, 1>::G>(lh, p, tid & (kNT - 1),
                                                                        ho.ws_in, ho.ws_out, ho.src,
                                                                        ho.dst);
    }
    // the pair walk (net_walk.inc): the lean chain's when the workgroup found the launch's
    // records lean, else the default one
    if constexpr (kLeanProg<T, PID>) {
        if (__builtin_amdgcn_readfirstlane(lean_flag) != 0) {
#define CGP_WALK_LEAN true
#include "net_walk.inc"
#undef CGP_WALK_LEAN
            return;
        }
    }
#define CGP_WALK_LEAN false
#include "net_walk.inc"
#undef CGP_WALK_LEAN
}

// waves per SIMD the LDS footprint of a workgroup allows (`waves` waves per workgroup,
// 4 SIMDs per CU), clamped to the instantiated register targets 3..5
constexpr int net_wpe(long long lds_bytes, int cap = 5, int waves = kNT / 64) {
    const long long wg = (160LL * 1024) / (lds_bytes + kStaticLds);
    const long long w = wg * waves / 4;
    return w < 3 ? 3 : (w > cap ? cap : (int)w);
}
// register target cap of the fp64 compiled programs (6 waves per SIMD: -1…-2% on the
// ResNets; the multi-pair stages at 4: slower than their 13 spilled VGPRs at 5,
// profiles/r3/ab_r3r_mp_wpe.log); the fp32 programs keep the plain 4 / 5 targets (from
// their LDS capped at 6 / 8: within ±1% except Residual +5%)
constexpr int kProgWpeMax = 5;

// the instantiation for (EX, DU, pairs, LDS footprint of the workgroup): the fp64 closed
// form — the production path — has a register target per occupancy level; fp32 one per
// (DU, pairs); the exact ReLU runs one pair per workgroup
template <typename T, int NP>
const void* net_fn_np(bool du, long long lds_bytes) {
    switch (net_wpe(lds_bytes, 5, kNTof<NP> / 64)) {
    case 3: return du ? (const void*)net_kernel<T, false, true, 3, NP>
                      : (const void*)net_kernel<T, false, false, 3, NP>;
    case 4: return du ? (const void*)net_kernel<T, false, true, 4, NP>
                      : (const void*)net_kernel<T, false, false, 4, NP>;
    default:   // the interpreter's dual-output instantiation spills at 5 waves: 4
        return du ? (const void*)net_kernel<T, false, true, 4, NP>
                  : (const void*)net_kernel<T, false, false, 5, NP>;
    }
}
template <typename T>
const void* net_fn(bool ex, bool du, int np, long long lds_bytes) {
    if (ex) {
        if (np != 1) return nullptr;
        return du ? (const void*)net_kernel<T, true, true, 3, 1>
                  : (const void*)net_kernel<T, true, false, 3, 1>;
    }
    if constexpr (sizeof(T) == 8) {
        switch (np) {
        case 1: return net_fn_np<T, 1>(du, lds_bytes);
        case 2: return net_fn_np<T, 2>(du, lds_bytes);
        case 4: return net_fn_np<T, 4>(du, lds_bytes);
        case 16: return net_fn_np<T, 16>(du, lds_bytes);
        default: return nullptr;
        }
    }
    // fp32: one register target per (DU, pairs)
    switch (np) {
    case 1: return du ? (const void*)net_kernel<T, false, true, 4, 1>
                      : (const void*)net_kernel<T, false, false, 5, 1>;
    case 2: return du ? (const void*)net_kernel<T, false, true, 4, 2>
                      : (const void*)net_kernel<T, false, false, 5, 2>;
    case 4: return du ? (const void*)net_kernel<T, false, true, 4, 4>
                      : (const void*)net_kernel<T, false, false, 5, 4>;
    case 16: return du ? (const void*)net_kernel<T, false, true, 4, 16>
                       : (const void*)net_kernel<T, false, false, 5, 16>;
    default: return nullptr;
    }
}

// program kernels: fp64 register target from the program's LDS footprint, fp32 as net_fn
template <typename T, int PID>
const void* prog_fn_one() {
    constexpr ProgInfo I = kProgs[PID];
    if constexpr ((I.sizes & (int)sizeof(T)) == 0) {
        return nullptr;
    } else {
        constexpr long long bytes =
            (long long)I.lds_elems * (long long)sizeof(T) * kUnitsOf<I.pairs>;
        constexpr int wpe = sizeof(T) == 8 ? net_wpe(bytes, kProgWpeMax, kNTof<I.pairs> / 64)
                                           : (I.dual ? 4 : 5);
        return (const void*)net_kernel<T, false, I.dual != 0, wpe, I.pairs, PID>;
    }
}
template <typename T>
const void* prog_fn(int pid) {
    switch (pid) {
#define CGP_PROG_CASE(k) \
    case k: return prog_fn_one<T, k>();
        CGP_NET_PROGRAMS(CGP_PROG_CASE)
#undef CGP_PROG_CASE
    default: return nullptr;
    }
}

// threads of a workgroup of np pairs (kNTof at run time)
int net_threads(int np) { return np == 2 ? kNTof<2> : kNT; }
// pair units (arenas) a workgroup of np pairs holds
int net_units(int np) { return np == 2 ? kUnitsOf<2> : np; }

int net_occupancy(const void* fn, int lds_bytes, int threads) {
    if (lds_bytes > 64 * 1024 &&
        hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) !=
            hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

template <typename T>
int net_occupancy_for(int lds_bytes, int flags, int np) {
    const void* fn = net_fn<T>(flags & CGP_FLAG_EXACT_RELU, flags & CGP_FLAG_NET_DUAL, np,
                               (long long)lds_bytes * net_units(np));
    return fn ? net_occupancy(fn, lds_bytes * net_units(np), net_threads(np)) : 0;
}

// Per-XCD unit counters for a launch: 8 × u64 slots of a 64-slot ring owned by the launch
// stream (one ring per (device, stream), allocated on the device that owns the stream),
// zeroed on that stream.  A slot is reused only by a later launch on the same stream, i.e.
// after this one has drained; launches on other streams never see it.  A ring lives as
// long as the process (a stream destroyed and re-created at the same address reuses its
// ring, which is safe: the old stream's launches have drained by then).  (Per-launch
// hipMallocAsync/hipFreeAsync was measured 5% slower on mnist_as_tf: the pool operations
// open gaps between back-to-back kernels.)
unsigned long long* work_counters(hipStream_t s) {
    constexpr int kSlots = 64;
    struct Ring {
        unsigned long long* buf = nullptr;
        unsigned next = 0;
    };
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, Ring> rings;
    int dev = 0;
    if (stream_device(s, &dev) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    unsigned long long* slot = nullptr;
    {
        std::lock_guard<std::mutex> lock(mu);
        Ring& r = rings[{dev, s}];
        if (!r.buf) {
            int cur = 0;
            hipError_t e = hipGetDevice(&cur);
            if (e == hipSuccess && cur != dev) e = hipSetDevice(dev);
            if (e == hipSuccess)
                e = hipMalloc(&r.buf, sizeof(unsigned long long) * 8 * kSlots);
            if (cur != dev) (void)hipSetDevice(cur);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                r.buf = nullptr;
                return nullptr;
            }
        }
        slot = r.buf + 8 * (r.next++ % kSlots);
    }
    if (hipMemsetAsync(slot, 0, sizeof(unsigned long long) * 8, s) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return slot;
}

template <typename T>
int net_launch(const NetP<T>& p, bool ex, bool du, int np, long long lds_bytes, int program,
               void* stream) {
    const long long wg_bytes = lds_bytes * net_units(np);
    const void* fn = program > 0 && !ex ? prog_fn<T>(program - 1) : net_fn<T>(ex, du, np, wg_bytes);
    if (!fn) return fail(CGP_EINVAL, "net: no instantiation for %d pairs per workgroup", np);
    const int per_cu = net_occupancy(fn, (int)wg_bytes, net_threads(np));
    if (per_cu <= 0)
        return fail(CGP_EINVAL, "net: kernel cannot be resident with %lld B LDS", wg_bytes);
    const long long groups = (p.uend - p.ubeg + net_units(np) - 1) / net_units(np);
    long long grid = (long long)per_cu * device_cus();
    if (grid > groups) grid = groups;
    grid = (grid + 7) / 8 * 8;                  // whole XCD rounds
    NetP<T> arg = p;
    hipStream_t s = as_stream(stream);
    arg.work = work_counters(s);
    if (!arg.work) return fail(CGP_EHIP, "net: work counters");
    void* args[] = {&arg};
    const hipError_t e = hipLaunchKernel(fn, dim3((unsigned)grid), dim3(net_threads(np)), args,
                                         (size_t)wg_bytes, s);
    if (e != hipSuccess) return fail(CGP_EHIP, "net_kernel launch: %s", hipGetErrorString(e));
    return check_launch("net_kernel");
}

template <typename T>
int net_impl(const cgp_net_args* a, void* stream) {
    if (!a) return fail(CGP_EINVAL, "net: args is NULL");
    if (!a->x || !a->y || !a->out || !a->ops || a->nops <= 0)
        return fail(CGP_EINVAL, "net: NULL pointer or empty op list");
    if (a->n1 <= 0 || a->n2 <= 0 || a->n1 >= (1LL << 31) || a->n2 >= (1LL << 31) ||
        a->ldo < a->n2)
        return fail(CGP_EINVAL, "net: bad sizes n1=%lld n2=%lld ldo=%lld", (long long)a->n1,
                    (long long)a->n2, (long long)a->ldo);
    if (a->same && (a->n1 != a->n2 || !a->kdiag))
        return fail(CGP_EINVAL, "net: same tile needs n1 == n2 and kdiag");
    if (a->channels <= 0 || a->h <= 0 || a->w <= 0)
        return fail(CGP_EINVAL, "net: bad image shape");
    const long long lds_bytes = (long long)a->lds_elems * (long long)sizeof(T);
    if (a->lds_elems <= 0 || lds_bytes + kStaticLds > 160 * 1024)
        return fail(CGP_EINVAL, "net: LDS footprint %lld bytes out of range", lds_bytes);
    if (a->final_slot < 0 || a->final_slot >= a->lds_elems || a->hs < 0 ||
        a->hs >= a->lds_elems || a->part < 0 || a->part + 2 > a->lds_elems)
        return fail(CGP_EINVAL, "net: slot offsets out of range");
    NetP<T> p;
    p.x = static_cast<const T*>(a->x);
    p.y = static_cast<const T*>(a->y);
    p.out = static_cast<T*>(a->out);
    p.kdiag = static_cast<const T*>(a->kdiag);
    p.ops = a->ops;
    p.ldo = a->ldo;
    p.n1 = (unsigned)a->n1;
    p.n2 = (unsigned)a->n2;
    p.nbi = (unsigned)((a->n1 + kST - 1) / kST);
    p.nbj = (unsigned)((a->n2 + kST - 1) / kST);
    const long long tiles = a->same ? (long long)p.nbi * (p.nbi + 1) / 2
                                    : (long long)p.nbi * p.nbj;
    if (tiles * kST * kST >= (1LL << 40)) return fail(CGP_EINVAL, "net: tile too large");
    p.units = tiles * kST * kST;
    p.nops = a->nops;
    p.channels = a->channels;
    p.hw_in = a->h * a->w;
    p.same = a->same;
    p.final_slot = a->final_slot;
    p.hs = a->hs;
    p.part = a->part;
    p.lds_elems = a->lds_elems;
    p.exact = (a->flags & CGP_FLAG_EXACT_RELU) ? 1 : 0;
    const int np = a->pairs <= 0 ? 1 : a->pairs;
    if (np != 1 && np != 2 && np != 4 && np != kMaxNP)
        return fail(CGP_EINVAL, "net: %d pairs per workgroup (1, 2, 4 or 16)", np);
    if (lds_bytes * net_units(np) + kStaticLds > 160 * 1024)
        return fail(CGP_EINVAL, "net: %d pairs need %lld B LDS (+ %lld B static)", np,
                    lds_bytes * net_units(np), kStaticLds);
    // multi-pair stages address a pair's variance maps (<= 8 * threads / np pixels) with
    // 32-bit byte offsets (VarSrc)
    if (np > 1 && (a->n1 > a->n2 ? a->n1 : a->n2) * (8LL * net_threads(np) / np) *
                          (long long)sizeof(T) >= (1LL << 32))
        return fail(CGP_EINVAL, "net: %lld images too many for %d pairs per workgroup",
                    (long long)(a->n1 > a->n2 ? a->n1 : a->n2), np);
    if (a->unit_begin == 0 && a->unit_end == 0) {
        p.ubeg = 0;
        p.uend = p.units;
    } else {
        p.ubeg = a->unit_begin;
        p.uend = a->unit_end;
    }
    if (p.ubeg < 0 || p.uend > p.units || p.ubeg >= p.uend || p.ubeg % np)
        return fail(CGP_EINVAL, "net: unit range [%lld, %lld) of %lld", (long long)p.ubeg,
                    (long long)p.uend, (long long)p.units);
    p.final_stage = a->final_stage;
    const bool du = (a->flags & CGP_FLAG_NET_DUAL) != 0;
    const int prog = a->program;
    if (prog < 0 || prog > kNumProgs)
        return fail(CGP_EINVAL, "net: program %d of %d", prog, kNumProgs);
    if (prog > 0) {
        const ProgInfo& I = kProgs[prog - 1];
        if (I.nops != a->nops || I.pairs != np || I.dual != (du ? 1 : 0) ||
            I.lds_elems != a->lds_elems || !(I.sizes & (int)sizeof(T)))
            return fail(CGP_EINVAL, "net: program %d does not fit this op list", prog);
        // the lean chain may leave a map halved when the program ends; NetPlan's final slot
        // is the last op's output, never such a map
        if (kReluLean && sizeof(T) == 8 && !p.exact && a->final_stage &&
            lean_final_clash(prog - 1, a->final_slot))
            return fail(CGP_EINVAL, "net: final slot %d of program %d is a map slot",
                        (int)a->final_slot, prog);
    }
    return net_launch<T>(p, p.exact != 0, du, np, lds_bytes, prog, stream);
}

}  // namespace

extern "C" {

int cgp_net_geometry(int32_t h, int32_t w, int32_t ho, int32_t wo, int32_t taps,
                     int32_t stride, int32_t offset) {
    for (int k = 0; k < kNumGeo; ++k) {
        const GeoRow& g = kGeoTable[k];
        if (g.h == h && g.w == w && g.ho == ho && g.wo == wo && g.taps == taps &&
            g.s == stride && g.off == offset)
            return k;
    }
    return -1;
}

int cgp_net_resolution(int32_t h, int32_t w) { return res_index(h, w); }

size_t cgp_net_op_size(void) { return sizeof(cgp_net_op); }
size_t cgp_net_args_size(void) { return sizeof(cgp_net_args); }

int cgp_net_supertile(void) { return kST; }
// the maps this file's relu_q_n was compiled to read (CGP_RELU_ONE_ROOT)
int cgp_net_var_form(void) { return kNetVarForm; }

int cgp_net_units(int32_t pairs) { return net_units(pairs <= 0 ? 1 : pairs); }

int cgp_net_hs_elems(int32_t code) {
    return (code >= 0 && code < kNumGeo) ? kGeoTable[code].hs_elems : -1;
}

int cgp_net_occupancy(int32_t lds_bytes, int32_t f64, int32_t flags, int32_t pairs) {
    if (pairs <= 0) pairs = 1;
    if (lds_bytes <= 0 || (long long)lds_bytes * pairs > 160 * 1024) return 0;
    return f64 ? net_occupancy_for<double>(lds_bytes, flags, pairs)
               : net_occupancy_for<float>(lds_bytes, flags, pairs);
}

int cgp_net_static_lds(void) { return (int)kStaticLds; }

int cgp_net_validate(const cgp_net_op* ops, int32_t nops, int32_t pairs) {
    if (!ops || nops <= 0) return fail(CGP_EINVAL, "net_validate: NULL or empty op list");
    const int np = pairs <= 0 ? 1 : pairs;
    auto geo = [](const cgp_net_op& r) -> const GeoRow* {
        const int g = r.code & CGP_NET_CODE_GEOMETRY;
        return r.kind == CGP_NET_CONV && r.code >= 0 && g < kNumGeo ? &kGeoTable[g] : nullptr;
    };
    for (int k = 0; k < nops; ++k) {
        const cgp_net_op& r = ops[k];
        const bool sum = r.kind == CGP_NET_CONV && r.code >= 0 && (r.code & CGP_NET_CODE_SUM);
        const bool from = r.kind == CGP_NET_CONV && r.code >= 0 && (r.code & CGP_NET_CODE_FROM_SUM);
        if (sum) {
            const GeoRow* g = geo(r);
            const bool point = g && g->taps == 1 && g->off == 0;
            const bool reduce = g && g->ho == 1 && g->wo == 1 && g->off == 0 &&
                                g->taps == g->h && g->taps == g->w;
            if (!g || g->taps <= 3 || point || reduce)
                return fail(CGP_EINVAL, "net_validate: op %d: CGP_NET_CODE_SUM needs a separable "
                                        "conv (more than 3 taps, not pointwise, not a reduction)", k);
            if (r.add >= 0 || r.dst2 >= 0)
                return fail(CGP_EINVAL, "net_validate: op %d: CGP_NET_CODE_SUM with an addend or "
                                        "a second output", k);
            if (np > 2)
                return fail(CGP_EINVAL, "net_validate: op %d: CGP_NET_CODE_SUM in a %d-pair stage "
                                        "(one pair per workgroup or half only)", k, np);
            if (k + 1 >= nops || !(ops[k + 1].kind == CGP_NET_CONV && ops[k + 1].code >= 0 &&
                                   (ops[k + 1].code & CGP_NET_CODE_FROM_SUM)) ||
                ops[k + 1].src != r.dst)
                return fail(CGP_EINVAL, "net_validate: op %d: CGP_NET_CODE_SUM not followed by the "
                                        "CGP_NET_CODE_FROM_SUM reduction of its map", k);
            for (int m = k + 2; m < nops; ++m)
                if (ops[m].src == r.dst || ops[m].add == r.dst)
                    return fail(CGP_EINVAL, "net_validate: op %d reads the map of SUM op %d, "
                                            "which is never stored", m, k);
        }
        if (from) {
            const GeoRow* g = geo(r);
            const bool reduce = g && g->ho == 1 && g->wo == 1 && g->off == 0 &&
                                g->taps == g->h && g->taps == g->w;
            if (!reduce || np > 2)
                return fail(CGP_EINVAL, "net_validate: op %d: CGP_NET_CODE_FROM_SUM needs a "
                                        "one-pair full-map reduction", k);
            if (k == 0 || !(ops[k - 1].kind == CGP_NET_CONV && ops[k - 1].code >= 0 &&
                            (ops[k - 1].code & CGP_NET_CODE_SUM)))
                return fail(CGP_EINVAL, "net_validate: op %d: CGP_NET_CODE_FROM_SUM without a "
                                        "CGP_NET_CODE_SUM conv before it", k);
        }
    }
    return CGP_OK;
}

int cgp_net_program(const cgp_net_op* ops, int32_t nops, int32_t pairs, int32_t flags,
                    int32_t lds_elems, int32_t itemsize) {
    if (!ops || nops <= 0) return 0;
    return prog_match(ops, nops, pairs <= 0 ? 1 : pairs, (flags & CGP_FLAG_NET_DUAL) ? 1 : 0,
                      lds_elems, itemsize);
}

int cgp_net_program_lean(const cgp_net_op* ops, int32_t nops, int32_t pairs, int32_t flags,
                         int32_t lds_elems, int32_t itemsize, int32_t* capfree,
                         int32_t* addfree) {
    if (!kReluLean || !ops || nops <= 0 || itemsize != 8 || (flags & CGP_FLAG_EXACT_RELU))
        return 0;
    const int k = prog_match(ops, nops, pairs <= 0 ? 1 : pairs,
                             (flags & CGP_FLAG_NET_DUAL) ? 1 : 0, lds_elems, itemsize);
    if (k <= 0) return 0;
    for (int n = 0; n < nops; ++n)
        if (ops[n].kind == CGP_NET_CONV && !lean_rec_ok(ops[n].weight, ops[n].bias)) return 0;
    const ProgLean& L = kLeanTab[k - 1];
    if (capfree) *capfree = L.capfree;
    if (addfree) *addfree = L.addfree;
    return 1;
}

int cgp_net_f64(const cgp_net_args* args, void* stream) { return net_impl<double>(args, stream); }
int cgp_net_f32(const cgp_net_args* args, void* stream) { return net_impl<float>(args, stream); }

}  // extern "C"
