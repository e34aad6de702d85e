// nonlin.hip — the entry points of every nonlinearity: ReLU, erf, GELU, the two-slope ReLU
// the sinusoid and the Hermite series on pair maps (cgp_relu_*, cgp_relu_ntk_*, cgp_erf_*,
// cgp_gelu_*, cgp_abrelu_*, cgp_sin_*, cgp_hermite_*), on the per-image variances (cgp_var_*)
// and on position-pair maps (cgp_cov_nonlin_*, cgp_covntk_nonlin_*, cgp_gelu_cov_*,
// cgp_abrelu_cov_*, cgp_sin_cov_*, cgp_hermite_cov_*), and the series' coefficient kernel
// (cgp_hermite_coef_*).  The kernels and the maps are
// nonlin_walk.h's; here each layout has one check and one launch, named by the entry point
// for the messages.  Every check returns CGP_EINVAL before any HIP call.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cnngp.h"
#include "nonlin_walk.h"

using namespace cgp;

namespace {

inline bool finite3(double s, double m, double h) {
    return std::isfinite(s) && std::isfinite(m) && std::isfinite(h);
}
inline int exact_relu(int flags) { return (flags & CGP_FLAG_EXACT_RELU) != 0; }

template <typename T>
ABReluMap<T> abrelu_map(double s, double m, double h, int flags) {
    return ABReluMap<T>{(T)s, (T)m, (T)h, exact_relu(flags)};
}

// the sinusoid's constants (A, B, C, D) = (a²/2, b²/2, cos 2θ, a²b²/2)
int sin_check(const char* name, double A, double B, double C, double D) {
    if (!(std::isfinite(A) && std::isfinite(B) && std::isfinite(C) && std::isfinite(D)))
        return fail(CGP_EINVAL, "%s: A, B, C or D is not finite", name);
    if (!(A > 0 && B > 0 && std::fabs(C) <= 1))
        return fail(CGP_EINVAL, "%s: needs A > 0, B > 0 and |C| <= 1", name);
    return CGP_OK;
}
template <typename T>
SinMap<T> sin_map(double A, double B, double C, double D) {
    return SinMap<T>{(T)A, (T)B, (T)C, (T)D};
}

// the Hermite series' order and tables (cgp_hermite_args / cgp_hermite_cov_args): n1h / n2h are
// the least strides, 1 where the entry point does not know the buffers' image counts
template <class A>
int hermite_check(const char* name, const A* a, bool need_y, long long n1h, long long n2h) {
    if (a->order < 1 || a->order > CGP_HERMITE_MAX_ORDER)
        return fail(CGP_EINVAL, "%s: order %d is not in [1, %d]", name, a->order,
                    CGP_HERMITE_MAX_ORDER);
    if (!a->ax || (need_y && !a->ay) || (a->theta && (!a->dax || (need_y && !a->day))))
        return fail(CGP_EINVAL, "%s: NULL coefficient table", name);
    if (a->stride_x < n1h || (need_y && a->stride_y < n2h))
        return fail(CGP_EINVAL, "%s: table stride below the variance buffer's size", name);
    return CGP_OK;
}
template <typename T, class A>
HermiteMap<T> hermite_map(const A* a) {
    return HermiteMap<T>{static_cast<const T*>(a->ax),  static_cast<const T*>(a->ay),
                         static_cast<const T*>(a->dax), static_cast<const T*>(a->day),
                         static_cast<const T*>(a->xx),  static_cast<const T*>(a->yy),
                         a->stride_x, a->stride_y, a->order};
}

int hermite_rule_check(const char* name, int phi, int order, int nq, const double* nodes) {
    if (phi < CGP_HERMITE_TANH || phi > CGP_HERMITE_GELU)
        return fail(CGP_EINVAL, "%s: phi %d is not a CGP_HERMITE_* id", name, phi);
    if (order < 1 || order > CGP_HERMITE_MAX_ORDER)
        return fail(CGP_EINVAL, "%s: order %d is not in [1, %d]", name, order,
                    CGP_HERMITE_MAX_ORDER);
    if (nq <= order || nq > CGP_HERMITE_MAX_NODES)
        return fail(CGP_EINVAL, "%s: %d nodes are not in (order, %d]", name, nq,
                    CGP_HERMITE_MAX_NODES);
    if (!nodes) return fail(CGP_EINVAL, "%s: NULL node table", name);
    return CGP_OK;
}

// one launch of the coefficient kernel in the order's bucket; da: grid y = 2
template <typename T>
int hermite_coef_launch(const HermiteCoefP<T>& p, void* stream) {
    const dim3 grid((unsigned)((p.count + kWalkBlock - 1) / kWalkBlock), p.da ? 2 : 1);
    const dim3 block(kWalkBlock);
    hipStream_t s = as_stream(stream);
    if (p.order <= 8)
        hipLaunchKernelGGL((hermite_coef_kernel<T, 8>), grid, block, 0, s, p);
    else if (p.order <= 16)
        hipLaunchKernelGGL((hermite_coef_kernel<T, 16>), grid, block, 0, s, p);
    else if (p.order <= 32)
        hipLaunchKernelGGL((hermite_coef_kernel<T, 32>), grid, block, 0, s, p);
    else
        hipLaunchKernelGGL((hermite_coef_kernel<T, 64>), grid, block, 0, s, p);
    return check_launch("hermite_coef_kernel");
}

template <typename T>
int hermite_coef_impl(const cgp_hermite_coef_args* a, void* stream) {
    if (!a || !a->var || !a->a) return fail(CGP_EINVAL, "hermite_coef: NULL argument");
    if (a->count <= 0 || a->count >= (1LL << 31))
        return fail(CGP_EINVAL, "hermite_coef: bad sizes");
    if (int e = hermite_rule_check("hermite_coef", a->phi, a->order, a->nq, a->nodes)) return e;
    return hermite_coef_launch(
        HermiteCoefP<T>{static_cast<const T*>(a->var), static_cast<T*>(a->a),
                        static_cast<T*>(a->da), nullptr, a->nodes, a->count, a->phi, a->order,
                        a->nq},
        stream);
}

// ----------------------------------------------------------------------------------
// the layer path.  theta == NULL is the forward-only form.
// ----------------------------------------------------------------------------------
struct PairArgs {
    const void* xy;
    const void* theta;
    void* out_xy;
    void* out_theta;
    const void* addend;
    const void* xx;
    const void* yy;
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag;
};
// of cgp_erf_args, cgp_gelu_args, cgp_abrelu_args, cgp_sin_args, cgp_hermite_args; a NULL record gives NULL fields
template <class A>
PairArgs pair_args(const A* a) {
    if (!a) return PairArgs{};
    return PairArgs{a->xy, a->theta, a->out_xy, a->out_theta, a->addend, a->xx, a->yy,
                    a->nmaps, a->n1, a->n2, a->hw, a->same, a->diag};
}
PairArgs pair_args(const cgp_relu_args* a) {
    if (!a) return PairArgs{};
    return PairArgs{a->xy, nullptr, a->out, nullptr, a->addend, a->xx, a->yy,
                    a->nmaps, a->n1, a->n2, a->hw, a->same, a->diag};
}
PairArgs pair_args(const cgp_relu_ntk_args* a) {
    if (!a) return PairArgs{};
    return PairArgs{a->xy, a->theta, a->out_xy, a->out_theta, nullptr, a->xx, a->yy,
                    a->nmaps, a->n1, a->n2, a->hw, a->same, a->diag};
}

// need_theta: cgp_relu_ntk_* has no forward-only form.  diag_only: cgp_relu_* asks n1 == n2
// of diag alone.
int pair_check(const char* name, const PairArgs& a, bool need_theta = false,
               bool diag_only = false) {
    if (!a.xy || !a.out_xy || !a.xx || (a.theta ? !a.out_theta : need_theta))
        return fail(CGP_EINVAL, "%s: NULL argument", name);
    if (a.hw <= 0 || a.nmaps <= 0 || a.nmaps >= (1LL << 31))
        return fail(CGP_EINVAL, "%s: bad sizes", name);
    if (a.n1 <= 0 || a.n2 <= 0 || (a.diag ? a.n1 : a.n1 * a.n2) != a.nmaps)
        return fail(CGP_EINVAL, "%s: nmaps inconsistent with n1/n2/diag", name);
    if (diag_only) {
        if (a.diag && a.n1 != a.n2) return fail(CGP_EINVAL, "%s: diag needs n1 == n2", name);
    } else if ((a.same || a.diag) && a.n1 != a.n2) {
        return fail(CGP_EINVAL, "%s: same / diag need n1 == n2", name);
    }
    if (!(a.same && a.diag) && !a.yy) return fail(CGP_EINVAL, "%s: yy is NULL", name);
    if (a.hw > kWalkChunk) return fail(CGP_EINVAL, "%s: map of %d pixels too large", name, a.hw);
    return CGP_OK;
}

template <typename T, class F>
int pair_launch(const PairArgs& a, const F& f, void* stream) {
    PairWalkP<T, F> p;
    p.xy = static_cast<const T*>(a.xy);
    p.theta = static_cast<const T*>(a.theta);
    p.out_xy = static_cast<T*>(a.out_xy);
    p.out_theta = static_cast<T*>(a.out_theta);
    p.addend = static_cast<const T*>(a.addend);
    p.xx = static_cast<const T*>(a.xx);
    p.yy = static_cast<const T*>(a.yy);
    p.nmaps = a.nmaps;
    p.n2 = make_fastdiv((unsigned)a.n2);
    p.dhw = make_fastdiv((unsigned)a.hw);
    p.hw = a.hw;
    p.same = a.same;
    p.diag = a.diag;
    // whole maps per workgroup, at most kWalkE elements per thread; blocks <= nmaps < 2^31
    p.mpb = std::max(1, kWalkChunk / a.hw);
    p.f = f;
    const dim3 grid((unsigned)((a.nmaps + p.mpb - 1) / p.mpb)), block(kWalkBlock);
    hipStream_t s = as_stream(stream);
    if (a.theta) {
        if (a.addend)
            hipLaunchKernelGGL((pair_walk_kernel<T, F, true, true>), grid, block, 0, s, p);
        else
            hipLaunchKernelGGL((pair_walk_kernel<T, F, true, false>), grid, block, 0, s, p);
    } else {
        if (a.addend)
            hipLaunchKernelGGL((pair_walk_kernel<T, F, false, true>), grid, block, 0, s, p);
        else
            hipLaunchKernelGGL((pair_walk_kernel<T, F, false, false>), grid, block, 0, s, p);
    }
    return check_launch("pair_walk_kernel");
}

template <typename T>
int relu_impl(const cgp_relu_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("relu", c, false, true)) return e;
    return pair_launch<T>(c, ReluMap<T>{exact_relu(a->flags)}, stream);
}
template <typename T>
int relu_ntk_impl(const cgp_relu_ntk_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("relu_ntk", c, true)) return e;
    return pair_launch<T>(c, ReluMap<T>{exact_relu(a->flags)}, stream);
}
template <typename T>
int erf_impl(const cgp_erf_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("erf", c)) return e;
    return pair_launch<T>(c, ErfMap<T>{}, stream);
}
template <typename T>
int gelu_impl(const cgp_gelu_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("gelu", c)) return e;
    return pair_launch<T>(c, GeluMap<T>{}, stream);
}
template <typename T>
int abrelu_impl(const cgp_abrelu_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("abrelu", c)) return e;
    if (!finite3(a->s, a->m, a->h)) return fail(CGP_EINVAL, "abrelu: s, m or h is not finite");
    return pair_launch<T>(c, abrelu_map<T>(a->s, a->m, a->h, a->flags), stream);
}
template <typename T>
int sin_impl(const cgp_sin_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("sin", c)) return e;
    if (int e = sin_check("sin", a->A, a->B, a->C, a->D)) return e;
    return pair_launch<T>(c, sin_map<T>(a->A, a->B, a->C, a->D), stream);
}
template <typename T>
int hermite_impl(const cgp_hermite_args* a, void* stream) {
    const PairArgs c = pair_args(a);
    if (int e = pair_check("hermite", c)) return e;
    if (int e = hermite_check("hermite", a, !(a->same && a->diag), a->n1 * a->hw,
                              a->n2 * a->hw))
        return e;
    return pair_launch<T>(c, hermite_map<T>(a), stream);
}

// ----------------------------------------------------------------------------------
// the per-image variances
// ----------------------------------------------------------------------------------
template <typename T>
struct VarArgs {
    const T* xx;
    const T* yy;
    int64_t n1, n2;
    int32_t hw, same;
    T* xo;
    T* yo;
};

template <typename T>
int var_check(const char* name, const VarArgs<T>& a) {
    if (!a.xx || !a.yy || !a.xo || !a.yo) return fail(CGP_EINVAL, "%s: NULL argument", name);
    if (a.n1 <= 0 || a.n2 <= 0 || a.hw <= 0) return fail(CGP_EINVAL, "%s: bad sizes", name);
    if (a.same && a.n1 != a.n2) return fail(CGP_EINVAL, "%s: same needs n1 == n2", name);
    return CGP_OK;
}

template <typename T, class F>
int var_launch(const VarArgs<T>& a, const F& f, void* stream) {
    const VarWalkP<T, F> p{a.xx, a.yy, a.xo, a.yo, a.n1 * a.hw, a.n2 * a.hw, a.same, f};
    hipLaunchKernelGGL((var_walk_kernel<T, F>), dim3(grid_for(p.n_xx + p.n_yy)),
                       dim3(kWalkBlock), 0, as_stream(stream), p);
    return check_launch("var_walk_kernel");
}

template <typename T, class F>
int var_impl(const char* name, const VarArgs<T>& a, const F& f, void* stream) {
    if (int e = var_check(name, a)) return e;
    return var_launch(a, f, stream);
}

template <typename T>
int var_abrelu_impl(const VarArgs<T>& a, double h, void* stream) {
    if (int e = var_check("var_abrelu", a)) return e;
    if (!std::isfinite(h)) return fail(CGP_EINVAL, "var_abrelu: h is not finite");
    return var_launch(a, ABReluMap<T>{T(0), T(0), (T)h, 0}, stream);
}

template <typename T>
int var_sin_impl(const VarArgs<T>& a, double A, double B, double C, double D, void* stream) {
    if (int e = var_check("var_sin", a)) return e;
    if (int e = sin_check("var_sin", A, B, C, D)) return e;
    return var_launch(a, sin_map<T>(A, B, C, D), stream);
}

// the coefficient kernel with var_out: xx -> xo, then (same ? xx : yy) -> yo
template <typename T>
int var_hermite_impl(const VarArgs<T>& a, int phi, int order, int nq, const double* nodes,
                     void* stream) {
    if (int e = var_check("var_hermite", a)) return e;
    if (int e = hermite_rule_check("var_hermite", phi, order, nq, nodes)) return e;
    if (a.n1 * a.hw >= (1LL << 31) || a.n2 * a.hw >= (1LL << 31))
        return fail(CGP_EINVAL, "var_hermite: bad sizes");
    if (int e = hermite_coef_launch(HermiteCoefP<T>{a.xx, nullptr, nullptr, a.xo, nodes,
                                                    a.n1 * a.hw, phi, order, nq},
                                    stream))
        return e;
    return hermite_coef_launch(HermiteCoefP<T>{a.same ? a.xx : a.yy, nullptr, nullptr, a.yo,
                                               nodes, a.n2 * a.hw, phi, order, nq},
                               stream);
}

// ----------------------------------------------------------------------------------
// position-pair maps.  theta == NULL is the forward-only form.
// ----------------------------------------------------------------------------------
struct CovArgs {
    const void* in;
    const void* theta;
    void* out;
    void* out_theta;
    const void* addend;
    const void* addend_theta;
    const void* xx;
    const void* yy;
    const int32_t* pair_i;
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w, same;
};
// of cgp_covntk_nonlin_args, cgp_abrelu_cov_args, cgp_sin_cov_args, cgp_hermite_cov_args; a NULL record gives NULL fields
template <class A>
CovArgs cov_args(const A* a) {
    if (!a) return CovArgs{};
    return CovArgs{a->in, a->theta, a->out, a->out_theta, a->addend, a->addend_theta, a->xx,
                   a->yy, a->pair_i, a->pair_j, a->npairs, a->h, a->w, a->same};
}
// of cgp_cov_nonlin_args, cgp_gelu_cov_args
template <class A>
CovArgs cov_args_forward(const A* a) {
    if (!a) return CovArgs{};
    return CovArgs{a->in, nullptr, a->out, nullptr, a->addend, nullptr, a->xx,
                   a->yy, a->pair_i, a->pair_j, a->npairs, a->h, a->w, a->same};
}

// need_theta: cgp_covntk_nonlin_* has no forward-only form
int cov_check(const char* name, const CovArgs& a, bool need_theta = false) {
    if (!a.in || !a.out || !a.xx || !a.yy || !a.pair_i || !a.pair_j ||
        (a.theta ? !a.out_theta : need_theta))
        return fail(CGP_EINVAL, "%s: NULL argument", name);
    if (a.theta && a.out == a.out_theta)
        return fail(CGP_EINVAL, "%s: out and out_theta are one buffer", name);
    if (a.npairs <= 0 || a.npairs >= (1LL << 31) || bad_map(a.h, a.w))
        return fail(CGP_EINVAL, "%s: bad sizes", name);
    return CGP_OK;
}

template <typename T, class F>
int cov_launch(const char* name, const CovArgs& a, const F& f, void* stream) {
    CovWalkP<T, F> p;
    p.in = static_cast<const T*>(a.in);
    p.theta = static_cast<const T*>(a.theta);
    p.out = static_cast<T*>(a.out);
    p.out_theta = static_cast<T*>(a.out_theta);
    p.addend = static_cast<const T*>(a.addend);
    p.addend_theta = static_cast<const T*>(a.addend_theta);
    p.xx = static_cast<const T*>(a.xx);
    p.yy = static_cast<const T*>(a.yy);
    p.pi = a.pair_i;
    p.pj = a.pair_j;
    p.total = (long long)a.npairs * a.h * a.w * a.h * a.w;
    p.g = make_idx(a.h, a.w);
    p.hw = a.h * a.w;
    p.same = a.same != 0;
    p.f = f;
    const long long blocks = (p.total + kWalkChunk - 1) / kWalkChunk;
    if (blocks >= (1LL << 31)) return fail(CGP_EINVAL, "%s: %lld elements", name, p.total);
    const dim3 grid((unsigned)blocks), block(kWalkBlock);
    hipStream_t s = as_stream(stream);
    if (a.theta) {
        if (a.addend || a.addend_theta)
            hipLaunchKernelGGL((cov_walk_kernel<T, F, true, true>), grid, block, 0, s, p);
        else
            hipLaunchKernelGGL((cov_walk_kernel<T, F, true, false>), grid, block, 0, s, p);
    } else {
        if (a.addend)
            hipLaunchKernelGGL((cov_walk_kernel<T, F, false, true>), grid, block, 0, s, p);
        else
            hipLaunchKernelGGL((cov_walk_kernel<T, F, false, false>), grid, block, 0, s, p);
    }
    return check_launch("cov_walk_kernel");
}

// the run-time kind of cgp_cov_nonlin_* / cgp_covntk_nonlin_*, checked by the caller
template <typename T>
int cov_launch_kind(const char* name, const CovArgs& a, int kind, int flags, void* stream) {
    switch (kind) {
        case CGP_COV_RELU: return cov_launch<T>(name, a, ReluMap<T>{exact_relu(flags)}, stream);
        case CGP_COV_ERF: return cov_launch<T>(name, a, ErfMap<T>{}, stream);
        default: return cov_launch<T>(name, a, GeluMap<T>{}, stream);
    }
}

template <typename T>
int cov_nonlin_impl(const cgp_cov_nonlin_args* a, void* stream) {
    const CovArgs c = cov_args_forward(a);
    if (int e = cov_check("cov_nonlin", c)) return e;
    if (a->kind != CGP_COV_RELU && a->kind != CGP_COV_ERF)
        return fail(CGP_EINVAL, "cov_nonlin: kind %d is neither ReLU nor erf", a->kind);
    return cov_launch_kind<T>("cov_nonlin", c, a->kind, a->flags, stream);
}
template <typename T>
int cov_nonlin_ntk_impl(const cgp_covntk_nonlin_args* a, void* stream) {
    const CovArgs c = cov_args(a);
    if (int e = cov_check("cov_nonlin_ntk", c, true)) return e;
    if (a->kind != CGP_COV_RELU && a->kind != CGP_COV_ERF && a->kind != CGP_COV_GELU)
        return fail(CGP_EINVAL, "cov_nonlin_ntk: kind %d is neither ReLU, erf nor GELU", a->kind);
    return cov_launch_kind<T>("cov_nonlin_ntk", c, a->kind, a->flags, stream);
}
template <typename T>
int gelu_cov_impl(const cgp_gelu_cov_args* a, void* stream) {
    const CovArgs c = cov_args_forward(a);
    if (int e = cov_check("gelu_cov", c)) return e;
    return cov_launch<T>("gelu_cov", c, GeluMap<T>{}, stream);
}
template <typename T>
int abrelu_cov_impl(const cgp_abrelu_cov_args* a, void* stream) {
    const CovArgs c = cov_args(a);
    if (int e = cov_check("abrelu_cov", c)) return e;
    if (!finite3(a->s, a->m, a->hh))
        return fail(CGP_EINVAL, "abrelu_cov: s, m or hh is not finite");
    return cov_launch<T>("abrelu_cov", c, abrelu_map<T>(a->s, a->m, a->hh, a->flags), stream);
}
template <typename T>
int sin_cov_impl(const cgp_sin_cov_args* a, void* stream) {
    const CovArgs c = cov_args(a);
    if (int e = cov_check("sin_cov", c)) return e;
    if (int e = sin_check("sin_cov", a->A, a->B, a->C, a->D)) return e;
    return cov_launch<T>("sin_cov", c, sin_map<T>(a->A, a->B, a->C, a->D), stream);
}
template <typename T>
int hermite_cov_impl(const cgp_hermite_cov_args* a, void* stream) {
    const CovArgs c = cov_args(a);
    if (int e = cov_check("hermite_cov", c)) return e;
    if (int e = hermite_check("hermite_cov", a, true, (long long)a->h * a->w,
                              (long long)a->h * a->w))
        return e;
    return cov_launch<T>("hermite_cov", c, hermite_map<T>(a), stream);
}

}  // namespace

extern "C" {

size_t cgp_relu_args_size(void) { return sizeof(cgp_relu_args); }
size_t cgp_relu_ntk_args_size(void) { return sizeof(cgp_relu_ntk_args); }
size_t cgp_erf_args_size(void) { return sizeof(cgp_erf_args); }
size_t cgp_gelu_args_size(void) { return sizeof(cgp_gelu_args); }
size_t cgp_abrelu_args_size(void) { return sizeof(cgp_abrelu_args); }
size_t cgp_cov_nonlin_args_size(void) { return sizeof(cgp_cov_nonlin_args); }
size_t cgp_covntk_nonlin_args_size(void) { return sizeof(cgp_covntk_nonlin_args); }
size_t cgp_gelu_cov_args_size(void) { return sizeof(cgp_gelu_cov_args); }
size_t cgp_abrelu_cov_args_size(void) { return sizeof(cgp_abrelu_cov_args); }
size_t cgp_sin_args_size(void) { return sizeof(cgp_sin_args); }
size_t cgp_sin_cov_args_size(void) { return sizeof(cgp_sin_cov_args); }
size_t cgp_hermite_coef_args_size(void) { return sizeof(cgp_hermite_coef_args); }
size_t cgp_hermite_args_size(void) { return sizeof(cgp_hermite_args); }
size_t cgp_hermite_cov_args_size(void) { return sizeof(cgp_hermite_cov_args); }

#define CGP_NONLIN_ENTRY(name, impl, args)                                                \
    int name##_f64(const args* a, void* stream) { return impl<double>(a, stream); }       \
    int name##_f32(const args* a, void* stream) { return impl<float>(a, stream); }
CGP_NONLIN_ENTRY(cgp_relu, relu_impl, cgp_relu_args)
CGP_NONLIN_ENTRY(cgp_relu_ntk, relu_ntk_impl, cgp_relu_ntk_args)
CGP_NONLIN_ENTRY(cgp_erf, erf_impl, cgp_erf_args)
CGP_NONLIN_ENTRY(cgp_gelu, gelu_impl, cgp_gelu_args)
CGP_NONLIN_ENTRY(cgp_abrelu, abrelu_impl, cgp_abrelu_args)
CGP_NONLIN_ENTRY(cgp_cov_nonlin, cov_nonlin_impl, cgp_cov_nonlin_args)
CGP_NONLIN_ENTRY(cgp_covntk_nonlin, cov_nonlin_ntk_impl, cgp_covntk_nonlin_args)
CGP_NONLIN_ENTRY(cgp_gelu_cov, gelu_cov_impl, cgp_gelu_cov_args)
CGP_NONLIN_ENTRY(cgp_abrelu_cov, abrelu_cov_impl, cgp_abrelu_cov_args)
CGP_NONLIN_ENTRY(cgp_sin, sin_impl, cgp_sin_args)
CGP_NONLIN_ENTRY(cgp_sin_cov, sin_cov_impl, cgp_sin_cov_args)
CGP_NONLIN_ENTRY(cgp_hermite_coef, hermite_coef_impl, cgp_hermite_coef_args)
CGP_NONLIN_ENTRY(cgp_hermite, hermite_impl, cgp_hermite_args)
CGP_NONLIN_ENTRY(cgp_hermite_cov, hermite_cov_impl, cgp_hermite_cov_args)
#undef CGP_NONLIN_ENTRY

#define CGP_VAR_ENTRY(name, T, sfx, Map)                                                   \
    int cgp_##name##_##sfx(const T* xx, const T* yy, int64_t n1, int64_t n2, int32_t hw,   \
                           int32_t same, T* xx_out, T* yy_out, void* stream) {             \
        return var_impl(#name, VarArgs<T>{xx, yy, n1, n2, hw, same, xx_out, yy_out},       \
                        Map<T>{}, stream);                                                 \
    }
CGP_VAR_ENTRY(var_relu, double, f64, ReluMap)
CGP_VAR_ENTRY(var_relu, float, f32, ReluMap)
CGP_VAR_ENTRY(var_erf, double, f64, ErfMap)
CGP_VAR_ENTRY(var_erf, float, f32, ErfMap)
CGP_VAR_ENTRY(var_gelu, double, f64, GeluMap)
CGP_VAR_ENTRY(var_gelu, float, f32, GeluMap)
#undef CGP_VAR_ENTRY

int cgp_var_abrelu_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                       int32_t same, double h, double* xx_out, double* yy_out, void* stream) {
    return var_abrelu_impl(VarArgs<double>{xx, yy, n1, n2, hw, same, xx_out, yy_out}, h, stream);
}
int cgp_var_abrelu_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                       int32_t same, double h, float* xx_out, float* yy_out, void* stream) {
    return var_abrelu_impl(VarArgs<float>{xx, yy, n1, n2, hw, same, xx_out, yy_out}, h, stream);
}

// the sinusoid's constants stand between `same` and the outputs
#define CGP_VAR_SIN_ENTRY(T, sfx)                                                            \
    int cgp_var_sin_##sfx(const T* xx, const T* yy, int64_t n1, int64_t n2, int32_t hw,      \
                          int32_t same, double A, double B, double C, double D, T* xx_out,   \
                          T* yy_out, void* stream) {                                         \
        return var_sin_impl(VarArgs<T>{xx, yy, n1, n2, hw, same, xx_out, yy_out}, A, B, C,   \
                            D, stream);                                                      \
    }
CGP_VAR_SIN_ENTRY(double, f64)
CGP_VAR_SIN_ENTRY(float, f32)
#undef CGP_VAR_SIN_ENTRY

// the series' rule (phi, order, nq, nodes) stands between `same` and the outputs
#define CGP_VAR_HERMITE_ENTRY(T, sfx)                                                        \
    int cgp_var_hermite_##sfx(const T* xx, const T* yy, int64_t n1, int64_t n2, int32_t hw,  \
                              int32_t same, int32_t phi, int32_t order, int32_t nq,          \
                              const double* nodes, T* xx_out, T* yy_out, void* stream) {     \
        return var_hermite_impl(VarArgs<T>{xx, yy, n1, n2, hw, same, xx_out, yy_out}, phi,   \
                                order, nq, nodes, stream);                                   \
    }
CGP_VAR_HERMITE_ENTRY(double, f64)
CGP_VAR_HERMITE_ENTRY(float, f32)
#undef CGP_VAR_HERMITE_ENTRY

}  // extern "C"
