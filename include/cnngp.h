/*
 * cnngp.h — C ABI of the MI355X-native CNN-GP hot path (libcnngp.so).
 *
 * The reference (waleedbinkhalid74/cnn-gp) is pure Python over PyTorch; it has no FFI of
 * its own.  Each entry point below replaces the PyTorch op sequence one reference
 * function issues, so a ctypes (or any C FFI) binding can drive the whole NNGP Gram
 * recursion and the GP solve without torch compute.  Citations are
 * /root/reference/<file>:<line>.
 *
 * Conventions
 *   - Every buffer is DEVICE memory owned by the caller (torch allocates it and passes
 *     data_ptr()).  The library never frees caller memory.  rocBLAS / rocSOLVER handles
 *     are owned by the library, cached per device.
 *   - Every compute entry point is asynchronous on `stream` (a hipStream_t passed as
 *     void*; NULL = the null stream).  No host synchronisation inside, except the solve,
 *     which returns potrf's `info` to the host.
 *   - Return value: 0 on success, otherwise a CGP_E* code; cgp_last_error() returns a
 *     thread-local message for the last failure.  No C++ exception crosses the ABI.
 *   - Layouts are row-major and dense.  A "map" is one H×W spatial plane.  The pair
 *     index of a non-diagonal tile is m = i·N2 + j (i over the N1 rows, j over the N2
 *     columns); for a diagonal (diag=1) tile m = i = j.
 *   - _f64 entry points compute in double, _f32 in float (the reference's production
 *     dtype).  Scalars (weight, bias) are passed as double and rounded to the compute
 *     type inside the f32 entry points.
 */
#ifndef CNNGP_H
#define CNNGP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGP_ABI_VERSION 12

/* error codes */
#define CGP_OK 0
#define CGP_EINVAL 1001   /* argument check failed (shapes, null pointers, ranges) */
#define CGP_EHIP 1002     /* a HIP runtime call or kernel launch failed */
#define CGP_EBLAS 1003    /* rocBLAS / rocSOLVER returned an error status */

/* cgp_conv_args.pre / .post */
#define CGP_PRE_NONE 0
#define CGP_PRE_RELU 1     /* apply the ReLU covariance map to the input while staging it */
#define CGP_PRE_MOMENTS 2  /* the input is (x, y) images; stage mean_c x·y instead of a map */
#define CGP_POST_NONE 0
#define CGP_POST_RELU 1    /* apply the ReLU covariance map to the conv output */

/* cgp_conv_args.flags / cgp_relu_args.flags */
#define CGP_FLAG_EXACT_RELU 1  /* evaluate the ReLU map op by op like the reference
                                  (correctly rounded 1/sqrt, sqrt, acos, division);
                                  default is the closed form max(c,0)/2 + sqrt(t)·x^1.5·P(x)
                                  of csrc/relu_poly.h, within 1e-14 of the exact map */
#define CGP_FLAG_GENERIC_CONV 2  /* force the generic conv kernel (tests / A-B timing); the
                                    other such knob is cgp_conv_args.max_groups */

int cgp_abi_version(void);
/* The factor cgp_net_f64's closed-form ReLU expects on its x-side variance maps (var_x /
 * var2_x without CGP_FLAG_EXACT_RELU): 1/16 from ABI 9 (1/4 in ABI 6-8).  cgp_var_chain_*
 * writes its qstore copies with it; a host scaling maps itself uses this value. */
double cgp_net_xvar_scale(void);
/* Which variance maps cgp_net_f64's closed-form ReLU reads through var_x / var_y (and
 * var2_x / var2_y) of its op records -- an addition to ABI 12 (no struct or existing entry
 * point changed); a host asks instead of assuming:
 *   CGP_VAR_FORM_SCALED  x side: v × cgp_net_xvar_scale(), y side: plain v (the two-root
 *                        form: every library before this query, and builds with
 *                        -DCGP_RELU_ONE_ROOT=0)
 *   CGP_VAR_FORM_RSQRT   both sides: m = 1/sqrt(v/8) as cgp_rsqrt_batch_f64 writes it
 *                        (+inf where v = 0, unclamped); the one-root form, DESIGN.md §4.1.
 *                        One map set serves an image on either side.
 * cgp_net_f32, and cgp_net_f64 with CGP_FLAG_EXACT_RELU, read plain v on both sides in
 * either form; kdiag is always the plain final variance. */
#define CGP_VAR_FORM_SCALED 0
#define CGP_VAR_FORM_RSQRT 1
int cgp_net_var_form(void);
const char* cgp_last_error(void);
/* sizeof of the argument structs, so an FFI can verify its mirror of the layout */
size_t cgp_conv_args_size(void);
size_t cgp_relu_args_size(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int cgp_device_count(void);
/* host-only self test of the library's integer helpers (no GPU needed); 0 = pass */
int cgp_selftest(void);

/*
 * Input moments — replaces NNGPKernel.forward's moment step, kernels.py:44-49:
 *   xy[m] = mean_c x[i,c]·y[j,c]   (diag: xy[i] = mean_c x[i,c]·y[i,c])
 * x: [n1][c][hw], y: [n2][c][hw]; xy: [n1·n2][hw] (diag: [n1][hw]).
 */
int cgp_moments_xy_f64(const double* x, const double* y, int64_t n1, int64_t n2,
                       int32_t c, int32_t hw, int32_t diag, double* xy, void* stream);
int cgp_moments_xy_f32(const float* x, const float* y, int64_t n1, int64_t n2,
                       int32_t c, int32_t hw, int32_t diag, float* xy, void* stream);
/*
 * Per-image variances — kernels.py:48-49: xx[i] = mean_c x[i,c]², yy[j] = mean_c y[j,c]².
 * Writes xx: [n1][hw] and yy: [n2][hw] (they may be one contiguous [n1+n2][hw] block).
 */
int cgp_moments_var_f64(const double* x, const double* y, int64_t n1, int64_t n2,
                        int32_t c, int32_t hw, double* xx, double* yy, void* stream);
int cgp_moments_var_f32(const float* x, const float* y, int64_t n1, int64_t n2,
                        int32_t c, int32_t hw, float* xx, float* yy, void* stream);

/*
 * Conv2d covariance stencil — replaces Conv2d.propagate, kernels.py:92-98
 * (F.conv2d with the constant kernel of kernels.py:78-88, then + var_bias):
 *   out[m,oh,ow] = weight · Σ_{a,b<taps} in[m, oh·s+off+a·d, ow·s+off+b·d] + bias
 * with zero padding outside [0,h)×[0,w).  `offset` is -padding, plus `dilation` when the
 * reference pads an even kernel to (k+1)² with a zero first row/column (kernels.py:73-84).
 * Optional fusions (one HBM pass instead of two or three):
 *   pre  = CGP_PRE_RELU:    the staged input is ReLU.propagate(in) (kernels.py:134-165),
 *                           using pre_xx/pre_yy = the variances at the ReLU's input;
 *   pre  = CGP_PRE_MOMENTS: the staged input is mean_c x·y of in (=x) and in_y (=y);
 *   post = CGP_POST_RELU:   out is ReLU.propagate of the conv output, using
 *                           post_xx/post_yy = the variances of the conv output;
 *   addend != NULL:         out += addend after everything else (Sum, kernels.py:252-254,
 *                           kernel_patch.py:43-63).
 * Variance maps (pre_xx etc.) are [n1][h·w] / [n2][h·w] at the resolution they apply to.
 */
typedef struct cgp_conv_args {
    const void* in;       /* [nmaps][h][w]; or x [n1][channels][h][w] with CGP_PRE_MOMENTS */
    const void* in_y;     /* y [n2][channels][h][w] with CGP_PRE_MOMENTS, else NULL */
    void* out;            /* [nmaps][ho][wo] */
    const void* addend;   /* [nmaps][ho][wo] or NULL */
    const void* pre_xx;   /* CGP_PRE_RELU: [n1][h][w] */
    const void* pre_yy;   /* CGP_PRE_RELU: [n2][h][w] */
    const void* post_xx;  /* CGP_POST_RELU: [n1][ho][wo] */
    const void* post_yy;  /* CGP_POST_RELU: [n2][ho][wo] */
    int64_t nmaps;        /* n1·n2, or n1 when diag */
    int64_t n1, n2;
    int32_t h, w, ho, wo;
    int32_t taps, offset, stride, dilation;
    int32_t channels;     /* CGP_PRE_MOMENTS only */
    int32_t pre, post;
    int32_t same, diag;   /* KernelPatch.same / .diag (kernel_patch.py:4-30) */
    int32_t maps_per_block; /* 0 = library default */
    int32_t flags;          /* CGP_FLAG_* */
    int32_t max_groups;     /* 0 = the library's persistent grid; > 0 caps the grid of either
                               conv kernel at min(grid, max_groups) workgroups, so each
                               walks more chunks (tests / A-B runs, like
                               CGP_FLAG_GENERIC_CONV: it does not change which kernel runs
                               or any result bit); < 0: CGP_EINVAL.  The field every
                               library before this addition to ABI 12 called `reserved`
                               and never read. */
    double weight, bias;
} cgp_conv_args;
int cgp_conv_f64(const cgp_conv_args* args, void* stream);
int cgp_conv_f32(const cgp_conv_args* args, void* stream);
/*
 * The launch cgp_conv_* would make for these arguments (an addition to ABI 12; host only:
 * nothing is launched and no buffer is touched).  Runs the checks of cgp_conv_* with their
 * return codes, then the dispatch cgp_conv_* itself runs, stopped before the launch:
 *   out[0]  kernel: 0 = the generic kernel, 1 = the compile-time-geometry kernel
 *   out[1]  whole maps per chunk
 *   out[2]  chunks = ceil(nmaps / out[1])
 *   out[3]  workgroups; each walks chunks blockIdx, blockIdx + out[3], ...
 * out[3] depends on the device (resident workgroups) unless max_groups caps it below that;
 * without a device it assumes one workgroup on each of 256 CUs.
 */
int cgp_conv_plan_f64(const cgp_conv_args* args, int32_t out[4]);
int cgp_conv_plan_f32(const cgp_conv_args* args, int32_t out[4]);

/*
 * ReLU covariance map on the pair maps — ReLU.propagate, kernels.py:134-165:
 *   t = xx[i]·yy[j] + f32_tiny; cos = clamp(xy·rsqrt(t), -1, 1);
 *   sin = sqrt(max(t - xy², 0)); out = (sin + (π - acos(cos))·xy) / 2π
 * same && !diag: out[i,i] = xx[i]/2; same && diag: out = xx/2.  Optional out += addend.
 * In-place (out == xy) is allowed.
 */
typedef struct cgp_relu_args {
    const void* xy;      /* [nmaps][hw] */
    void* out;           /* [nmaps][hw] */
    const void* addend;  /* [nmaps][hw] or NULL */
    const void* xx;      /* [n1][hw] variances at the ReLU input */
    const void* yy;      /* [n2][hw] */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag, flags;   /* flags: CGP_FLAG_* */
} cgp_relu_args;
int cgp_relu_f64(const cgp_relu_args* args, void* stream);
int cgp_relu_f32(const cgp_relu_args* args, void* stream);

/*
 * ABI 12: the ReLU step of the neural tangent kernel recursion (no reference counterpart:
 * the reference reaches the NTK only through autograd on its torch ops).  Beside the pair
 * maps xy the recursion carries a second pair map theta; one pass writes
 *   out_xy    = the map of cgp_relu_* above, the same bits in both ReLU modes;
 *   out_theta = theta · (π - acos(cos)) / 2π,  cos as above from the same variances —
 *               the derivative of the ReLU map in xy at fixed variances.
 * Where cgp_relu_* overrides the map (same && !diag: pairs i == j; same && diag: all),
 * cos = 1 and out_theta = theta/2 exactly.  With CGP_FLAG_EXACT_RELU cos is evaluated op by
 * op like the reference's (correctly rounded 1/sqrt); else with the closed form's refined
 * hardware rsqrt.  In-place (out_xy == xy, out_theta == theta) is allowed, and theta may be
 * xy itself (the first ReLU after a conv, where theta == xy).  same or diag need n1 == n2.
 */
typedef struct cgp_relu_ntk_args {
    const void* xy;      /* [nmaps][hw] */
    const void* theta;   /* [nmaps][hw] */
    void* out_xy;        /* [nmaps][hw] */
    void* out_theta;     /* [nmaps][hw] */
    const void* xx;      /* [n1][hw] variances at the ReLU input */
    const void* yy;      /* [n2][hw] (may be NULL when same && diag) */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag, flags;   /* flags: CGP_FLAG_EXACT_RELU */
} cgp_relu_ntk_args;
size_t cgp_relu_ntk_args_size(void);
int cgp_relu_ntk_f64(const cgp_relu_ntk_args* args, void* stream);
int cgp_relu_ntk_f32(const cgp_relu_ntk_args* args, void* stream);

/*
 * ReLU on the per-image variances — kernels.py:154-164: xx' = xx/2;
 * yy' = xx' if same else yy/2.  xx: [n1][hw], yy: [n2][hw].
 */
int cgp_var_relu_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                     int32_t same, double* xx_out, double* yy_out, void* stream);
int cgp_var_relu_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                     int32_t same, float* xx_out, float* yy_out, void* stream);

/*
 * The erf nonlinearity (an addition to ABI 12: no struct or existing entry point changed;
 * no reference counterpart, the reference ships ReLU only).  The layer kernel of erf in
 * closed form (Williams 1997; the paper's second nonlinearity), in the conventions of the
 * ReLU entry points above -- per pixel (xy, xx, yy) = (c, v1, v2), no rescaling:
 *   pair map    D = 1 + 2(v1 + v2) + 4(v1·v2 - c²), raised to 1 where it falls below 1
 *               (D = (1+2v1)(1+2v2) - 4c² >= 1 for a valid covariance);
 *               out_xy = (2/π)·atan(2c/√D)     [= (2/π)·asin(2c/√((1+2v1)(1+2v2)))]
 *   variances   v' = (2/π)·atan(2v/√(1 + 4v)), the pair map at c = v1 = v2 = v
 *   NTK         out_theta = theta·κ̇,  κ̇ = (4/π)/√D = ∂out_xy/∂c at fixed variances
 *                                                   = E[erf'(u1)·erf'(u2)]
 * Where cgp_relu_* overrides its map (same && !diag: pairs i == j; same && diag: all),
 * out_xy = v'[i], the same bits cgp_var_erf_* writes, and κ̇ = (4/π)/√(1 + 4v).  A zero
 * variance needs no guard (c = v = 0: out_xy = 0, κ̇ = 4/π).  One evaluation mode: division
 * and square root correctly rounded, atan from the device math library; flags is ignored
 * (CGP_FLAG_EXACT_RELU has no effect).
 *
 * theta == NULL: the forward-only pass (one map read, one write; out_theta unused).  With
 * theta, one pass writes both maps.  In-place (out_xy == xy, out_theta == theta) is
 * allowed, and theta may be xy itself: every element is read before it is written, by one
 * thread.  addend (optional) is added to out_xy only, as a separate rounding.  same or diag
 * need n1 == n2; hw is at most 2048; nmaps < 2^31.
 */
typedef struct cgp_erf_args {
    const void* xy;         /* [nmaps][hw] */
    const void* theta;      /* [nmaps][hw] or NULL */
    void* out_xy;           /* [nmaps][hw] */
    void* out_theta;        /* [nmaps][hw] (unused when theta is NULL) */
    const void* addend;     /* [nmaps][hw] or NULL */
    const void* xx;         /* [n1][hw] variances at the erf input */
    const void* yy;         /* [n2][hw] (may be NULL when same && diag) */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag, flags;
} cgp_erf_args;
size_t cgp_erf_args_size(void);
int cgp_erf_f64(const cgp_erf_args* args, void* stream);
int cgp_erf_f32(const cgp_erf_args* args, void* stream);

/*
 * erf on the per-image variances: xx' = (2/π)·atan(2·xx/√(1 + 4·xx));
 * yy' = xx' if same else the same map of yy.  xx: [n1][hw], yy: [n2][hw].
 */
int cgp_var_erf_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                    int32_t same, double* xx_out, double* yy_out, void* stream);
int cgp_var_erf_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                    int32_t same, float* xx_out, float* yy_out, void* stream);

/*
 * Position-pair maps: networks that end in global average pooling (additions to ABI 12: no
 * struct or existing entry point changed; no reference counterpart, the reference has no
 * pooling layer).  A pooled head averages the covariance of every pixel p of
 * x_i with every pixel q of y_j, so the recursion carries S[p, q] per pair instead of one
 * [h][w] map.  Layout of a position-pair map of an h×w value, dense:
 *
 *     S[m][p_row][q_row][p_col][q_col]        (h·w)² elements per pair, at most 2^30
 *
 * (the w×w block of one row pair is contiguous).  Pairs are listed by two DEVICE int32
 * arrays: pair m is (x image pair_i[m], y image pair_j[m]); the entry points cannot check
 * the indices against the image counts, the caller does.  Variance maps are the per-image
 * maps of the entry points above, [n][h·w], indexed xx[pair_i[m]][p] and yy[pair_j[m]][q].
 * With `same` (y is x) the reference's override of a nonlinearity (kernels.py:155-162)
 * applies where both arguments are one pre-activation: pair_i[m] == pair_j[m] and p == q;
 * every other element, p != q of a self pair included, takes the ordinary map.  Every
 * kernel sums in a fixed order and uses no atomics: a pair's result depends on that pair's
 * data only, so it does not change with the rest of the pair list or from run to run.
 */
#define CGP_COV_NONE 0
#define CGP_COV_RELU 1   /* the map of cgp_relu_* (closed form, or CGP_FLAG_EXACT_RELU) */
#define CGP_COV_ERF 2    /* the map of cgp_erf_* */
/* S[m][p, q] = mean_c x[pair_i[m]][c][p]·y[pair_j[m]][c][q]; x: [n1][c][h·w], y likewise;
 * out: [npairs] maps.  Summed over c like cgp_moments_var_*. */
int cgp_cov_moments_f64(const double* x, const double* y, const int32_t* pair_i,
                        const int32_t* pair_j, int64_t npairs, int32_t c, int32_t h, int32_t w,
                        double* out, void* stream);
int cgp_cov_moments_f32(const float* x, const float* y, const int32_t* pair_i,
                        const int32_t* pair_j, int64_t npairs, int32_t c, int32_t h, int32_t w,
                        float* out, void* stream);
/*
 * Conv2d on position-pair maps: the stencil of cgp_conv_* along the diagonal, p and q
 * shifted by the same tap,
 *   out[m][p, q] = weight · Σ_{a,b<taps} in[m][(p_row·s+off+a·d, p_col·s+off+b·d),
 *                                           (q_row·s+off+a·d, q_col·s+off+b·d)] + bias
 * with a term zero when either pixel leaves the h×w map; column taps are summed first,
 * then row taps, like cgp_conv_*'s generic kernel.  Then, optionally, the nonlinearity
 * `post` with xx / yy = the variances of the conv output, and `+ addend` last (a separate
 * rounding).  out must not be in (out == addend is allowed).  One workgroup stages `taps`
 * w×w blocks: taps·w²·itemsize must not exceed 64 KB.  A 1×1 value (h = w = 1: one element
 * per pair) is a map like any other, which is how a Conv2d after the pool runs.
 */
typedef struct cgp_cov_conv_args {
    const void* in;          /* [npairs][h][h][w][w] */
    void* out;               /* [npairs][ho][ho][wo][wo] */
    const void* addend;      /* like out, or NULL */
    const void* xx;          /* post != CGP_COV_NONE: [n1][ho][wo], else unused */
    const void* yy;          /* post != CGP_COV_NONE: [n2][ho][wo] (same: may be xx) */
    const int32_t* pair_i;   /* device [npairs]; read only with a post-nonlinearity */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w, ho, wo;
    int32_t taps, offset, stride, dilation;   /* as cgp_conv_args */
    int32_t post;            /* CGP_COV_* */
    int32_t same;
    int32_t flags;           /* CGP_FLAG_EXACT_RELU */
    int32_t reserved;
    double weight, bias;
} cgp_cov_conv_args;
size_t cgp_cov_conv_args_size(void);
int cgp_cov_conv_f64(const cgp_cov_conv_args* args, void* stream);
int cgp_cov_conv_f32(const cgp_cov_conv_args* args, void* stream);
/*
 * A standalone ReLU or erf on position-pair maps, out = map(in) [+ addend].  In-place
 * (out == in) is allowed: every element is read and written by one thread.
 */
typedef struct cgp_cov_nonlin_args {
    const void* in;          /* [npairs][h][h][w][w] */
    void* out;
    const void* addend;      /* like out, or NULL */
    const void* xx;          /* [n1][h][w] variances at the nonlinearity's input */
    const void* yy;          /* [n2][h][w] (same: may be xx) */
    const int32_t* pair_i;   /* device [npairs] */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w;
    int32_t kind;            /* CGP_COV_RELU or CGP_COV_ERF */
    int32_t same;
    int32_t flags;           /* CGP_FLAG_EXACT_RELU (ReLU only) */
    int32_t reserved;
} cgp_cov_nonlin_args;
size_t cgp_cov_nonlin_args_size(void);
int cgp_cov_nonlin_f64(const cgp_cov_nonlin_args* args, void* stream);
int cgp_cov_nonlin_f32(const cgp_cov_nonlin_args* args, void* stream);
/*
 * GlobalAvgPool: out[m] = mean of the n elements of pair m's map (n = (h·w)²), accumulated
 * in double for both types, one workgroup per pair, fixed order.
 */
int cgp_cov_pool_f64(const double* in, int64_t npairs, int64_t n, double* out, void* stream);
int cgp_cov_pool_f32(const float* in, int64_t npairs, int64_t n, float* out, void* stream);
/*
 * AvgPool2d on position-pair maps (additions to ABI 12: no struct or existing entry point
 * changed).  A windowed average moves p and q independently, unlike a conv:
 *   out[m][P][Q][U][V] = k⁻⁴ · Σ_{a,a'<k} Σ_{b,b'<k} in[m][P·s+a][Q·s+a'][U·s+b][V·s+b']
 * with no padding: ho = floor((h - k)/s) + 1 and wo likewise (rows and columns that do not
 * fill a window are dropped), which the entry point checks.  The k² row blocks are summed
 * first, then the k×k column window, all in the map's type, and the sum is divided once by
 * k⁴; k = 1, s = 1 copies the map bit for bit.  Both sums add an offset pair (a, a') to its
 * mirror (a', a) before anything else, so a map that is symmetric bit for bit under p <-> q
 * (a self pair's) stays so.  out must not be in.  One workgroup holds a w×w block of sums:
 * w²·itemsize must not exceed 64 KB.
 */
typedef struct cgp_covmap_avgpool_args {
    const void* in;          /* [npairs][h][h][w][w] */
    void* out;               /* [npairs][ho][ho][wo][wo] */
    int64_t npairs;
    int32_t h, w, ho, wo;
    int32_t k, stride;       /* kernel_size and stride, both >= 1; k <= h and k <= w */
} cgp_covmap_avgpool_args;
size_t cgp_covmap_avgpool_args_size(void);
int cgp_covmap_avgpool_f64(const cgp_covmap_avgpool_args* args, void* stream);
int cgp_covmap_avgpool_f32(const cgp_covmap_avgpool_args* args, void* stream);
/*
 * The p = q diagonal of position-pair maps: out[pair_i[m]][r][c] = in[m][r][r][c][c], with
 * in [npairs][h][h][w][w] and out [n][h][w] per-image maps.  Of the self pairs (i, i) of an
 * image set these are the per-image variance maps of the value (the only way to them
 * downstream of an AvgPool2d).  Images no pair names are left untouched; the
 * pair_i[m] must differ from each other.
 */
int cgp_covmap_diag_f64(const double* in, const int32_t* pair_i, int64_t npairs, int32_t h,
                        int32_t w, double* out, void* stream);
int cgp_covmap_diag_f32(const float* in, const int32_t* pair_i, int64_t npairs, int32_t h,
                        int32_t w, float* out, void* stream);
/*
 * A conv or readout with correlated weights on position-pair maps (additions to ABI 12: no
 * struct or existing entry point changed).  Taps δ and δ' of one filter have
 * the correlation R[δ, δ'], separable into rows and columns, so p and q move by different
 * taps:
 *   out[m][P][Q][U][V] = weight · Σ_{a,a'<taps} Rr[a][a'] · Σ_{b,b'<taps} Rc[b][b'] ·
 *                        in[m][P·s+off+a·d][Q·s+off+a'·d][U·s+off+b·d][V·s+off+b'·d] + bias
 * with a term zero where an index leaves the map.  Rr = Rc = I is cgp_cov_conv_*'s stencil,
 * all-ones cgp_covmap_avgpool_*'s window sum (times k⁴).  Both tables must be symmetric; the
 * entries [a][a'] with a <= a' are the ones read.  The row sum is taken first, then the
 * column sum, all in the map's type, then weight and bias once.  Both sums run over the
 * offset pairs a <= a' in row-major order and take an offset pair with its mirror first,
 * Rr[a][a']·(t(a, a') + t(a', a)), so a map that is symmetric bit for bit under p <-> q (a
 * self pair's) stays so.  The order depends on the geometry alone, not on the grid, the pair
 * count or how the caller chunks the pairs (several lanes may share one output's column sum:
 * they take the offset pairs of the list round robin and add their parts in a fixed tree).
 * A row-offset pair whose Rr entry is exactly zero is not fetched: Rr = I costs taps block
 * loads per output row pair, a band of half-width c (2c + 1)·taps.  out must not be in.
 * ho, wo: every output row and column must have a tap inside the map.  One workgroup holds
 * a w×w block of sums and both tables: they must fit 64 KB of LDS.
 */
typedef struct cgp_corrconv_args {
    const void* in;          /* [npairs][h][h][w][w] */
    void* out;               /* [npairs][ho][ho][wo][wo] */
    const void* corr_rows;   /* device [taps][taps], the maps' type */
    const void* corr_cols;   /* device [taps][taps], the maps' type */
    int64_t npairs;
    int32_t h, w, ho, wo;
    int32_t taps, offset, stride, dilation;   /* as cgp_cov_conv_args */
    double weight, bias;     /* var_weight/k² and var_bias */
} cgp_corrconv_args;
size_t cgp_corrconv_args_size(void);
int cgp_corrconv_f64(const cgp_corrconv_args* args, void* stream);
int cgp_corrconv_f32(const cgp_corrconv_args* args, void* stream);

/*
 * A conv whose taps carry individual weights (additions to ABI 12: no struct or existing
 * entry point changed).  Conv2d.propagate of the reference is F.conv2d with the
 * module's `kernel` buffer (kernels.py:92-98); these entry points run it for a buffer that is
 * not the constant box of cgp_conv_*.  A pure map op, with no n1 / n2 / same / diag:
 *   out[m][oh][ow] = ( Σ_{a<extent} p_a ) + bias  [+ addend[m][oh][ow]]
 *   p_a            =   Σ_{b<extent} table[a][b] · in[m][oh·s + off + a·d][ow·s + off + b·d]
 * with a term zero where an index leaves the h×w map.  `extent` is the buffer's edge (k + 1
 * for an even "same" kernel) and `offset` is -padding: the first row and column of an even
 * "same" buffer are taps like any other.  The arithmetic, all in the maps' type:
 *   - table is given in the maps' type (the caller rounds it once);
 *   - every product is rounded (the library is built with -ffp-contract=off);
 *   - p_a accumulates its products left to right, b = 0, 1, ...;
 *   - the p_a are added top to bottom, a = 0, 1, ..., then bias; the addend is added last,
 *     a separate rounding;
 *   - a tap whose weight is exactly zero may be skipped (the zero row and column of an even
 *     "same" kernel cost nothing); for finite inputs that changes no value.
 * The order depends on the geometry alone, not on the grid, nmaps or the maps a workgroup
 * takes: where a map has fewer than 64 outputs the tap rows a of one output are split over
 * the lanes of a wave, each p_a still summed by one lane, and the p_a are then added top to
 * bottom by one lane -- the same bits as one lane doing all of it.
 * out must not be in (out == addend is allowed).  ho, wo must be F.conv2d's,
 *   ho = floor((h - 2·offset - d·(extent - 1) - 1)/s) + 1, wo likewise,
 * and every output row and column must have a tap inside the map.  LDS budget: a workgroup
 * stages whole maps with the zero border the taps reach, [(ho-1)·s + (extent-1)·d + 1] x
 * [(wo-1)·s + (extent-1)·d + 1] elements; one such map, plus extent p_a per output where the
 * rows are split, must fit 64 KB (32×32 maps with 7×7 taps and a 28×28 readout do, in either
 * type).  Every check returns CGP_EINVAL before any launch.
 */
typedef struct cgp_tapconv_args {
    const void* in;          /* [nmaps][h][w] */
    void* out;               /* [nmaps][ho][wo] */
    const void* addend;      /* like out, or NULL */
    const void* table;       /* device [extent][extent], the maps' type */
    int64_t nmaps;
    int32_t h, w, ho, wo;
    int32_t extent, offset, stride, dilation;
    int32_t max_groups;      /* as cgp_conv_args.max_groups: 0 = the library's grid, > 0 caps
                                it (each workgroup walks more chunks; no result bit changes),
                                < 0: CGP_EINVAL */
    int32_t reserved;
    double bias;
} cgp_tapconv_args;
size_t cgp_tapconv_args_size(void);
int cgp_tapconv_f64(const cgp_tapconv_args* args, void* stream);
int cgp_tapconv_f32(const cgp_tapconv_args* args, void* stream);
/*
 * The same conv on position-pair maps, in the layout and with the pair conventions of
 * cgp_cov_conv_*: p and q move by the same tap,
 *   out[m][P][Q][U][V] = ( Σ_a p_a ) + bias [+ addend]
 *   p_a = Σ_b table[a][b] · in[m][P·s+off+a·d][Q·s+off+a·d][U·s+off+b·d][V·s+off+b·d]
 * in the order above, so the P = Q, U = V entries of a self pair's map equal cgp_tapconv_* on
 * the image's variance map bit for bit.  No post-nonlinearity, no pair lists: nothing reads
 * variances.  out must not be in (out == addend is allowed).  One workgroup stages `extent`
 * w×w blocks: extent·w²·itemsize, and 8 bytes per tap row, must not exceed 64 KB.  A 1×1
 * value is a map of one element.
 */
typedef struct cgp_tapconv_cov_args {
    const void* in;          /* [npairs][h][h][w][w] */
    void* out;               /* [npairs][ho][ho][wo][wo] */
    const void* addend;      /* like out, or NULL */
    const void* table;       /* device [extent][extent], the maps' type */
    int64_t npairs;
    int32_t h, w, ho, wo;
    int32_t extent, offset, stride, dilation;
    double bias;
} cgp_tapconv_cov_args;
size_t cgp_tapconv_cov_args_size(void);
int cgp_tapconv_cov_f64(const cgp_tapconv_cov_args* args, void* stream);
int cgp_tapconv_cov_f32(const cgp_tapconv_cov_args* args, void* stream);

/*
 * The GELU nonlinearity φ(x) = x·Φ(x) (additions to ABI 12: no struct or existing entry
 * point changed; no reference counterpart).  The exact GELU, not its tanh
 * approximation.  Its layer kernel in closed form (Tsuchida, Pearce et al. 2021, "Avoiding
 * kernel fixed points: computing with ELU and GELU infinite networks"), in the conventions
 * of the ReLU and erf entry points above -- per pixel (xy, xx, yy) = (c, v1, v2), no
 * rescaling.  With P = v1·v2, P1 = (1 + v1)(1 + v2), Δ² = P1 - c², raised to 1 where it
 * falls below 1 (NaN kept; Δ² >= 1 + v1 + v2 for a valid covariance, so there is no
 * singularity at ρ = ±1), Δ = √Δ², t = c/Δ and a = atan(t):
 *   pair map    out_xy = ((c² + P·Δ²)/(P1·Δ) + c·a)/(2π) + c/4
 *   variances   s = √(1 + 2v): v' = (2v²/((1 + v)·s) + v·atan(v/s))/(2π) + v/4, the pair
 *               map at c = v1 = v2 = v
 *   NTK         out_theta = theta·κ̇,  κ̇ = (1/Δ² + (1 - P)/P1 + 1)·t/(2π) + 1/4 + a/(2π)
 *               = ∂out_xy/∂c at fixed variances = E[φ'(u1)·φ'(u2)]
 * Where cgp_relu_* overrides its map (same && !diag: pairs i == j; same && diag: all),
 * out_xy = v'[i], the same bits cgp_var_gelu_* writes, and κ̇ is the NTK line at
 * c = v1 = v2 = v: (1/(1 + 2v) + (1 - v)/(1 + v) + 1)·(v/s)/(2π) + 1/4 + atan(v/s)/(2π).
 * A zero variance needs no guard (c = v = 0: out_xy = 0, κ̇ = 1/4).  out_xy can be negative,
 * and the map is not homogeneous: the input scale matters.  One evaluation mode: division
 * and square root correctly rounded, atan from the device math library, every op rounded in
 * the map's type (the /(2π) above is a product with the constant 1/(2π)); flags is ignored.
 *
 * cgp_gelu_args has the fields and the rules of cgp_erf_args: theta == NULL is the
 * forward-only pass; in-place (out_xy == xy, out_theta == theta) is allowed, and theta may
 * be xy itself; addend (optional) is added to out_xy only, as a separate rounding; same or
 * diag need n1 == n2; hw is at most 2048; nmaps < 2^31.
 */
typedef struct cgp_gelu_args {
    const void* xy;         /* [nmaps][hw] */
    const void* theta;      /* [nmaps][hw] or NULL */
    void* out_xy;           /* [nmaps][hw] */
    void* out_theta;        /* [nmaps][hw] (unused when theta is NULL) */
    const void* addend;     /* [nmaps][hw] or NULL */
    const void* xx;         /* [n1][hw] variances at the GELU input */
    const void* yy;         /* [n2][hw] (may be NULL when same && diag) */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag, flags;
} cgp_gelu_args;
size_t cgp_gelu_args_size(void);
int cgp_gelu_f64(const cgp_gelu_args* args, void* stream);
int cgp_gelu_f32(const cgp_gelu_args* args, void* stream);
/* GELU on the per-image variances: xx' = v'(xx); yy' = xx' if same else v'(yy).
 * xx: [n1][hw], yy: [n2][hw]. */
int cgp_var_gelu_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                     int32_t same, double* xx_out, double* yy_out, void* stream);
int cgp_var_gelu_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                     int32_t same, float* xx_out, float* yy_out, void* stream);
/*
 * GELU on position-pair maps, out = map(in) [+ addend], with cgp_cov_nonlin_*'s element
 * rule: (c, v1, v2) = (in[m][p, q], xx[pair_i[m]][p], yy[pair_j[m]][q]), and the override
 * (out = v'[pair_i[m]][p]) where same, pair_i[m] == pair_j[m] and p == q.  In-place
 * (out == in) is allowed: every element is read and written by one thread.
 */
typedef struct cgp_gelu_cov_args {
    const void* in;          /* [npairs][h][h][w][w] */
    void* out;
    const void* addend;      /* like out, or NULL */
    const void* xx;          /* [n1][h][w] variances at the GELU input */
    const void* yy;          /* [n2][h][w] (same: may be xx) */
    const int32_t* pair_i;   /* device [npairs] */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w;
    int32_t same;
    int32_t flags;           /* ignored */
    int32_t reserved;
} cgp_gelu_cov_args;
size_t cgp_gelu_cov_args_size(void);
int cgp_gelu_cov_f64(const cgp_gelu_cov_args* args, void* stream);
int cgp_gelu_cov_f32(const cgp_gelu_cov_args* args, void* stream);

/*
 * The NTK on position-pair maps (additions to ABI 12: no struct or existing entry point
 * changed).  A second map Θ[m][p, q] travels beside S[m][p, q], in the layout and
 * with the conventions of "Position-pair maps" above.  Every linear entry point there
 * (cgp_cov_conv_* with an addend, cgp_covmap_avgpool_*, cgp_corrconv_*, cgp_cov_pool_*,
 * cgp_axpby_*) is linear in its input and serves Θ as it is; the two below are the steps that
 * need both streams.  CGP_COV_GELU is valid in these two entry points only (the forward GELU
 * is cgp_gelu_cov_*).
 */
#define CGP_COV_GELU 3   /* the map of cgp_gelu_* */
/*
 * The nonlinearity step on both streams in one pass:
 *   out       = map(in) [+ addend]          the bits of cgp_cov_nonlin_* / cgp_gelu_cov_*
 *   out_theta = theta·κ̇ [+ addend_theta]    each a separate rounding
 * with (c, v1, v2) = (in[m][p, q], xx[pair_i[m]][p], yy[pair_j[m]][q]) and κ̇ = d map / dc at
 * fixed variances, the layer path's: cgp_relu_ntk_*'s (π - θ)/2π (honours
 * CGP_FLAG_EXACT_RELU), cgp_erf_*'s (4/π)/√D, cgp_gelu_*'s.  Where same, pair_i[m] ==
 * pair_j[m] and p == q, out is the variance map's value and κ̇ the layer path's override:
 * exactly 1/2 (ReLU), (4/π)/√(1 + 4v) (erf), the GELU line at c = v1 = v2 = v.
 * theta may be in (the first nonlinearity after the first conv, where Θ is K's buffer), and
 * in-place (out == in, out_theta == theta) is allowed: every element is read before it is
 * written, by one thread.  out and out_theta are two buffers.
 */
typedef struct cgp_covntk_nonlin_args {
    const void* in;            /* [npairs][h][h][w][w] */
    const void* theta;         /* like in */
    void* out;
    void* out_theta;
    const void* addend;        /* like out, or NULL */
    const void* addend_theta;  /* like out_theta, or NULL */
    const void* xx;            /* [n1][h][w] variances at the nonlinearity's input */
    const void* yy;            /* [n2][h][w] (same: may be xx) */
    const int32_t* pair_i;     /* device [npairs] */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w;
    int32_t kind;              /* CGP_COV_RELU, CGP_COV_ERF or CGP_COV_GELU */
    int32_t same;
    int32_t flags;             /* CGP_FLAG_EXACT_RELU (ReLU only) */
    int32_t reserved;
} cgp_covntk_nonlin_args;
size_t cgp_covntk_nonlin_args_size(void);
int cgp_covntk_nonlin_f64(const cgp_covntk_nonlin_args* args, void* stream);
int cgp_covntk_nonlin_f32(const cgp_covntk_nonlin_args* args, void* stream);
/*
 * Conv2d on both streams from one staging: with A the stencil sum of cgp_cov_conv_* (column
 * taps first, then row taps, left to right),
 *   k' = weight·A(in) + bias
 *   t' = weight·A(theta) + k'            the product rounded, then the sum
 * and then, with post in {CGP_COV_RELU, CGP_COV_ERF, CGP_COV_GELU}, the nonlinearity step
 * above on (k', t') with xx / yy = the variances of the conv output:
 *   out = map(k') [+ addend],  out_theta = t'·κ̇(k') [+ addend_theta]
 * or, with post == CGP_COV_NONE, out = k' [+ addend], out_theta = t' [+ addend_theta].
 * out has the bits of cgp_cov_conv_*; out_theta has the bits of the launch-by-launch sequence
 * (cgp_cov_conv_* on theta with bias 0 and addend k', then cgp_covntk_nonlin_*).
 * theta == NULL is Θ = 0 upstream (the first conv): t' = k', and nothing is staged for Θ.
 * out / out_theta must not be in / theta, nor each other.  One workgroup stages `taps` w×w
 * blocks of each stream it reads: streams·taps·w²·itemsize must not exceed 64 KB, checked
 * before any launch.  A 1×1 value (h = w = 1) is a map like any other.
 */
typedef struct cgp_covntk_conv_args {
    const void* in;            /* [npairs][h][h][w][w] */
    const void* theta;         /* like in, or NULL: Θ = 0 */
    void* out;                 /* [npairs][ho][ho][wo][wo] */
    void* out_theta;           /* like out */
    const void* addend;        /* like out, or NULL */
    const void* addend_theta;  /* like out_theta, or NULL */
    const void* xx;            /* post != CGP_COV_NONE: [n1][ho][wo], else unused */
    const void* yy;            /* post != CGP_COV_NONE: [n2][ho][wo] (same: may be xx) */
    const int32_t* pair_i;     /* device [npairs]; read only with a post-nonlinearity */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w, ho, wo;
    int32_t taps, offset, stride, dilation;   /* as cgp_conv_args */
    int32_t post;              /* CGP_COV_* */
    int32_t same;
    int32_t flags;             /* CGP_FLAG_EXACT_RELU */
    int32_t reserved;
    double weight, bias;
} cgp_covntk_conv_args;
size_t cgp_covntk_conv_args_size(void);
int cgp_covntk_conv_f64(const cgp_covntk_conv_args* args, void* stream);
int cgp_covntk_conv_f32(const cgp_covntk_conv_args* args, void* stream);

/*
 * The two-slope ReLU φ(x) = a·min(x, 0) + b·max(x, 0) (additions to ABI 12: no struct or
 * existing entry point changed; no reference counterpart): the leaky ReLU
 * (a = slope, b = 1), |x| (a = -1, b = 1), a damped identity (a = b), the ReLU itself (a = 0,
 * b = 1).  In the conventions of the ReLU entry points above -- per pixel (xy, xx, yy) =
 * (c, v1, v2), no rescaling.  With R(c, v1, v2) the map of cgp_relu_* (closed form, or op by
 * op with CGP_FLAG_EXACT_RELU) and k(c, v1, v2) = (π - θ)/2π the κ̇ of cgp_relu_ntk_*, the
 * same device functions, and three constants the caller computes in double,
 *   s = (a - b)²,  m = a·b,  h = (a² + b²)/2     (each rounded once to the map's type),
 *   pair map    out_xy = fma(s, R, m·c)          (the product rounded, then one fma)
 *   variances   v' = h·v
 *   NTK         out_theta = theta·κ̇,  κ̇ = fma(s, k, m) = E[φ'(u1)·φ'(u2)]
 * from φ(x) = b·relu(x) - a·relu(-x) and R(θ) - R(π - θ) = c/2.  Where cgp_relu_* overrides
 * its map (same && !diag: pairs i == j; same && diag: all), out_xy = h·v1, the bits
 * cgp_var_abrelu_* writes, and out_theta = theta·h.  So for finite inputs (s, m, h) =
 * (1, 0, 1/2) gives the bits of cgp_relu_* / cgp_relu_ntk_* / cgp_var_relu_*, and (0, 1, 1)
 * returns xy, theta and the variances unchanged.  The map is homogeneous of degree 1;
 * out_xy can be negative (c < 0, or a·b < 0).  A non-finite s, m or h is CGP_EINVAL.
 *
 * cgp_abrelu_args has the fields and the rules of cgp_erf_args, then s, m, h: theta == NULL
 * is the forward-only pass; in-place (out_xy == xy, out_theta == theta) is allowed, and theta
 * may be xy itself; addend (optional) is added to out_xy only, as a separate rounding; same
 * or diag need n1 == n2; hw is at most 2048; nmaps < 2^31.
 */
typedef struct cgp_abrelu_args {
    const void* xy;         /* [nmaps][hw] */
    const void* theta;      /* [nmaps][hw] or NULL */
    void* out_xy;           /* [nmaps][hw] */
    void* out_theta;        /* [nmaps][hw] (unused when theta is NULL) */
    const void* addend;     /* [nmaps][hw] or NULL */
    const void* xx;         /* [n1][hw] variances at the nonlinearity's input */
    const void* yy;         /* [n2][hw] (may be NULL when same && diag) */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag;
    int32_t flags;          /* CGP_FLAG_EXACT_RELU */
    double s, m, h;         /* (a - b)², a·b, (a² + b²)/2 */
} cgp_abrelu_args;
size_t cgp_abrelu_args_size(void);
int cgp_abrelu_f64(const cgp_abrelu_args* args, void* stream);
int cgp_abrelu_f32(const cgp_abrelu_args* args, void* stream);
/* The two-slope ReLU on the per-image variances: xx' = h·xx; yy' = xx' if same else h·yy.
 * xx: [n1][hw], yy: [n2][hw]. */
int cgp_var_abrelu_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                       int32_t same, double h, double* xx_out, double* yy_out, void* stream);
int cgp_var_abrelu_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                       int32_t same, double h, float* xx_out, float* yy_out, void* stream);
/*
 * The two-slope ReLU on position-pair maps, one entry point for both runs:
 *   out       = map(in) [+ addend]               theta == NULL: this alone
 *   out_theta = theta·κ̇ [+ addend_theta]         each a separate rounding
 * with cgp_cov_nonlin_*'s element rule: (c, v1, v2) = (in[m][p, q], xx[pair_i[m]][p],
 * yy[pair_j[m]][q]), and the override (out = h·xx[pair_i[m]][p], κ̇ = h) where same,
 * pair_i[m] == pair_j[m] and p == q.  At (s, m, h) = (1, 0, 1/2) the outputs are the bits of
 * cgp_cov_nonlin_* / cgp_covntk_nonlin_* with kind CGP_COV_RELU.  theta may be in, and
 * in-place (out == in, out_theta == theta) is allowed: every element is read before it is
 * written, by one thread.  out and out_theta are two buffers.  addend_theta is read only
 * with theta.
 */
typedef struct cgp_abrelu_cov_args {
    const void* in;            /* [npairs][h][h][w][w] */
    const void* theta;         /* like in, or NULL: the forward-only pass */
    void* out;
    void* out_theta;           /* (unused when theta is NULL) */
    const void* addend;        /* like out, or NULL */
    const void* addend_theta;  /* like out_theta, or NULL */
    const void* xx;            /* [n1][h][w] variances at the nonlinearity's input */
    const void* yy;            /* [n2][h][w] (same: may be xx) */
    const int32_t* pair_i;     /* device [npairs] */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w;
    int32_t same;
    int32_t flags;             /* CGP_FLAG_EXACT_RELU */
    double s, m, hh;           /* (a - b)², a·b, (a² + b²)/2 (hh: h is the map's height) */
} cgp_abrelu_cov_args;
size_t cgp_abrelu_cov_args_size(void);
int cgp_abrelu_cov_f64(const cgp_abrelu_cov_args* args, void* stream);
int cgp_abrelu_cov_f32(const cgp_abrelu_cov_args* args, void* stream);

/*
 * The sinusoid φ(x) = a·sin(b·x + θ) (additions to ABI 12: no struct or existing entry point
 * changed; no reference counterpart): sine and cosine networks, and with
 * (a, b, θ) = (√2, √(2γ), π/4) the random-Fourier-feature map whose layer kernel is the
 * squared-exponential exp(-γ·d).  In the conventions of the ReLU entry points above -- per
 * pixel (xy, xx, yy) = (c, v1, v2), no rescaling.  For u1, u2 jointly Gaussian with zero mean,
 * sin P·sin Q = (cos(P - Q) - cos(P + Q))/2 and E cos(g + μ) = cos μ·exp(-Var g/2) give, with
 * four constants the caller computes in double,
 *   A = a²/2,  B = b²/2,  C = cos 2θ,  D = a²b²/2    (each rounded once to the map's type),
 *   d = v1 + v2 - 2c,  s = v1 + v2 + 2c,  e_d = exp(-B·d),  e_s = exp(-B·s)
 *   pair map    out_xy = A·(e_d - C·e_s)
 *   variances   v' = A·(1 - C·exp(-4B·v)), the pair map at c = v1 = v2 = v
 *   NTK         out_theta = theta·κ̇,  κ̇ = D·(e_d + C·e_s) = E[φ'(u1)·φ'(u2)] = ∂out_xy/∂c
 * d and s are raised to 0 where rounding made them negative (a NaN is kept), so e_d <= 1 and
 * |out_xy| <= a².  Where cgp_relu_* overrides its map (same && !diag: pairs i == j; same &&
 * diag: all), out_xy = v'[i], the same bits cgp_var_sin_* writes, and κ̇ =
 * D·(1 + C·exp(-4B·v)).  At C == 0 the second exponential is not evaluated; for finite inputs
 * the bits are those of the full form.  (A, B, C, D) = (1, γ, 0, 2γ) is the squared-exponential
 * kernel: out_xy = exp(-γ·d) in (0, 1], v' = 1, κ̇ = 2γ·out_xy.  The exponential is the device
 * math library's exp / expf; flags is ignored.  A non-finite constant, A <= 0, B <= 0 or
 * |C| > 1 is CGP_EINVAL.
 *
 * cgp_sin_args has the fields and the rules of cgp_erf_args, then A, B, C, D: theta == NULL
 * is the forward-only pass; in-place (out_xy == xy, out_theta == theta) is allowed, and theta
 * may be xy itself; addend (optional) is added to out_xy only, as a separate rounding; same
 * or diag need n1 == n2; hw is at most 2048; nmaps < 2^31.
 */
typedef struct cgp_sin_args {
    const void* xy;         /* [nmaps][hw] */
    const void* theta;      /* [nmaps][hw] or NULL */
    void* out_xy;           /* [nmaps][hw] */
    void* out_theta;        /* [nmaps][hw] (unused when theta is NULL) */
    const void* addend;     /* [nmaps][hw] or NULL */
    const void* xx;         /* [n1][hw] variances at the nonlinearity's input */
    const void* yy;         /* [n2][hw] (may be NULL when same && diag) */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag;
    int32_t flags;          /* ignored */
    double A, B, C, D;      /* a²/2, b²/2, cos 2θ, a²b²/2 */
} cgp_sin_args;
size_t cgp_sin_args_size(void);
int cgp_sin_f64(const cgp_sin_args* args, void* stream);
int cgp_sin_f32(const cgp_sin_args* args, void* stream);
/* The sinusoid on the per-image variances: xx' = A·(1 - C·exp(-4B·xx)); yy' = xx' if same
 * else the same map of yy.  xx: [n1][hw], yy: [n2][hw].  D is checked and not used. */
int cgp_var_sin_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                    int32_t same, double A, double B, double C, double D, double* xx_out,
                    double* yy_out, void* stream);
int cgp_var_sin_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                    int32_t same, double A, double B, double C, double D, float* xx_out,
                    float* yy_out, void* stream);
/*
 * The sinusoid on position-pair maps, one entry point for both runs:
 *   out       = map(in) [+ addend]               theta == NULL: this alone
 *   out_theta = theta·κ̇ [+ addend_theta]         each a separate rounding
 * with cgp_cov_nonlin_*'s element rule: (c, v1, v2) = (in[m][p, q], xx[pair_i[m]][p],
 * yy[pair_j[m]][q]), and the override (out = v' of xx[pair_i[m]][p], κ̇ as above) where same,
 * pair_i[m] == pair_j[m] and p == q.  theta may be in, and in-place (out == in, out_theta ==
 * theta) is allowed: every element is read before it is written, by one thread.  out and
 * out_theta are two buffers.  addend_theta is read only with theta.
 */
typedef struct cgp_sin_cov_args {
    const void* in;            /* [npairs][h][h][w][w] */
    const void* theta;         /* like in, or NULL: the forward-only pass */
    void* out;
    void* out_theta;           /* (unused when theta is NULL) */
    const void* addend;        /* like out, or NULL */
    const void* addend_theta;  /* like out_theta, or NULL */
    const void* xx;            /* [n1][h][w] variances at the nonlinearity's input */
    const void* yy;            /* [n2][h][w] (same: may be xx) */
    const int32_t* pair_i;     /* device [npairs] */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w;
    int32_t same;
    int32_t flags;             /* ignored */
    double A, B, C, D;         /* a²/2, b²/2, cos 2θ, a²b²/2 */
} cgp_sin_cov_args;
size_t cgp_sin_cov_args_size(void);
int cgp_sin_cov_f64(const cgp_sin_cov_args* args, void* stream);
int cgp_sin_cov_f32(const cgp_sin_cov_args* args, void* stream);

/*
 * Any smooth φ by its Hermite (Mehler) series (additions to ABI 12: no struct or existing
 * entry point changed; no reference counterpart): tanh, sigmoid, softplus, SiLU,
 * GELU's tanh approximation, and erf and the exact GELU as cross-checks of cgp_erf_* and
 * cgp_gelu_*.  In the conventions of the ReLU entry points above -- per pixel (xy, xx, yy) =
 * (c, v1, v2), no rescaling.  With h_n = He_n/√n! and z ~ N(0, 1),
 *   a_n(v)  = E_z[φ(√v·z)·h_n(z)],   a'_n(v) = E_z[φ'(√v·z)·h_n(z)]    n = 0 .. order
 *   ρ       = c/√(v1·v2), 0 where v1·v2 is not positive, clamped to [-1, 1] (a NaN is kept)
 *   pair map    out_xy = Σ_n a_n(v1)·a_n(v2)·ρⁿ
 *   variances   v' = Σ_n a_n(v)²: the truncated sum, the pair map at ρ = 1, not E φ²
 *   NTK         out_theta = theta·κ̇,  κ̇ = Σ_n a'_n(v1)·a'_n(v2)·ρⁿ = ∂out_xy/∂c
 * Where cgp_relu_* overrides its map (same && !diag: pairs i == j; same && diag: all), out_xy
 * = v'[i], the same bits cgp_var_hermite_* writes, and κ̇ = Σ_n a'_n(v)².  The series is summed
 * by Horner from n = order down, one fma per term on the rounded product of the two
 * coefficients, so the map is symmetric in its two images bit for bit.
 *
 * cgp_hermite_coef_* computes the coefficients of `count` variances (every pixel of every
 * image of a variance buffer) by a Gauss–Hermite rule of nq nodes, in double whatever the
 * type, and stores them rounded once as tables a[n][count] (and da[n][count] of φ' when da is
 * not NULL).  nodes: device double [2][nq], the nodes z_q and then the weights w_q of a rule
 * for the standard normal, E_z[f(z)] = Σ_q w_q·f(z_q): the package uploads the probabilists'
 * Gauss–Hermite rule (numpy.polynomial.hermite_e.hermegauss, weights over √(2π)) compressed to
 * |z| <= 12.5 (program.hermite_rule).  A negative variance counts as 0.  1 <= order <= CGP_HERMITE_MAX_ORDER, order < nq <= CGP_HERMITE_MAX_NODES, count <
 * 2^31; otherwise CGP_EINVAL.
 */
#define CGP_HERMITE_TANH 0
#define CGP_HERMITE_SIGMOID 1
#define CGP_HERMITE_SOFTPLUS 2
#define CGP_HERMITE_SILU 3
#define CGP_HERMITE_GELU_TANH 4
#define CGP_HERMITE_ERF 5
#define CGP_HERMITE_GELU 6
#define CGP_HERMITE_MAX_ORDER 64
#define CGP_HERMITE_MAX_NODES 256
typedef struct cgp_hermite_coef_args {
    const void* var;        /* [count] variances */
    void* a;                /* [order + 1][count] */
    void* da;               /* [order + 1][count], or NULL: no table of φ' */
    const double* nodes;    /* device [2][nq] */
    int64_t count;
    int32_t phi;            /* CGP_HERMITE_* */
    int32_t order, nq;
    int32_t flags;          /* ignored */
} cgp_hermite_coef_args;
size_t cgp_hermite_coef_args_size(void);
int cgp_hermite_coef_f64(const cgp_hermite_coef_args* args, void* stream);
int cgp_hermite_coef_f32(const cgp_hermite_coef_args* args, void* stream);
/*
 * The series on pair maps.  cgp_hermite_args has the fields and the rules of cgp_erf_args
 * (theta == NULL is the forward-only pass; in-place is allowed, and theta may be xy itself;
 * addend is added to out_xy only, as a separate rounding; same or diag need n1 == n2; hw is at
 * most 2048; nmaps < 2^31), then the tables: ax / ay of the images of xx / yy (cgp_hermite_coef_*
 * over [n1·hw] and over [n2·hw] variances, or one call over a buffer that holds both), dax /
 * day with theta, and stride_x / stride_y, the elements between two n of each table (that
 * call's count), at least n1·hw and n2·hw.  ay may be ax where yy holds xx's values (same);
 * ay and day are not read when same && diag.
 */
typedef struct cgp_hermite_args {
    const void* xy;         /* [nmaps][hw] */
    const void* theta;      /* [nmaps][hw] or NULL */
    void* out_xy;           /* [nmaps][hw] */
    void* out_theta;        /* [nmaps][hw] (unused when theta is NULL) */
    const void* addend;     /* [nmaps][hw] or NULL */
    const void* xx;         /* [n1][hw] variances at the nonlinearity's input */
    const void* yy;         /* [n2][hw] (may be NULL when same && diag) */
    int64_t nmaps, n1, n2;
    int32_t hw, same, diag;
    int32_t flags;          /* ignored */
    const void* ax;         /* [order + 1][stride_x] */
    const void* ay;         /* [order + 1][stride_y] */
    const void* dax;        /* like ax, of φ' (unused when theta is NULL) */
    const void* day;
    int64_t stride_x, stride_y;
    int32_t order;
    int32_t reserved;
} cgp_hermite_args;
size_t cgp_hermite_args_size(void);
int cgp_hermite_f64(const cgp_hermite_args* args, void* stream);
int cgp_hermite_f32(const cgp_hermite_args* args, void* stream);
/* The series on the per-image variances: xx' = Σ_n a_n(xx)²; yy' = xx' if same else the same
 * of yy.  xx: [n1][hw], yy: [n2][hw].  It runs the coefficient kernel itself and squares and
 * sums the rounded coefficients in registers; no table is written. */
int cgp_var_hermite_f64(const double* xx, const double* yy, int64_t n1, int64_t n2, int32_t hw,
                        int32_t same, int32_t phi, int32_t order, int32_t nq,
                        const double* nodes, double* xx_out, double* yy_out, void* stream);
int cgp_var_hermite_f32(const float* xx, const float* yy, int64_t n1, int64_t n2, int32_t hw,
                        int32_t same, int32_t phi, int32_t order, int32_t nq,
                        const double* nodes, float* xx_out, float* yy_out, void* stream);
/*
 * The series on position-pair maps, one entry point for both runs, with cgp_sin_cov_*'s
 * fields and rules (the element rule, the override where same, pair_i[m] == pair_j[m] and
 * p == q, in-place, the addends), then the tables as in cgp_hermite_args: over the whole
 * buffers xx and yy, whatever images the pairs name.
 */
typedef struct cgp_hermite_cov_args {
    const void* in;            /* [npairs][h][h][w][w] */
    const void* theta;         /* like in, or NULL: the forward-only pass */
    void* out;
    void* out_theta;           /* (unused when theta is NULL) */
    const void* addend;        /* like out, or NULL */
    const void* addend_theta;  /* like out_theta, or NULL */
    const void* xx;            /* [n1][h][w] variances at the nonlinearity's input */
    const void* yy;            /* [n2][h][w] (same: may be xx) */
    const int32_t* pair_i;     /* device [npairs] */
    const int32_t* pair_j;
    int64_t npairs;
    int32_t h, w;
    int32_t same;
    int32_t flags;             /* ignored */
    const void* ax;            /* [order + 1][stride_x] */
    const void* ay;            /* [order + 1][stride_y] */
    const void* dax;           /* like ax, of φ' (unused when theta is NULL) */
    const void* day;
    int64_t stride_x, stride_y;
    int32_t order;
    int32_t reserved;
} cgp_hermite_cov_args;
size_t cgp_hermite_cov_args_size(void);
int cgp_hermite_cov_f64(const cgp_hermite_cov_args* args, void* stream);
int cgp_hermite_cov_f32(const cgp_hermite_cov_args* args, void* stream);

/*
 * out = alpha·a + beta·b (b may be NULL: out = alpha·a), n elements.  The unfused form
 * of Sum (alpha = beta = 1, kernel_patch.py:43-63) and Mixture (kernels.py:220-225).
 * Products and the sum are rounded separately (no FMA contraction), like torch.
 */
int cgp_axpby_f64(double alpha, const double* a, double beta, const double* b, double* out,
                  int64_t n, void* stream);
int cgp_axpby_f32(double alpha, const float* a, double beta, const float* b, float* out,
                  int64_t n, void* stream);

/*
 * dst[k] = alpha·src[k] (n[k] elements) for count buffers, in one launch per 32 (host
 * arrays of device pointers).  No reference counterpart: it fills the quartered x-side
 * variance maps the fp64 closed-form ReLU of cgp_net_f64 reads (one launch per tile instead
 * of one cgp_axpby_f64 per map; cnn_gp/netplan.py).
 */
int cgp_scale_batch_f64(int32_t count, const double* const* src, double* const* dst,
                        const int64_t* n, double alpha, void* stream);
/*
 * dst[k] = 1/sqrt(src[k]/8) (n[k] elements) for count buffers, in one launch per 32: the
 * maps cgp_net_f64's closed-form ReLU reads when cgp_net_var_form() is CGP_VAR_FORM_RSQRT
 * (an addition to ABI 12).  src holds plain variance maps; a zero variance gives +inf.  The
 * division and the square root are correctly rounded, so every producer of these maps
 * agrees bit for bit.  Every argument is checked before the first launch (CGP_EINVAL).
 */
int cgp_rsqrt_batch_f64(int32_t count, const double* const* src, double* const* dst,
                        const int64_t* n, void* stream);

/* load_kern's float32 → float64 widening, classify_gp.py:45-48 */
int cgp_cast_f32_f64(const float* in, double* out, int64_t n, void* stream);
/* dst[c][r] = src[r][c]; src [rows][cols] row-major */
int cgp_transpose_f64(const double* src, int64_t rows, int64_t cols, double* dst, void* stream);

/*
 * GP solve — replaces classify_gp.solve_system + diag_add (classify_gp.py:17-36):
 * scipy.linalg.solve(K, Y, assume_a='pos', lower=False) reads only the UPPER triangle
 * of the row-major K (its strictly-lower tiles are NaN in the reference's HDF5 files).
 *   K:  [n][ldk] row-major fp64; overwritten by the Cholesky factor of the column-major
 *       view's lower triangle (= the row-major upper triangle): for n > CGP_CHOL_NB (env,
 *       default 2048) a blocked right-looking factorisation (rocsolver_dpotrf_64 per
 *       diagonal block, rocblas_dtrsm_64 panel, rocblas_dsyrk_64 trailing update), else
 *       rocsolver_dpotrf_64 on the whole matrix; then rocsolver_dpotrs_64.
 *   bt: the right-hand sides TRANSPOSED, [nrhs][ldb] row-major (= column-major n×nrhs);
 *       overwritten by the solution (transposed).
 *   jitter is added to K's diagonal first (diag_add, classify_gp.py:30-36).
 *   *info (host): 0 = success; > 0 = the leading minor of that order is not positive
 *   definite (scipy raises LinAlgError in that case).
 * Synchronises `stream` before returning.
 */
int cgp_chol_solve_f64(double* k, int64_t n, int64_t ldk, double* bt, int64_t nrhs,
                       int64_t ldb, double jitter, int64_t* info, void* stream);
/*
 * Phase times (ms, HIP events on the call's stream) of the last cgp_chol_solve_f64 on
 * `stream`'s device: ms[0] = jitter (diag_add, classify_gp.py:30-36), ms[1] = the
 * Cholesky factorisation, ms[2] = dpotrs (0 when the factorisation failed).  Lets a
 * caller split the solve_system wall time of classify_gp.py:17-27 (no reference
 * counterpart: the reference times nothing).  CGP_EINVAL before any solve on that device.
 */
int cgp_chol_last_phases(void* stream, double* ms);
/*
 * ABI 10: cgp_chol_solve_f64 that also returns ITS OWN phase times in phase_ms[3] (ms:
 * jitter, factor, potrs; NULL: none), taken under the device's solver lock — another
 * thread's solve on the same device cannot overwrite them between the call and a later
 * cgp_chol_last_phases.  phase_ms is -1 in every slot when the call fails before timing.
 */
int cgp_chol_solve_f64_timed(double* k, int64_t n, int64_t ldk, double* bt, int64_t nrhs,
                             int64_t ldb, double jitter, int64_t* info, double* phase_ms,
                             void* stream);
/*
 * ABI 11: the solution check (no reference counterpart: scipy's solve never hands back a
 * wrong factor silently; rocSOLVER / rocBLAS factorisations in processes sharing one GPU
 * have, with info = 0 — round 5).  classify_gp.py:17-27's system K·X = Y, K given by its
 * row-major upper triangle, the triangle cgp_chol_solve_f64 reads and overwrites:
 *   cgp_sym_mirror_f64: K[i][j] = K[j][i] for every i > j (the strictly-lower triangle,
 *     unread by the solve, takes the system) and diag[i] = K[i][i] ([n], device).  Call
 *     before the factorisation (after any jitter: diag then holds K + jitter·I's).
 *   cgp_sym_residual_f64: r −= (L + Lᵀ + diag(d))·X with L the strictly-lower triangle
 *     of k: X and r are [nrhs][ldx] row-major (transposed, as cgp_chol_solve_f64's bt);
 *     r holds Y on entry and Y − K·X on return; *sumsq (device) += Σ_{i>j} K[i][j]² (so
 *     ‖K‖_F² = 2·sumsq + Σ d²).  Atomic accumulation: the last bits vary run to run.
 * One pass over the lower triangle each (n²/2 · 8 bytes read; the mirror writes as much).
 */
int cgp_sym_mirror_f64(double* k, int64_t n, int64_t ldk, double* diag, void* stream);
int cgp_sym_residual_f64(const double* k, int64_t n, int64_t ldk, const double* diag,
                         const double* x, double* r, int64_t nrhs, int64_t ldx, double* sumsq,
                         void* stream);
/*
 * Row-major C[m][n] = A[m][kdim] @ B[kdim][n] (fp64, rocBLAS) — the Kxz @ α product of
 * print_accuracy, classify_gp.py:39-42.
 */
int cgp_gemm_f64(const double* a, const double* b, double* c, int64_t m, int64_t n,
                 int64_t kdim, void* stream);
/*
 * GP predictive variance of m test points (the Kv_diag / Kt_diag
 * datasets save_kernel.py:33-36 writes are the prior variances this subtracts from):
 *   var[t] = kz_diag[t] − Kzx[t,:] · Kxx⁻¹ · Kxz[:,t]
 * given the factor cgp_chol_solve_f64 left in k (row-major upper triangle U, Kxx = UᵀU;
 * only that triangle is read, the NaN lower tiles of the reference's files are ignored).
 *   kxz: Kzx as [m][ldz] row-major (one test point per row, ldz >= n) — overwritten by
 *        V = U⁻ᵀ Kxz (rocblas_dtrsm_64, in place), so var[t] = kz_diag[t] − Σ_r V[t][r]².
 *   kz_diag: [m] prior variances (DiagIterator output); var: [m] out (may alias kz_diag).
 */
int cgp_pred_var_f64(const double* k, int64_t n, int64_t ldk, double* kxz, int64_t m,
                     int64_t ldz, const double* kz_diag, double* var, void* stream);
/* out[r] = argmax_c a[r][c] (first maximum, like torch.argmax), a: [rows][cols] */
int cgp_argmax_rows_f64(const double* a, int64_t rows, int64_t cols, int64_t* out,
                        void* stream);


/* ---------------------------------------------------------------------------------
 * Whole-network pair kernel.  Replaces the per-layer loop of Sequential.propagate
 * (kernels.py:184-187) over ALL layers for a tile: one workgroup owns one (i, j) pair
 * at a time and carries its covariance map through every op in LDS; only the images,
 * the per-image variance maps (read-only, L2-resident) and the final K[i, j] touch
 * global memory.  The host lowers the module tree to a list of cgp_net_op over LDS
 * "slots" (row-major planes with zero column halos) and supplies the
 * variance maps from the per-image pipeline (cgp_conv_* / cgp_var_relu_* on xx, yy).
 *
 *   CGP_NET_MOMENTS  dst = mean_c x_i[c]·y_j[c]                   kernels.py:44-47
 *   CGP_NET_CONV     dst = w·Σ_window src + b  [→ ReLU] [+ add]    kernels.py:92-98
 *   CGP_NET_RELU     dst = relu(src)           [+ add]            kernels.py:134-165
 *   CGP_NET_LINEAR   dst = weight·src + bias·add   (Sum / Mixture: kernels.py:220-254)
 *   CGP_NET_LOAD / CGP_NET_STORE   move a map between a slot and the per-unit state
 *                    record (var_x = the state buffer of the launch's units: record of
 *                    unit u at (u - unit_begin)·code elements; add = the map's offset in
 *                    the record) at a stage boundary
 *
 * Stages.  A network whose tail runs on small maps (a ResNet's 14x14 and 7x7 blocks)
 * is split at the resolution drops: the tail stages run several pairs per workgroup
 * (`pairs` = 4 at <= 16x16, 16 at <= 8x8), so a small map's ops still fill the
 * workgroup; the live maps cross a boundary through the state buffer.
 *
 * Same tiles (same=1) evaluate only i < j, mirror K[j, i] = K[i, j] (the recursion is
 * symmetric in (i, j) when y = x) and take K[i, i] = kdiag[i] — the per-image
 * pipeline's final value, which is exactly what the reference's same/diag override of
 * every ReLU (kernels.py:155-162) makes the (i, i) pair map equal to.
 * --------------------------------------------------------------------------------- */
#define CGP_NET_CONV 0
#define CGP_NET_RELU 1
#define CGP_NET_MOMENTS 2
#define CGP_NET_LINEAR 3
#define CGP_NET_LOAD 4     /* stage input:  slot dst <- state[unit][add .. add + h·w) */
#define CGP_NET_STORE 5    /* stage output: state[unit][add .. add + h·w) <- slot src */
/* CONV code flag: a separable conv writes the rows of its row-sum scratch that lie outside
 * its input as zeros before its column pass; with this flag it skips them (the host has
 * proved no op since their last zeroing wrote there — cyclically over the stage's op
 * list, which repeats for every pair a workgroup walks).  The scratch is the LDS arena's
 * first cells: separable row passes write their input rows there and a one-pair
 * full-map reduction its two wave partial sums. */
#define CGP_NET_CODE_HS_CLEAN 0x100
/* CONV code flags of a map that only a full-map reduction reads (ABI 9; the host sets
 * both or neither):
 *   CGP_NET_CODE_SUM       a separable conv does not store its output map: each wave adds
 *                          its outputs (after the ReLU) into the pair's two wave partial sums
 *   CGP_NET_CODE_FROM_SUM  the next op, a full-map reduction (1x1 output, window = map) of
 *                          that map, reads those partial sums instead of the map
 * Preconditions (cgp_net_validate checks them on a host copy of the op list; the kernels
 * do not, since the list they read is in device memory):
 *   - SUM only on a separable conv: more than 3 taps, not pointwise, not a full-map
 *     reduction (the direct, pointwise and reduction forms store their map regardless);
 *   - SUM with add < 0 and dst2 < 0 (the summed outputs are the conv+ReLU values only);
 *   - one pair per workgroup or half (pairs 1 or 2): multi-pair stages ignore both flags;
 *   - the op right after a SUM conv is the FROM_SUM reduction of its dst map, and no later
 *     op reads that map (it is never stored); FROM_SUM only right after a SUM conv.
 * A list that breaks them reads zeroed partial sums (deterministic, wrong). */
#define CGP_NET_CODE_SUM 0x200
#define CGP_NET_CODE_FROM_SUM 0x400
#define CGP_NET_CODE_GEOMETRY 0xff  /* the cgp_net_geometry() code in the low bits */

typedef struct cgp_net_op {
    int32_t kind;          /* CGP_NET_* */
    int32_t code;          /* CONV: cgp_net_geometry(), | CGP_NET_CODE_HS_CLEAN when the row
                              sums' zero rows are known to be zero already, | CGP_NET_CODE_SUM
                              / CGP_NET_CODE_FROM_SUM for a map only a reduction reads;
                              RELU/LINEAR/MOMENTS: cgp_net_resolution() of the map, or -1
                              (generic) */
    int32_t src, dst, add; /* LDS element offsets of the slots' (0, 0) pixel; add < 0: none */
    int32_t ws_in, ws_out; /* row strides (elements) of the src slot / dst and add slots */
    int32_t relu;          /* CONV: apply the ReLU map to the conv output (then + add) */
    int32_t h, w;          /* RELU / LINEAR / MOMENTS: map size (CONV: output size) */
    uint32_t div_m, div_s; /* w as a multiply-high divisor (host: make_fastdiv(w)) */
    int32_t dst2;          /* CONV/RELU/LINEAR: also write relu(result) here (< 0: no) */
    int32_t zero_halo;     /* before the op, zero the halo cells of the dst slot (bits 0-15)
                              and of the dst2 slot (bits 16-31), each (HL << 8) | gap:
                              HL cells before pixel (0, 0) and `gap` = ws_out - w cells
                              after every row; 0 = none.  Set on a slot placed on cells
                              another slot used as data (the LDS arena is shared across
                              map sizes). */
    double weight, bias;   /* CONV: w·Σ + b;  LINEAR: dst = weight·src + bias·add */
    const void* var_x;     /* ReLU input variances of the x images, [n1][h·w]; for
                              cgp_net_f64 without CGP_FLAG_EXACT_RELU: SCALED by
                              cgp_net_xvar_scale() (v/16 from ABI 9, v/4 before; the
                              scaled closed form; var2_x likewise) when
                              cgp_net_var_form() is CGP_VAR_FORM_SCALED; with
                              CGP_VAR_FORM_RSQRT all four fields point at 1/sqrt(v/8)
                              maps (cgp_rsqrt_batch_f64) instead of variances */
    const void* var_y;     /* ... of the y images, [n2][h·w] */
    const void* var2_x;    /* dst2's ReLU: variances of the result, [n1][h·w] */
    const void* var2_y;    /* [n2][h·w] */
} cgp_net_op;

typedef struct cgp_net_args {
    const void* x;         /* images [n1][channels][h][w] */
    const void* y;         /* images [n2][channels][h][w] (== x when same) */
    void* out;             /* K tile [n1][ldo] */
    const void* kdiag;     /* same tiles: K[i, i] (the per-image final variance), [n1] */
    const cgp_net_op* ops; /* DEVICE array of nops ops */
    int64_t n1, n2, ldo;
    int32_t nops, channels, h, w;
    int32_t same;          /* 1: y is x (Kxx diagonal tile) */
    int32_t final_slot;    /* LDS offset of the 1x1 result */
    int32_t hs;            /* LDS offset of the row-sum scratch */
    int32_t lds_elems;     /* LDS footprint of ONE pair (elements of the compute type) */
    int32_t flags;         /* CGP_FLAG_EXACT_RELU */
    int32_t pairs;         /* pairs per workgroup: 1; 2 = two one-pair slices of a 256-thread
                              workgroup (units u, u + 1: the same image i), any op list; or
                              4 / 16 for a stage whose maps are at most 16x16 / 8x8 (each
                              pair gets its own lds_elems arena) */
    int64_t unit_begin;    /* the tile's pair units this launch covers, [begin, end): unit */
    int64_t unit_end;      /* u = 64·supertile + 8·(i % 8) + j % 8; 0, 0 = the whole tile */
    int32_t final_stage;   /* 1: write K (the last stage); 0: the ops end in CGP_NET_STORE */
    int32_t program;       /* 0: interpret the op records; k > 0: run compiled program k,
                              the value cgp_net_program() returned for these records */
    int32_t part;          /* LDS offset of the two wave partial sums of a one-pair
                              full-map reduction (ABI 8): cells the host keeps off the
                              scratch's zero rows (CGP_NET_CODE_HS_CLEAN) */
} cgp_net_args;

/*
 * The per-image variance maps of a network in ONE launch (replaces the layer-by-layer
 * variance pipeline of cnn_gp/program.py Plan.run_variances: one launch per op).  A self
 * pair's recursion is linear (kernels.py:44-49 moments of x with itself, :92-98 convs,
 * :154-164 the ReLU of a variance is xx/2, :252-254 Sums), so one workgroup walks an image
 * through the whole op list in LDS and stores the maps the whole-network kernel reads.
 *   CGP_VAR_MOMENTS  dst = mean_c x·x                       (src unused)
 *   CGP_VAR_CONV     dst = w·Σ_window src + b   (zero padding; row sums, then columns)
 *   CGP_VAR_HALF     dst = src / 2
 *   CGP_VAR_SUM      dst = c0·t0 (+ c_k·t_k, k = 1..3, left to right; term slot -1 ends)
 * A value is stored when store >= 0: image g's map at out[n·store + g·ho·wo] (n = n1 + n2
 * images, the x images first), and, for g < n1, cgp_net_xvar_scale() × the map at
 * out[n·store_total + n1·qstore + g·ho·wo] when qstore >= 0 (the scaled x-side maps of
 * cgp_net_f64; store_total = Σ of every stored value's ho·wo).  Slots are LDS element
 * offsets, maps row-major [ho][wo].
 */
#define CGP_VAR_MOMENTS 0
#define CGP_VAR_CONV 1
#define CGP_VAR_HALF 2
#define CGP_VAR_SUM 3
typedef struct cgp_var_op {
    int32_t kind;
    int32_t dst;
    int32_t src[4];        /* CONV / HALF: src[0]; SUM: terms, -1 after the last */
    int32_t h, w, ho, wo;  /* input and output map sizes */
    int32_t taps, offset, stride, dilation;   /* CONV, as cgp_conv_args */
    int64_t store;         /* per-image element offset of the stored map, -1: not stored */
    int64_t qstore;        /* ... of its scaled x-side copy, -1: none */
    double weight, bias;   /* CONV */
    double coef[4];        /* SUM */
} cgp_var_op;
typedef struct cgp_var_args {
    const void* x;         /* images [n1][channels][h][w] */
    const void* y;         /* images [n2][channels][h][w] (n2 = 0: x only, e.g. same tiles) */
    void* out;             /* stored maps, see above */
    const cgp_var_op* ops; /* DEVICE array of nops ops */
    int64_t n1, n2;
    int64_t store_total;   /* Σ ho·wo of the stored values */
    int32_t nops, channels, h, w;
    int32_t lds_elems;     /* LDS of one image (elements of the compute type), scratch incl. */
    int32_t scratch;       /* LDS offset of the convs' row-sum scratch ([h][wo] elements) */
} cgp_var_args;
size_t cgp_var_op_size(void);
size_t cgp_var_args_size(void);
int cgp_var_chain_f64(const cgp_var_args* args, void* stream);
int cgp_var_chain_f32(const cgp_var_args* args, void* stream);

/* Geometry code of a conv for CGP_NET_CONV, or -1 if the fused kernel has no
 * instantiation for it (the caller then runs the layer-by-layer path). */
int cgp_net_geometry(int32_t h, int32_t w, int32_t ho, int32_t wo, int32_t taps,
                     int32_t stride, int32_t offset);
/* elements of row-sum scratch the conv of geometry `code` needs (-1: bad code) */
int cgp_net_hs_elems(int32_t code);
/* supertile edge of the pair walk: a tile's pairs are numbered in kST×kST blocks (upper
 * triangle of blocks when same), kST² units each; hosts size unit ranges with it */
int cgp_net_supertile(void);
size_t cgp_net_op_size(void);
size_t cgp_net_args_size(void);
/* Elementwise-op size code for cgp_net_op.code, or -1 (generic runtime-size path). */
int cgp_net_resolution(int32_t h, int32_t w);
/* cgp_net_args.flags: CGP_FLAG_EXACT_RELU, and CGP_FLAG_NET_DUAL when any op has dst2
 * (selects the kernel instantiation with the dual output stage) */
#define CGP_FLAG_NET_DUAL 4
/* workgroups per CU the fused kernel reaches with lds_bytes of LDS per pair and `pairs`
 * pairs per workgroup (0 if it cannot run) */
int cgp_net_occupancy(int32_t lds_bytes, int32_t f64, int32_t flags, int32_t pairs);
/* LDS arenas (one per pair unit) a workgroup of `pairs` pairs holds: `pairs`, except for
 * the two-pair head stage, whose workgroup holds two one-pair slices.  A stage needs
 * lds_bytes × cgp_net_units(pairs) + cgp_net_static_lds() <= 160 KB. */
int cgp_net_units(int32_t pairs);
/* The compiled program (k > 0) whose op list equals ops[0, nops) (HOST memory) in every
 * field but weight, bias and the variance / state pointers, for `pairs` pairs per
 * workgroup, flags (CGP_FLAG_NET_DUAL), the per-pair LDS footprint and the item size
 * (4 or 8); 0 if none.  The library holds the lowered programs of the reference configs
 * (net_programs.h); a program kernel runs them with every offset an immediate. */
int cgp_net_program(const cgp_net_op* ops, int32_t nops, int32_t pairs, int32_t flags,
                    int32_t lds_elems, int32_t itemsize);
/* An addition to ABI 12 (a query: nothing on the production path calls it).  A compiled fp64
 * program holds a second, lean op chain beside the default one: conv+ReLU sites without the
 * cap of the one-root form ("cap-free") and, on non-negative inputs, without its max(c, 0)
 * add ("add-free": the site stores out/2 and its reader convs take 2w), bit-identical to
 * the default chain.  Every workgroup picks the lean chain by itself
 * when each CGP_NET_CONV record of the launch has a finite weight 0 <= w <= 2^60 and a bias
 * 2^-60 <= b <= 2^60.  Returns 1 and writes the number of ReLU sites of the program that
 * then run cap-free and add-free when ops[0, nops) (HOST memory) matches a program
 * (cgp_net_program's arguments) whose kernel would take the lean chain on these records;
 * 0 when no program matches, a record fails that condition, itemsize is not 8, flags has
 * CGP_FLAG_EXACT_RELU, or the library was built with CGP_RELU_LEAN=0 or
 * CGP_RELU_ONE_ROOT=0.  capfree / addfree may be NULL. */
int cgp_net_program_lean(const cgp_net_op* ops, int32_t nops, int32_t pairs, int32_t flags,
                         int32_t lds_elems, int32_t itemsize, int32_t* capfree,
                         int32_t* addfree);
/* ABI 10: CGP_OK, or CGP_EINVAL (message in cgp_last_error) when the op list (HOST memory)
 * breaks the CGP_NET_CODE_SUM / CGP_NET_CODE_FROM_SUM preconditions for `pairs` pairs per
 * workgroup.  cnn_gp.netplan calls it once per stage before the first launch. */
int cgp_net_validate(const cgp_net_op* ops, int32_t nops, int32_t pairs);
/* ABI 10: bytes of LDS the fused kernel declares statically per workgroup (pair table, SUM
 * partial sums, program records, work-counter slots), on top of lds_bytes ×
 * cgp_net_units(pairs): a stage fits when the sum is <= 160 KB. */
int cgp_net_static_lds(void);
/* ABI 6: cgp_net_f64's fast path reads var_x / var2_x quartered (see cgp_net_op). */
int cgp_net_f64(const cgp_net_args* args, void* stream);
int cgp_net_f32(const cgp_net_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CNNGP_H */
