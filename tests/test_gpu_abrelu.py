"""GPU tests of the two-slope ReLU (cnn_gp.ABReLU / cnn_gp.LeakyReLU): cgp_abrelu_* /
cgp_var_abrelu_* / cgp_abrelu_cov_* alone, models through forward, ntk, position_covariance,
ntk_maps and position_ntk against the test-time oracle (tests/abrelu_oracle.py), the bit
identities at (a, b) = (0, 1) and (1, 1), the Gram builds, the plan cache following a slope,
and that a ReLU-only model makes the launches it made before.

Tolerances are the project's own (tests/test_gpu_ntk.py, tests/test_gpu_erf.py): float64 with
set_exact_relu 1e-10, float64 closed form 1e-8, float32 against the float64 oracle on
float32-representable inputs 2e-5, each times A(a, b) = ((a − b)² + 2|ab|)/(a² + b²)
(abrelu_oracle.tol_factor: derived, not measured).  The metric is max|got − ref| / max|ref|,
because these kernels cross zero."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp.kernel_save_tools import save_K

import abrelu_oracle as AB
import pool_oracle as PO
from test_gpu_erf import OP_CASES, PARENT_CALLS, MemH5, patches, recorded_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}
# (dtype, set_exact_relu) -> the project's tolerance
TOL = {("f64", True): 1e-10, ("f64", False): 1e-8, ("f32", True): 2e-5, ("f32", False): 2e-5}
SLOPES = [(0.01, 1.0), (0.2, 1.0), (-1.0, 1.0), (1.0, 1.0), (0.0, 1.0), (-0.5, 2.0)]
ORACLE_SLOPES = [s for s in SLOPES if s not in ((1.0, 1.0), (0.0, 1.0))]

m = cnn_gp
S, C, R, G, A, CC, AR, LR = (m.Sequential, m.Conv2d, m.ReLU, m.GlobalAvgPool, m.AvgPool2d,
                             m.CorrelatedConv2d, m.ABReLU, m.LeakyReLU)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def assert_bits(got, want):
    """the same bit patterns, the sign of zero included"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    np.testing.assert_array_equal(got.view(u), want.view(u))


def smh(a, b):
    return AR(a, b).constants()


# ------------------------------------------------------------------------------------
# a. the layer-path op alone
# ------------------------------------------------------------------------------------
def run_abrelu(ab, xy, theta, xx, yy, n1, n2, same, diag, dtn, exact, addend=None,
               inplace=False, alias=False):
    """cgp_abrelu_*: theta None is the forward-only form; ``alias`` passes xy itself as theta;
    ``inplace`` writes over the inputs.  Returns (K', Θ' or None) as numpy arrays."""
    dt = TORCH_DT[dtn]
    c, vx, vy = dev(xy, dt), dev(xx, dt), dev(yy, dt)
    th = c if alias else (None if theta is None else dev(theta, dt))
    ad = None if addend is None else dev(addend, dt)
    oc = c if inplace else torch.empty_like(c)
    oth = None if th is None else (th if inplace and not alias else torch.empty_like(c))
    a = N.ABReluArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(c), N.ptr(th), N.ptr(oc), N.ptr(oth)
    a.addend, a.xx, a.yy = N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2 = xy.shape[0], n1, n2
    a.hw, a.same, a.diag = xy.shape[1], int(same), int(diag)
    a.flags = N.CGP_FLAG_EXACT_RELU if exact else 0
    a.s, a.m, a.h = smh(*ab)
    N.check(getattr(N.load(), f"cgp_abrelu_{dtn}")(ctypes.byref(a), stream()), "cgp_abrelu")
    torch.cuda.synchronize()
    return oc.cpu().numpy(), None if oth is None else oth.cpu().numpy()


def run_var_abrelu(ab, xx, yy, same, dtn):
    dt = TORCH_DT[dtn]
    vx, vy = dev(xx, dt), dev(yy, dt)
    ox, oy = torch.empty_like(vx), torch.empty_like(vy)
    N.call(f"cgp_var_abrelu_{dtn}", N.ptr(vx), N.ptr(vy), xx.shape[0], yy.shape[0], xx.shape[1],
           int(same), smh(*ab)[2], N.ptr(ox), N.ptr(oy), stream())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oy.cpu().numpy()


def run_relu_twins(xy, theta, xx, yy, n1, n2, same, diag, dtn, exact, addend):
    """cgp_relu_* (plain and with the addend), cgp_relu_ntk_* and cgp_var_relu_* on the same
    inputs: (K', K' + addend, (K', Θ') of the NTK step, (xx', yy'))"""
    dt = TORCH_DT[dtn]
    lib = N.load()
    c, th, vx, vy, ad = (dev(v, dt) for v in (xy, theta, xx, yy, addend))
    flags = N.CGP_FLAG_EXACT_RELU if exact else 0
    outs = []
    for add in (None, ad):
        o = torch.empty_like(c)
        r = N.ReluArgs()
        r.xy, r.out, r.addend, r.xx, r.yy = N.ptr(c), N.ptr(o), N.ptr(add), N.ptr(vx), N.ptr(vy)
        r.nmaps, r.n1, r.n2 = xy.shape[0], n1, n2
        r.hw, r.same, r.diag, r.flags = xy.shape[1], int(same), int(diag), flags
        N.check(getattr(lib, f"cgp_relu_{dtn}")(ctypes.byref(r), stream()), "cgp_relu")
        outs.append(o)
    ok, ot = torch.empty_like(c), torch.empty_like(c)
    r = N.ReluNtkArgs()
    r.xy, r.theta, r.out_xy, r.out_theta = N.ptr(c), N.ptr(th), N.ptr(ok), N.ptr(ot)
    r.xx, r.yy = N.ptr(vx), N.ptr(vy)
    r.nmaps, r.n1, r.n2 = xy.shape[0], n1, n2
    r.hw, r.same, r.diag, r.flags = xy.shape[1], int(same), int(diag), flags
    N.check(getattr(lib, f"cgp_relu_ntk_{dtn}")(ctypes.byref(r), stream()), "cgp_relu_ntk")
    ox, oy = torch.empty_like(vx), torch.empty_like(vy)
    N.call(f"cgp_var_relu_{dtn}", N.ptr(vx), N.ptr(vy), xx.shape[0], yy.shape[0], xx.shape[1],
           int(same), N.ptr(ox), N.ptr(oy), stream())
    torch.cuda.synchronize()
    cpu = lambda t: t.cpu().numpy()                                             # noqa: E731
    return cpu(outs[0]), cpu(outs[1]), (cpu(ok), cpu(ot)), (cpu(ox), cpu(oy))


@pytest.mark.parametrize("exact", [False, True], ids=["closed", "exact"])
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_abrelu_op(case, dtn, exact):
    """erf's op cases and patches (v in (0, 3] with 10% zero variances, |ρ| <= 0.98, signed c,
    the overridden pairs at c = v).  At (0, 1) every output has the bits of the ReLU entry
    points; at (1, 1) the bits of the inputs; every other slope pair against the float64
    oracle; every calling form bit-equal to the plain one."""
    n1, n2, hw, same, diag = case
    xy, theta, xx, yy, addend = patches(n1, n2, hw, same, diag, 300 + hw + n1, NP_DT[dtn])
    xy = xy + NP_DT[dtn](0)                                  # no -0 (ρ < 0 at v = 0) in the inputs
    run = functools.partial(run_abrelu, xy=xy, xx=xx, yy=yy, n1=n1, n2=n2, same=same, diag=diag,
                            dtn=dtn, exact=exact)

    # (0, 1): the ReLU entry points, bit for bit
    rk, rka, (nk, nth), (rvx, rvy) = run_relu_twins(xy, theta, xx, yy, n1, n2, same, diag, dtn,
                                                    exact, addend)
    k0, none = run((0.0, 1.0), theta=None)
    assert none is None
    assert_bits(k0, rk)
    assert_bits(run((0.0, 1.0), theta=None, addend=addend)[0], rka)
    k, th = run((0.0, 1.0), theta=theta)
    assert_bits(k, nk)
    assert_bits(th, nth)
    assert_bits(nk, rk)
    vx, vy = run_var_abrelu((0.0, 1.0), xx, yy, same, dtn)
    assert_bits(vx, rvx)
    assert_bits(vy, rvy)

    # (1, 1): the identity, bit for bit
    k, th = run((1.0, 1.0), theta=theta)
    assert_bits(k, xy)
    assert_bits(th, theta)
    assert_bits(run((1.0, 1.0), theta=None)[0], xy)
    vx, vy = run_var_abrelu((1.0, 1.0), xx, yy, same, dtn)
    assert_bits(vx, xx)
    assert_bits(vy, xx if same else yy)

    # the other slopes against the oracle
    sel = np.arange(n1) if diag else np.arange(n1) * (n2 + 1)
    for ab in ORACLE_SLOPES:
        tol = TOL[dtn, exact] * AB.tol_factor(*ab)
        ok, oth, ovx, ovy = AB.pair_op(xy, theta, xx, yy, same, diag, *ab)
        k0, _ = run(ab, theta=None)
        k, th = run(ab, theta=theta)
        assert_bits(k, k0)                                   # one device function for K'
        vx, vy = run_var_abrelu(ab, xx, yy, same, dtn)
        errs = dict(K=max_err(k, ok), T=max_err(th, oth), xx=max_err(vx, ovx),
                    yy=max_err(vy, ovy))
        print(f"abrelu op {ab} {dtn} exact={exact} {case}: "
              + " ".join(f"{n}={e:.2e}" for n, e in errs.items()) + f" (tol {tol:.1e})")
        assert max(errs.values()) < tol, errs
        if same:
            assert_bits(vy, vx)
            assert_bits(k[sel], vx)                          # K' = h·v[i], the same bits
            h = NP_DT[dtn](smh(*ab)[2])
            assert_bits(th[sel], theta[sel] * h)             # Θ' = Θ·h

    # in place; theta aliasing xy; the addend (a separate rounding, on K' only)
    ab = (-0.5, 2.0)
    k, th = run(ab, theta=theta)
    ki, thi = run(ab, theta=theta, inplace=True)
    assert_bits(ki, k)
    assert_bits(thi, th)
    assert_bits(run(ab, theta=None, inplace=True)[0], k)
    ka, tha = run(ab, theta=None, alias=True)
    kx, thx = run(ab, theta=xy)
    assert_bits(ka, k)
    assert_bits(kx, k)
    assert_bits(tha, thx)
    kai, thai = run(ab, theta=None, alias=True, inplace=True)
    assert_bits(kai, k)
    assert_bits(thai, thx)
    kd, thd = run(ab, theta=theta, addend=addend)
    assert_bits(kd, k + addend)
    assert_bits(thd, th)
    assert_bits(run(ab, theta=None, addend=addend)[0], kd)


# ------------------------------------------------------------------------------------
# b. the position-pair entry point alone
# ------------------------------------------------------------------------------------
def cov_launch(name, rec, s, theta, xx, yy, pi, pj, dtn, same, exact, addend=None,
               addend_theta=None, fill=None, inplace=False):
    """one launch of a position-pair nonlinearity entry point on [m, p_row, p_col, q_row,
    q_col] arrays (the oracle's layout); theta None: the forward form.  ``fill(a)`` sets the
    record's own fields.  Returns (out, out_theta or None)."""
    dt = TORCH_DT[dtn]
    h, w = s.shape[1:3]
    lay = lambda v: None if v is None else dev(PO.to_device_layout(v), dt)      # noqa: E731
    idx32 = lambda v: torch.as_tensor(np.asarray(v)).to(DEV, torch.int32)       # noqa: E731
    sd, td, ad, atd = lay(s), lay(theta), lay(addend), lay(addend_theta)
    di, dj, vx, vy = idx32(pi), idx32(pj), dev(xx, dt), dev(yy, dt)
    out = sd if inplace else torch.empty_like(sd)
    a = rec()
    a.in_, a.out, a.addend, a.xx, a.yy = N.ptr(sd), N.ptr(out), N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.pair_i, a.pair_j, a.npairs = N.ptr(di), N.ptr(dj), len(pi)
    a.h, a.w, a.same = h, w, int(same)
    a.flags = N.CGP_FLAG_EXACT_RELU if exact else 0
    tout = None
    if theta is not None:
        tout = td if inplace else torch.empty_like(sd)
        a.theta, a.out_theta, a.addend_theta = N.ptr(td), N.ptr(tout), N.ptr(atd)
    if fill is not None:
        fill(a)
    N.check(getattr(N.load(), f"{name}_{dtn}")(ctypes.byref(a), stream()), name)
    torch.cuda.synchronize()
    back = lambda t: None if t is None else PO.from_device_layout(t.cpu().numpy(), h, w)   # noqa
    return back(out), back(tout)


def run_abrelu_cov(ab, *args, **kw):
    def fill(a):
        a.s, a.m, a.hh = smh(*ab)
    return cov_launch("cgp_abrelu_cov", N.ABReluCovArgs, *args, fill=fill, **kw)


def set_relu_kind(a):
    a.kind = N.CGP_COV_RELU


# 7 pairs of 5x5 maps: 625 elements per pair, so 2048-element chunks straddle pairs;
# 3 pairs of 7x7 maps: 2401 elements per pair, so one pair spans chunks.  Both have i = j pairs
COV_CASES = {"7x5x5": (5, [0, 1, 1, 3, 2, 0, 2], [1, 1, 2, 3, 0, 3, 2]),
             "3x7x7": (7, [0, 1, 2], [1, 1, 0])}


@pytest.mark.parametrize("exact", [False, True], ids=["closed", "exact"])
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("same", [True, False], ids=["same", "xz"])
@pytest.mark.parametrize("case", list(COV_CASES))
def test_abrelu_cov_op(case, same, dtn, exact):
    """The layer-path test's patches on position-pair maps: v in (0, 3] with 10% zero
    variances, S[p, q] = ρ·√(v1[p]·v2[q]) with signed |ρ| <= 0.98 (the oracle's own acos is
    ill-conditioned beyond: its slope 1/√(1 − ρ²) is 5 at 0.98 and 1e8 one ulp from 1), and
    with ``same`` the overridden elements at c = v.  At (0, 1) bit-equal to cgp_cov_nonlin_*
    with kind RELU and to cgp_covntk_nonlin_*; every other slope pair against the oracle; with
    ``same`` the p = q entries of the i = j pairs are the override's h·v and Θ·h."""
    side, pi, pj = COV_CASES[case]
    pi, pj = np.array(pi), np.array(pj)
    rng = np.random.default_rng(50 + side)
    npdt = NP_DT[dtn]
    rnd = lambda v: v.astype(npdt).astype(np.float64)                            # noqa: E731

    def variances():
        v = 3.0 * (1.0 - rng.random((4, side, side)))
        v[rng.random(v.shape) < 0.1] = 0.0
        v[:, 0, 0] = 0.0                                     # a zero-variance pixel per image
        return rnd(v)
    vx = variances()
    vy = vx if same else variances()
    rho = rng.uniform(-0.98, 0.98, (len(pi),) + (side, side) * 2)
    s0 = rho * np.sqrt(vx[pi][:, :, :, None, None] * vy[pj][:, None, None, :, :])
    if same:
        v1 = np.broadcast_to(vx[pi][:, :, :, None, None], s0.shape)
        s0 = np.where(PO._self_mask(s0, pi, pj), v1, s0)
    s0 = rnd(s0) + 0.0                                       # no -0 in the inputs
    theta, addend, addend_t = (rnd(rng.standard_normal(s0.shape)) for _ in range(3))
    args = (vx, vy, pi, pj, dtn)
    kw = dict(same=same, exact=exact)

    # (0, 1): the ReLU entry points of the position-pair maps, bit for bit
    rk, _ = cov_launch("cgp_cov_nonlin", N.CovNonlinArgs, s0, None, *args, fill=set_relu_kind,
                       **kw)
    rka, _ = cov_launch("cgp_cov_nonlin", N.CovNonlinArgs, s0, None, *args, fill=set_relu_kind,
                        addend=addend, **kw)
    nk, nth = cov_launch("cgp_covntk_nonlin", N.CovNonlinNtkArgs, s0, theta, *args,
                         fill=set_relu_kind, **kw)
    nka, ntha = cov_launch("cgp_covntk_nonlin", N.CovNonlinNtkArgs, s0, theta, *args,
                           fill=set_relu_kind, addend=addend, addend_theta=addend_t, **kw)
    relu = (0.0, 1.0)
    assert_bits(run_abrelu_cov(relu, s0, None, *args, **kw)[0], rk)
    assert_bits(run_abrelu_cov(relu, s0, None, *args, addend=addend, **kw)[0], rka)
    k, th = run_abrelu_cov(relu, s0, theta, *args, **kw)
    assert_bits(k, nk)
    assert_bits(th, nth)
    k, th = run_abrelu_cov(relu, s0, theta, *args, addend=addend, addend_theta=addend_t, **kw)
    assert_bits(k, nka)
    assert_bits(th, ntha)
    # (1, 1): the identity
    k, th = run_abrelu_cov((1.0, 1.0), s0, theta, *args, **kw)
    assert_bits(k.astype(npdt), s0.astype(npdt))
    assert_bits(th.astype(npdt), theta.astype(npdt))

    self_pairs = pi == pj
    for ab in ORACLE_SLOPES:
        tol = TOL[dtn, exact] * AB.tol_factor(*ab)
        ok, okd = AB.abrelu_map(s0, vx, vy, pi, pj, same, *ab)
        k0, none = run_abrelu_cov(ab, s0, None, *args, **kw)
        assert none is None
        k, th = run_abrelu_cov(ab, s0, theta, *args, **kw)
        assert_bits(k, k0)
        errs = dict(K=max_err(k, ok), T=max_err(th, theta * okd))
        print(f"abrelu_cov {ab} {case} {dtn} exact={exact} same={same}: "
              + " ".join(f"{n}={e:.2e}" for n, e in errs.items()) + f" (tol {tol:.1e})")
        assert max(errs.values()) < tol, errs
        # the p = q entries of the self pairs: with same the variance entry point's bits
        var = run_var_abrelu(ab, vx.reshape(4, -1), vy.reshape(4, -1), same, dtn)[0]
        var = var.reshape(vx.shape)
        self_pq = np.einsum("mabab->mab", k)[self_pairs]
        if same:
            assert_bits(self_pq, var[pi[self_pairs]])
            h = npdt(smh(*ab)[2])
            assert_bits(np.einsum("mabab->mab", th)[self_pairs].astype(npdt),
                        np.einsum("mabab->mab", theta)[self_pairs].astype(npdt) * h)
        else:
            assert not np.array_equal(self_pq, var[pi[self_pairs]])

    # in place, theta aliasing in, and the addends (separate roundings)
    ab = (-0.5, 2.0)
    k, th = run_abrelu_cov(ab, s0, theta, *args, **kw)
    ki, thi = run_abrelu_cov(ab, s0, theta, *args, inplace=True, **kw)
    assert_bits(ki, k)
    assert_bits(thi, th)
    ka, tha = run_abrelu_cov(ab, s0, theta, *args, addend=addend, addend_theta=addend_t, **kw)
    assert_bits(ka.astype(npdt), k.astype(npdt) + addend.astype(npdt))
    assert_bits(tha.astype(npdt), th.astype(npdt) + addend_t.astype(npdt))
    ka2, tha2 = run_abrelu_cov(ab, s0, theta, *args, addend_theta=addend_t, **kw)
    assert_bits(ka2, k)
    assert_bits(tha2, tha)
    assert_bits(run_abrelu_cov(ab, s0, None, *args, addend=addend, **kw)[0], ka)


# ------------------------------------------------------------------------------------
# c. models against the oracle
# ------------------------------------------------------------------------------------
def bodies():
    """name -> (body modules, head modules, layer: the model also runs on the layer path).
    8x8 inputs; the body ends in a map, the head makes it 1x1."""
    return {
        "leaky_chain": ([C(3, var_bias=0.1), LR(), C(3, var_weight=1.5, var_bias=0.05), LR(0.2)],
                        [C(8, padding=0, var_bias=0.1)], True),
        "sum_block": ([C(3, var_bias=0.1), m.Sum([S(), S(C(3, var_weight=1.5), AR(-1, 1))]),
                       AR(0.3, 1.2)], [C(8, padding=0)], True),
        "strided": ([C(3, stride=2, var_bias=0.1), LR(0.2), C(3), AR(-0.5, 2)],
                    [C(4, padding=0, var_bias=0.2)], True),
        "pooled_head": ([C(3, var_bias=0.1), LR(0.2), A(2), C(3, var_weight=1.5, var_bias=0.1),
                         AR(-1, 1)], [G(), C(1, var_weight=2.0, var_bias=0.3)], False),
        "correlated": ([C(3, var_bias=0.1), LR(0.2), CC(3, lengthscale=1.5, var_bias=0.05),
                        AR(-0.5, 2)], [CC(8, padding=0, lengthscale=2.0, var_bias=0.2)], False),
    }


def model_factor(mods):
    return max(AB.tol_factor(mod.a, mod.b) for mm in mods for mod in mm.modules()
               if isinstance(mod, AR))


MODES = ["xx", "xz", "same_diag", "xz_diag"]


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:2], Z, False, True)}[mode]


def images(signed):
    """a 3 x 2 tile of 8x8 images with 3 channels, float32-representable"""
    rng = np.random.default_rng(31 + signed)
    draw = (lambda n: rng.standard_normal((n, 3, 8, 8)).astype(np.float32)) if signed else \
        (lambda n: rng.random((n, 3, 8, 8), dtype=np.float32))
    return draw(3).astype(np.float64), draw(2).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, signed):
    """mode -> (K, Θ, S, Θ maps) from the float64 oracle, once per model and image set: K and
    Θ of body + head (the layer oracle where the model has a layer path, which the host test
    ties to the walk on position-pair maps; that walk otherwise), S and Θ[p, q] of the body"""
    body, head, layer = bodies()[name]
    full, bod = S(*body, *head).double(), S(*body).double()
    X, Z = images(signed)
    out = {}
    for mode in MODES:
        args = mode_args(X, Z, mode)
        k, th = AB.ntk_stepwise(full, *args) if layer else AB.pool_ntk(full, *args)
        s, ts = AB.position_ntk(bod, *args)
        out[mode] = (k, th, s, ts)
    return out


@pytest.mark.parametrize("signed", [False, True], ids=["unit", "signed"])
@pytest.mark.parametrize("prec", ["f64-exact", "f64", "f32"])
@pytest.mark.parametrize("name", list(bodies()))
def test_model_against_the_oracle(name, prec, signed):
    dtn, exact = prec.split("-")[0], prec.endswith("exact")
    body, head, layer = bodies()[name]
    tol = TOL[dtn, exact] * model_factor(body)
    ref = reference(name, signed)
    full = S(*body, *head).to(DEV, TORCH_DT[dtn]).set_exact_relu(exact)
    bod = S(*body).to(DEV, TORCH_DT[dtn]).set_exact_relu(exact)
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(signed))
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            rk, rth, rs, rts = ref[mode]
            fwd = full(*args)
            assert tuple(fwd.shape) == rk.shape and fwd.dtype == X.dtype
            errs["K_" + mode] = max_err(fwd.cpu(), rk)
            if layer:
                k, th = full.ntk(*args, return_nngp=True)
                errs["T_" + mode] = max_err(th.cpu(), rth)
                errs["Kn_" + mode] = max_err(k.cpu(), rk)
            km, tm = full.ntk_maps(*args, return_nngp=True)
            errs["Km_" + mode] = max_err(km.cpu(), rk)
            errs["Tm_" + mode] = max_err(tm.cpu(), rth)
            s = bod.position_covariance(*args)
            assert tuple(s.shape) == rs.shape
            errs["S_" + mode] = max_err(s.cpu(), rs)
            sk, st = bod.position_ntk(*args, return_nngp=True)
            errs["Sn_" + mode] = max_err(sk.cpu(), rs)
            errs["TS_" + mode] = max_err(st.cpu(), rts)
            if mode == "xx":
                kxx = fwd.cpu().numpy()
            if mode == "same_diag":
                errs["diag"] = max_err(fwd.cpu(), np.diag(kxx))
    print(f"abrelu model {name} {prec}{' signed' if signed else ''} (tol {tol:.1e}): "
          + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, errs


# ------------------------------------------------------------------------------------
# d. model-level bit checks and behaviour
# ------------------------------------------------------------------------------------
def twin_nets(act):
    return {
        "chain": S(C(3, var_bias=0.1), act(), C(3, var_weight=1.5), act(), C(3), act(),
                   C(8, padding=0, var_bias=0.1)),
        "residual": S(C(3, var_bias=0.1), m.Sum([S(), S(act(), C(3), act(), C(3))]), act(),
                      C(8, padding=0)),
        "projection": S(C(3), act(), m.Sum([C(1, stride=2), S(C(3, stride=2), act(), C(3))]),
                        act(), C(4, padding=0)),
    }


@pytest.mark.parametrize("exact", [False, True], ids=["closed", "exact"])
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", list(twin_nets(R)))
def test_abrelu_0_1_model_has_the_relu_models_bits(name, dtn, exact):
    """ABReLU(0, 1) against the same model with ReLU() on the unfused layer path (set_fusion
    and set_fused_network off: every ReLU a cgp_relu_* / cgp_relu_ntk_* launch), forward and
    ntk, signed inputs"""
    dt = TORCH_DT[dtn]
    ab = twin_nets(lambda: AR(0, 1))[name].to(DEV, dt).set_exact_relu(exact)
    relu = twin_nets(R)[name].to(DEV, dt).set_exact_relu(exact)
    relu.set_fusion(False).set_fused_network(False)
    X, Z = (dev(a, dt) for a in images(True))
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            assert torch.equal(ab(*args), relu(*args)), mode
            k, th = ab.ntk(*args, return_nngp=True)
            rk, rth = relu.ntk(*args, return_nngp=True)
            assert torch.equal(k, rk) and torch.equal(th, rth), mode
        # fusion changes no arithmetic of the ABReLU model either
        k = ab(X, Z, False)
        assert torch.equal(ab.set_fusion(False)(X, Z, False), k)
        assert torch.equal(ab.set_fused_network(False)(X, Z, False), k)


def test_abrelu_1_1_model_is_the_linear_model():
    """ABReLU(1, 1) returns its input bit for bit, so the model is the one without it"""
    mods = lambda act: [C(3, var_bias=0.1)] + act + [C(3, var_weight=1.5)] + act + \
        [C(8, padding=0, var_bias=0.1)]                                         # noqa: E731
    ident = S(*mods([AR(1, 1)])).to(DEV, torch.float64)
    lin = S(*mods([])).to(DEV, torch.float64).set_fusion(False).set_fused_network(False)
    X, Z = (dev(a) for a in images(True))
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            assert torch.equal(ident(*args), lin(*args)), mode
            k, th = ident.ntk(*args, return_nngp=True)
            lk, lth = lin.ntk(*args, return_nngp=True)
            assert torch.equal(k, lk) and torch.equal(th, lth), mode


def test_changing_the_slope_changes_the_next_forward():
    """negative_slope is a plain attribute: assigning it goes through NNGPKernel.__setattr__,
    the plan cache's key follows, and the next call runs the new slope"""
    model = S(C(3, var_bias=0.1), LR(0.01), C(3), LR(0.01), C(8, padding=0)).to(DEV,
                                                                                  torch.float64)
    X, Z = images(True)
    Xd, Zd = dev(X), dev(Z)
    with torch.no_grad():
        k1 = model(Xd, Zd, False).cpu().numpy()
        assert max_err(k1, AB.kernel(model, X, Z, False, False)) < 1e-8
        for mod in model.mods:
            if isinstance(mod, LR):
                mod.negative_slope = 0.5
        k2 = model(Xd, Zd, False).cpu().numpy()
        ref2 = AB.kernel(S(C(3, var_bias=0.1), LR(0.5), C(3), LR(0.5), C(8, padding=0)).double(),
                         X, Z, False, False)
        assert max_err(k2, ref2) < 1e-8
        assert max_err(k1, ref2) > 1e-3                     # the two slopes are far apart
        th = model.ntk(Xd, Zd, False).cpu().numpy()
        assert max_err(th, AB.ntk_stepwise(model, X, Z, False, False)[1]) < 1e-8
        model.mods[1].a = 0.01                              # one slope back
        k3 = model(Xd, Zd, False).cpu().numpy()
        assert max_err(k3, AB.kernel(model, X, Z, False, False)) < 1e-8
        assert max_err(k3, ref2) > 1e-4


# ------------------------------------------------------------------------------------
# e. Gram builds
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gram_case():
    model = S(C(3), LR(), m.Sum([C(1, stride=2), S(C(3, stride=2), LR(0.2), C(3))]), LR(),
              C(4, padding=0)).to(DEV, torch.float64)
    X = torch.from_numpy(np.random.default_rng(4).standard_normal((10, 2, 8, 8))
                         .astype(np.float32).astype(np.float64))
    with torch.no_grad():
        k, th = model.ntk(X.to(DEV), return_nngp=True)
        assert torch.equal(k, model(X.to(DEV)))
    return model, X, k.cpu().numpy(), th.cpu().numpy()


def test_leaky_gram_matrix(gram_case):
    model, X, k, th = gram_case
    assert model.image_variances(X.to(DEV)) is None          # declines: the per-tile fallback
    iu = np.triu_indices(10)
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], k[iu])
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4, ntk=True)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], th[iu])


def test_leaky_save_K(gram_case):
    from torch.utils.data import TensorDataset
    model, X, k, th = gram_case
    ds = TensorDataset(X, torch.zeros(len(X), dtype=torch.int64))
    f = MemH5()
    nngp = gram.model_kern(model)
    save_K(f, lambda x, x2, same, diag: nngp(x, x2, same).cpu().numpy(), "K", ds, None, False,
           4, print_interval=1e9)
    save_K(f, gram.ntk_kern(model), "T", ds, None, False, 4, print_interval=1e9)
    for key, ref in (("K", k), ("T", th)):
        keep = ~np.isnan(f.d[key][0])
        assert keep[np.triu_indices(10)].all()
        np.testing.assert_array_equal(f.d[key][0][keep], ref.astype(np.float32)[keep])
    save_K(f, gram.ntk_kern(model), "Td", ds, None, True, 4, print_interval=1e9)
    np.testing.assert_array_equal(f.d["Td"][0], np.diag(th).astype(np.float32))


# ------------------------------------------------------------------------------------
# f. the launches: a model with the op, and models without it
# ------------------------------------------------------------------------------------
def record(fn):
    seen = []
    real = N.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    N.check = check
    try:
        with torch.no_grad():
            fn()
    finally:
        N.check = real
    torch.cuda.synchronize()
    return seen


def test_leaky_model_launches():
    """every op a launch of the new entry points: one variance launch and one pair launch per
    LeakyReLU on the layer path, one cgp_abrelu_cov_* per op (and stream) on position-pair maps"""
    model = S(C(3), LR(), C(3), LR(), C(8, padding=0)).to(DEV, torch.float64)
    X, Z = (dev(a) for a in images(False))
    seen = record(lambda: model(X, Z, False))
    assert seen.count("cgp_abrelu") == 2 and seen.count("cgp_var_abrelu_f64") == 2
    assert not any("relu" in s.replace("abrelu", "") or "net" in s for s in seen)
    seen = record(lambda: model.ntk(X, Z, False))
    assert seen.count("cgp_abrelu") == 2 and "cgp_relu_ntk" not in seen
    seen = record(lambda: model.ntk_maps(X, Z, False))
    assert seen.count("cgp_abrelu_cov") == 2
    assert "cgp_covntk_nonlin" not in seen and "cgp_cov_nonlin" not in seen
    pooled = S(C(3), LR(), A(2), C(3), LR(), G()).to(DEV, torch.float64)
    seen = record(lambda: pooled(X, Z, False))
    cov = [s for s in seen if s.startswith(("cgp_cov", "cgp_abrelu"))]
    mo, co, av, ab, po, di = ("cgp_cov_moments", "cgp_cov_conv", "cgp_covmap_avgpool",
                              "cgp_abrelu_cov", "cgp_cov_pool", "cgp_covmap_diag")
    assert cov == [mo, co, ab, av, co, di] * 2 + [mo, co, ab, av, co, ab, po]


@pytest.mark.parametrize("path", ["net", "layer"])
def test_relu_only_model_makes_the_same_calls(path, monkeypatch):
    import configs_util
    model = configs_util.model("mnist_paper_convnet_gp").double().to(DEV)
    model.set_fused_network(path == "net")
    x = dev(np.random.default_rng(0).random((4, 1, 28, 28)))
    seen = recorded_calls(model, x, monkeypatch)
    assert seen == PARENT_CALLS["mnist_paper_convnet_gp", path]
    assert not any("abrelu" in s for s in seen)


def test_pooled_relu_model_makes_the_same_calls():
    model = S(C(3), R(), A(2), C(3), R(), G()).to(DEV, torch.float64)
    X, Z = (dev(a) for a in images(False))
    seen = record(lambda: model(X, Z, False))
    mo, co, av, no, po, di = ("cgp_cov_moments", "cgp_cov_conv", "cgp_covmap_avgpool",
                              "cgp_cov_nonlin", "cgp_cov_pool", "cgp_covmap_diag")
    assert [s for s in seen if s.startswith("cgp_cov")] == \
        [mo, co, av, co, di] * 2 + [mo, co, av, co, no, po]
    assert not any("abrelu" in s for s in seen)
    seen = record(lambda: model.ntk_maps(X, Z, False))
    assert not any("abrelu" in s for s in seen) and "cgp_covntk_conv" in seen
