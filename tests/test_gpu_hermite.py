"""GPU tests of the Hermite-series nonlinearities (cnn_gp.HermiteNonlin, Tanh, Sigmoid, Softplus,
SiLU, GeluTanh): cgp_hermite_coef_* / cgp_hermite_* / cgp_var_hermite_* / cgp_hermite_cov_*
alone, models through forward, ntk and ntk_maps against the test-time oracle
(tests/hermite_oracle.py), HermiteNonlin("erf") / ("gelu") against Erf() / Gelu() on the
device, and the plan cache following an attribute.

Shapes: the smallest at which the walk can still go wrong.  3 x 5 x 7 images with n1 = 3,
n2 = 2 (an odd hw, a last workgroup that is partly filled); 1 x 28 x 28 with 3 x 1 maps (two
maps per workgroup, an odd map count); 1 x 6 x 6 on position-pair maps (1296 elements per
pair, so a 2048-element chunk straddles pairs).  The layer-path networks end in a Conv2d with
a square kernel over the whole map, so they run on 3 x 5 x 5 images; the pooled network runs
on 3 x 5 x 7.  The inputs hold exact-zero variance pixels and a duplicated image, so |ρ| = 1
at i != j.

Tolerances: the device against the oracle as max|Δ| / max|ref|, for K' and for Θ'.  The caps
are 1e-12 in float64 and 1e-5 in float32 (the README's north-star tolerance); the constants
below are the worst value measured on an MI355X times 4, rounded up to a power of ten, and never
above the cap (profiles/hermite/pytest_hermite.txt has every figure)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N

import hermite_oracle as HO
import pool_oracle as PO
from test_gpu_abrelu import assert_bits, cov_launch, record

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAP = {"f64": 1e-12, "f32": 1e-5}
# measured worst x 4, rounded up to a power of ten, capped (module docstring).  Worsts: the
# coefficient tables 7.9e-16 / 5.6e-8, the two walks 1.2e-15 / 1.5e-7 (order 64: 6.6e-16 /
# 1.2e-7, so the float32 Horner chain stays under its cap at every order), networks and the
# closed-form cross-check 7.8e-16 / 1.4e-7
COEF_TOL = {"f64": 1e-14, "f32": 1e-6}
OP_TOL = {"f64": 1e-14, "f32": 1e-6}
NET_TOL = {"f64": 1e-14, "f32": 1e-6}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}

m = cnn_gp
S, C, G, A, H = m.Sequential, m.Conv2d, m.GlobalAvgPool, m.AvgPool2d, m.HermiteNonlin

# order -> the φ the entry-point tests run at that order
ORDER_PHI = {1: "sigmoid", 2: "softplus", 32: "tanh", 64: "silu"}


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def check(what, errs, tol, cap):
    print(f"{what}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items())
          + f" (tol {tol:.0e}, cap {cap:.0e})")
    assert tol <= cap and max(errs.values()) < tol, errs


def nodes(nq):
    from cnn_gp.program import Plan
    return Plan._hermite_nodes(torch.device(DEV, torch.cuda.current_device()), nq)


def rule_ids(rule):
    return HO.PHI_ID[rule[0]], rule[1], rule[2]


def device_tables(var_ptr, count, rule, dtn, deriv, like):
    """cgp_hermite_coef_* over ``count`` variances at ``var_ptr``: (a, da or None) as device
    tensors [order + 1, count]"""
    phi, order, nq = rule_ids(rule)
    a = torch.empty((order + 1, count), dtype=like.dtype, device=like.device)
    da = torch.empty_like(a) if deriv else None
    c = N.HermiteCoefArgs()
    c.var, c.a, c.da, c.nodes, c.count = var_ptr, N.ptr(a), N.ptr(da), N.ptr(nodes(nq)), count
    c.phi, c.order, c.nq = phi, order, nq
    N.check(getattr(N.load(), f"cgp_hermite_coef_{dtn}")(ctypes.byref(c), stream()),
            "cgp_hermite_coef")
    return a, da


def set_tables(a, rule, dtn, n1h, n2h, same, deriv, like):
    """the tables of a record whose xx / yy are set; returns them (alive until the launch)"""
    ax, dax = device_tables(a.xx, n1h, rule, dtn, deriv, like)
    ay, day = (ax, dax) if same else device_tables(a.yy, n2h, rule, dtn, deriv, like)
    a.ax, a.ay, a.dax, a.day = N.ptr(ax), N.ptr(ay), N.ptr(dax), N.ptr(day)
    a.stride_x, a.stride_y, a.order = n1h, (n1h if same else n2h), rule[1]
    return ax, ay, dax, day


# ------------------------------------------------------------------------------------
# inputs: the moments of small random images with zero pixels, a duplicate and a negated copy
# ------------------------------------------------------------------------------------
def pixel_images(n1, n2, hw, same, seed, np_dt):
    """x [n1, 3, hw], y [n2, 3, hw] (y = x with same), rounded to np_dt: per-pixel scales in
    [0.2, 1.5], a tenth of the pixels of every image exactly zero, and |ρ| = 1 at i != j: with
    same x[2] = x[0]; otherwise y[0] = x[1] and y[1] = −x[2]"""
    rng = np.random.default_rng(seed)

    def draw(n):
        v = rng.standard_normal((n, 3, hw)) * rng.uniform(0.2, 1.5, (n, 1, hw))
        v = np.where(rng.random((n, 1, hw)) < 0.1, 0.0, v)
        v[:, :, 0] = 0.0
        return v.astype(np_dt).astype(np.float64)
    x = draw(n1)
    if same:
        if n1 > 2:
            x[2] = x[0]
        return x, x
    y = draw(n2)
    y[0] = x[1]
    if n2 > 1:
        y[1] = -x[2]
    return x, y


def pair_patches(n1, n2, hw, same, diag, seed, np_dt):
    """(xy, theta, xx, yy, addend) as [maps, hw] arrays of np_dt, from pixel_images"""
    x, y = pixel_images(n1, n2, hw, same, seed, np_dt)
    xx, yy = (x * x).mean(1), (y * y).mean(1)
    xy = (x * y).mean(1) if diag else (x[:, None] * y[None]).mean(2).reshape(n1 * n2, hw)
    rng = np.random.default_rng(seed + 1)
    theta, addend = rng.standard_normal(xy.shape), rng.standard_normal(xy.shape)
    return tuple(np.ascontiguousarray(v.astype(np_dt)) for v in (xy, theta, xx, yy, addend))


# ------------------------------------------------------------------------------------
# a. the coefficient kernel
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("phi", HO.PHIS)
def test_hermite_coef(phi, dtn):
    """the tables of φ and φ' of 5 x 35 variances (zeros among them, up to 3) at orders 1, 2,
    32 and 64 (every bucket of the kernel) against the oracle's coefficients, as max|Δ| over
    the largest coefficient; without da the same bits of a"""
    npdt = NP_DT[dtn]
    var = pair_patches(5, 5, 35, True, False, 7, npdt)[2].reshape(-1)
    assert (var == 0).any() and var.max() > 1
    vd = dev(var, TORCH_DT[dtn])
    errs = {}
    for order, nq in ((1, 2), (2, 96), (32, 96), (64, 96), (64, 256)):
        rule = (phi, order, nq)
        a, da = device_tables(N.ptr(vd), var.size, rule, dtn, True, vd)
        a0, none = device_tables(N.ptr(vd), var.size, rule, dtn, False, vd)
        torch.cuda.synchronize()
        assert none is None and torch.equal(a0, a)
        v64 = var.astype(np.float64)
        errs[f"a{order}/{nq}"] = max_err(a.cpu().numpy().T, HO.coefficients(v64, rule))
        errs[f"da{order}/{nq}"] = max_err(da.cpu().numpy().T, HO.coefficients(v64, rule, True))
    check(f"hermite_coef {phi} {dtn}", errs, COEF_TOL[dtn], CAP[dtn])


# ------------------------------------------------------------------------------------
# b. the layer-path op alone
# ------------------------------------------------------------------------------------
def run_hermite(rule, xy, theta, xx, yy, n1, n2, same, diag, dtn, addend=None, inplace=False,
                alias=False):
    """cgp_hermite_*: theta None is the forward-only form; ``alias`` passes xy itself as theta;
    ``inplace`` writes over the inputs.  Returns (K', Θ' or None) as numpy arrays."""
    dt = TORCH_DT[dtn]
    c, vx, vy = dev(xy, dt), dev(xx, dt), dev(yy, dt)
    th = c if alias else (None if theta is None else dev(theta, dt))
    ad = None if addend is None else dev(addend, dt)
    oc = c if inplace else torch.empty_like(c)
    oth = None if th is None else (th if inplace and not alias else torch.empty_like(c))
    a = N.HermiteArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(c), N.ptr(th), N.ptr(oc), N.ptr(oth)
    a.addend, a.xx, a.yy = N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2 = xy.shape[0], n1, n2
    a.hw, a.same, a.diag = xy.shape[1], int(same), int(diag)
    hw = xy.shape[1]
    keep = set_tables(a, rule, dtn, n1 * hw, n2 * hw, same, th is not None, c)  # noqa: F841
    N.check(getattr(N.load(), f"cgp_hermite_{dtn}")(ctypes.byref(a), stream()), "cgp_hermite")
    torch.cuda.synchronize()
    return oc.cpu().numpy(), None if oth is None else oth.cpu().numpy()


def run_var_hermite(rule, xx, yy, same, dtn):
    dt = TORCH_DT[dtn]
    vx, vy = dev(xx, dt), dev(yy, dt)
    ox, oy = torch.empty_like(vx), torch.empty_like(vy)
    phi, order, nq = rule_ids(rule)
    N.call(f"cgp_var_hermite_{dtn}", N.ptr(vx), N.ptr(vy), xx.shape[0], yy.shape[0],
           xx.shape[1], int(same), phi, order, nq, N.ptr(nodes(nq)), N.ptr(ox), N.ptr(oy),
           stream())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oy.cpu().numpy()


# (n1, n2, hw, same, diag): 5 x 7 maps in every mode, and 3 x 1 maps of 28 x 28
OP_CASES = [(3, 2, 35, 0, 0), (3, 3, 35, 1, 0), (3, 3, 35, 0, 1), (3, 3, 35, 1, 1),
            (3, 1, 784, 0, 0)]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("order", list(ORDER_PHI))
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_hermite_op(case, order, dtn):
    """K', Θ' and the variance maps against the float64 oracle; every calling form (forward
    only, in place, Θ aliasing K, the addend) bit-equal to the plain one; the overridden K'
    with the bits of cgp_var_hermite_*; the map symmetric in its two images bit for bit"""
    n1, n2, hw, same, diag = case
    npdt = NP_DT[dtn]
    xy, theta, xx, yy, addend = pair_patches(n1, n2, hw, same, diag, 300 + hw + n2, npdt)
    assert (xx == 0).any()
    rule = (ORDER_PHI[order], order, 96)
    run = functools.partial(run_hermite, rule, xy=xy, xx=xx, yy=yy, n1=n1, n2=n2, same=same,
                            diag=diag, dtn=dtn)
    ok, oth, ovx, ovy = HO.pair_op(xy, theta, xx, yy, same, diag, rule)
    k0, none = run(theta=None)
    assert none is None
    k, th = run(theta=theta)
    assert_bits(k, k0)                                       # one device function for K'
    vx, vy = run_var_hermite(rule, xx, yy, same, dtn)
    errs = dict(K=max_err(k, ok), T=max_err(th, oth), xx=max_err(vx, ovx), yy=max_err(vy, ovy))
    check(f"hermite op {rule} {dtn} {case}", errs, OP_TOL[dtn], CAP[dtn])
    if same:
        sel = np.arange(n1) if diag else np.arange(n1) * (n2 + 1)
        assert_bits(vy, vx)
        assert_bits(k[sel], vx)                              # K' = v'[i], the same bits
        if not diag:                                         # x[2] is x[0]: ρ = 1 at i != j
            assert max_err(k[2], k[0]) < CAP[dtn]
    elif not diag:
        # the two images exchanged: the transposed maps, bit for bit
        perm = np.arange(n1 * n2).reshape(n1, n2).T.ravel()
        kt, tht = run_hermite(rule, xy[perm], theta[perm], yy, xx, n2, n1, same, diag, dtn)
        assert_bits(kt, k[perm])
        assert_bits(tht, th[perm])

    # in place; theta aliasing xy; the addend (a separate rounding, on K' only)
    ki, thi = run(theta=theta, inplace=True)
    assert_bits(ki, k)
    assert_bits(thi, th)
    assert_bits(run(theta=None, inplace=True)[0], k)
    ka, tha = run(theta=None, alias=True)
    kx, thx = run(theta=xy)
    assert_bits(ka, k)
    assert_bits(kx, k)
    assert_bits(tha, thx)
    kai, thai = run(theta=None, alias=True, inplace=True)
    assert_bits(kai, k)
    assert_bits(thai, thx)
    kd, thd = run(theta=theta, addend=addend)
    assert_bits(kd, k + addend)
    assert_bits(thd, th)
    assert_bits(run(theta=None, addend=addend)[0], kd)


# ------------------------------------------------------------------------------------
# c. the position-pair entry point alone
# ------------------------------------------------------------------------------------
def run_hermite_cov(rule, s, theta, xx, yy, pi, pj, dtn, same, **kw):
    keep = []
    count = xx.size

    def fill(a):
        keep.append(set_tables(a, rule, dtn, count, yy.size, same, theta is not None,
                               torch.empty(0, dtype=TORCH_DT[dtn], device=DEV)))
    return cov_launch("cgp_hermite_cov", N.HermiteCovArgs, s, theta, xx, yy, pi, pj, dtn,
                      same=same, exact=False, fill=fill, **kw)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("order", list(ORDER_PHI))
@pytest.mark.parametrize("same", [True, False], ids=["same", "xz"])
def test_hermite_cov_op(same, order, dtn):
    """5 pairs of 6 x 6 maps, 1296 elements each, so the 2048-element chunks straddle pairs and
    the last is partial; self pairs, a duplicated and a negated image.  The forward and
    two-stream forms against the oracle, the K stream bit-equal between them, in place, both
    addends, and one launch over all pairs bit-equal to one launch per pair."""
    npdt = NP_DT[dtn]
    x, y = pixel_images(3, 3, 36, same, 90, npdt)
    x, y = x.reshape(3, 3, 6, 6), y.reshape(3, 3, 6, 6)
    pi, pj = (np.array([0, 1, 1, 2, 0]), np.array([1, 1, 2, 2, 2])) if same else \
        (np.array([0, 1, 1, 2, 0]), np.array([1, 0, 2, 1, 0]))
    rnd = lambda v: v.astype(npdt).astype(np.float64)                            # noqa: E731
    vx, vy = rnd(PO.variances(x)), rnd(PO.variances(y))
    s0 = rnd(PO.moments(x, y, pi, pj))
    assert (vx == 0).any()
    rng = np.random.default_rng(91)
    theta, addend, addend_t = (rnd(rng.standard_normal(s0.shape)) for _ in range(3))
    rule = (ORDER_PHI[order], order, 96)
    args = (vx, vy, pi, pj, dtn)
    ok, oth = HO.map_op(s0, theta, vx, vy, pi, pj, same, rule)
    k0, none = run_hermite_cov(rule, s0, None, *args, same=same)
    assert none is None
    k, th = run_hermite_cov(rule, s0, theta, *args, same=same)
    assert_bits(k, k0)
    errs = dict(K=max_err(k, ok), T=max_err(th, oth))
    check(f"hermite_cov {rule} {dtn} same={same}", errs, OP_TOL[dtn], CAP[dtn])
    if same:
        # the p = q entries of the self pairs: the variance entry point's bits
        var = run_var_hermite(rule, vx.reshape(3, -1), vy.reshape(3, -1), same, dtn)[0]
        self_pairs = pi == pj
        assert_bits(np.einsum("mabab->mab", k)[self_pairs].astype(npdt),
                    var.reshape(vx.shape)[pi[self_pairs]])

    # in place, and the addends (separate roundings)
    ki, thi = run_hermite_cov(rule, s0, theta, *args, same=same, inplace=True)
    assert_bits(ki, k)
    assert_bits(thi, th)
    ka, tha = run_hermite_cov(rule, s0, theta, *args, same=same, addend=addend,
                              addend_theta=addend_t)
    assert_bits(ka.astype(npdt), k.astype(npdt) + addend.astype(npdt))
    assert_bits(tha.astype(npdt), th.astype(npdt) + addend_t.astype(npdt))
    ka2, tha2 = run_hermite_cov(rule, s0, theta, *args, same=same, addend_theta=addend_t)
    assert_bits(ka2, k)
    assert_bits(tha2, tha)
    assert_bits(run_hermite_cov(rule, s0, None, *args, same=same, addend=addend)[0], ka)
    # one launch over all pairs against one launch per pair
    for p in range(len(pi)):
        k1, th1 = run_hermite_cov(rule, s0[p:p + 1], theta[p:p + 1], vx, vy, pi[p:p + 1],
                                  pj[p:p + 1], dtn, same=same)
        assert_bits(k1, k[p:p + 1])
        assert_bits(th1, th[p:p + 1])


# ------------------------------------------------------------------------------------
# d. networks
# ------------------------------------------------------------------------------------
MODES = ["xx", "xz", "same_diag", "xz_diag"]


def images(h, w, scale=1.0):
    """X [3, 3, h, w], Z [2, 3, h, w], float32-representable: the two left columns zero (a
    zero-variance column under the bias-free first conv) and Z[0] = X[1]"""
    rng = np.random.default_rng(17 * h + w)
    X, Z = ((rng.standard_normal((n, 3, h, w)) * scale).astype(np.float32).astype(np.float64)
            for n in (3, 2))
    X[:, :, :, :2], Z[:, :, :, :2] = 0.0, 0.0
    Z[0] = X[1]
    return X, Z


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:len(Z)], Z, False, True)}[mode]


def layer_net(act):
    """conv → φ → conv → φ → readout on 5 x 5 images"""
    return S(C(3), act(), C(3, var_weight=1.5, var_bias=0.1), act(), C(5, padding=0, var_bias=0.1))


def pooled_net(act):
    """the same with an AvgPool2d(2) and a GlobalAvgPool, on 5 x 7 images"""
    return S(C(3), act(), A(2), C(3, var_weight=1.5, var_bias=0.1), act(), G(),
             C(1, var_weight=2.0, var_bias=0.1))


ACTS = {"tanh": m.Tanh, "sigmoid": m.Sigmoid, "softplus": m.Softplus, "silu": m.SiLU,
        "gelu_tanh": m.GeluTanh, "erf": lambda: H("erf"), "gelu": lambda: H("gelu")}


@functools.lru_cache(maxsize=None)
def layer_reference(phi):
    model = layer_net(ACTS[phi]).double()
    X, Z = images(5, 5)
    out = {}
    for mode in MODES:
        args = mode_args(X, Z, mode)
        k = HO.kernel(model, *args)
        sk, th = HO.ntk_stepwise(model, *args)
        assert max_err(sk, k) < 1e-13
        out[mode] = (k, th)
    return out


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("phi", list(ACTS))
def test_network_against_the_oracle(phi, dtn):
    ref = layer_reference(phi)
    model = layer_net(ACTS[phi]).to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(5, 5))
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            rk, rth = ref[mode]
            fwd = model(*args)
            assert tuple(fwd.shape) == rk.shape and fwd.dtype == X.dtype
            k, th = model.ntk(*args, return_nngp=True)
            assert torch.equal(k, fwd), mode                 # K from ntk is forward's
            errs["K_" + mode] = max_err(fwd.cpu(), rk)
            errs["T_" + mode] = max_err(th.cpu(), rth)
            if mode == "xx":
                kxx, txx = fwd.cpu().numpy(), th.cpu().numpy()
                for a in (kxx, txx):
                    assert np.max(np.abs(a - a.T)) <= 1e-13 * np.max(np.abs(a))
            if mode == "same_diag":
                errs["diag"] = max_err(fwd.cpu(), np.diag(kxx))
    check(f"hermite network {phi} {dtn}", errs, NET_TOL[dtn], CAP[dtn])


@functools.lru_cache(maxsize=None)
def pooled_reference(phi):
    model = pooled_net(ACTS[phi]).double()
    X, Z = images(5, 7)
    return {mode: HO.pool_ntk(model, *mode_args(X, Z, mode)) for mode in MODES}


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("phi", list(ACTS))
def test_pooled_network_against_the_oracle(phi, dtn):
    """forward and ntk_maps of the pooled model against the walk on position-pair maps; with
    a workspace of two pairs and a half the same bits (the tables are rebuilt per chunk)"""
    ref = pooled_reference(phi)
    dt = TORCH_DT[dtn]
    model = pooled_net(ACTS[phi]).to(DEV, dt)
    X, Z = (dev(a, dt) for a in images(5, 7))
    plan = model._plan(5, 7)
    item = X.element_size()
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            rk, rth = ref[mode]
            fwd = model(*args)
            assert tuple(fwd.shape) == rk.shape and fwd.dtype == X.dtype
            errs["K_" + mode] = max_err(fwd.cpu(), rk)
            km, tm = model.ntk_maps(*args, return_nngp=True)
            assert torch.equal(km, fwd), mode
            errs["T_" + mode] = max_err(tm.cpu(), rth)
        args = mode_args(X, Z, "xz")
        steps = plan.pool_ntk(False, True, item)
        model.set_pool_workspace(2 * steps.peak * item + steps.peak * item // 2)
        try:
            km2, tm2 = model.ntk_maps(*args, return_nngp=True)
        finally:
            model.set_pool_workspace(None)
        km, tm = model.ntk_maps(*args, return_nngp=True)
        assert torch.equal(km2, km) and torch.equal(tm2, tm)
    check(f"hermite pooled network {phi} {dtn}", errs, NET_TOL[dtn], CAP[dtn])


def test_readme_model_runs_on_every_path():
    make = lambda: [C(3, var_bias=0.1), m.Tanh(), A(2), C(3), m.SiLU(), G(),     # noqa: E731
                    C(1, var_weight=2.0)]
    model, body = S(*make()).to(DEV, torch.float64), S(*make()[:5]).to(DEV, torch.float64)
    Xh, Zh = images(5, 7)
    X, Z = dev(Xh), dev(Zh)
    with torch.no_grad():
        k = model(X, Z, False)
        km, tm = model.ntk_maps(X, Z, False, return_nngp=True)
        s = body.position_covariance(X, Z, False)
        sk, st = body.position_ntk(X, Z, False, return_nngp=True)
    rk, rth = HO.pool_ntk(S(*make()).double(), Xh, Zh, False, False)
    assert torch.equal(km, k) and torch.equal(sk, s) and st.shape == s.shape
    check("README model", dict(K=max_err(k.cpu(), rk), T=max_err(tm.cpu(), rth)),
          NET_TOL["f64"], CAP["f64"])


# ------------------------------------------------------------------------------------
# e. against the closed forms on the device
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("phi", ["erf", "gelu"])
def test_series_matches_the_closed_form_kernels(phi, dtn):
    """HermiteNonlin("erf") against Erf() and HermiteNonlin("gelu") against Gelu(), K and Θ on
    every mode, on images scaled so that every pre-activation variance is at most 0.25 (asserted
    from the oracle's variance maps): there the series carries no truncation error above
    rounding, so the two kernels agree to the networks' tolerance"""
    closed = {"erf": m.Erf, "gelu": m.Gelu}[phi]
    X, Z = images(5, 5, scale=0.25)
    for imgs in (X, Z):
        for v in HO.nonlin_input_variances(layer_net(closed).double(), imgs):
            assert 0.0 <= v.min() and v.max() <= 0.25
    dt = TORCH_DT[dtn]
    series, exact = layer_net(ACTS[phi]).to(DEV, dt), layer_net(closed).to(DEV, dt)
    Xd, Zd = dev(X, dt), dev(Z, dt)
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(Xd, Zd, mode)
            (k, th), (ck, cth) = (net.ntk(*args, return_nngp=True) for net in (series, exact))
            errs["K_" + mode] = max_err(k.cpu(), ck.cpu())
            errs["T_" + mode] = max_err(th.cpu(), cth.cpu())
    check(f"hermite {phi} vs closed form {dtn}", errs, NET_TOL[dtn], CAP[dtn])


# ------------------------------------------------------------------------------------
# f. behaviour
# ------------------------------------------------------------------------------------
def test_assigning_an_attribute_changes_the_next_call():
    """order, quad_nodes and phi are plain attributes: assigning one goes through
    NNGPKernel.__setattr__, the plan cache's key follows, and the next call gives a freshly
    built model's bits"""
    build = lambda **kw: S(C(3, var_bias=0.1), H(**kw), C(5, padding=0)).to(     # noqa: E731
        DEV, torch.float64)
    model = build(phi="tanh")
    X, Z = (dev(a) for a in images(5, 5))
    with torch.no_grad():
        k1 = model(X, Z, False)
        model.mods[1].order = 8
        k2 = model(X, Z, False)
        assert torch.equal(k2, build(phi="tanh", order=8)(X, Z, False))
        assert not torch.equal(k2, k1)
        model.mods[1].quad_nodes = 128
        k3, t3 = model.ntk(X, Z, False, return_nngp=True)
        kf, tf = build(phi="tanh", order=8, quad_nodes=128).ntk(X, Z, False, return_nngp=True)
        assert torch.equal(k3, kf) and torch.equal(t3, tf)
        model.mods[1].phi = "silu"
        assert torch.equal(model(X, Z, False),
                           build(phi="silu", order=8, quad_nodes=128)(X, Z, False))
        model.mods[1].phi, model.mods[1].order, model.mods[1].quad_nodes = "tanh", 32, 96
        assert torch.equal(model(X, Z, False), k1)


def test_hermite_model_launches():
    """per op one variance launch, and on the pair maps the coefficient launches and the walk;
    the whole-network kernel and image_variances decline"""
    model = S(C(3), m.Tanh(), C(3), m.SiLU(), C(5, padding=0)).to(DEV, torch.float64)
    X, Z = (dev(a) for a in images(5, 5))
    assert model.image_variances(X) is None
    seen = record(lambda: model(X, Z, False))
    assert seen.count("cgp_hermite") == 2 and seen.count("cgp_var_hermite_f64") == 2
    assert seen.count("cgp_hermite_coef") == 4              # the tables of xx and of yy
    assert not any("relu" in s or "net" in s for s in seen)
    seen = record(lambda: model(X))
    assert seen.count("cgp_hermite") == 2 and seen.count("cgp_hermite_coef") == 2
    seen = record(lambda: model.ntk(X, Z, False))
    assert seen.count("cgp_hermite") == 2 and seen.count("cgp_hermite_coef") == 4
    seen = record(lambda: model.ntk_maps(X, Z, False))
    assert seen.count("cgp_hermite_cov") == 2
    assert "cgp_covntk_nonlin" not in seen and "cgp_cov_nonlin" not in seen


def test_node_table_is_cached_and_resident():
    """one device table per (device, quad_nodes), the host's nodes and weights bit for bit"""
    from cnn_gp.program import hermite_rule
    for nq in (40, 96):
        tab = nodes(nq)
        assert nodes(nq) is tab and tuple(tab.shape) == (2, nq) and tab.dtype == torch.float64
        assert_bits(tab.cpu().numpy(), np.stack(hermite_rule(nq)))
        assert_bits(tab.cpu().numpy(), np.stack(HO.tables(1, nq)[:2]))
