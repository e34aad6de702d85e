"""GPU tests of the GELU nonlinearity: cgp_gelu_* / cgp_var_gelu_* / cgp_gelu_cov_* alone,
networks with cnn_gp.Gelu through forward and ntk against the test-time oracle
(tests/gelu_oracle.py), the pooled path, the Gram builds on a GELU model, and that a
ReLU-only model makes no GELU launch.

Tolerances are the project's own (tests/test_gpu_erf.py): the op alone in float64 1e-12,
float64 end to end 1e-10, float32 against the float64 oracle on float32-representable inputs
2e-5.  Inputs in [0, 1) use the relative error; signed inputs and single ops use
max|got - ref| / max|ref|, because GELU kernels cross zero."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp import program as P
from cnn_gp.kernel_save_tools import save_K

import gelu_oracle as GO
from test_gpu_erf import OP_CASES, MODES, PARENT_CALLS, MemH5, mode_args, recorded_calls

pytestmark = pytest.mark.gpu

DEV = "cuda"
OP_TOL = {"f64": 1e-12, "f32": 2e-5}
NET_TOL = {"f64": 1e-10, "f32": 2e-5}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}

m = cnn_gp
S, C, R, E, GE, G, A, CC = (m.Sequential, m.Conv2d, m.ReLU, m.Erf, m.Gelu, m.GlobalAvgPool,
                            m.AvgPool2d, m.CorrelatedConv2d)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def max_err(got, ref):
    """max|got - ref| / max|ref| over the entries where ref is not NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    keep = ~np.isnan(ref)
    assert keep.any() and np.all(np.isfinite(got[keep]))
    return float(np.max(np.abs(got[keep] - ref[keep])) / np.max(np.abs(ref[keep])))


# ------------------------------------------------------------------------------------
# a. the layer-path op alone
# ------------------------------------------------------------------------------------
def patches(n1, n2, hw, same, diag, seed, np_dt, zero_frac=0.1):
    """Random valid patches: v in [0, 3] with ``zero_frac`` exact zeros (on both sides), rho
    in [-1, 1] with about one pair in ten at exactly -1 or +1, signed c.  With same, yy = xx
    and the overridden pairs hold c = v; Θ and the addend are standard normal.  Arrays already
    rounded to np_dt."""
    rng = np.random.default_rng(seed)

    def variances(n):
        v = 3.0 * (1.0 - rng.random((n, hw)))
        v[rng.random((n, hw)) < zero_frac] = 0.0
        return v
    xx = variances(n1)
    yy = xx if same else variances(n2)
    shape = (n1, hw) if diag else (n1, n2, hw)
    rho = rng.uniform(-1.0, 1.0, shape)
    ends = rng.random(shape) < 0.1
    rho[ends] = np.sign(rho[ends])
    xy = rho * np.sqrt(xx * yy if diag else xx[:, None] * yy[None])
    if same and not diag:
        idx = np.arange(n1)
        xy[idx, idx] = xx
    if same and diag:
        xy = xx.copy()
    theta = rng.standard_normal(xy.shape)
    addend = rng.standard_normal(xy.shape)
    return tuple(np.ascontiguousarray(v.reshape(-1, hw).astype(np_dt))
                 for v in (xy, theta, xx, yy, addend))


def run_gelu(xy, theta, xx, yy, n1, n2, same, diag, dtn, addend=None, inplace=False,
             alias=False):
    """cgp_gelu_*: theta None is the forward-only form; ``alias`` passes xy itself as theta;
    ``inplace`` writes over the inputs.  Returns (K', Θ' or None) as numpy arrays."""
    dt = TORCH_DT[dtn]
    c, vx, vy = dev(xy, dt), dev(xx, dt), dev(yy, dt)
    th = c if alias else (None if theta is None else dev(theta, dt))
    ad = None if addend is None else dev(addend, dt)
    oc = c if inplace else torch.empty_like(c)
    oth = None if th is None else (th if inplace and not alias else torch.empty_like(c))
    a = N.GeluArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(c), N.ptr(th), N.ptr(oc), N.ptr(oth)
    a.addend, a.xx, a.yy = N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2 = xy.shape[0], n1, n2
    a.hw, a.same, a.diag = xy.shape[1], int(same), int(diag)
    N.check(getattr(N.load(), f"cgp_gelu_{dtn}")(ctypes.byref(a), stream()), "cgp_gelu")
    torch.cuda.synchronize()
    return oc.cpu().numpy(), None if oth is None else oth.cpu().numpy()


def run_var_gelu(xx, yy, same, dtn):
    dt = TORCH_DT[dtn]
    vx, vy = dev(xx, dt), dev(yy, dt)
    ox, oy = torch.empty_like(vx), torch.empty_like(vy)
    N.call(f"cgp_var_gelu_{dtn}", N.ptr(vx), N.ptr(vy), xx.shape[0], yy.shape[0], xx.shape[1],
           int(same), N.ptr(ox), N.ptr(oy), stream())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oy.cpu().numpy()


def op_ref(xy, theta, xx, yy, same, diag):
    """float64 oracle (K', Θ', xx', yy') of one GELU step on [n][hw] arrays"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))[:, None, None, :]  # noqa
    c, th, vx, vy = t(xy), t(theta), t(xx), t(yy)
    _, _, k, vx2, vy2 = GO._gelu((bool(same), bool(diag), c, vx, vy))
    kd = GO.gelu_kdot(c, vx, vy, bool(same), bool(diag))
    flat = lambda a: a.reshape(-1, xy.shape[1]).numpy()                         # noqa: E731
    return flat(k), flat(th * kd), flat(vx2), flat(vy2)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gelu_op(case, dtn):
    """K', Θ' and the variance maps against the float64 oracle, and every calling form
    bit-equal to the plain one.  The shapes are test_gpu_erf.py's: a partial chunk of maps in
    the last workgroup, the i = j overrides, both diag forms, a 1x1 map, and 784 pixels with an
    odd map in the last chunk.

    float32 (inputs are float32-representable, so only the arithmetic errs): Δ² = P1 - c² >=
    1 + v1 + v2 is summed from terms of magnitude at most P1 + c² <= 2·P1, and
    P1/(1 + v1 + v2) <= 16/7 at v <= 3, so Δ² carries at most 2·(16/7)·3 roundings of 6e-8 =
    8e-7 relative, and nothing downstream amplifies it (atan and the quotients are
    well-conditioned: no singularity at rho = ±1).  The formulas evaluated in float32 over
    this range err by 1.7e-7 (K') and 6.8e-8 (κ̇) absolute, two orders inside the project's
    float32 bound 2e-5, which is asserted; measured values are printed."""
    n1, n2, hw, same, diag = case
    xy, theta, xx, yy, addend = patches(n1, n2, hw, same, diag, 300 + hw + n1, NP_DT[dtn])
    rk, rth, rvx, rvy = op_ref(xy, theta, xx, yy, same, diag)
    tol = OP_TOL[dtn]

    k0, none = run_gelu(xy, None, xx, yy, n1, n2, same, diag, dtn)
    assert none is None
    k, th = run_gelu(xy, theta, xx, yy, n1, n2, same, diag, dtn)
    np.testing.assert_array_equal(k, k0)                    # one device function for K'
    vx, vy = run_var_gelu(xx, yy, same, dtn)
    errs = dict(K=max_err(k, rk), T=max_err(th, rth), xx=max_err(vx, rvx), yy=max_err(vy, rvy))
    print(f"gelu op {dtn} {case}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) < tol, errs
    assert np.all(np.isfinite(k)) and np.all(np.isfinite(th))
    if hw > 1 and not (same and diag):
        assert k.min() < 0 < k.max()                        # K' takes both signs
    if same:
        np.testing.assert_array_equal(vy, vx)
        sel = np.arange(n1) if diag else np.arange(n1) * (n2 + 1)
        np.testing.assert_array_equal(k[sel], vx)           # K' = v'[i], the same bits
        want = theta[sel].astype(np.float64) * GO.gelu_var_kdot(xx.astype(np.float64))
        assert max_err(th[sel], want) < tol
        # zero-variance pixels of an overridden pair: c = v = 0 gives 0 and Θ/4 = Θ·Φ(0)²
        z = xx == 0
        assert z.any()
        np.testing.assert_array_equal(k[sel][z], 0)
        np.testing.assert_array_equal(th[sel][z], theta[sel][z] / 4)

    # in place; theta aliasing xy; the addend (a separate rounding, on K' only)
    ki, thi = run_gelu(xy, theta, xx, yy, n1, n2, same, diag, dtn, inplace=True)
    np.testing.assert_array_equal(ki, k)
    np.testing.assert_array_equal(thi, th)
    ki, _ = run_gelu(xy, None, xx, yy, n1, n2, same, diag, dtn, inplace=True)
    np.testing.assert_array_equal(ki, k)
    ka, tha = run_gelu(xy, None, xx, yy, n1, n2, same, diag, dtn, alias=True)
    kx, thx = run_gelu(xy, xy, xx, yy, n1, n2, same, diag, dtn)
    np.testing.assert_array_equal(ka, k)
    np.testing.assert_array_equal(kx, k)
    np.testing.assert_array_equal(tha, thx)
    kai, thai = run_gelu(xy, None, xx, yy, n1, n2, same, diag, dtn, alias=True, inplace=True)
    np.testing.assert_array_equal(kai, k)
    np.testing.assert_array_equal(thai, thx)
    kd, thd = run_gelu(xy, theta, xx, yy, n1, n2, same, diag, dtn, addend=addend)
    np.testing.assert_array_equal(kd, k + addend)
    np.testing.assert_array_equal(thd, th)
    kd0, _ = run_gelu(xy, None, xx, yy, n1, n2, same, diag, dtn, addend=addend)
    np.testing.assert_array_equal(kd0, kd)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_gelu_op_all_zero(dtn):
    """v = c = 0 everywhere, no override in play: K' = 0 exactly and Θ' = Θ/4"""
    n1, n2, hw = 3, 2, 10
    zeros = lambda n: np.zeros((n, hw), dtype=NP_DT[dtn])                       # noqa: E731
    theta = np.random.default_rng(1).standard_normal((n1 * n2, hw)).astype(NP_DT[dtn])
    k, th = run_gelu(zeros(n1 * n2), theta, zeros(n1), zeros(n2), n1, n2, 0, 0, dtn)
    np.testing.assert_array_equal(k, 0)
    np.testing.assert_array_equal(th, theta / 4)
    vx, vy = run_var_gelu(zeros(n1), zeros(n2), 0, dtn)
    np.testing.assert_array_equal(vx, 0)
    np.testing.assert_array_equal(vy, 0)


# ------------------------------------------------------------------------------------
# b. the position-pair op alone
# ------------------------------------------------------------------------------------
def run_gelu_cov(s, xx, yy, pi, pj, dtn, addend=None, same=False, inplace=False):
    """cgp_gelu_cov_* on [m, p_row, p_col, q_row, q_col] arrays (the oracle's layout)"""
    dt = TORCH_DT[dtn]
    h, w = s.shape[1:3]
    idx32 = lambda a: torch.as_tensor(np.asarray(a)).to(DEV, torch.int32)       # noqa: E731
    sd, di, dj = dev(GO.CO.to_device_layout(s), dt), idx32(pi), idx32(pj)
    ad = None if addend is None else dev(GO.CO.to_device_layout(addend), dt)
    vx, vy = dev(xx, dt), dev(yy, dt)
    out = sd if inplace else torch.empty_like(sd)
    a = N.GeluCovArgs()
    a.in_, a.out, a.addend, a.xx, a.yy = N.ptr(sd), N.ptr(out), N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.pair_i, a.pair_j, a.npairs = N.ptr(di), N.ptr(dj), len(pi)
    a.h, a.w, a.same = h, w, int(same)
    N.check(getattr(N.load(), f"cgp_gelu_cov_{dtn}")(ctypes.byref(a), stream()), "cgp_gelu_cov")
    torch.cuda.synchronize()
    return GO.CO.from_device_layout(out.cpu().numpy(), h, w)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("same", [True, False], ids=["same", "xz"])
@pytest.mark.parametrize("side", [7, 1])
def test_gelu_cov_op(side, same, dtn):
    """6 pairs of 4 images, two of them self pairs; at 7x7 a pair holds 2401 elements: two
    chunks with the second partial, and chunks that straddle pairs.  Signed images, so S takes
    both signs; some images have zero pixels (zero variance)."""
    rng = np.random.default_rng(40 + side)
    x = rng.standard_normal((4, 3, side, side)).astype(np.float32).astype(np.float64)
    x[rng.random(x.shape) < 0.15] = 0.0
    if side > 1:
        x[:, :, 0, 0] = 0.0                                # a zero-variance pixel per image
    y = x if same else rng.standard_normal(x.shape).astype(np.float32).astype(np.float64)
    pi, pj = np.array([0, 1, 1, 3, 2, 0]), np.array([1, 1, 2, 3, 0, 3])
    rnd = lambda a: a.astype(NP_DT[dtn]).astype(np.float64)                      # noqa: E731
    s0 = rnd(GO.CO.moments(x, y, pi, pj))
    vx, vy = rnd((x * x).mean(1)), rnd((y * y).mean(1))
    addend = rnd(rng.standard_normal(s0.shape))
    ref = GO.gelu_map(s0, vx, vy, pi, pj, same)
    got = run_gelu_cov(s0, vx, vy, pi, pj, dtn, same=same)
    err = max_err(got, ref)
    print(f"gelu_cov {dtn} {side}x{side} same={same}: {err:.2e}")
    assert err < OP_TOL[dtn]
    np.testing.assert_array_equal(run_gelu_cov(s0, vx, vy, pi, pj, dtn, same=same, inplace=True),
                                  got)
    gadd = run_gelu_cov(s0, vx, vy, pi, pj, dtn, same=same, addend=addend)
    np.testing.assert_array_equal(gadd, (got.astype(NP_DT[dtn])
                                         + addend.astype(NP_DT[dtn])).astype(np.float64))
    gin = run_gelu_cov(s0, vx, vy, pi, pj, dtn, same=same, addend=addend, inplace=True)
    np.testing.assert_array_equal(gin, gadd)
    # the p = q entries of the self pairs: with same the variance entry point's bits (the
    # override), without it the ordinary map of (c, v1, v2) = (S[p, p], xx[p], yy[p])
    self_pq = np.einsum("mabab->mab", got)[pi == pj]
    var = run_var_gelu(vx.reshape(4, -1), vy.reshape(4, -1), same, dtn)[0].reshape(vx.shape)
    if same:
        np.testing.assert_array_equal(self_pq, var[pi[pi == pj]])
        assert side == 1 or np.all(self_pq[:, 0, 0] == 0)
    elif side > 1:
        assert not np.array_equal(self_pq, var[pi[pi == pj]])


# ------------------------------------------------------------------------------------
# c. networks
# ------------------------------------------------------------------------------------
def nets(side):
    """name -> (fresh float32-built model, pure): ``pure`` networks hold no ReLU, so the
    autograd Θ is valid on every pair"""

    def convnet(b):
        return S(C(3, var_bias=2 * b), GE(), C(3, var_weight=1.5, var_bias=b), GE(), C(3), GE(),
                 C(side, padding=0, var_bias=b))

    return {
        "convnet_bias": (convnet(0.1), True),
        "convnet_nobias": (convnet(0.0), True),
        "residual": (S(C(3, var_bias=0.1), m.Sum([S(), S(GE(), C(3), GE(), C(3))]), GE(),
                       C(side, padding=0)), True),
        "mixed": (S(C(3, var_bias=0.1), R(), C(3), GE(), C(3, var_weight=2.0), E(), C(3),
                    GE(), C(side, padding=0)), False),
    }


NET_NAMES = list(nets(8))
SIZES = [(8, 1), (7, 3)]


def images(side, channels, signed=False):
    rng = np.random.default_rng(20 * side + channels)
    draw = (lambda n: rng.standard_normal((n, channels, side, side)).astype(np.float32)) \
        if signed else (lambda n: rng.random((n, channels, side, side), dtype=np.float32))
    X, Z = draw(5).astype(np.float64), draw(3).astype(np.float64)
    if signed:
        # two images are the negation of another: c = -v there, where GELU's K' is negative
        X[1], X[3] = -X[0], -X[2]
    return X, Z


@functools.lru_cache(maxsize=None)
def reference(name, side, channels, signed=False):
    """mode -> (K, Θ) from the float64 oracle, computed once per network and size.  K from
    the walk; Θ by autograd where it is valid on every entry (no ReLU), stepwise otherwise."""
    model, pure = nets(side)[name]
    model = model.double()
    X, Z = images(side, channels, signed)
    out = {}
    for mode in MODES:
        args = mode_args(X, Z, mode)
        k = GO.kernel(model, *args)
        if pure:
            th = GO.ntk_autograd(model, args[0], None if mode == "xx" else args[1],
                                 diag=mode.endswith("diag"))[1]
            assert not np.isnan(th).any()
        else:
            sk, th = GO.ntk_stepwise(model, *args)
            assert max_err(sk, k) < 1e-13
        out[mode] = (k, th)
    return out


def check_network(name, side, channels, dtn, signed=False):
    ref = reference(name, side, channels, signed)
    model = nets(side)[name][0].to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(side, channels, signed))
    err = max_err if signed else rel_err
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            rk, rth = ref[mode]
            fwd = model(*args)
            k, th = model.ntk(*args, return_nngp=True)
            assert tuple(fwd.shape) == rk.shape
            errs["K_" + mode] = err(fwd.cpu(), rk)
            errs["T_" + mode] = err(th.cpu(), rth)
            # one device function per stream: K of the NTK run is forward's K
            assert max_err(k.cpu(), fwd.cpu().numpy()) < 1e-12, mode
            if mode == "xx":
                kxx, txx = fwd.cpu().numpy(), th.cpu().numpy()
            if mode == "same_diag":
                assert max_err(fwd.cpu(), np.diag(kxx)) < 1e-12
                assert max_err(th.cpu(), np.diag(txx)) < 1e-12
    assert np.max(np.abs(txx - txx.T)) <= 1e-13 * np.max(np.abs(txx))
    assert np.max(np.abs(kxx - kxx.T)) <= 1e-13 * np.max(np.abs(kxx))
    print(f"gelu net {name} {side}x{side}x{channels} {dtn}{' signed' if signed else ''}: "
          + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs
    return kxx


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NET_NAMES)
def test_gelu_network(name, size, dtn):
    check_network(name, size[0], size[1], dtn)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_gelu_network_signed_inputs(dtn):
    """standard normal images, two of them the negation of another: the GELU kernel goes
    negative between those (K' = v' - v/2 at c = -v), which no ReLU network's does.  The
    residual net: its skip carries the sign to the readout, where a plain chain of GELU
    layers has averaged it away (K'(c = 0) = v1 v2/(2π √((1 + v1)(1 + v2))) > 0)."""
    kxx = check_network("residual", 7, 3, dtn, signed=True)
    assert kxx.min() < 0 < kxx.max()


def test_gelu_ignores_exact_relu_and_fusion():
    model = nets(8)["residual"][0].to(DEV, torch.float64)
    X = dev(images(8, 1)[0])
    with torch.no_grad():
        k = model(X)
        assert torch.equal(model.set_exact_relu(True)(X), k)
        model.set_exact_relu(False)
        assert torch.equal(model.set_fusion(False)(X), k)      # fusion changes no arithmetic
        assert torch.equal(model.set_fused_network(False)(X), k)


def test_ntk_without_a_conv_returns_forwards_K():
    """a model without a Conv2d has Θ = 0 and its ntk K is forward's, bit for bit"""
    model = S(GE())
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((24, 2, 1, 1))).to(DEV)
    z = torch.from_numpy(np.random.default_rng(12).standard_normal((24, 2, 1, 1))).to(DEV)
    with torch.no_grad():
        for args in ((x,), (x, z, False, False), (x, x, True, True)):
            k, th = model.ntk(*args, return_nngp=True)
            assert torch.equal(k, model(*args))
            assert torch.equal(th, torch.zeros_like(k))


# ------------------------------------------------------------------------------------
# d. the pooled path
# ------------------------------------------------------------------------------------
def pooled_nets():
    """a gelu before and after an AvgPool2d(2), on 8x8 images (4x4 after the pool)"""
    body = lambda: [C(3, var_bias=0.1), GE(), A(2), C(3, var_weight=1.5, var_bias=0.1),   # noqa
                    GE()]
    return {"global_pool": S(*body(), G(), C(1, var_weight=2.0, var_bias=0.3)),
            "corr_readout": S(*body(), CC(4, padding=0, lengthscale=1.5, var_bias=0.2))}


def pool_images(side=8):
    rng = np.random.default_rng(77 + side)
    draw = lambda n: rng.random((n, 2, side, side), dtype=np.float32).astype(np.float64)   # noqa
    return draw(5), draw(3)


@functools.lru_cache(maxsize=None)
def pooled_reference(name):
    X, Z = pool_images()
    model = pooled_nets()[name].double()
    return {mode: GO.pooled_kernel(model, *mode_args(X, Z, mode)) for mode in MODES}


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", list(pooled_nets()))
def test_pooled_network_with_gelu(name, dtn):
    ref = pooled_reference(name)
    model = pooled_nets()[name].to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in pool_images())
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            k = model(*mode_args(X, Z, mode))
            assert tuple(k.shape) == ref[mode].shape and k.dtype == X.dtype
            errs[mode] = max_err(k.cpu(), ref[mode])
            if mode == "xx":
                kxx = k
            if mode == "same_diag":
                assert max_err(k.cpu(), torch.diagonal(kxx).cpu().numpy()) < 1e-12
    print(f"gelu pooled net {name} {dtn}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs


def test_position_covariance_ties_to_the_layer_path():
    """position_covariance of a Conv2d, Gelu body against the oracle; its [i, j, p, p] entries
    through a dense readout against the layer-path forward of body + Conv2d(H, padding=0);
    and, on a same tile, its i = j, p = q entries against run_variances' map bit for bit.
    6x6 images: no conv here has a compile-time instantiation in cgp_conv_*, whose generic
    kernel sums in the order the position-pair conv follows (tests/test_gpu_pool.py)."""
    X, Z = pool_images(6)
    body = S(C(3, var_bias=0.1), GE()).to(DEV, torch.float64)
    Xd, Zd = dev(X), dev(Z)
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(Xd, Zd, mode)
            s = body.position_covariance(*args)
            ref = GO.position_covariance(body, *mode_args(X, Z, mode))
            assert tuple(s.shape) == ref.shape
            assert max_err(s.cpu(), ref) < NET_TOL["f64"], mode
            dense = C(6, padding=0, var_weight=1.7, var_bias=0.2).to(DEV, torch.float64)
            g = P.conv_geometry(dense)
            want = g.weight * torch.einsum("...abab->...", s) + g.bias
            k = S(body, dense)(*args)
            assert max_err(k.cpu(), want.cpu().numpy()) < NET_TOL["f64"], mode
            if mode == "xx":
                assert torch.equal(s, s.permute(1, 0, 4, 5, 2, 3))     # S_ji[q, p] = S_ij[p, q]
                sxx = s
        n, c, h, w = Xd.shape
        plan = body._plan(h, w)
        var0 = torch.empty((2 * n, h, w), dtype=Xd.dtype, device=DEV)
        N.call("cgp_moments_var_f64", N.ptr(Xd), N.ptr(Xd), n, n, c, h * w, N.ptr(var0[:n]),
               N.ptr(var0[n:]), stream())
        var = plan.run_variances(var0[:n], var0[n:], n, n, True, stream(), need={plan.vf})
        assert torch.equal(torch.einsum("iiabab->iab", sxx), var[plan.vf][0])


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_self_pass_diagonal_is_the_variance_pipeline(dtn):
    """upstream of the pool both routes to the variances exist: the diagonals the self pass
    extracts of the first gelu's output and of the conv after it equal run_variances' maps bit
    for bit (6x6 images, as above)"""
    dt = TORCH_DT[dtn]
    body = S(C(3, var_bias=0.1), GE(), C(3, var_weight=1.5), A(2), GE()).to(DEV, dt)
    X = dev(pool_images(6)[0], dt)
    n, c, h, w = X.shape
    plan = body._plan(h, w)
    ps = plan.pool
    gelu1, conv2, pool = (plan.prog.ops[k].dst for k in (1, 2, 3))
    assert ps.self_var == {pool} and not {gelu1, conv2} & ps.avgpooled
    var0 = torch.empty((2 * n, h, w), dtype=dt, device=DEV)
    N.call(f"cgp_moments_var_{dtn}", N.ptr(X), N.ptr(X), n, n, c, h * w, N.ptr(var0[:n]),
           N.ptr(var0[n:]), stream())
    up = set(ps.need_var - ps.self_var)
    var = plan.run_variances(var0[:n], var0[n:], n, n, True, stream(), need=up | {gelu1, conv2})
    assert set(var) == up | {gelu1, conv2}                          # nothing past the pool
    side = {v: pair[0] for v, pair in var.items() if v in up}
    got = plan.run_self_variances(X, side, stream(), ps, None, want={gelu1, conv2})
    torch.cuda.synchronize()
    assert set(got) == {gelu1, conv2}
    assert torch.equal(got[gelu1], var[gelu1][0]) and torch.equal(got[conv2], var[conv2][0])
    # and the pass the model itself makes: the pooled value's variances against the oracle's
    own = plan.run_self_variances(X, side, stream(), ps, 4 * ps.peak * X.element_size())
    sxx = GO.position_covariance(S(*list(body.mods)[:4]), X.cpu().numpy())
    want = np.stack([GO.CO.diag(sxx[i, i][None])[0] for i in range(n)])
    assert max_err(own[pool].cpu(), want) < NET_TOL[dtn]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_chunking_changes_no_bit(dtn):
    """a workspace that holds one pair per chunk, the self pass included"""
    dt = TORCH_DT[dtn]
    model = pooled_nets()["global_pool"].to(DEV, dt)
    X, Z = (dev(a, dt) for a in pool_images())
    with torch.no_grad():
        whole = model(X, Z, False), model(X)
        seen = []
        real = N.check

        def check(rc, what):
            seen.append(what)
            return real(rc, what)
        N.check = check
        try:
            per_pair = model._plan(8, 8).pool.peak * X.element_size()
            model.set_pool_workspace(per_pair + per_pair // 2)
            parts = model(X, Z, False), model(X)
        finally:
            N.check = real
        # two gelu launches per chunk of the pairs, one per chunk of a self pass (which stops
        # at the conv after the pool): self passes over x and z, 15 pairs, x again, 15 pairs
        assert seen.count("cgp_gelu_cov") == (5 + 3) + 2 * 15 + 5 + 2 * 15
        assert seen.count("cgp_covmap_diag") == 5 + 3 + 5
        assert seen.count("cgp_cov_nonlin") == 0
        for got, want in zip(parts, whole):
            assert torch.equal(got, want)
        model.set_pool_workspace(None)
        assert torch.equal(model(X, Z, False), whole[0])


# ------------------------------------------------------------------------------------
# e. Gram builds
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gram_case():
    model = S(C(3), GE(), m.Sum([C(1, stride=2), S(C(3, stride=2), GE(), C(3))]), GE(),
              C(4, padding=0)).to(DEV, torch.float64)
    X = torch.from_numpy(np.random.default_rng(4).random((10, 2, 8, 8), dtype=np.float32)
                         .astype(np.float64))
    with torch.no_grad():
        k, th = model.ntk(X.to(DEV), return_nngp=True)
        tiles = [[model(X[a:a + 4].to(DEV), X[b:b + 4].to(DEV), a == b).cpu().numpy()
                  for b in range(0, 10, 4)] for a in range(0, 10, 4)]
    return model, X, k.cpu().numpy(), th.cpu().numpy(), np.block(tiles)


def test_gelu_gram_matrix(gram_case):
    model, X, k, th, tiled = gram_case
    assert model.image_variances(X.to(DEV)) is None          # declines: the per-tile fallback
    iu = np.triu_indices(10)
    np.testing.assert_array_equal(tiled[iu], k[iu])          # per-tile forward is the whole K
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], tiled[iu])
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4, ntk=True)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], th[iu])


def test_gelu_save_K(gram_case):
    from torch.utils.data import TensorDataset
    model, X, k, th, tiled = gram_case
    ds = TensorDataset(X, torch.zeros(len(X), dtype=torch.int64))
    f = MemH5()
    nngp = gram.model_kern(model)
    save_K(f, lambda x, x2, same, diag: nngp(x, x2, same).cpu().numpy(), "K", ds, None, False,
           4, print_interval=1e9)
    save_K(f, gram.ntk_kern(model), "T", ds, None, False, 4, print_interval=1e9)
    for key, ref in (("K", tiled), ("T", th)):
        keep = ~np.isnan(f.d[key][0])
        assert keep[np.triu_indices(10)].all()
        np.testing.assert_array_equal(f.d[key][0][keep], ref.astype(np.float32)[keep])
    save_K(f, gram.ntk_kern(model), "Td", ds, None, True, 4, print_interval=1e9)
    np.testing.assert_array_equal(f.d["Td"][0], np.diag(th).astype(np.float32))


# ------------------------------------------------------------------------------------
# f. a model without a Gelu is untouched
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["net", "layer"])
def test_relu_only_model_makes_no_gelu_call(path, monkeypatch):
    import configs_util
    model = configs_util.model("mnist_paper_convnet_gp").double().to(DEV)
    model.set_fused_network(path == "net")
    x = dev(np.random.default_rng(0).random((4, 1, 28, 28)))
    seen = recorded_calls(model, x, monkeypatch)
    assert seen == PARENT_CALLS["mnist_paper_convnet_gp", path]
    assert not any("gelu" in s for s in seen)


def test_pooled_relu_model_makes_no_gelu_call(monkeypatch):
    model = S(C(3), R(), A(2), C(3), R(), G()).to(DEV, torch.float64)
    X, Z = (dev(a) for a in pool_images(6))
    seen = []
    real = N.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)
    monkeypatch.setattr(N, "check", check)
    with torch.no_grad():
        model(X, Z, False)
    monkeypatch.setattr(N, "check", real)
    mo, co, av, no, po, di = ("cgp_cov_moments", "cgp_cov_conv", "cgp_covmap_avgpool",
                              "cgp_cov_nonlin", "cgp_cov_pool", "cgp_covmap_diag")
    assert [s for s in seen if s.startswith("cgp_cov")] == \
        [mo, co, av, co, di] * 2 + [mo, co, av, co, no, po]
    assert not any("gelu" in s for s in seen)
