"""GPU tests of the sinusoid family (cnn_gp.Sin / cnn_gp.Cos / cnn_gp.Rbf): cgp_sin_* /
cgp_var_sin_* / cgp_sin_cov_* alone, models through forward, ntk, position_covariance,
ntk_maps and position_ntk against the test-time oracle (tests/sin_oracle.py), the bit
identities (Cos against Sin at π/2, the override against the variance entry point, Rbf's
range), the plan cache following a parameter, and that a ReLU-only model makes no new launch.

Tolerances are the project's own (tests/test_gpu_erf.py, tests/test_gpu_gelu.py): the op alone
in float64 1e-12, float64 networks 1e-10, float32 against the float64 oracle on
float32-representable inputs 2e-5.  The metric is max|got − ref| / max|ref|, because these
kernels cross zero.  The float32 bound has room: the formulas evaluated in numpy float32 on
the patches of test_gpu_gelu.py err by at most 6.0e-7 at these parameter sets; the device's
own figures are printed by the tests."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N

import pool_oracle as PO
import sin_oracle as SO
from test_gpu_abrelu import COV_CASES, assert_bits, cov_launch, record
from test_gpu_erf import MODES, OP_CASES, PARENT_CALLS, recorded_calls
from test_gpu_gelu import patches

pytestmark = pytest.mark.gpu

DEV = "cuda"
OP_TOL = {"f64": 1e-12, "f32": 2e-5}
NET_TOL = {"f64": 1e-10, "f32": 2e-5}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}

m = cnn_gp
S, C, R, G, A, CC, SI, CO, RB = (m.Sequential, m.Conv2d, m.ReLU, m.GlobalAvgPool, m.AvgPool2d,
                                 m.CorrelatedConv2d, m.Sin, m.Cos, m.Rbf)

# name -> a module of the family
PARAMS = {"sin": lambda: SI(1, 1, 0), "sin-1.5-2-0.3": lambda: SI(1.5, 2, 0.3),
          "cos-1-2": lambda: CO(1, 2), "rbf-0.5": lambda: RB(0.5)}


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


# ------------------------------------------------------------------------------------
# a. the layer-path op alone
# ------------------------------------------------------------------------------------
def run_sin(k4, xy, theta, xx, yy, n1, n2, same, diag, dtn, addend=None, inplace=False,
            alias=False):
    """cgp_sin_*: theta None is the forward-only form; ``alias`` passes xy itself as theta;
    ``inplace`` writes over the inputs.  Returns (K', Θ' or None) as numpy arrays."""
    dt = TORCH_DT[dtn]
    c, vx, vy = dev(xy, dt), dev(xx, dt), dev(yy, dt)
    th = c if alias else (None if theta is None else dev(theta, dt))
    ad = None if addend is None else dev(addend, dt)
    oc = c if inplace else torch.empty_like(c)
    oth = None if th is None else (th if inplace and not alias else torch.empty_like(c))
    a = N.SinArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(c), N.ptr(th), N.ptr(oc), N.ptr(oth)
    a.addend, a.xx, a.yy = N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2 = xy.shape[0], n1, n2
    a.hw, a.same, a.diag = xy.shape[1], int(same), int(diag)
    a.A, a.B, a.C, a.D = k4
    N.check(getattr(N.load(), f"cgp_sin_{dtn}")(ctypes.byref(a), stream()), "cgp_sin")
    torch.cuda.synchronize()
    return oc.cpu().numpy(), None if oth is None else oth.cpu().numpy()


def run_var_sin(k4, xx, yy, same, dtn):
    dt = TORCH_DT[dtn]
    vx, vy = dev(xx, dt), dev(yy, dt)
    ox, oy = torch.empty_like(vx), torch.empty_like(vy)
    N.call(f"cgp_var_sin_{dtn}", N.ptr(vx), N.ptr(vy), xx.shape[0], yy.shape[0], xx.shape[1],
           int(same), *k4, N.ptr(ox), N.ptr(oy), stream())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oy.cpu().numpy()


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_sin_op(case, dtn):
    """erf's op cases on gelu's patches (v in [0, 3] with 10% exact zeros, ρ in [−1, 1] with a
    tenth at ±1, the overridden pairs at c = v): K', Θ' and the variance maps against the
    float64 oracle; every calling form bit-equal to the plain one; the overridden K' with the
    bits of v'; Rbf in (0, 1]; Cos(1, 2) bit-equal to Sin(1, 2, π/2)."""
    n1, n2, hw, same, diag = case
    npdt = NP_DT[dtn]
    xy, theta, xx, yy, addend = patches(n1, n2, hw, same, diag, 400 + hw + n1, npdt)
    tol = OP_TOL[dtn]
    sel = np.arange(n1) if diag else np.arange(n1) * (n2 + 1)
    for name, make in PARAMS.items():
        mod = make()
        k4 = mod.constants()
        run = functools.partial(run_sin, k4, xy=xy, xx=xx, yy=yy, n1=n1, n2=n2, same=same,
                                diag=diag, dtn=dtn)
        ok, oth, ovx, ovy = SO.pair_op(xy, theta, xx, yy, same, diag, SO.consts_of(mod))
        k0, none = run(theta=None)
        assert none is None
        k, th = run(theta=theta)
        assert_bits(k, k0)                                   # one device function for K'
        vx, vy = run_var_sin(k4, xx, yy, same, dtn)
        errs = dict(K=max_err(k, ok), T=max_err(th, oth), xx=max_err(vx, ovx),
                    yy=max_err(vy, ovy))
        print(f"sin op {name} {dtn} {case}: "
              + " ".join(f"{n}={e:.2e}" for n, e in errs.items()) + f" (tol {tol:.1e})")
        assert max(errs.values()) < tol, errs
        A_, B_, C_, D_ = (npdt(c) for c in k4)
        if same:
            assert_bits(vy, vx)
            assert_bits(k[sel], vx)                          # K' = v'[i], the same bits
            zero = xx == 0
            assert zero.any()
            assert_bits(k[sel][zero], np.full(zero.sum(), A_ * (npdt(1) - C_)))
            assert_bits(th[sel][zero], theta[sel][zero] * (D_ * (npdt(1) + C_)))
        if name.startswith("rbf"):
            assert np.all(k > 0) and np.all(k <= 1)
            assert_bits(vx, np.ones_like(vx))
            if same:
                assert_bits(k[sel], np.ones_like(vx))
        if name == "cos-1-2":
            ks, ths = run_sin(SI(1, 2, math.pi / 2).constants(), xy, theta, xx, yy, n1, n2, same,
                              diag, dtn)
            assert_bits(k, ks)
            assert_bits(th, ths)

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


def test_rbf_bits_are_those_of_the_full_form():
    """The exponential skipped at C == 0 changes no bit: C = 5e-324 (float64's smallest
    denormal) takes the full path, and C·e_s <= 5e-324 is absorbed by e_d >= exp(−6) and by 1."""
    n1, n2, hw, same, diag = OP_CASES[1]
    xy, theta, xx, yy, _ = patches(n1, n2, hw, same, diag, 77, np.float64)
    k, th = run_sin((1.0, 0.5, 0.0, 1.0), xy, theta, xx, yy, n1, n2, same, diag, "f64")
    kf, thf = run_sin((1.0, 0.5, 5e-324, 1.0), xy, theta, xx, yy, n1, n2, same, diag, "f64")
    assert_bits(k, kf)
    assert_bits(th, thf)


# ------------------------------------------------------------------------------------
# b. the position-pair entry point alone
# ------------------------------------------------------------------------------------
def run_sin_cov(k4, *args, **kw):
    def fill(a):
        a.A, a.B, a.C, a.D = k4
    return cov_launch("cgp_sin_cov", N.SinCovArgs, *args, fill=fill, exact=False, **kw)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("same", [True, False], ids=["same", "xz"])
@pytest.mark.parametrize("case", list(COV_CASES))
def test_sin_cov_op(case, same, dtn):
    """7 pairs of 5x5 maps (2048-element chunks straddle pairs) and 3 pairs of 7x7 maps (a pair
    spans chunks, the last chunk partial), both with i = j pairs: v in [0, 3] with zeros,
    S[p, q] = ρ·√(v1[p]·v2[q]) with ρ in [−1, 1] and a tenth at ±1, and with ``same`` the
    overridden elements at c = v.  The forward and two-stream forms against the oracle, the K
    stream bit-equal between them, both addends, and a launch over all pairs bit-equal to
    launches over the pairs one at a time."""
    side, pi, pj = COV_CASES[case]
    pi, pj = np.array(pi), np.array(pj)
    rng = np.random.default_rng(60 + side)
    npdt = NP_DT[dtn]
    rnd = lambda v: v.astype(npdt).astype(np.float64)                            # noqa: E731

    def variances():
        v = 3.0 * (1.0 - rng.random((4, side, side)))
        v[rng.random(v.shape) < 0.1] = 0.0
        v[:, 0, 0] = 0.0                                     # a zero-variance pixel per image
        return rnd(v)
    vx = variances()
    vy = vx if same else variances()
    rho = rng.uniform(-1.0, 1.0, (len(pi),) + (side, side) * 2)
    ends = rng.random(rho.shape) < 0.1
    rho[ends] = np.sign(rho[ends])
    s0 = rho * np.sqrt(vx[pi][:, :, :, None, None] * vy[pj][:, None, None, :, :])
    if same:
        v1 = np.broadcast_to(vx[pi][:, :, :, None, None], s0.shape)
        s0 = np.where(PO._self_mask(s0, pi, pj), v1, s0)
    s0 = rnd(s0)
    theta, addend, addend_t = (rnd(rng.standard_normal(s0.shape)) for _ in range(3))
    args = (vx, vy, pi, pj, dtn)
    tol = OP_TOL[dtn]
    self_pairs = pi == pj
    assert self_pairs.any()
    for name, make in PARAMS.items():
        mod = make()
        k4 = mod.constants()
        ok, oth = SO.map_op(s0, theta, vx, vy, pi, pj, same, SO.consts_of(mod))
        k0, none = run_sin_cov(k4, s0, None, *args, same=same)
        assert none is None
        k, th = run_sin_cov(k4, s0, theta, *args, same=same)
        assert_bits(k, k0)
        errs = dict(K=max_err(k, ok), T=max_err(th, oth))
        print(f"sin_cov {name} {case} {dtn} same={same}: "
              + " ".join(f"{n}={e:.2e}" for n, e in errs.items()) + f" (tol {tol:.1e})")
        assert max(errs.values()) < tol, errs
        # the p = q entries of the self pairs: with same the variance entry point's bits
        var = run_var_sin(k4, vx.reshape(4, -1), vy.reshape(4, -1), same, dtn)[0]
        var = var.reshape(vx.shape)
        if same:
            assert_bits(np.einsum("mabab->mab", k)[self_pairs].astype(npdt),
                        var[pi[self_pairs]])
        if name.startswith("rbf"):
            assert np.all(k > 0) and np.all(k <= 1)

        # in place, and the addends (separate roundings)
        ki, thi = run_sin_cov(k4, s0, theta, *args, same=same, inplace=True)
        assert_bits(ki, k)
        assert_bits(thi, th)
        ka, tha = run_sin_cov(k4, s0, theta, *args, same=same, addend=addend,
                              addend_theta=addend_t)
        assert_bits(ka.astype(npdt), k.astype(npdt) + addend.astype(npdt))
        assert_bits(tha.astype(npdt), th.astype(npdt) + addend_t.astype(npdt))
        ka2, tha2 = run_sin_cov(k4, s0, theta, *args, same=same, addend_theta=addend_t)
        assert_bits(ka2, k)
        assert_bits(tha2, tha)
        assert_bits(run_sin_cov(k4, s0, None, *args, same=same, addend=addend)[0], ka)

    # one launch over all pairs against one launch per pair (the last parameter set)
    for p in range(len(pi)):
        k1, th1 = run_sin_cov(k4, s0[p:p + 1], theta[p:p + 1], vx, vy, pi[p:p + 1], pj[p:p + 1],
                              dtn, same=same)
        assert_bits(k1, k[p:p + 1])
        assert_bits(th1, th[p:p + 1])


# ------------------------------------------------------------------------------------
# c. networks on the layer path
# ------------------------------------------------------------------------------------
def nets(side):
    return {
        "chain": lambda: S(C(3, var_bias=0.1), SI(1.5, 2, 0.3), C(3, var_weight=1.5), CO(1, 2),
                           C(3), RB(0.5), C(side, padding=0, var_bias=0.1)),
        "residual": lambda: S(C(3, var_bias=0.1),
                              m.Sum([S(), S(SI(1, 1, 0), C(3), RB(0.5), C(3))]), CO(1, 2),
                              C(side, padding=0)),
        "mixed": lambda: S(C(3, var_bias=0.1), R(), C(3, var_weight=1.5), SI(1.5, 2, 0.3), C(3),
                           R(), C(3), RB(0.5), C(side, padding=0, var_bias=0.1)),
    }


def images(side, signed, n=(3, 2)):
    rng = np.random.default_rng(40 * side + signed)
    draw = (lambda k: rng.standard_normal((k, 3, side, side)).astype(np.float32)) if signed \
        else (lambda k: rng.random((k, 3, side, side), dtype=np.float32))
    return draw(n[0]).astype(np.float64), draw(n[1]).astype(np.float64)


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:len(Z)], Z, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def reference(name, side, signed):
    """mode -> (K, Θ) from the float64 oracle, once per network, size and image set: K from
    the walk, Θ launch by launch (valid with a ReLU as well), its K tied to the walk's"""
    model = nets(side)[name]().double()
    X, Z = images(side, signed)
    out = {}
    for mode in MODES:
        args = mode_args(X, Z, mode)
        k = SO.kernel(model, *args)
        sk, th = SO.ntk_stepwise(model, *args)
        assert max_err(sk, k) < 1e-13
        out[mode] = (k, th)
    return out


@pytest.mark.parametrize("signed", [False, True], ids=["unit", "signed"])
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("side", [7, 8])
@pytest.mark.parametrize("name", list(nets(7)))
def test_network_against_the_oracle(name, side, dtn, signed):
    ref = reference(name, side, signed)
    model = nets(side)[name]().to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(side, signed))
    tol = NET_TOL[dtn]
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
    print(f"sin network {name} {side}x{side} {dtn}{' signed' if signed else ''} "
          f"(tol {tol:.1e}): " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, errs


# ------------------------------------------------------------------------------------
# d. the pooled path
# ------------------------------------------------------------------------------------
def pooled_nets():
    """name -> (body modules, head modules) on 8x8 images: the body ends in a map"""
    return {
        "pooled_head": lambda: ([C(3, var_bias=0.1), SI(1.5, 2, 0.3), A(2),
                                 C(3, var_weight=1.5, var_bias=0.1), RB(0.5)],
                                [G(), C(1, var_weight=2.0, var_bias=0.3)]),
        "correlated": lambda: ([C(3, var_bias=0.1), CO(1, 2),
                                CC(3, lengthscale=1.5, var_bias=0.05), SI(1, 1, 0)],
                               [CC(8, padding=0, lengthscale=2.0, var_bias=0.2)]),
    }


@functools.lru_cache(maxsize=None)
def pooled_reference(name):
    body, head = pooled_nets()[name]()
    full, bod = S(*body, *head).double(), S(*body).double()
    X, Z = images(8, True)
    out = {}
    for mode in MODES:
        args = mode_args(X, Z, mode)
        out[mode] = SO.pool_ntk(full, *args) + SO.position_ntk(bod, *args)
    return out


def chunked(model, call, steps, itemsize):
    """``call()`` with the workspace of ``model`` holding two pairs and a half of ``steps``"""
    model.set_pool_workspace(2 * steps.peak * itemsize + steps.peak * itemsize // 2)
    try:
        return call()
    finally:
        model.set_pool_workspace(None)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", list(pooled_nets()))
def test_pooled_model_against_the_oracle(name, dtn):
    """forward, ntk_maps, position_covariance and position_ntk against the walk on
    position-pair maps; with a workspace of two pairs and a half (6 pairs: 3 chunks; the diag
    modes' 3 and 2 pairs: 2 chunks and 1) the same bits"""
    body, head = pooled_nets()[name]()
    dt = TORCH_DT[dtn]
    full, bod = S(*body, *head).to(DEV, dt), S(*body).to(DEV, dt)
    X, Z = (dev(a, dt) for a in images(8, True))
    ref = pooled_reference(name)
    item = X.element_size()
    fplan, bplan = full._plan(8, 8), bod._plan(8, 8)
    fbody = not any(o.kind == "pool" for o in fplan.prog.ops)
    tol = NET_TOL[dtn]
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            rk, rth, rs, rts = ref[mode]
            fwd = full(*args)
            assert tuple(fwd.shape) == rk.shape and fwd.dtype == X.dtype
            errs["K_" + mode] = max_err(fwd.cpu(), rk)
            km, tm = full.ntk_maps(*args, return_nngp=True)
            assert torch.equal(km, fwd), mode
            errs["Tm_" + mode] = max_err(tm.cpu(), rth)
            s = bod.position_covariance(*args)
            assert tuple(s.shape) == rs.shape
            errs["S_" + mode] = max_err(s.cpu(), rs)
            sk, st = bod.position_ntk(*args, return_nngp=True)
            assert torch.equal(sk, s), mode
            errs["TS_" + mode] = max_err(st.cpu(), rts)

            assert torch.equal(chunked(full, lambda: full(*args), fplan.pool, item), fwd)
            km2, tm2 = chunked(full, lambda: full.ntk_maps(*args, return_nngp=True),
                               fplan.pool_ntk(fbody, True, item), item)
            assert torch.equal(km2, km) and torch.equal(tm2, tm), mode
            assert torch.equal(chunked(bod, lambda: bod.position_covariance(*args),
                                       bplan.body_steps(), item), s)
            sk2, st2 = chunked(bod, lambda: bod.position_ntk(*args, return_nngp=True),
                               bplan.pool_ntk(True, True, item), item)
            assert torch.equal(sk2, sk) and torch.equal(st2, st), mode
    print(f"sin pooled {name} {dtn} (tol {tol:.1e}): "
          + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < tol, errs


def test_workspace_of_the_pooled_test_forces_chunks():
    """what test_pooled_model_against_the_oracle relies on: two pairs per chunk"""
    body, head = pooled_nets()["pooled_head"]()
    full = S(*body, *head).to(DEV, torch.float64)
    X, Z = (dev(a) for a in images(8, True))
    plan = full._plan(8, 8)
    whole = record(lambda: full(X, Z, False))
    parts = record(lambda: chunked(full, lambda: full(X, Z, False), plan.pool, 8))
    assert parts.count("cgp_cov_pool") == 3 and whole.count("cgp_cov_pool") == 1


# ------------------------------------------------------------------------------------
# e. behaviour
# ------------------------------------------------------------------------------------
def test_assigning_a_parameter_changes_the_next_call():
    """b and gamma are plain attributes: assigning one goes through NNGPKernel.__setattr__,
    the plan cache's key follows, and the next call gives a freshly built model's bits"""
    build = lambda b, g: S(C(3, var_bias=0.1), SI(1.5, b, 0.3), C(3), RB(g),     # noqa: E731
                           C(8, padding=0)).to(DEV, torch.float64)
    model = build(2.0, 0.5)
    X, Z = (dev(a) for a in images(8, True))
    with torch.no_grad():
        k1 = model(X, Z, False)
        model.mods[1].b = 1.25
        k2 = model(X, Z, False)
        assert torch.equal(k2, build(1.25, 0.5)(X, Z, False)) and not torch.equal(k2, k1)
        model.mods[3].gamma = 0.125
        k3, t3 = model.ntk(X, Z, False, return_nngp=True)
        kf, tf = build(1.25, 0.125).ntk(X, Z, False, return_nngp=True)
        assert torch.equal(k3, kf) and torch.equal(t3, tf) and not torch.equal(k3, k2)
        model.mods[1].b, model.mods[3].gamma = 2.0, 0.5
        assert torch.equal(model(X, Z, False), k1)


def test_sin_model_launches():
    """every op a launch of the new entry points, on both paths; the whole-network kernel and
    image_variances decline"""
    model = S(C(3), SI(), C(3), RB(), C(8, padding=0)).to(DEV, torch.float64)
    X, Z = (dev(a) for a in images(8, False))
    assert model.image_variances(X) is None
    seen = record(lambda: model(X, Z, False))
    assert seen.count("cgp_sin") == 2 and seen.count("cgp_var_sin_f64") == 2
    assert not any("relu" in s or "net" in s for s in seen)
    seen = record(lambda: model.ntk(X, Z, False))
    assert seen.count("cgp_sin") == 2
    seen = record(lambda: model.ntk_maps(X, Z, False))
    assert seen.count("cgp_sin_cov") == 2
    assert "cgp_covntk_nonlin" not in seen and "cgp_cov_nonlin" not in seen


@pytest.mark.parametrize("path", ["net", "layer"])
def test_relu_only_model_makes_the_same_calls(path, monkeypatch):
    import configs_util
    model = configs_util.model("mnist_paper_convnet_gp").double().to(DEV)
    model.set_fused_network(path == "net")
    x = dev(np.random.default_rng(0).random((4, 1, 28, 28)))
    seen = recorded_calls(model, x, monkeypatch)
    assert seen == PARENT_CALLS["mnist_paper_convnet_gp", path]
    assert not any("sin" in s for s in seen)
