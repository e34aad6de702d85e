"""GPU tests of the neural tangent kernel on position-pair maps: cgp_covntk_nonlin_* and
cgp_covntk_conv_* alone, networks through ntk_maps and position_ntk against the test-time
oracle (tests/pool_ntk_oracle.py, pinned to the definition of Θ by tests/test_pool_ntk_host.py),
the identities that tie the new route to model.ntk and to forward, chunking, fusion, the
Gram build and stream ordering.

Tolerances are the project's own (tests/test_gpu_pool.py): the op alone in float64 1e-12,
float64 end to end 1e-10 -- the closed-form ReLU included, so test_gpu_ntk.py's wider 1e-8 is
not used -- and float32 against the float64 oracle on float32-representable inputs 2e-5;
errors are max|got - ref| / max|ref|.  Inputs follow op_inputs' four-channel recipe, for the
reason its docstring gives."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp import program as P

import pool_ntk_oracle as NO
import pool_oracle as PO
from stream_util import Control, delay
from test_gpu_gelu import run_gelu_cov
from test_gpu_pool import (DEV, NET_TOL, NP_DT, OP_TOL, TORCH_DT, dev, idx32, max_err,
                           op_inputs, run_conv, run_nonlin, stream)

pytestmark = pytest.mark.gpu

m = cnn_gp
S, C, R, E, GE, G, A, CC = (m.Sequential, m.Conv2d, m.ReLU, m.Erf, m.Gelu, m.GlobalAvgPool,
                            m.AvgPool2d, m.CorrelatedConv2d)
KIND = {"relu": N.CGP_COV_RELU, "erf": N.CGP_COV_ERF, "gelu": N.CGP_COV_GELU}


def rnd(a, dtn):
    return np.asarray(a).astype(NP_DT[dtn]).astype(np.float64)


def to_dev(a, dtn):
    return None if a is None else dev(PO.to_device_layout(a), TORCH_DT[dtn])


def back(t, h, w):
    return PO.from_device_layout(t.cpu().numpy(), h, w)


# ------------------------------------------------------------------------------------
# a. cgp_covntk_nonlin_* alone
# ------------------------------------------------------------------------------------
def run_nonlin_ntk(kind, s, th, xx, yy, pi, pj, dtn, same=False, flags=0, addend=None,
                   addend_theta=None, inplace=False, alias=False, rc=0):
    """cgp_covntk_nonlin_*; ``alias``: theta is in's buffer (th is ignored); ``inplace``:
    out is in and out_theta is theta (with alias: out_theta is a buffer of its own)"""
    dt = TORCH_DT[dtn]
    h, w = s.shape[1:3]
    sd = to_dev(s, dtn)
    td = sd if alias else to_dev(th, dtn)
    ad, atd = to_dev(addend, dtn), to_dev(addend_theta, dtn)
    out = sd if inplace else torch.empty_like(sd)
    tout = td if inplace and not alias else torch.empty_like(sd)
    di, dj, vx, vy = idx32(pi), idx32(pj), dev(xx, dt), dev(yy, dt)
    a = N.CovNonlinNtkArgs()
    a.in_, a.theta, a.out, a.out_theta = N.ptr(sd), N.ptr(td), N.ptr(out), N.ptr(tout)
    a.addend, a.addend_theta, a.xx, a.yy = N.ptr(ad), N.ptr(atd), N.ptr(vx), N.ptr(vy)
    a.pair_i, a.pair_j, a.npairs = N.ptr(di), N.ptr(dj), len(pi)
    a.h, a.w, a.kind, a.same, a.flags = h, w, KIND[kind], int(same), flags
    got = getattr(N.load(), f"cgp_covntk_nonlin_{dtn}")(ctypes.byref(a), stream())
    assert got == rc, N.load().cgp_last_error()
    torch.cuda.synchronize()
    return back(out, h, w), back(tout, h, w)


def forward_nonlin(kind, s, xx, yy, pi, pj, dtn, **kw):
    """the forward-only entry point of the same map: cgp_cov_nonlin_* / cgp_gelu_cov_*"""
    if kind == "gelu":
        kw.pop("flags", None)
        return run_gelu_cov(s, xx, yy, pi, pj, dtn, **kw)
    return run_nonlin(s, KIND[kind], xx, yy, pi, pj, dtn, **kw)


# 7x7: 2401 elements per pair, so 2048-element chunks straddle pair boundaries; 5x3 catches
# transposed indices
NONLIN_CASES = [(h, w, pairs) for h, w in ((7, 7), (5, 3)) for pairs in ("all", "triu", "diag")]
FORMS = [("relu", 0), ("relu", N.CGP_FLAG_EXACT_RELU), ("erf", 0), ("gelu", 0)]
ids = lambda c: "-".join(map(str, c))                                            # noqa: E731


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("form", FORMS, ids=ids)
@pytest.mark.parametrize("case", NONLIN_CASES, ids=ids)
def test_cov_nonlin_ntk(case, form, dtn):
    h, w, pairs = case
    kind, flags = form
    x, y, pi, pj, same, s0, vx, vy = op_inputs(h, w, pairs, dtn)
    rng = np.random.default_rng(11)
    th, addend, addend_t = (rnd(rng.standard_normal(s0.shape), dtn) for _ in range(3))
    ref, ref_t = NO.nonlin_ntk(kind, s0, th, vx, vy, pi, pj, same)
    got, got_t = run_nonlin_ntk(kind, s0, th, vx, vy, pi, pj, dtn, same=same, flags=flags)
    errs = max_err(got, ref), max_err(got_t, ref_t)
    print(f"cov_nonlin_ntk {dtn} {case} {form}: K' {errs[0]:.2e}, Θ' {errs[1]:.2e}")
    assert max(errs) < OP_TOL[dtn]
    # out: the forward-only entry point's bits
    fwd = forward_nonlin(kind, s0, vx, vy, pi, pj, dtn, same=same, flags=flags)
    np.testing.assert_array_equal(got, fwd)
    # in place, and with both addends (each a separate rounding)
    gi, gti = run_nonlin_ntk(kind, s0, th, vx, vy, pi, pj, dtn, same=same, flags=flags,
                             inplace=True)
    np.testing.assert_array_equal(gi, got)
    np.testing.assert_array_equal(gti, got_t)
    t = NP_DT[dtn]
    plus = lambda a, b: (a.astype(t) + b.astype(t)).astype(np.float64)           # noqa: E731
    for inplace in (False, True):
        ga, gat = run_nonlin_ntk(kind, s0, th, vx, vy, pi, pj, dtn, same=same, flags=flags,
                                 addend=addend, addend_theta=addend_t, inplace=inplace)
        np.testing.assert_array_equal(ga, plus(got, addend))
        np.testing.assert_array_equal(gat, plus(got_t, addend_t))
    ga, gat = run_nonlin_ntk(kind, s0, th, vx, vy, pi, pj, dtn, same=same, flags=flags,
                             addend=addend)
    np.testing.assert_array_equal(ga, plus(got, addend))
    np.testing.assert_array_equal(gat, got_t)
    # theta aliasing in: Θ is K's buffer after the first conv
    want = NO.nonlin_ntk(kind, s0, s0, vx, vy, pi, pj, same)[1]
    for inplace in (False, True):
        ga, gat = run_nonlin_ntk(kind, s0, None, vx, vy, pi, pj, dtn, same=same, flags=flags,
                                 alias=True, inplace=inplace)
        np.testing.assert_array_equal(ga, got)
        assert max_err(gat, want) < OP_TOL[dtn]
    if same:
        # the override elements: K' is the variance map's value, κ̇ the layer path's
        self_t = np.einsum("mabab->mab", got_t)[pi == pj]
        self_th = np.einsum("mabab->mab", th)[pi == pj]
        if kind == "relu":
            np.testing.assert_array_equal(self_t, self_th / 2)               # Θ/2 exactly
        off = got_t[pi == pj][:, 0, 0, 0, 1] / th[pi == pj][:, 0, 0, 0, 1]
        on = self_t[:, 0, 0] / self_th[:, 0, 0]
        assert np.all(np.abs(off - on) > 1e-4)                # p != q takes the ordinary κ̇


def test_cov_nonlin_ntk_exact_flag_selects_another_form():
    x, y, pi, pj, same, s0, vx, vy = op_inputs(7, 7, "all", "f64")
    th = np.random.default_rng(1).standard_normal(s0.shape)
    a = run_nonlin_ntk("relu", s0, th, vx, vy, pi, pj, "f64")
    b = run_nonlin_ntk("relu", s0, th, vx, vy, pi, pj, "f64", flags=N.CGP_FLAG_EXACT_RELU)
    assert not np.array_equal(a[1], b[1]) and max_err(a[1], b[1]) < 2 * OP_TOL["f64"]


# ------------------------------------------------------------------------------------
# b. cgp_covntk_conv_* against the launch-by-launch sequence and the oracle
# ------------------------------------------------------------------------------------
def conv_args(cls, mod, shape, npairs, bias=None):
    h, w = shape
    ho, wo = P.conv_out_hw(mod, h, w)
    g = P.conv_geometry(mod)
    a = cls()
    a.npairs, a.h, a.w, a.ho, a.wo = npairs, h, w, ho, wo
    a.taps, a.offset, a.stride, a.dilation = g.taps, g.offset, g.stride, g.dilation
    a.weight, a.bias = g.weight, g.bias if bias is None else bias
    return a, (ho, wo)


def run_conv_ntk(s, th, mod, pi, pj, dtn, post=N.CGP_COV_NONE, xx=None, yy=None, same=False,
                 flags=0, addend=None, addend_theta=None, rc=0):
    dt = TORCH_DT[dtn]
    sd, td = to_dev(s, dtn), to_dev(th, dtn)
    ad, atd = to_dev(addend, dtn), to_dev(addend_theta, dtn)
    vx = None if xx is None else dev(xx, dt)
    vy = None if yy is None else dev(yy, dt)
    di, dj = idx32(pi), idx32(pj)
    a, (ho, wo) = conv_args(N.CovConvNtkArgs, mod, s.shape[1:3], len(pi))
    out = torch.empty((len(pi), (ho * wo) ** 2), dtype=dt, device=DEV)
    tout = torch.empty_like(out)
    a.in_, a.theta, a.out, a.out_theta = N.ptr(sd), N.ptr(td), N.ptr(out), N.ptr(tout)
    a.addend, a.addend_theta, a.xx, a.yy = N.ptr(ad), N.ptr(atd), N.ptr(vx), N.ptr(vy)
    a.pair_i, a.pair_j = N.ptr(di), N.ptr(dj)
    a.post, a.same, a.flags = post, int(same), flags
    got = getattr(N.load(), f"cgp_covntk_conv_{dtn}")(ctypes.byref(a), stream())
    assert got == rc, N.load().cgp_last_error()
    torch.cuda.synchronize()
    return back(out, ho, wo), back(tout, ho, wo)


def run_sequence(s, th, mod, pi, pj, dtn, kind=None, xx=None, yy=None, same=False, flags=0,
                 addend=None, addend_theta=None):
    """the yardstick: cgp_cov_conv_* on K, cgp_cov_conv_* on Θ with bias 0 and addend K', then
    cgp_covntk_nonlin_* (or the two addends by cgp_axpby_*)"""
    dt = TORCH_DT[dtn]
    di, dj = idx32(pi), idx32(pj)

    def conv(src, bias, add):
        a, (ho, wo) = conv_args(N.CovConvArgs, mod, s.shape[1:3], len(pi), bias)
        out = torch.empty((len(pi), (ho * wo) ** 2), dtype=dt, device=DEV)
        a.in_, a.out, a.addend = N.ptr(src), N.ptr(out), N.ptr(add)
        N.check(getattr(N.load(), f"cgp_cov_conv_{dtn}")(ctypes.byref(a), stream()), "conv")
        return out, (ho, wo)

    kp, (ho, wo) = conv(to_dev(s, dtn), None, None)
    tp = kp if th is None else conv(to_dev(th, dtn), 0.0, kp)[0]
    ad, atd = to_dev(addend, dtn), to_dev(addend_theta, dtn)
    if kind is not None:
        vx, vy = dev(xx, dt), dev(yy, dt)
        out, tout = torch.empty_like(kp), torch.empty_like(kp)
        a = N.CovNonlinNtkArgs()
        a.in_, a.theta, a.out, a.out_theta = N.ptr(kp), N.ptr(tp), N.ptr(out), N.ptr(tout)
        a.addend, a.addend_theta, a.xx, a.yy = N.ptr(ad), N.ptr(atd), N.ptr(vx), N.ptr(vy)
        a.pair_i, a.pair_j, a.npairs = N.ptr(di), N.ptr(dj), len(pi)
        a.h, a.w, a.kind, a.same, a.flags = ho, wo, KIND[kind], int(same), flags
        N.check(getattr(N.load(), f"cgp_covntk_nonlin_{dtn}")(ctypes.byref(a), stream()),
                "nonlin_ntk")
    else:
        out, tout = kp, tp
        if ad is not None:
            out, tout = torch.empty_like(kp), torch.empty_like(kp)
            for src, add, dst in ((kp, ad, out), (tp, atd, tout)):
                N.call(f"cgp_axpby_{dtn}", 1.0, N.ptr(src), 1.0, N.ptr(add), N.ptr(dst),
                       src.numel(), stream())
    torch.cuda.synchronize()
    return back(out, ho, wo), back(tout, ho, wo)


CONV_GEOMETRIES = {
    "same3": (5, 4, lambda: C(3, var_weight=1.3, var_bias=0.2)),
    "stride2": (7, 7, lambda: C(3, stride=2, var_bias=0.1)),
    "even_valid": (5, 4, lambda: C(2, padding=0, var_bias=0.1)),
    "dilation2": (7, 7, lambda: C(3, dilation=2, var_weight=0.7)),
    "readout_to_1x1": (4, 4, lambda: C(4, padding=0, var_bias=0.3)),
    "1x1": (1, 1, lambda: C(1, var_weight=2.0, var_bias=0.3)),
}


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", list(CONV_GEOMETRIES))
def test_cov_conv_ntk(name, dtn):
    """every post-stage, theta NULL and given, with and without both addends, on every pair
    list: bit for bit against the sequence, within OP_TOL of the oracle"""
    h, w, make = CONV_GEOMETRIES[name]
    mod = make()
    worst = 0.0
    for pairs in ("all", "triu", "diag"):
        x, y, pi, pj, same, s0, vx, vy = op_inputs(h, w, pairs, dtn)
        rng = np.random.default_rng(5)
        theta = rnd(rng.standard_normal(s0.shape), dtn)
        ox, oy = rnd(PO.conv_var(vx, mod), dtn), rnd(PO.conv_var(vy, mod), dtn)
        lin = PO.conv_map(s0, mod)
        adds = tuple(rnd(rng.standard_normal(lin.shape), dtn) for _ in range(2))
        for th in (theta, None):
            kp, tp = NO.conv_ntk(s0, th, mod)
            for kind, flags in [(None, 0)] + FORMS:
                if kind is None:
                    ref, ref_t = kp, tp
                    kw = {}
                else:
                    ref, ref_t = NO.nonlin_ntk(kind, kp, tp, ox, oy, pi, pj, same)
                    kw = dict(xx=ox, yy=oy, same=same, flags=flags)
                post = N.CGP_COV_NONE if kind is None else KIND[kind]
                for ad, adt in ((None, None), adds):
                    got, got_t = run_conv_ntk(s0, th, mod, pi, pj, dtn, post=post, addend=ad,
                                              addend_theta=adt, **kw)
                    seq, seq_t = run_sequence(s0, th, mod, pi, pj, dtn, kind=kind, addend=ad,
                                              addend_theta=adt, **kw)
                    np.testing.assert_array_equal(got, seq)
                    np.testing.assert_array_equal(got_t, seq_t)
                    if ad is None:
                        worst = max(worst, max_err(got, ref), max_err(got_t, ref_t))
                    else:
                        worst = max(worst, max_err(got, ref + ad), max_err(got_t, ref_t + adt))
                # out: cgp_cov_conv_*'s bits (the forward GELU is a launch of its own)
                if kind != "gelu":
                    fwd = run_conv(s0, mod, pi, pj, dtn, post=post, **kw)
                    np.testing.assert_array_equal(
                        run_conv_ntk(s0, th, mod, pi, pj, dtn, post=post, **kw)[0], fwd)
    print(f"cov_conv_ntk {dtn} {name}: {worst:.2e}")
    assert worst < OP_TOL[dtn]


def test_cov_conv_ntk_over_the_lds_cap_is_an_error_without_a_launch():
    """7 taps, w = 28, float64: both streams' blocks are 87 808 bytes > 64 KB"""
    mod = C(7)
    s = np.zeros((1, 28, 28, 28, 28))
    lib = N.load()
    sd = to_dev(s, "f64")
    td, out, tout = (torch.full_like(sd, 3.0) for _ in range(3))
    a, _ = conv_args(N.CovConvNtkArgs, mod, (28, 28), 1)
    a.in_, a.theta, a.out, a.out_theta = N.ptr(sd), N.ptr(td), N.ptr(out), N.ptr(tout)
    assert lib.cgp_covntk_conv_f64(ctypes.byref(a), stream()) == 1001
    assert b"87808 bytes, more than the 65536 of LDS" in lib.cgp_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == float(tout.max()) == 3.0                  # nothing ran
    # one stream fits (theta NULL), and float32 fits both
    a.theta = None
    assert lib.cgp_covntk_conv_f64(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, tout) and float(out.abs().max()) == 0.0


# ------------------------------------------------------------------------------------
# c. networks against the oracle
# ------------------------------------------------------------------------------------
def nets():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)                          # noqa: E731
    return {
        "gap": (S(C(3, var_bias=.1), R(), C(3, var_weight=1.5), R(), C(3, var_bias=.2), R(),
                  G()), (6, 5)),
        "gap_readout": (S(C(3), R(), C(3), G(), C(1, var_weight=2., var_bias=.3)), (6, 5)),
        "myrtle": (S(C(3, var_bias=.1), R(), C(3), R(), A(2), C(3, var_bias=.2), R(), A(2), G(),
                     C(1, var_weight=2., var_bias=.3)), (8, 8)),
        "avgpool_7x7": (S(C(3, var_bias=.1), R(), A(2), C(3), R(), C(3, padding=0)), (7, 7)),
        "corrconv": (S(C(3, var_bias=.1), R(), CC(3, lengthscale=1., var_weight=1.5,
                                                   var_bias=.1), R(),
                       CC(4, padding=0, lengthscale=1.5, var_bias=.2)), (4, 4)),
        "erf": (S(C(3, var_bias=.2), E(), C(3, var_weight=1.5), E(), G()), (6, 5)),
        "gelu": (S(C(3, var_bias=.2), GE(), C(3, var_weight=1.5), GE(), A(2), GE(),
                   C(2, padding=0)), (4, 4)),
        "residual": (S(C(3), m.Sum([S(), S(R(), C(3, var_bias=.1), R(), C(3))]), R(), G()),
                     (6, 5)),
        "mixture": (S(C(3), m.Mixture([S(R(), C(3)), S(E(), C(3, var_bias=.2)), S()],
                                      t(0.3, -0.5, 0.1)), R(), G()), (6, 5)),
    }


NET_NAMES = list(nets())
MODES = ["xx", "xz", "same_diag", "xz_diag"]


def images(hw):
    rng = np.random.default_rng(10 * hw[0] + hw[1])
    draw = lambda n: rng.random((n, 4) + tuple(hw), dtype=np.float32).astype(np.float64)   # noqa
    return draw(3), draw(2)


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:2], Z, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def net_reference(name):
    model, hw = nets()[name]
    X, Z = images(hw)
    return {mode: NO.ntk(model.double(), *mode_args(X, Z, mode)) for mode in MODES}


RUNS = [("f64", True), ("f64", False), ("f32", False)]


@pytest.mark.parametrize("run", RUNS, ids=lambda r: f"{r[0]}-{'exact' if r[1] else 'closed'}")
@pytest.mark.parametrize("name", NET_NAMES)
def test_network(name, run):
    dtn, exact = run
    ref = net_reference(name)
    model, hw = nets()[name]
    model = model.to(DEV, TORCH_DT[dtn]).set_exact_relu(exact)
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(hw))
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            k, th = model.ntk_maps(*args, return_nngp=True)
            assert tuple(k.shape) == tuple(th.shape) == ref[mode][0].shape
            assert th.dtype == X.dtype and th.device == X.device
            errs[mode] = max(max_err(k.cpu(), ref[mode][0]), max_err(th.cpu(), ref[mode][1]))
            # e. K is forward's, bit for bit; Θ alone is the same Θ
            assert torch.equal(k, model(*args))
            assert torch.equal(th, model.ntk_maps(*args))
            if mode == "xx":
                kxx, txx = k, th
                assert torch.equal(th, th.T) and torch.equal(k, k.T)     # mirrored
            if mode == "same_diag":
                assert torch.equal(th, torch.diagonal(txx))
        assert torch.equal(model.ntk_maps(X, X.clone(), True), txx)
        tc = model.ntk_maps(X.cpu(), Z.cpu(), False)
        assert tc.device.type == "cpu" and torch.equal(tc, model.ntk_maps(X, Z, False).cpu())
    print(f"ntk_maps {name} {dtn} exact={exact}: " + " ".join(f"{k}={v:.1e}"
                                                               for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_position_ntk(dtn):
    """Θ[i, j, p, q] of a body, elementwise; its mean is what the pooled head returns"""
    body = S(C(3, var_bias=.1), R(), C(3, stride=2, var_weight=1.5), R(), C(3), E())
    hw = (6, 5)
    X, Z = images(hw)
    Xd, Zd = (dev(a, TORCH_DT[dtn]) for a in (X, Z))
    body = body.to(DEV, TORCH_DT[dtn])
    with torch.no_grad():
        for mode in MODES:
            rs, rt = NO.position_ntk(body, *mode_args(X, Z, mode))
            s, th = body.position_ntk(*mode_args(Xd, Zd, mode), return_nngp=True)
            assert tuple(th.shape) == rt.shape == tuple(s.shape)
            assert max_err(s.cpu(), rs) < NET_TOL[dtn] and max_err(th.cpu(), rt) < NET_TOL[dtn]
            assert torch.equal(s, body.position_covariance(*mode_args(Xd, Zd, mode)))
            if mode == "xx":
                assert torch.equal(th, th.permute(1, 0, 4, 5, 2, 3))     # Θ_ji[q, p] = Θ_ij[p, q]
                txx = th
            if mode == "same_diag":
                assert torch.equal(th, txx[torch.arange(3), torch.arange(3)])
            if mode == "xz":
                pooled = S(body, G()).ntk_maps(Xd, Zd, False)
                assert max_err(pooled.cpu(), th.mean(dim=(2, 3, 4, 5)).cpu().numpy()) \
                    < NET_TOL[dtn]


# ------------------------------------------------------------------------------------
# d. identities that tie the new route to tested code
# ------------------------------------------------------------------------------------
def assert_same_ntk(a, b, hw, dtn, tol, bits=False):
    """ntk_maps of model a against b's (b without position-pair maps: model.ntk)"""
    X, Z = (dev(t, TORCH_DT[dtn]) for t in images(hw))
    a, b = a.to(DEV, TORCH_DT[dtn]), b.to(DEV, TORCH_DT[dtn])
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            ka, ta = a.ntk_maps(*args, return_nngp=True)
            kb, tb = (b.ntk if b._plan(*hw).pool is None else b.ntk_maps)(*args, return_nngp=True)
            if bits:
                assert torch.equal(ka, kb) and torch.equal(ta, tb), mode
            else:
                assert max_err(ka.cpu(), kb.cpu()) < tol and max_err(ta.cpu(), tb.cpu()) < tol, mode


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_without_a_pooling_layer_is_model_ntk(dtn):
    layers = lambda: [C(3, var_bias=.1), R(), C(3, var_weight=1.5), E(),         # noqa: E731
                      m.Sum([S(), S(C(3), GE())]), C(4, padding=0, var_bias=.2)]
    assert_same_ntk(S(*layers()), S(*layers()), (4, 4), dtn, NET_TOL[dtn])
    for mod in (S(), S(R())):                                # no conv: Θ = 0
        mod = mod.to(DEV, TORCH_DT[dtn])
        x = dev(np.random.default_rng(0).random((3, 2, 1, 1)), TORCH_DT[dtn])
        k, th = mod.ntk_maps(x, return_nngp=True)
        assert float(th.abs().max()) == 0.0 and max_err(k.cpu(), mod(x).cpu().numpy()) < NET_TOL[dtn]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_identity_correlation_is_the_conv_nets_ntk(dtn):
    l1, l2 = dict(var_weight=2.25, var_bias=.1), dict(padding=0, var_weight=4., var_bias=.2)
    assert_same_ntk(S(CC(3, lengthscale=0, **l1), R(), CC(4, lengthscale=0, **l2)),
                    S(C(3, **l1), R(), C(4, **l2)), (4, 4), dtn, NET_TOL[dtn])


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_all_ones_readout_is_the_pooled_head(dtn):
    """R = ones, k = H, padding 0, var_weight w against GlobalAvgPool + Conv2d(1, w·H·W)"""
    body = lambda: [C(3, var_bias=.1), R(), C(3, var_weight=1.5), R()]           # noqa: E731
    assert_same_ntk(
        S(*body(), CC(4, padding=0, lengthscale=float("inf"), var_weight=1.5, var_bias=.3)),
        S(*body(), G(), C(1, var_weight=1.5 * 16, var_bias=.3)), (4, 4), dtn, NET_TOL[dtn])


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_avgpool_of_one_changes_no_bit(dtn):
    body = lambda: [C(3, var_bias=.1), R(), C(3, var_weight=1.5), E()]           # noqa: E731
    assert_same_ntk(S(*body(), A(1), G()), S(*body(), G()), (6, 5), dtn, 0.0, bits=True)


# ------------------------------------------------------------------------------------
# e. invariants
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", ["myrtle", "corrconv", "residual"])
def test_chunking_and_fusion_change_no_bit(name, dtn):
    dt = TORCH_DT[dtn]
    model, hw = nets()[name]
    model = model.to(DEV, dt)
    X, Z = (dev(a, dt) for a in images(hw))
    plan = model._plan(*hw)
    body = not any(o.kind == "pool" for o in plan.prog.ops)
    ns = plan.pool_ntk(body, True, X.element_size())
    assert any(st.fn == "conv_ntk" for st in ns.steps)
    per_pair = ns.peak * X.element_size()
    with torch.no_grad():
        whole = model.ntk_maps(X, Z, False, return_nngp=True), model.ntk_maps(X, return_nngp=True)
        # 6 pairs each (3 x 2, and the upper triangle of 3 x 3) in chunks of 2: 3 chunks
        model.set_pool_workspace(2 * per_pair + per_pair // 2)
        seen = []
        real = N.check

        def check(rc, what):
            seen.append(what)
            return real(rc, what)
        N.check = check
        try:
            parts = model.ntk_maps(X, Z, False, return_nngp=True), \
                model.ntk_maps(X, return_nngp=True)
        finally:
            N.check = real
        # moments launches: 3 chunks per call, plus the self passes' (one chunk per image set)
        assert seen.count("cgp_cov_moments") >= 6 and "cgp_covntk_conv" in seen
        for p, w in zip(parts, whole):
            assert torch.equal(p[0], w[0]) and torch.equal(p[1], w[1])
        model.set_pool_workspace(per_pair - 1)
        with pytest.raises(RuntimeError, match=f"{per_pair} bytes.*workspace of {per_pair - 1}"):
            model.ntk_maps(X, Z, False)
        model.set_pool_workspace(None)
        # the launch-by-launch lowering: the same bits
        model.set_ntk_maps_fusion(False)
        seen.clear()
        N.check = check
        try:
            unfused = model.ntk_maps(X, Z, False, return_nngp=True), \
                model.ntk_maps(X, return_nngp=True)
        finally:
            N.check = real
        assert "cgp_covntk_conv" not in seen and "cgp_covntk_nonlin" in seen
        for p, w in zip(unfused, whole):
            assert torch.equal(p[0], w[0]) and torch.equal(p[1], w[1])


def test_gram_matrix_ntk_maps_is_the_tiles_of_ntk_maps():
    model, hw = nets()["gap"]
    model = model.to(DEV, torch.float64)
    X = torch.from_numpy(np.random.default_rng(4).random((5, 4) + hw, dtype=np.float32)
                         .astype(np.float64)).to(DEV)
    with torch.no_grad():
        th = model.ntk_maps(X)
        g = gram.gram_matrix(model, X, batch_size=2, ntk="maps")
        gz = gram.gram_matrix(model, X[:3], X[3:], batch_size=2, ntk="maps")
        iu = np.triu_indices(5)
        np.testing.assert_array_equal(g.cpu().numpy()[iu], th.cpu().numpy()[iu])
        assert torch.equal(gz, model.ntk_maps(X[:3], X[3:], False))
        with pytest.raises(NotImplementedError):
            gram.gram_matrix(model, X, batch_size=2, ntk=True)       # model.ntk still raises


# ------------------------------------------------------------------------------------
# f. stream ordering
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["myrtle", "corrconv"])
def test_ntk_maps_queued_behind_a_held_producer(name):
    """ntk_maps on a side stream, its images still being produced behind a delay when the
    call is made, equals the quiesced call bit for bit"""
    model, hw = nets()[name]
    model = model.to(DEV, torch.float64)
    Xf, Zf = (dev(a) for a in images(hw))
    with torch.no_grad():
        want = [t.cpu().numpy() for t in model.ntk_maps(Xf, Zf, False, return_nngp=True)] + \
            [model.ntk_maps(Xf).cpu().numpy()]
    Xd, Zd = torch.zeros_like(Xf), torch.zeros_like(Zf)
    ctl = Control(Xd)                                        # synchronises
    side = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(side):
        delay()
        Xd.copy_(Xf)
        Zd.copy_(Zf)
        ctl.check()
        got = [t.cpu().numpy() for t in model.ntk_maps(Xd, Zd, False, return_nngp=True)] + \
            [model.ntk_maps(Xd).cpu().numpy()]
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
