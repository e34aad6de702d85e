"""CPU-only tests of the Hermite-series nonlinearities (cnn_gp.HermiteNonlin, Tanh, Sigmoid,
Softplus, SiLU, GeluTanh): the oracle's truncated series against an independent 2-D
Gauss–Hermite rule and against the closed forms of erf and GELU, its identities (a'_n against
a_{n+1}, symmetry, positive semi-definiteness), the modules, the lowering on every path, the
plan-cache key, and the host side of cgp_hermite_coef_* / cgp_hermite_* / cgp_var_hermite_* /
cgp_hermite_cov_*."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import program as P
from cnn_gp.program import Plan, compile_program, ntk_steps, pool_ntk_steps, pool_steps

from conftest import ROOT
import hermite_oracle as HO

m = cnn_gp
S, C, R, G, A, H = m.Sequential, m.Conv2d, m.ReLU, m.GlobalAvgPool, m.AvgPool2d, m.HermiteNonlin
CLASSES = {"tanh": m.Tanh, "sigmoid": m.Sigmoid, "softplus": m.Softplus, "silu": m.SiLU,
           "gelu_tanh": m.GeluTanh}

# ------------------------------------------------------------------------------------
# the series against the truth
# ------------------------------------------------------------------------------------
VS = (0.0, 0.05, 0.25, 1.0)
RHOS = (-1.0, -0.9, 0.0, 0.5, 0.99, 1.0)
ORDER = 32
_TRUTH, _TAIL = {}, {}


def truth(name, v1, v2, rho, deriv):
    """HO.truth, symmetric in (v1, v2), computed once per point"""
    key = (name, min(v1, v2), max(v1, v2), rho, deriv)
    if key not in _TRUTH:
        _TRUTH[key] = HO.truth(name, key[1], key[2], rho, deriv)
    return _TRUTH[key]


def tail(name, v, deriv):
    """t(v) = E φ² − Σ_{n<=32} a_n(v)², summed from the dropped coefficients themselves,
    Σ_{32<n<=160} a_n² by a 340-node rule: the difference of the two O(1) numbers carries their
    rounding, 1e-17, which is above t itself at v <= 0.25 (1e-19 for erf) and under the square
    root of the bound would stand for 1e-13.  What lies past n = 160 is dropped, so this is a
    lower estimate of t and the bound below is no wider for it."""
    key = (name, v, deriv)
    if key not in _TAIL:
        a = HO.coefficients(v, (name, 160, 340), deriv)
        _TAIL[key] = float((a[ORDER + 1:] ** 2).sum())
    return _TAIL[key]


def series_misses(name, nq, deriv):
    """[(v1, v2, ρ, error, bound)] of the points of VS² x RHOS where the series of order 32 and
    nq nodes is further from the truth than √(t(v1)·t(v2))·|ρ|³³ + 1e-13·√(E φ²(v1)·E φ²(v2)),
    and the worst error over the scale"""
    rule, misses, worst = (name, ORDER, nq), [], 0.0
    for v1 in VS:
        for v2 in VS:
            scale = math.sqrt(HO.second_moment(name, v1, deriv) * HO.second_moment(name, v2, deriv))
            dropped = math.sqrt(tail(name, v1, deriv) * tail(name, v2, deriv))
            for rho in RHOS:
                got = HO.series(rho * math.sqrt(v1 * v2), v1, v2, rule)[int(deriv)]
                err = abs(float(got) - truth(name, v1, v2, rho, deriv))
                bound = dropped * abs(rho) ** (ORDER + 1) + 1e-13 * scale
                if not err <= bound:
                    misses.append((v1, v2, rho, err, bound))
                if scale:
                    worst = max(worst, err / scale)
    return misses, worst


@pytest.mark.parametrize("name", HO.PHIS)
def test_series_is_within_its_tail_of_the_truth(name):
    """K' of the series at order 32 and 96 nodes against the 300 x 300 rule, at v in {0, 0.05,
    0.25, 1}² and ρ in {−1, −0.9, 0, 0.5, 0.99, 1}: the error is at most the Cauchy–Schwarz
    bound on the dropped terms, √(t(v1)·t(v2))·|ρ|³³, plus 1e-13 of the scale; the same for κ̇
    with the tail of φ'.  The bound has no term for the coefficient quadrature, so it also pins
    the 96-node rule: with numpy's rule as it comes, tanh (poles at ±iπ/2) is 7.3e-13 from the
    truth at v = (1, 1), ρ = 0.5, 19 times the bound; with the rule compressed to |z| <= 12.5
    (program.hermite_rule) it is at the rounding level."""
    for deriv in (False, True):
        misses, worst = series_misses(name, 96, deriv)
        print(f"{name}: order 32, 96 nodes, {'kdot' if deriv else 'K'}: worst error "
              f"{worst:.2e} of the scale, {len(misses)} points past the bound")
        for v1, v2, rho, err, bound in misses:
            print(f"  v = ({v1}, {v2}), rho = {rho}: {err:.2e} against {bound:.2e}")
        assert not misses


def test_the_rule_is_the_compressed_gauss_hermite_rule():
    """program.hermite_rule: numpy's rule up to 46 nodes, beyond that its nodes pulled in to
    |z| <= 12.5 with the weights of the substitution; the oracle's rule bit for bit; still a rule
    for the standard normal on what the coefficients integrate, h_n times a φ of at most linear
    growth: the moments 1, 0, 1, 0, 3 and E[h_n] = δ_n0, E[z·h_n] = δ_n1 for n <= 64 to 1e-13.
    The compressed rule is no longer exact on polynomials; its error is what lies beyond
    |z| = 12.5, where |h_n(z)|·exp(−z²/2) <= exp(−z²/4) = 1e-17.  It is not a rule for
    products h_n·h_m of high degree, which the coefficients never form."""
    for nq in (2, 40, 46):
        z, w = np.polynomial.hermite_e.hermegauss(nq)
        rz, rw = P.hermite_rule(nq)
        assert np.array_equal(rz, z) and np.array_equal(rw, w / math.sqrt(2 * math.pi))
    for nq in (47, 96, 128, 256):
        z, w = P.hermite_rule(nq)
        oz, ow, h = HO.tables(64, nq)
        assert np.array_equal(z, oz) and np.array_equal(w, ow)
        assert abs(np.abs(z).max() - P.HERMITE_RANGE) < 1e-12 and np.all(w > 0)
        for k, want in enumerate((1.0, 0.0, 1.0, 0.0, 3.0)):
            assert abs(float(w @ z ** k) - want) < 1e-13, (nq, k)
        for k in (0, 1):
            assert np.max(np.abs((h * z ** k) @ w - (np.arange(65) == k))) < 1e-13, (nq, k)


def test_truncation_table():
    """Σ_{n>32} a_n² / E φ² at v = 1 and v = 4 (DESIGN §3.11's table): within a factor of 1.5
    of the figures the defaults were chosen by, and growing with the variance"""
    want = {"tanh": (2e-7, 2e-4), "sigmoid": (6e-14, 6e-8), "softplus": (6e-16, 1e-9),
            "silu": (3e-13, 9e-8), "gelu_tanh": (4e-12, 4e-6), "erf": (1.5e-8, 3e-4)}
    for name, figures in want.items():
        for v, fig in zip((1.0, 4.0), figures):
            a = HO.coefficients(v, (name, 300, 340))
            got = float((a[ORDER + 1:] ** 2).sum()) / HO.second_moment(name, v)
            print(f"{name} v = {v}: tail {got:.2e}")
            assert fig / 1.5 < got < fig * 1.5, (name, v, got)


def _draws(n=400, seed=3, vmax=0.25):
    """variances in [0, vmax] with exact zeros, ρ in [−1, 1] with exact ±1"""
    rng = np.random.default_rng(seed)
    v1, v2 = vmax * rng.random(n), vmax * rng.random(n)
    v1[:5], v2[3:8] = 0.0, 0.0
    rho = rng.uniform(-1, 1, n)
    rho[10:30], rho[30:50] = 1.0, -1.0
    return rho * np.sqrt(v1 * v2), v1, v2


@pytest.mark.parametrize("name", ["erf", "gelu"])
def test_series_matches_the_closed_form_at_small_variances(name):
    """at v <= 0.25 the series of erf and of the exact GELU carry no truncation error above
    rounding: 1e-12 of max|K'| from the closed forms of erf_oracle.py / gelu_oracle.py"""
    c, v1, v2 = _draws()
    k, kd = HO.series(c, v1, v2, (name, 32, 96))
    ck, ckd = HO.closed_form(name, c, v1, v2)
    ek, ekd = np.max(np.abs(k - ck)) / np.max(np.abs(ck)), np.max(np.abs(kd - ckd)) / np.max(np.abs(ckd))
    print(f"{name}: series vs closed form at v <= 0.25: K' {ek:.2e}, kdot {ekd:.2e}")
    assert ek < 1e-12 and ekd < 1e-12
    # the variances: the closed form at c = v1 = v2
    cv, _ = HO.closed_form(name, v1, v1, v1)
    assert np.max(np.abs(HO.var(v1, (name, 32, 96)) - cv)) < 1e-12 * np.max(np.abs(cv))


@pytest.mark.parametrize("name", HO.PHIS)
def test_derivative_coefficients_are_steins_identity(name):
    """a'_n(v) = a_{n+1}(v)·√(n+1)/√v, the coefficients of φ' formed from φ' directly against
    those of φ one order up.  At 256 nodes, where the rule is converged for every φ here, to
    1e-12 of max|a'_n|, the package's float64 tolerance: both sides are 256-term sums in
    double."""
    n = np.arange(ORDER + 1)
    for v in (0.05, 0.25, 1.0):
        a = HO.coefficients(v, (name, ORDER + 1, 256))
        da = HO.coefficients(v, (name, ORDER, 256), True)
        err = np.max(np.abs(da - a[1:] * np.sqrt(n + 1) / math.sqrt(v))) / np.max(np.abs(da))
        assert err < 1e-12, (name, v, err)


@pytest.mark.parametrize("name", HO.PHIS)
def test_series_is_symmetric_and_positive_semidefinite(name):
    rule = (name, 32, 96)
    c, v1, v2 = _draws(vmax=2.0)
    for a, b in zip(HO.series(c, v1, v2, rule), HO.series(c, v2, v1, rule)):
        assert np.array_equal(a, b)                          # bit for bit
    # the Gram matrix of 12 one-pixel images, a zero image and a duplicate among them
    rng = np.random.default_rng(11)
    x = rng.standard_normal((12, 5))
    x[3], x[7] = 0.0, x[2]
    cov = x @ x.T / 5
    cov = (cov + cov.T) / 2                                  # the BLAS product need not be
    v = np.diag(cov).copy()
    for fn in (0, 1):
        gram = HO.series(cov, v[:, None], v[None, :], rule)[fn]
        np.fill_diagonal(gram, (HO.var_kdot if fn else HO.var)(v, rule))
        assert np.array_equal(gram, gram.T)
        assert np.linalg.eigvalsh(gram).min() >= -1e-14 * np.trace(gram)
    # a zero-variance pixel: the series is φ(0)·a_0(v2) and φ'(0)·a'_0(v2), up to the rounding
    # of the weights' sum (a_0(0) = φ(0)·Σ w_q) and of the terms n >= 1 times ρ = 0
    k, kd = (float(t) for t in HO.series(np.float64(0.0), np.float64(0.0), np.float64(0.7), rule))
    want = float(HO.phi(name, 0.0) * HO.coefficients(0.7, rule)[0])
    wantd = float(HO.phi(name, 0.0, True) * HO.coefficients(0.7, rule, True)[0])
    assert abs(k - want) <= 1e-15 * abs(want) and abs(kd - wantd) <= 1e-15 * abs(wantd)


def small_net():
    return S(C(3, var_bias=0.2), m.Tanh(), m.Sum([S(), S(C(3, var_weight=1.5), m.SiLU(order=8),
                                                          C(3))]),
             m.Sigmoid(order=16, quad_nodes=64), C(6, padding=0)).double()


def test_oracle_walks_agree():
    """the layer walk, program.ntk_steps launch by launch and the walk on position-pair maps"""
    rng = np.random.default_rng(8)
    X, Z = rng.standard_normal((3, 2, 6, 6)), rng.standard_normal((2, 2, 6, 6))
    model = small_net()
    for args in ((X, Z, False, False), (X,)):
        k = HO.kernel(model, *args)
        ks, ths = HO.ntk_stepwise(model, *args)
        km, thm = HO.pool_ntk(model, *args)
        for got in (ks, km):
            assert np.max(np.abs(got - k)) < 1e-13 * np.max(np.abs(k))
        assert np.max(np.abs(thm - ths)) < 1e-13 * np.max(np.abs(ths))


# ------------------------------------------------------------------------------------
# the modules
# ------------------------------------------------------------------------------------
def test_exports_and_module_surface():
    for name in ("HermiteNonlin", "Tanh", "Sigmoid", "Softplus", "SiLU", "GeluTanh"):
        assert name in cnn_gp.__all__ and name in cnn_gp.kernels.__all__
    assert N.HERMITE_PHI == HO.PHI_ID
    for phi, cls in CLASSES.items():
        assert issubclass(cls, H) and issubclass(H, m.NNGPKernel)
        mod = cls()
        assert (mod.phi, mod.order, mod.quad_nodes) == (phi, 32, 96)
        assert mod.rule() == (HO.PHI_ID[phi], 32, 96) == H(phi).rule()
        assert cls(order=8, quad_nodes=40).rule() == (HO.PHI_ID[phi], 8, 40)
        assert mod.layers() == 0 and mod.extra_repr() == "order=32, quad_nodes=96"
    assert H("erf", 16, 64).rule() == (5, 16, 64) and H("gelu").rule() == (6, 32, 96)
    assert H("erf", 16).extra_repr() == "phi='erf', order=16, quad_nodes=96"
    assert S(C(3), m.Tanh(), C(4, padding=0)).layers() == 2
    # set_exact_relu is ignored: the same program either way
    model = S(C(3), m.Tanh(), C(4, padding=0))
    ops = lambda p: [(o.kind, o.rule) for o in p.pair_ops]                       # noqa: E731
    assert ops(model._plan(4, 4)) == ops(model.set_exact_relu(True)._plan(4, 4))


def test_bad_parameters_raise():
    for phi in ("relu", "Tanh", None, 0):
        with pytest.raises(ValueError, match="phi"):
            H(phi)
    for kw, word in ((dict(order=0), "0"), (dict(order=65), "65"), (dict(order=-3), "-3"),
                     (dict(order=2.0), "2.0"), (dict(order=True), "True"),
                     (dict(quad_nodes=32), "32"), (dict(quad_nodes=257), "257"),
                     (dict(order=64, quad_nodes=64), "64"), (dict(quad_nodes=96.0), "96.0"),
                     (dict(quad_nodes=None), "None")):
        with pytest.raises(ValueError) as e:
            m.Tanh(**kw)
        assert word in str(e.value), kw
    m.Tanh(order=1, quad_nodes=2), m.Tanh(order=64, quad_nodes=256)       # the ends are fine
    # an attribute assigned later is checked when it is used
    mod = S(C(3), m.SiLU(), C(4, padding=0))
    mod.mods[1].order = 65
    with pytest.raises(ValueError, match="65"):
        Plan(mod, 4, 4)
    with pytest.raises(ValueError, match="65"):
        mod._structure_key()
    bad = m.Tanh()
    bad.phi = "elu"
    with pytest.raises(ValueError, match="elu"):
        compile_program(S(bad), 4, 4)


def test_structure_key_carries_the_rule():
    build = lambda act: S(C(3), act, C(4, padding=0))                            # noqa: E731
    k1 = build(m.Tanh())._structure_key()
    assert ("hermite", 0, 32, 96) in k1
    assert k1 == build(H("tanh"))._structure_key() != build(m.Tanh(order=16))._structure_key()
    assert k1 != build(m.Sigmoid())._structure_key()
    model = build(m.Tanh())
    plan = model._plan(4, 4)
    assert model._plan(4, 4) is plan and plan.pair_ops[1].rule == (0, 32, 96)
    for attr, val, rule in (("order", 16, (0, 16, 96)), ("quad_nodes", 128, (0, 16, 128)),
                            ("phi", "silu", (3, 16, 128))):
        before = model._plan(4, 4)
        setattr(model.mods[1], attr, val)                   # through __setattr__: a new key
        after = model._plan(4, 4)
        assert after is not before and after.pair_ops[1].rule == rule
    model.mods[1].phi, model.mods[1].order, model.mods[1].quad_nodes = "tanh", 32, 96
    assert model._plan(4, 4) is plan                        # back: the first plan is reused


# ------------------------------------------------------------------------------------
# the lowering: one sequential model, one residual model, one pooled model
# ------------------------------------------------------------------------------------
def seq_net():
    return S(C(3), m.Tanh(), C(3), m.SiLU(order=16), C(4, padding=0))


def res_net():
    return S(C(3), m.Sum([S(), S(C(3), m.Sigmoid())]), C(4, padding=0))


def pooled_net():
    return S(C(3, var_bias=0.1), m.Tanh(), A(2), C(3), m.SiLU(), G(), C(1, var_weight=2.0))


def test_lowering_of_the_sequential_model():
    model = seq_net()
    prog, v0, vf = compile_program(model, 4, 4)
    assert [o.kind for o in prog.ops] == ["conv", "hermite", "conv", "hermite", "conv"]
    assert [o.rule for o in prog.ops if o.kind == "hermite"] == [(0, 32, 96), (3, 16, 96)]
    assert prog.ops[0].rule is None and prog.ops[1].consts is None and prog.ops[1].smh is None
    plan = Plan(model, 4, 4)
    assert [(o.kind, o.pre, o.post) for o in plan.pair_ops] == [
        ("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_NONE), ("hermite", N.CGP_PRE_NONE, N.CGP_POST_NONE),
        ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE), ("hermite", N.CGP_PRE_NONE, N.CGP_POST_NONE),
        ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]
    srcs = {o.src for o in plan.pair_ops if o.kind == "hermite"}
    assert plan.need_var == srcs == plan.ntk_need_var() and plan.pool is None
    assert [s.fn for s in plan.layer_list()[0]] == ["conv", "hermite", "conv", "hermite", "conv"]
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["conv", "hermite_ntk", "conv", "conv", "hermite_ntk", "conv",
                                     "conv"]
    assert steps[1].theta == steps[1].src == steps[0].dst and steps[1].var == steps[0].dst[1]
    assert steps[1].dst_theta == ("T", steps[1].op.dst) and steps[3].src == steps[1].dst_theta
    assert kbuf == ("K", vf) and tbuf == ("T", vf)
    # before any conv Θ = 0: the forward-only launch
    prog2, v0, vf = compile_program(S(m.Tanh(), C(4, padding=0)), 4, 4)
    steps2, kbuf, tbuf = ntk_steps(prog2, v0, vf)
    assert [s.fn for s in steps2] == ["hermite", "conv"]
    assert steps2[0].theta is None and steps2[0].dst_theta is None and tbuf == ("K", vf)
    # the buffer lifetimes: the same reads and writes as the erf twin's
    twin = ntk_steps(*compile_program(S(C(3), m.Erf(), C(3), m.Erf(), C(4, padding=0)), 4, 4))[0]
    assert [(s.reads(), s.writes()) for s in steps] == [(s.reads(), s.writes()) for s in twin]
    # on position-pair maps (position_covariance / ntk_maps of a model without a pool)
    bs = pool_steps(prog, *compile_program(model, 4, 4)[1:], body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "hermite", "conv", "hermite", "conv"]
    ns = pool_ntk_steps(prog, *compile_program(model, 4, 4)[1:], body=True)
    assert [s.fn for s in ns.steps] == ["moments", "conv", "hermite_ntk", "conv_ntk",
                                        "hermite_ntk", "conv_ntk"]
    assert all(s.post == N.CGP_COV_NONE for s in ns.steps)  # never a conv's post-stage
    assert ns.steps[2].theta == ns.steps[2].src             # Θ is K's buffer after the first conv


def test_lowering_of_the_residual_model():
    plan = Plan(res_net(), 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "conv", "hermite", "add", "conv"]
    # rule 2: the identity skip becomes the addend of the block's last op
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "hermite", "conv"]
    op = plan.pair_ops[2]
    assert op.addend == plan.pair_ops[0].dst and op.rule == (1, 32, 96)
    steps, kbuf, tbuf = ntk_steps(plan.prog, plan.v0, plan.vf)
    assert [s.fn for s in steps] == ["conv", "conv", "conv", "hermite_ntk", "axpby", "axpby",
                                     "conv", "conv"]
    bs = pool_steps(plan.prog, plan.v0, plan.vf, body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "conv", "hermite", "conv"]
    assert bs.steps[3].addend == bs.steps[1].dst and bs.self_var == frozenset()
    ns = pool_ntk_steps(plan.prog, plan.v0, plan.vf, body=True)
    assert [s.fn for s in ns.steps] == ["moments", "conv", "conv_ntk", "hermite_ntk", "conv_ntk"]
    st = ns.steps[3]
    # both addends ride on the launch: K of the skip, and its Θ (the first conv's K buffer)
    assert st.addend == ("K", bs.steps[1].dst) and st.addend_theta == ("K", bs.steps[1].dst)
    assert st.dst_theta == ("T", st.dst[1]) and st.var == bs.steps[3].var


def test_lowering_of_the_pooled_model():
    """upstream and downstream of an AvgPool2d: each a launch of its own, counted in need_var
    like a nonlinearity, the one downstream in self_var"""
    plan = Plan(pooled_net(), 4, 4)
    ps = plan.pool
    assert [o.kind for o in plan.prog.ops] == ["conv", "hermite", "avgpool", "conv", "hermite",
                                               "pool", "conv"]
    v = [o.dst for o in plan.prog.ops]
    assert [s.fn for s in ps.steps] == ["moments", "conv", "hermite", "avgpool", "conv",
                                        "hermite", "pool", "conv"]
    g1, g2 = ps.steps[2], ps.steps[5]
    assert (g1.src, g1.var, g1.dst, g1.addend) == (v[0], v[0], v[1], None)
    assert (g2.src, g2.var, g2.dst, g2.addend) == (v[3], v[3], v[4], None)
    assert g1.op.rule == (0, 32, 96) and g2.op.rule == (3, 32, 96)
    assert ps.need_var == {v[0], v[3]} and ps.self_var == {v[3]} and ps.self_last == 4
    assert plan.need_var == {v[0], v[3]} == plan.ntk_need_var()
    for fused in (True, False):
        ns = plan.pool_ntk(False, fused, 8)
        conv2 = ["conv_ntk"] if fused else ["conv", "conv"]
        assert [s.fn for s in ns.steps] == ["moments", "conv", "hermite_ntk", "avgpool",
                                            "avgpool"] + conv2 + ["hermite_ntk", "pool", "pool"] \
            + conv2
        assert all(s.post == N.CGP_COV_NONE for s in ns.steps)
        a2 = [s for s in ns.steps if s.fn == "hermite_ntk"][1]
        assert a2.theta == ("T", v[3]) and a2.dst_theta == ("T", v[4]) and a2.var == v[3]
    # Θ = None upstream: the forward-only launch of the same entry point
    ns = pool_ntk_steps(*compile_program(S(m.Tanh(), C(3), G(), C(1)), 4, 4))
    assert [s.fn for s in ns.steps][:3] == ["moments", "hermite", "conv"]


def test_a_model_without_the_modules_compiles_to_the_same_program():
    model = S(C(3), R(), m.Sum([S(), S(C(3), m.Erf())]), m.Gelu(), C(3), m.Sin(), C(4, padding=0))
    plan = Plan(model, 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "relu", "conv", "erf", "add", "gelu",
                                               "conv", "sin", "conv"]
    assert all(o.rule is None for o in plan.prog.ops)
    assert not any("hermite" in s.fn for s in ntk_steps(plan.prog, plan.v0, plan.vf)[0])
    assert P.NONLIN_KINDS[-1] == "hermite" and P.NONLIN_CALLS["hermite"][:4] == \
        (N.HermiteArgs, "out_xy", False, None)
    assert P.NONLIN_CALLS["hermite"][4](Plan(seq_net(), 4, 4).prog.ops[1]) == (0, 32, 96)


def test_after_the_global_pool_is_rejected():
    for act in CLASSES.values():
        with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
            Plan(S(C(3), m.Tanh(), G(), act()), 4, 4)
        assert str(e.value) == P.HERMITE_RULE_GLOBAL
    assert "HermiteNonlin" in P.HERMITE_RULE_GLOBAL
    assert P.POOL_RULES["hermite"] == P.HERMITE_RULE_GLOBAL
    assert P.HERMITE_RULE_GLOBAL not in (P.GELU_RULE_GLOBAL, P.ABRELU_RULE_GLOBAL,
                                         P.SIN_RULE_GLOBAL, P.POOL_RULE_NONLIN)
    with pytest.raises(NotImplementedError) as e:
        pool_ntk_steps(*compile_program(S(C(3), G(), H("erf")), 4, 4))
    assert str(e.value) == P.HERMITE_RULE_GLOBAL
    # the other rules hold with the module in the model
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), m.Tanh(), G(), R()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN
    with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
        S(C(3), m.Tanh(), G()).ntk(torch.ones(2, 1, 4, 4))
    assert str(e.value) == P.POOL_RULE_NTK


def test_models_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(C(3), m.Tanh(), C(4, padding=0)).double()
    plan = model._plan(4, 4)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    # at a geometry the whole-network kernel has (the reference ConvNet's), the op is the reason
    big = S(C(3), m.SiLU(), C(28, padding=0)).double()
    with pytest.raises(Unsupported) as e:
        NetPlan(big._plan(28, 28), 8)
    assert str(e.value) == "op hermite"
    # the variance chain has no record for it: it declines instead of raising
    assert plan._var_chain({plan.vf}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {f"cgp_{stem}{end}" for stem in ("hermite_coef", "hermite", "hermite_cov")
               for end in ("_args_size", "_f64", "_f32")} | \
    {"cgp_var_hermite_f64", "cgp_var_hermite_f32"}


def test_abi_and_symbols():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    assert lib.cgp_hermite_coef_args_size() == ctypes.sizeof(N.HermiteCoefArgs) == 56
    assert lib.cgp_hermite_args_size() == ctypes.sizeof(N.HermiteArgs) == \
        ctypes.sizeof(N.ErfArgs) + 56
    assert lib.cgp_hermite_cov_args_size() == ctypes.sizeof(N.HermiteCovArgs) == \
        ctypes.sizeof(N.SinCovArgs) + 24
    tables = ["ax", "ay", "dax", "day", "stride_x", "stride_y", "order", "reserved"]
    assert [f[0] for f in N.HermiteArgs._fields_] == [f[0] for f in N.ErfArgs._fields_] + tables
    assert [f[0] for f in N.HermiteCovArgs._fields_] == \
        [f[0] for f in N.SinCovArgs._fields_][:-4] + tables
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    syms = set(re.findall(r"\b(cgp_(?:var_)?hermite_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if re.match(r"cgp_(var_)?hermite_", s)}
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    for name in ("cgp_hermite_coef_args", "cgp_hermite_args", "cgp_hermite_cov_args"):
        assert f"typedef struct {name}" in txt
    for name, k in HO.PHI_ID.items():
        assert f"#define CGP_HERMITE_{name.upper()} {k}\n" in txt
    assert f"#define CGP_HERMITE_MAX_ORDER {N.CGP_HERMITE_MAX_ORDER}\n" in txt
    assert f"#define CGP_HERMITE_MAX_NODES {N.CGP_HERMITE_MAX_NODES}\n" in txt
    assert "#define CGP_ABI_VERSION 12" in txt


def coef_args(**kw):
    a = N.HermiteCoefArgs()
    a.var, a.a, a.nodes, a.count = 64, 128, 192, 12
    a.phi, a.order, a.nq = 0, 32, 96
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# rules the entry points refuse: (fields, the message)
BAD_RULES = [(dict(phi=-1), b"phi"), (dict(phi=7), b"phi"), (dict(order=0), b"order"),
             (dict(order=65), b"order"), (dict(nq=32), b"nodes"), (dict(nq=257), b"nodes"),
             (dict(nodes=None), b"NULL node table")]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_hermite_coef_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_hermite_coef_{sfx}")
    assert fn(None, None) == 1001
    for field in ("var", "a"):
        assert fn(ctypes.byref(coef_args(**{field: None})), None) == 1001, field
        assert b"hermite_coef" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    for count in (0, -1, 1 << 31):
        assert fn(ctypes.byref(coef_args(count=count)), None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    for kw, msg in BAD_RULES:
        assert fn(ctypes.byref(coef_args(**kw)), None) == 1001, kw
        assert msg in lib.cgp_last_error(), kw


def hermite_args(**kw):
    a = N.HermiteArgs()
    a.xy, a.theta, a.out_xy, a.out_theta, a.xx, a.yy = 64, 128, 192, 256, 320, 384
    a.nmaps, a.n1, a.n2, a.hw = 6, 3, 2, 4
    a.ax, a.ay, a.dax, a.day, a.stride_x, a.stride_y, a.order = 512, 1024, 2048, 4096, 12, 8, 32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# tables the walks refuse
BAD_TABLES = [(dict(order=0), b"order"), (dict(order=65), b"order"), (dict(ax=None), b"table"),
              (dict(ay=None), b"table"), (dict(dax=None), b"table"), (dict(day=None), b"table")]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_hermite_rejects_bad_arguments_on_host(sfx):
    """cgp_erf_*'s checks, and last the tables (so every call below that reaches them has valid
    maps and sizes)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_hermite_{sfx}")
    args = hermite_args
    assert fn(None, None) == 1001
    for field in ("xy", "out_xy", "out_theta", "xx", "yy"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"hermite" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(nmaps=5)), None) == 1001
    assert b"nmaps inconsistent" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(same=1)), None) == 1001           # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(hw=2049)), None) == 1001          # larger than one chunk
    assert b"too large" in lib.cgp_last_error()
    for kw, msg in BAD_TABLES + [(dict(stride_x=11), b"stride"), (dict(stride_y=7), b"stride")]:
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert msg in lib.cgp_last_error(), kw
    # the forward-only pass needs no table of φ'
    assert fn(ctypes.byref(args(theta=None, dax=None, day=None, order=65)), None) == 1001
    assert b"order" in lib.cgp_last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_var_hermite_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_var_hermite_{sfx}")
    rule = (0, 32, 96, 512)
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] = None
        assert fn(p[0], p[1], 2, 2, 4, 0, *rule, p[2], p[3], None) == 1001
        assert b"var_hermite" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    assert fn(64, 128, 2, 3, 4, 1, *rule, 192, 256, None) == 1001  # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    for n1, n2, hw in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4), (1 << 29, 2, 4)):
        assert fn(64, 128, n1, n2, hw, 0, *rule, 192, 256, None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    for kw, msg in BAD_RULES:
        r = {**dict(phi=0, order=32, nq=96, nodes=512), **kw}
        assert fn(64, 128, 2, 2, 4, 0, r["phi"], r["order"], r["nq"], r["nodes"], 192, 256,
                  None) == 1001, kw
        assert msg in lib.cgp_last_error(), kw


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_hermite_cov_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_hermite_cov_{sfx}")

    def args(**kw):
        a = N.HermiteCovArgs()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        a.npairs, a.h, a.w = 3, 4, 4
        a.ax, a.ay, a.stride_x, a.stride_y, a.order = 512, 1024, 48, 32, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert fn(None, None) == 1001
    for field in ("in_", "out", "xx", "yy", "pair_i", "pair_j"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"hermite_cov" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    # with theta the second output is needed, is a buffer of its own, and so are the tables of φ'
    assert fn(ctypes.byref(args(theta=512)), None) == 1001
    assert b"NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(theta=512, out_theta=128)), None) == 1001
    assert b"one buffer" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(theta=512, out_theta=640)), None) == 1001
    assert b"table" in lib.cgp_last_error()
    for kw in (dict(npairs=0), dict(npairs=1 << 31), dict(h=0), dict(w=-4), dict(h=182, w=182)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert b"bad sizes" in lib.cgp_last_error()
    for kw, msg in BAD_TABLES[:4] + [(dict(stride_x=15), b"stride"), (dict(stride_y=0), b"stride")]:
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert msg in lib.cgp_last_error(), kw


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_model_without_gpu_raises_like_relu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device") as relu:
        S(C(3), R(), C(4, padding=0))(x)
    with pytest.raises(RuntimeError, match="HIP device") as got:
        seq_net()(x)
    assert str(got.value) == str(relu.value)
    with pytest.raises(RuntimeError, match="HIP device"):
        seq_net().ntk(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        pooled_net()(x)


def test_model_empty_batches():
    model = seq_net()
    x0, x = torch.zeros(0, 1, 4, 4), torch.ones(3, 1, 4, 4)
    assert tuple(model(x0).shape) == (0, 0)
    assert tuple(model(x0, x, False).shape) == (0, 3)
    assert tuple(model(x0, x0, True, True).shape) == (0,)
    k, th = model.ntk(x0, x, False, return_nngp=True)
    assert tuple(k.shape) == tuple(th.shape) == (0, 3)
