"""CPU-only tests of the two-slope ReLU (cnn_gp.ABReLU / cnn_gp.LeakyReLU): the closed forms
against a piecewise Gauss-Legendre angular integral, the test-time oracle against the ReLU
oracle, the identity and autograd, the lowering (program, fusion, NTK steps, both launch lists
on position-pair maps, the whole-network path declining), the plan-cache key, and the host
side of cgp_abrelu_* / cgp_var_abrelu_* / cgp_abrelu_cov_*."""
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
import abrelu_oracle as AB
import erf_oracle as EO

m = cnn_gp
S, C, R, G, A, AR, LR = (m.Sequential, m.Conv2d, m.ReLU, m.GlobalAvgPool, m.AvgPool2d, m.ABReLU,
                         m.LeakyReLU)

SLOPES = [(0.01, 1.0), (0.2, 1.0), (-1.0, 1.0), (1.0, 1.0), (0.0, 1.0), (-0.5, 2.0)]


# ------------------------------------------------------------------------------------
# the formulas
# ------------------------------------------------------------------------------------
GL_X, GL_W = np.polynomial.legendre.leggauss(12)


def _angular(a, b, v1, v2, rho):
    """E[φ(u1)φ(u2)] = √(v1 v2)/π · ∫₀^{2π} f(cos φ)·f(cos(φ − θ)) dφ and E[φ'(u1)φ'(u2)] =
    (1/2π)·∫ f'(cos φ)·f'(cos(φ − θ)) dφ with f the two-slope function: u = r·√v·cos(angle)
    with r² chi-squared of 2 degrees (E r² = 2) and a uniform angle.  Split at the four
    kinks, 12-point Gauss-Legendre on each piece (the integrand is a trigonometric polynomial
    of degree 2 there)."""
    theta = math.acos(max(-1.0, min(1.0, rho)))
    f = lambda x: np.where(x < 0, a * x, b * x)                                 # noqa: E731
    df = lambda x: np.where(x < 0, a, b)                                        # noqa: E731
    kinks = sorted({0.0, 2 * math.pi, math.pi / 2, 3 * math.pi / 2,
                    (theta + math.pi / 2) % (2 * math.pi),
                    (theta + 3 * math.pi / 2) % (2 * math.pi)})
    k = kd = 0.0
    for lo, hi in zip(kinks[:-1], kinks[1:]):
        ph = (hi + lo) / 2 + (hi - lo) / 2 * GL_X
        w = (hi - lo) / 2 * GL_W
        k += float(np.sum(w * f(np.cos(ph)) * f(np.cos(ph - theta))))
        kd += float(np.sum(w * df(np.cos(ph)) * df(np.cos(ph - theta))))
    return math.sqrt(v1 * v2) / math.pi * k, kd / (2 * math.pi)


def quad_points():
    """(v1, v2, rho): v <= 3, with ρ = ±1, 0 and −0.999, then random ones"""
    pts = [(1.0, 1.0, 1.0), (3.0, 0.2, 1.0), (2.0, 2.0, -1.0), (0.3, 3.0, -1.0),
           (1.0, 0.7, 0.0), (3.0, 3.0, 0.0), (3.0, 3.0, -0.999), (0.5, 2.5, -0.999),
           (0.05, 0.05, 0.999)]
    rng = np.random.default_rng(11)
    pts += [(3 * (1 - rng.random()), 3 * (1 - rng.random()), rng.uniform(-1, 1))
            for _ in range(40)]
    return pts


@pytest.mark.parametrize("ab", SLOPES, ids=lambda s: f"{s[0]}_{s[1]}")
def test_closed_form_matches_the_angular_integral(ab):
    """K' and κ̇ of the oracle (and so of the contract: s·R + m·c, s·k + m) against the angular
    integral, which shares no code with them.  Bound 1e-13 relative to h·√(v1 v2), the value
    at θ = 0; a run over 200 random points per slope pair measured 9e-16 for both.  Measured here: at most
    1.4e-15 (K') and 1.7e-15 (κ̇), at (−1, 1)."""
    a, b = ab
    h = (a * a + b * b) / 2
    worst_k = worst_kd = 0.0
    for v1, v2, rho in quad_points():
        c = rho * math.sqrt(v1 * v2)
        k, kd = AB.abrelu_pair(np.float64(c), np.float64(v1), np.float64(v2), a, b)
        ik, ikd = _angular(a, b, v1, v2, rho)
        worst_k = max(worst_k, abs(float(k) - ik) / (h * math.sqrt(v1 * v2)))
        worst_kd = max(worst_kd, abs(float(kd) - ikd) / h)
    print(f"closed form vs angular integral ({a}, {b}): K' {worst_k:.2e}, kdot {worst_kd:.2e}")
    assert worst_k < 1e-13 and worst_kd < 1e-13


def test_contract_lines_are_the_theta_form():
    """the constants the kernels take: (s, m, h) of a module, and K' = s·R + m·c, κ̇ = s·k + m
    with R and k the ReLU's own"""
    for a, b in SLOPES:
        s, mm, h = AR(a, b).constants()
        assert (s, mm, h) == ((a - b) * (a - b), a * b, (a * a + b * b) / 2)
    assert AR(0, 1).constants() == (1.0, 0.0, 0.5) and AR(1, 1).constants() == (0.0, 1.0, 1.0)
    rng = np.random.default_rng(2)
    v1, v2 = 3 * (1 - rng.random(200)), 3 * (1 - rng.random(200))
    c = rng.uniform(-1, 1, 200) * np.sqrt(v1 * v2)
    r, k = AB.abrelu_pair(c, v1, v2, 0.0, 1.0)
    for a, b in SLOPES:
        s, mm, h = AR(a, b).constants()
        kk, kd = AB.abrelu_pair(c, v1, v2, a, b)
        assert np.max(np.abs(kk - (s * r + mm * c))) < 1e-15 * h * 3
        assert np.max(np.abs(kd - (s * k + mm))) < 1e-15 * h * 3
        # κ̇ = ∂K'/∂c at fixed variances
        ct = torch.from_numpy(c * 0.98).requires_grad_()
        kt, kdt = AB.abrelu_pair(ct, torch.from_numpy(v1), torch.from_numpy(v2), a, b)
        g, = torch.autograd.grad(kt.sum(), ct)
        assert float((g - kdt.detach()).abs().max()) < 1e-13 * max(h, 1)
    # the tolerance factor: 1 for ab >= 0, at most 3
    assert [AB.tol_factor(a, b) for a, b in SLOPES[:2]] == [1.0, 1.0]
    assert AB.tol_factor(-1, 1) == 3.0 and AB.tol_factor(1, 1) == 1.0
    assert 1.0 < AB.tol_factor(-0.5, 2.0) <= 3.0


# ------------------------------------------------------------------------------------
# the oracle against the ReLU oracle, the identity and autograd
# ------------------------------------------------------------------------------------
def small_net(act, side=6):
    return S(C(3, var_bias=0.2), act(), m.Sum([S(), S(C(3, var_weight=1.5), act(), C(3))]),
             act(), C(side, padding=0)).double()


def images(seed=3, side=6, signed=True):
    rng = np.random.default_rng(seed)
    draw = (lambda n: rng.standard_normal((n, 8, side, side))) if signed else \
        (lambda n: rng.random((n, 8, side, side)))
    return draw(4), draw(3)


def max_err(got, ref):
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(ref))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def test_oracle_at_0_1_is_the_relu_oracle():
    X, Z = images()
    for args in ((X,), (X, Z, False, False), (X, X, True, True), (X[:3], Z, False, True)):
        got = AB.kernel(small_net(lambda: AR(0, 1)), *args)
        want = EO.kernel(small_net(R), *args)                # torch_cpu's _relu
        assert max_err(got, want) < 1e-14
    # and the NTK recursion: κ̇ = k, the override 1/2
    k, th = AB.ntk_stepwise(small_net(lambda: AR(0, 1)), X)
    rk, rth = AB.ntk_stepwise(small_net(R), X)
    assert max_err(k, rk) < 1e-14 and max_err(th, rth) < 1e-14


def test_oracle_at_1_1_is_the_identity():
    X, Z = images()
    lin = S(C(3, var_bias=0.2), m.Sum([S(), S(C(3, var_weight=1.5), C(3))]),
            C(6, padding=0)).double()
    for args in ((X,), (X, Z, False, False), (X, X, True, True)):
        assert max_err(AB.kernel(small_net(lambda: AR(1, 1)), *args),
                       EO.kernel(lin, *args)) < 1e-14
    k, th = AB.ntk_stepwise(small_net(lambda: AR(1, 1)), X, Z, False, False)
    lk, lth = AB.ntk_stepwise(lin, X, Z, False, False)
    assert max_err(k, lk) < 1e-14 and max_err(th, lth) < 1e-14
    c = np.linspace(-1, 1, 9)
    kk, kd = AB.abrelu_pair(c, np.ones(9), np.ones(9), 1.0, 1.0)
    assert np.array_equal(kk, c) and np.array_equal(kd, np.ones(9))


@pytest.mark.parametrize("ab", SLOPES, ids=lambda s: f"{s[0]}_{s[1]}")
def test_oracle_autograd_matches_stepwise(ab):
    """same=False pairs of independent images: |ρ| stays well inside 0.98 at every pixel of
    every layer (asserted on the input moments, the least mixed layer)"""
    model = small_net(lambda: AR(*ab))
    X, Z = images()
    xy, xx, yy = EO._moments(*EO._inputs(X, Z, False)[:2], False)
    rho = xy.view(4, 3, 6, 6) / torch.sqrt(xx.view(4, 1, 6, 6) * yy.view(1, 3, 6, 6))
    assert float(rho.abs().max()) <= 0.98
    k, th = AB.ntk_autograd(model, X, Z)
    sk, sth = AB.ntk_stepwise(model, X, Z, False, False)
    assert max_err(k, sk) < 1e-12 and max_err(th, sth) < 1e-12
    assert max_err(AB.kernel(model, X, Z, False, False), sk) < 1e-12


def test_pooled_oracle_matches_the_layer_oracle():
    """a dense readout reads the p = p entries only: the walk on position-pair maps and the
    layer walk are two routes to one K and one Θ"""
    body = lambda: [C(3, var_bias=0.1), LR(0.2), C(3, var_weight=1.5), AR(-0.5, 2)]   # noqa
    X, Z = images(side=4)
    head = C(4, padding=0, var_bias=0.2)
    full = S(*body(), head).double()
    for args in ((X, Z, False, False), (X,)):
        want_k, want_t = AB.ntk_stepwise(full, *args)
        got_k, got_t = AB.pool_ntk(full, *args)
        assert max_err(got_k, want_k) < 1e-13 and max_err(got_t, want_t) < 1e-13
    s, t = AB.position_ntk(S(*body()).double(), X, Z, False)
    got = head.var_weight / 16 * np.einsum("ijabab->ij", s) + head.var_bias
    assert max_err(got, AB.kernel(full, X, Z, False, False)) < 1e-13


# ------------------------------------------------------------------------------------
# the package surface
# ------------------------------------------------------------------------------------
def test_modules_are_exported():
    for name in ("ABReLU", "LeakyReLU"):
        assert name in cnn_gp.__all__ and name in cnn_gp.kernels.__all__
    assert issubclass(AR, cnn_gp.NNGPKernel) and issubclass(LR, AR)
    assert AR(0.3, 2).layers() == 0 and LR().layers() == 0
    lr = LR()
    assert (lr.a, lr.b, lr.negative_slope) == (0.01, 1.0, 0.01)
    assert type(lr.a) is float and type(AR(1, 2).b) is float
    assert LR(0.2).extra_repr() == "negative_slope=0.2" and "0.2" in repr(LR(0.2))
    assert AR(-1, 1).extra_repr() == "a=-1.0, b=1.0"
    assert S(C(3), LR(), C(4, padding=0)).layers() == 2


def test_bad_slopes_raise():
    for a, b in ((float("nan"), 1), (1, float("inf")), (float("-inf"), 0), (0, 0), (0.0, -0.0)):
        with pytest.raises(ValueError):
            AR(a, b)
    for s in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            LR(s)
    LR(0.0)                                                 # the ReLU itself is fine
    # a slope assigned later is checked when the program is compiled
    mod = S(C(3), LR(0.1), C(4, padding=0))
    mod.mods[1].negative_slope = float("nan")
    with pytest.raises(ValueError):
        Plan(mod, 4, 4)
    bad = AR(0, 1)
    bad.b = 0.0
    with pytest.raises(ValueError):
        compile_program(S(bad), 4, 4)


def test_structure_key_carries_the_slopes():
    k1 = S(C(3), LR(0.1), C(4, padding=0))._structure_key()
    k2 = S(C(3), LR(0.2), C(4, padding=0))._structure_key()
    assert k1 != k2 and k1 == S(C(3), LR(0.1), C(4, padding=0))._structure_key()
    assert S(C(3), AR(0.1, 1), C(4, padding=0))._structure_key() == k1     # the same program
    assert S(C(3), AR(0.1, 2), C(4, padding=0))._structure_key() != k1
    model = S(C(3), LR(0.1), C(4, padding=0))
    plan = model._plan(4, 4)
    assert model._plan(4, 4) is plan and plan.pair_ops[1].slopes == (0.1, 1.0)
    model.mods[1].negative_slope = 0.2                      # through __setattr__: a new key
    assert model._structure_key() == k2
    plan2 = model._plan(4, 4)
    assert plan2 is not plan and plan2.pair_ops[1].slopes == (0.2, 1.0)
    assert plan2.pair_ops[1].smh == LR(0.2).constants()
    model.mods[1].b = 3.0
    assert model._plan(4, 4).pair_ops[1].slopes == (0.2, 3.0)
    model.mods[1].a, model.mods[1].b = 0.1, 1.0             # back: the first plan is reused
    assert model._plan(4, 4) is plan


# ------------------------------------------------------------------------------------
# the lowering: one sequential model, one residual model, one pooled model
# ------------------------------------------------------------------------------------
def seq_net():
    return S(C(3), LR(0.2), C(3), LR(), C(4, padding=0))


def res_net():
    return S(C(3), m.Sum([S(), S(C(3), AR(-1, 1))]), C(4, padding=0))


def pooled_net():
    return S(C(3), LR(0.2), A(2), C(3, var_bias=0.1), AR(-1, 1), G(), C(1))


def test_lowering_of_the_sequential_model():
    model = seq_net()
    prog, v0, vf = compile_program(model, 4, 4)
    assert [o.kind for o in prog.ops] == ["conv", "abrelu", "conv", "abrelu", "conv"]
    assert [o.slopes for o in prog.ops if o.kind == "abrelu"] == [(0.2, 1.0), (0.01, 1.0)]
    assert prog.ops[1].smh == LR(0.2).constants() and prog.ops[0].smh is None
    plan = Plan(model, 4, 4)
    assert [(o.kind, o.pre, o.post) for o in plan.pair_ops] == [
        ("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_NONE), ("abrelu", N.CGP_PRE_NONE, N.CGP_POST_NONE),
        ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE), ("abrelu", N.CGP_PRE_NONE, N.CGP_POST_NONE),
        ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]
    srcs = {o.src for o in plan.pair_ops if o.kind == "abrelu"}
    assert plan.need_var == srcs == plan.ntk_need_var() and plan.pool is None
    assert [o.kind for o in Plan(model, 4, 4, enable_fusion=False).pair_ops] == \
        [o.kind for o in prog.ops]
    # NTK: Θ of the first conv's output is its K' buffer, so the first op already carries Θ
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["conv", "abrelu_ntk", "conv", "conv", "abrelu_ntk", "conv",
                                     "conv"]
    assert steps[1].theta == steps[1].src == steps[0].dst and steps[1].var == steps[0].dst[1]
    assert steps[1].dst_theta == ("T", steps[1].op.dst) and steps[3].src == steps[1].dst_theta
    assert kbuf == ("K", vf) and tbuf == ("T", vf)
    # before any conv Θ = 0: the forward-only launch
    prog2, v0, vf = compile_program(S(LR(), C(4, padding=0)), 4, 4)
    steps2, kbuf, tbuf = ntk_steps(prog2, v0, vf)
    assert [s.fn for s in steps2] == ["abrelu", "conv"]
    assert steps2[0].theta is None and steps2[0].dst_theta is None and tbuf == ("K", vf)
    # the erf steps' buffer lifetimes: the same reads and writes as the erf twin's
    twin = ntk_steps(*compile_program(S(C(3), m.Erf(), C(3), m.Erf(), C(4, padding=0)), 4, 4))[0]
    assert [(s.reads(), s.writes()) for s in steps] == [(s.reads(), s.writes()) for s in twin]
    # on position-pair maps (position_covariance / ntk_maps of a model without a pool)
    bs = pool_steps(prog, *compile_program(model, 4, 4)[1:], body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "abrelu", "conv", "abrelu", "conv"]
    ns = pool_ntk_steps(prog, *compile_program(model, 4, 4)[1:], body=True)
    assert [s.fn for s in ns.steps] == ["moments", "conv", "abrelu_ntk", "conv_ntk", "abrelu_ntk",
                                        "conv_ntk"]
    assert all(s.post == N.CGP_COV_NONE for s in ns.steps)  # never a conv's post-stage
    assert ns.steps[2].theta == ns.steps[2].src             # Θ is K's buffer after the first conv


def test_lowering_of_the_residual_model():
    model = res_net()
    plan = Plan(model, 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "conv", "abrelu", "add", "conv"]
    # rule 2: the identity skip becomes the addend of the block's last op
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "abrelu", "conv"]
    ab = plan.pair_ops[2]
    assert ab.addend == plan.pair_ops[0].dst and ab.slopes == (-1.0, 1.0)
    assert ab.smh == (4.0, -1.0, 1.0)
    steps, kbuf, tbuf = ntk_steps(plan.prog, plan.v0, plan.vf)
    assert [s.fn for s in steps] == ["conv", "conv", "conv", "abrelu_ntk", "axpby", "axpby",
                                     "conv", "conv"]
    bs = pool_steps(plan.prog, plan.v0, plan.vf, body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "conv", "abrelu", "conv"]
    assert bs.steps[3].addend == bs.steps[1].dst and bs.self_var == frozenset()
    ns = pool_ntk_steps(plan.prog, plan.v0, plan.vf, body=True)
    assert [s.fn for s in ns.steps] == ["moments", "conv", "conv_ntk", "abrelu_ntk", "conv_ntk"]
    st = ns.steps[3]
    # both addends ride on the launch: K of the skip, and its Θ (the first conv's K buffer)
    assert st.addend == ("K", bs.steps[1].dst) and st.addend_theta == ("K", bs.steps[1].dst)
    assert st.dst_theta == ("T", st.dst[1]) and st.var == bs.steps[3].var


def test_lowering_of_the_pooled_model():
    """upstream and downstream of an AvgPool2d: each a launch of its own, counted in need_var
    like a nonlinearity, the one downstream in self_var"""
    plan = Plan(pooled_net(), 4, 4)
    ps = plan.pool
    assert [o.kind for o in plan.prog.ops] == ["conv", "abrelu", "avgpool", "conv", "abrelu",
                                               "pool", "conv"]
    v = [o.dst for o in plan.prog.ops]
    assert [s.fn for s in ps.steps] == ["moments", "conv", "abrelu", "avgpool", "conv", "abrelu",
                                        "pool", "conv"]
    g1, g2 = ps.steps[2], ps.steps[5]
    assert (g1.src, g1.var, g1.dst, g1.addend) == (v[0], v[0], v[1], None)
    assert (g2.src, g2.var, g2.dst, g2.addend) == (v[3], v[3], v[4], None)
    assert g1.op.slopes == (0.2, 1.0) and g2.op.slopes == (-1.0, 1.0)
    assert ps.need_var == {v[0], v[3]} and ps.self_var == {v[3]} and ps.self_last == 4
    assert ps.avgpooled == set(v[2:]) and ps.pooled == set(v[5:])
    assert ps.maps == {plan.v0} | set(v[:5]) and ps.scalars == set(v[5:])
    # the variance pipeline stops at the AvgPool2d; the NTK's needed variances are the same
    assert plan.need_var == {v[0], v[3]} == plan.ntk_need_var()
    for fused in (True, False):
        ns = plan.pool_ntk(False, fused, 8)
        conv2 = ["conv_ntk"] if fused else ["conv", "conv"]
        assert [s.fn for s in ns.steps] == ["moments", "conv", "abrelu_ntk", "avgpool", "avgpool"] \
            + conv2 + ["abrelu_ntk", "pool", "pool"] + conv2
        assert all(s.post == N.CGP_COV_NONE for s in ns.steps)
        a2 = [s for s in ns.steps if s.fn == "abrelu_ntk"][1]
        assert a2.theta == ("T", v[3]) and a2.dst_theta == ("T", v[4]) and a2.var == v[3]
    # Θ = None upstream: the forward-only launch of the same entry point
    ns = pool_ntk_steps(*compile_program(S(LR(), C(3), G(), C(1)), 4, 4))
    assert [s.fn for s in ns.steps][:3] == ["moments", "abrelu", "conv"]
    # a ReLU twin keeps its launch lists: no abrelu step appears without the module
    twin = Plan(S(C(3), R(), A(2), C(3, var_bias=0.1), R(), G(), C(1)), 4, 4)
    assert [s.fn for s in twin.pool.steps] == ["moments", "conv", "avgpool", "conv", "nonlin",
                                               "pool", "conv"]
    assert not any("abrelu" in s.fn for s in twin.pool_ntk(False, True, 8).steps)


def test_a_model_without_the_modules_compiles_to_the_same_program():
    model = S(C(3), R(), m.Sum([S(), S(C(3), m.Erf())]), m.Gelu(), C(4, padding=0))
    plan = Plan(model, 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "relu", "conv", "erf", "add", "gelu", "conv"]
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "erf", "gelu", "conv"]
    assert all(o.slopes is None and o.smh is None for o in plan.prog.ops)
    steps, _, _ = ntk_steps(plan.prog, plan.v0, plan.vf)
    assert not any("abrelu" in s.fn for s in steps)


def test_after_the_global_pool_is_rejected():
    for act in (lambda: LR(), lambda: AR(-1, 1)):
        with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
            Plan(S(C(3), LR(), G(), act()), 4, 4)
        assert str(e.value) == P.ABRELU_RULE_GLOBAL
    assert "LeakyReLU" in P.ABRELU_RULE_GLOBAL and P.POOL_RULES["abrelu"] == P.ABRELU_RULE_GLOBAL
    assert P.ABRELU_RULE_GLOBAL not in (P.GELU_RULE_GLOBAL, P.POOL_RULE_NONLIN)
    with pytest.raises(NotImplementedError) as e:
        pool_ntk_steps(*compile_program(S(C(3), G(), LR()), 4, 4))
    assert str(e.value) == P.ABRELU_RULE_GLOBAL
    # the other rules hold with the module in the model
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), LR(), G(), R()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), LR(), G(), G()), 4, 4)
    assert str(e.value) == P.POOL_RULE_ONE
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
        S(C(3), LR(), G()).ntk(x)
    assert str(e.value) == P.POOL_RULE_NTK


def test_models_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(C(3), LR(), C(4, padding=0)).double()
    plan = model._plan(4, 4)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    # at a geometry the whole-network kernel has (the reference ConvNet's), the op is the reason
    big = S(C(3), LR(), C(28, padding=0)).double()
    with pytest.raises(Unsupported) as e:
        NetPlan(big._plan(28, 28), 8)
    assert str(e.value) == "op abrelu"
    NetPlan(S(C(3), R(), C(28, padding=0)).double()._plan(28, 28), 8)     # the ReLU twin lowers
    # the variance chain has no record for it: it declines instead of raising
    assert plan._var_chain({plan.vf}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {"cgp_abrelu_args_size", "cgp_abrelu_f64", "cgp_abrelu_f32", "cgp_var_abrelu_f64",
               "cgp_var_abrelu_f32", "cgp_abrelu_cov_args_size", "cgp_abrelu_cov_f64",
               "cgp_abrelu_cov_f32"}


def test_abi_and_symbols():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    assert lib.cgp_abrelu_args_size() == ctypes.sizeof(N.ABReluArgs) == \
        ctypes.sizeof(N.ErfArgs) + 24
    assert lib.cgp_abrelu_cov_args_size() == ctypes.sizeof(N.ABReluCovArgs) == \
        ctypes.sizeof(N.CovNonlinNtkArgs) - 8 + 24
    names = [f[0] for f in N.ABReluArgs._fields_]
    assert names == [f[0] for f in N.ErfArgs._fields_] + ["s", "m", "h"]
    assert [f[0] for f in N.ABReluCovArgs._fields_] == \
        [f[0] for f in N.CovNonlinNtkArgs._fields_ if f[0] not in ("kind", "reserved")] + \
        ["s", "m", "hh"]
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    syms = set(re.findall(r"\b(cgp_(?:var_)?abrelu_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if "abrelu" in s}
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    # the object that holds every nonlinearity's entry points (csrc/nonlin.hip)
    assert "build/nonlin.o" in open(os.path.join(ROOT, "cnn-gp_amd", "csrc", "Makefile")).read()


def abrelu_args(**kw):
    a = N.ABReluArgs()
    a.xy, a.theta, a.out_xy, a.out_theta, a.xx, a.yy = 64, 128, 192, 256, 320, 384
    a.nmaps, a.n1, a.n2, a.hw = 6, 3, 2, 4
    a.s, a.m, a.h = 1.0, 0.0, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_abrelu_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed); cgp_erf_*'s, and
    last the constants (so every call below that reaches them has valid maps and sizes)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_abrelu_{sfx}")
    args = abrelu_args
    assert fn(None, None) == 1001
    for field in ("xy", "out_xy", "out_theta", "xx", "yy"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"abrelu" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    for kw in (dict(theta=None), dict(theta=None, out_theta=None)):
        assert fn(ctypes.byref(args(nmaps=5, **kw)), None) == 1001
        assert b"nmaps inconsistent" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(yy=None, same=1, n2=3, nmaps=9)), None) == 1001
    assert b"yy is NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(yy=None, same=1, diag=1, n2=3, nmaps=3, hw=4096)), None) == 1001
    assert b"too large" in lib.cgp_last_error()                    # past the yy check
    assert fn(ctypes.byref(args(same=1)), None) == 1001           # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    for kw in (dict(nmaps=1 << 31, n1=1 << 16, n2=1 << 15), dict(nmaps=0, n1=0), dict(hw=0),
               dict(hw=-1)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(hw=2049)), None) == 1001          # larger than one chunk
    assert b"too large" in lib.cgp_last_error()
    for kw in (dict(s=NAN), dict(m=INF), dict(h=-INF), dict(s=INF, m=NAN, h=NAN)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert b"not finite" in lib.cgp_last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_var_abrelu_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_var_abrelu_{sfx}")
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] = None
        assert fn(p[0], p[1], 2, 2, 4, 0, 0.5, p[2], p[3], None) == 1001
        assert b"var_abrelu" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    assert fn(64, 128, 2, 3, 4, 1, 0.5, 192, 256, None) == 1001    # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    for n1, n2, hw in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4)):
        assert fn(64, 128, n1, n2, hw, 0, 0.5, 192, 256, None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    for h in (NAN, INF, -INF):
        assert fn(64, 128, 2, 2, 4, 0, h, 192, 256, None) == 1001
        assert b"not finite" in lib.cgp_last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_abrelu_cov_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_abrelu_cov_{sfx}")

    def args(**kw):
        a = N.ABReluCovArgs()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        a.npairs, a.h, a.w = 3, 4, 4
        a.s, a.m, a.hh = 1.0, 0.0, 0.5
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert fn(None, None) == 1001
    for field in ("in_", "out", "xx", "yy", "pair_i", "pair_j"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"abrelu_cov" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    # with theta the second output is needed, and is a buffer of its own
    assert fn(ctypes.byref(args(theta=512)), None) == 1001
    assert b"NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(theta=512, out_theta=128)), None) == 1001
    assert b"one buffer" in lib.cgp_last_error()
    for kw in (dict(npairs=0), dict(npairs=-1), dict(npairs=1 << 31), dict(h=0), dict(w=0),
               dict(h=-4), dict(h=256, w=256), dict(h=182, w=182)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert b"bad sizes" in lib.cgp_last_error()
    for kw in (dict(s=NAN), dict(m=INF), dict(hh=-INF), dict(theta=512, out_theta=640, hh=NAN)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert b"not finite" in lib.cgp_last_error()
    # pairs·elements past what one launch counts in int32 blocks
    assert fn(ctypes.byref(args(npairs=(1 << 31) - 1, h=181, w=181)), None) == 1001
    assert b"elements" in lib.cgp_last_error()
    # the entry points of the other nonlinearities keep rejecting unknown kinds
    for name, rec in (("cgp_cov_nonlin", N.CovNonlinArgs), ("cgp_covntk_nonlin",
                                                            N.CovNonlinNtkArgs)):
        a = rec()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        if name == "cgp_covntk_nonlin":
            a.theta, a.out_theta = 512, 640
        a.npairs, a.h, a.w, a.kind = 3, 4, 4, 4
        assert getattr(lib, f"{name}_{sfx}")(ctypes.byref(a), None) == 1001
        assert b"kind" in lib.cgp_last_error()
    c = N.CovConvArgs()
    c.in_, c.out, c.xx, c.yy, c.pair_i, c.pair_j = 64, 128, 192, 256, 320, 384
    c.npairs, c.h, c.w, c.ho, c.wo, c.taps, c.stride, c.dilation, c.post = 3, 4, 4, 4, 4, 3, 1, 1, 4
    assert getattr(lib, f"cgp_cov_conv_{sfx}")(ctypes.byref(c), None) == 1001
    assert b"post" in lib.cgp_last_error()


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_model_without_gpu_raises_like_relu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device") as gelu:
        S(C(3), m.Gelu(), C(4, padding=0))(x)
    with pytest.raises(RuntimeError, match="HIP device") as ab:
        seq_net()(x)
    assert str(ab.value) == str(gelu.value)
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
