"""CPU-only tests of the sinusoid family (cnn_gp.Sin / cnn_gp.Cos / cnn_gp.Rbf): the closed
forms against a Gauss–Hermite product quadrature, κ̇ against autograd, the oracle's identities,
the modules, the lowering (program, fusion, NTK steps, both launch lists on position-pair
maps, the whole-network path declining), the plan-cache key, and the host side of cgp_sin_* /
cgp_var_sin_* / cgp_sin_cov_*."""
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
import sin_oracle as SO

m = cnn_gp
S, C, R, G, A, SI, CO, RB = (m.Sequential, m.Conv2d, m.ReLU, m.GlobalAvgPool, m.AvgPool2d, m.Sin,
                             m.Cos, m.Rbf)


# ------------------------------------------------------------------------------------
# the formulas
# ------------------------------------------------------------------------------------
GH_X, GH_W = np.polynomial.hermite_e.hermegauss(120)       # weight exp(−x²/2)
GH_W = GH_W / math.sqrt(2 * math.pi)


def _quadrature(a, b, th, v1, v2, rho):
    """E[φ(u1)φ(u2)] and E[φ'(u1)φ'(u2)] of φ(x) = a·sin(b·x + θ) by a 120 x 120 Gauss–Hermite
    product rule over independent standard normals (z1, z2): u1 = √v1·z1, u2 = √v2·(ρ·z1 +
    √(1 − ρ²)·z2).  It shares nothing with the closed form."""
    z1, z2 = GH_X[:, None], GH_X[None, :]
    w = GH_W[:, None] * GH_W[None, :]
    u1 = math.sqrt(v1) * z1
    u2 = math.sqrt(v2) * (rho * z1 + math.sqrt(max(0.0, 1 - rho * rho)) * z2)
    k = np.sum(w * (a * np.sin(b * u1 + th)) * (a * np.sin(b * u2 + th)))
    kd = np.sum(w * (a * b * np.cos(b * u1 + th)) * (a * b * np.cos(b * u2 + th)))
    return float(k), float(kd)


def test_closed_form_matches_the_quadrature():
    """200 draws with a in [0.5, 1.5], b in [0.3, 2], θ in [0, π], v in [0.05, 3], ρ in [−1, 1];
    absolute difference below 1e-13 (the quadrature agrees with the closed form to 6.7e-16
    over this range, so the bound is a margin of about 150x, not a fit)."""
    rng = np.random.default_rng(5)
    worst_k = worst_kd = 0.0
    for _ in range(200):
        a, b, th = rng.uniform(0.5, 1.5), rng.uniform(0.3, 2), rng.uniform(0, math.pi)
        v1, v2, rho = rng.uniform(0.05, 3), rng.uniform(0.05, 3), rng.uniform(-1, 1)
        c = rho * math.sqrt(v1 * v2)
        k, kd = SO.sin_pair(np.float64(c), np.float64(v1), np.float64(v2),
                            SO.constants(a, b, th))
        qk, qkd = _quadrature(a, b, th, v1, v2, rho)
        worst_k = max(worst_k, abs(float(k) - qk))
        worst_kd = max(worst_kd, abs(float(kd) - qkd))
    print(f"closed form vs Gauss-Hermite quadrature: K' {worst_k:.2e}, kdot {worst_kd:.2e}")
    assert worst_k < 1e-13 and worst_kd < 1e-13


def _draws(n=200, seed=3):
    rng = np.random.default_rng(seed)
    v1, v2 = 3 * (1 - rng.random(n)), 3 * (1 - rng.random(n))
    return rng.uniform(-1, 1, n) * np.sqrt(v1 * v2), v1, v2


PARAMS = [(1.0, 1.0, 0.0), (1.5, 2.0, 0.3), (1.0, 2.0, math.pi / 2), (0.7, 0.4, 2.0)]


def test_kdot_is_the_derivative_of_the_oracle():
    c, v1, v2 = _draws()
    for k4 in [SO.constants(*p) for p in PARAMS] + [SO.rbf_constants(0.5)]:
        ct = torch.from_numpy(c).requires_grad_()
        kt, kdt = SO.sin_pair(ct, torch.from_numpy(v1), torch.from_numpy(v2), k4)
        g, = torch.autograd.grad(kt.sum(), ct)
        assert float((g - kdt.detach()).abs().max()) < 1e-14 * k4[3]
        # the override's κ̇ is that derivative at c = v1 = v2 = v
        vt = torch.from_numpy(v1)
        assert torch.equal(SO.sin_pair(vt, vt, vt, k4)[1], SO.sin_var_kdot(vt, k4))


def test_oracle_identities():
    c, v1, v2 = _draws()
    # Cos(a, b) is Sin(a, b, π/2), bit for bit: cos π is exactly −1
    assert math.cos(math.pi) == -1.0
    assert CO(1.3, 2.0).constants() == SI(1.3, 2.0, math.pi / 2).constants() == \
        SO.constants(1.3, 2.0, math.pi / 2)
    assert SO.consts_of(CO(1.3, 2.0)) == SO.consts_of(SI(1.3, 2.0, math.pi / 2))
    for fn in (0, 1):
        assert np.array_equal(SO.sin_pair(c, v1, v2, SO.consts_of(CO(1.3, 2.0)))[fn],
                              SO.sin_pair(c, v1, v2, SO.constants(1.3, 2.0, math.pi / 2))[fn])
    # Rbf(γ) is Sin(√2, √(2γ), π/4) to rounding, with C exactly 0 and v' exactly 1
    for g in (0.125, 0.5, 1.7):
        rb = RB(g).constants()
        assert rb == (1.0, g, 0.0, 2 * g) == SO.rbf_constants(g) == SO.consts_of(RB(g))
        full = SO.constants(math.sqrt(2), math.sqrt(2 * g), math.pi / 4)
        assert abs(full[2]) < 1e-16 and full[2] != 0.0
        # 1e-15 in the project's metric max|a − b| / max|a|: (√(2γ))²/2 is γ to an ulp, which
        # exp(−B·d) turns into B·d ulps of a small value (5e-15 of it at d = 12), so no
        # pointwise-relative bound of 1e-15 can hold between the two roundings of B
        for a, b in zip(SO.sin_pair(c, v1, v2, rb), SO.sin_pair(c, v1, v2, full)):
            assert np.max(np.abs(a - b)) / np.max(np.abs(a)) < 1e-15
        assert np.array_equal(SO.sin_var(v1, rb), np.ones_like(v1))
        k, kd = SO.sin_pair(c, v1, v2, rb)
        assert np.all(k > 0) and np.all(k <= 1) and np.array_equal(kd, 2 * g * k)
    # at v1 = v2 = c = 0: K' = A·(1 − C) exactly
    z = np.zeros(3)
    for p in PARAMS:
        k4 = SO.constants(*p)
        want = k4[0] * (1 - k4[2])
        assert np.array_equal(SO.sin_pair(z, z, z, k4)[0], np.full(3, want))
        assert np.array_equal(SO.sin_var(z, k4), np.full(3, want))
    # |K'| <= a²
    for p in PARAMS:
        assert np.max(np.abs(SO.sin_pair(c, v1, v2, SO.constants(*p))[0])) <= p[0] ** 2


def small_net(side=6):
    return S(C(3, var_bias=0.2), SI(1.5, 2, 0.3), m.Sum([S(), S(C(3, var_weight=1.5), RB(0.5),
                                                                   C(3))]),
             CO(1, 2), C(side, padding=0)).double()


def test_oracle_stepwise_matches_autograd_and_the_map_walk():
    """the three forms of the oracle agree: the layer walk, program.ntk_steps launch by launch
    (same=False pairs against autograd) and the walk on position-pair maps"""
    rng = np.random.default_rng(8)
    X, Z = rng.standard_normal((3, 2, 6, 6)), rng.standard_normal((2, 2, 6, 6))
    model = small_net()
    k = SO.kernel(model, X, Z, False, False)
    ka, tha = SO.ntk_autograd(model, X, Z)
    ks, ths = SO.ntk_stepwise(model, X, Z, False, False)
    km, thm = SO.pool_ntk(model, X, Z, False, False)
    for got in (ka, ks, km):
        assert np.max(np.abs(got - k)) < 1e-13 * np.max(np.abs(k))
    for got in (ths, thm):
        assert np.max(np.abs(got - tha)) < 1e-12 * np.max(np.abs(tha))
    # with the overrides: same tile, layer walk against the walk on maps
    kx, thx = SO.ntk_stepwise(model, X)
    kmx, thmx = SO.pool_ntk(model, X)
    assert np.max(np.abs(kmx - kx)) < 1e-13 * np.max(np.abs(kx))
    assert np.max(np.abs(thmx - thx)) < 1e-13 * np.max(np.abs(thx))
    assert np.max(np.abs(kx - SO.kernel(model, X))) < 1e-13 * np.max(np.abs(kx))


# ------------------------------------------------------------------------------------
# the modules
# ------------------------------------------------------------------------------------
def test_exports_and_module_surface():
    for name in ("Sin", "Cos", "Rbf"):
        assert name in cnn_gp.__all__ and name in cnn_gp.kernels.__all__
    assert issubclass(CO, SI) and issubclass(RB, SI) and issubclass(SI, m.NNGPKernel)
    s = SI()
    assert (s.a, s.b, s.phase) == (1.0, 1.0, 0.0) and s.constants() == (0.5, 0.5, 1.0, 0.5)
    assert type(SI(2, 3, 1).a) is float and SI(2, 3, 1).layers() == 0
    assert SI(1.5, 2, 0.3).constants() == (1.125, 2.0, math.cos(0.6), 4.5)
    assert CO().phase == math.pi / 2 and CO(2, 3).constants() == (2.0, 4.5, -1.0, 18.0)
    assert RB().gamma == 1.0 and RB(0.5).constants() == (1.0, 0.5, 0.0, 1.0)
    assert SI(1, 2, 0.5).extra_repr() == "a=1.0, b=2.0, phase=0.5"
    assert CO(1, 2).extra_repr() == "a=1.0, b=2.0" and RB(0.5).extra_repr() == "gamma=0.5"
    assert S(C(3), RB(), C(4, padding=0)).layers() == 2
    # set_exact_relu is ignored: the same program either way
    model = S(C(3), SI(), C(4, padding=0))
    ops = lambda p: [(o.kind, o.consts) for o in p.pair_ops]                     # noqa: E731
    assert ops(model._plan(4, 4)) == ops(model.set_exact_relu(True)._plan(4, 4))


NAN, INF = float("nan"), float("inf")


def test_bad_parameters_raise():
    for args in ((NAN, 1, 0), (1, INF, 0), (1, 1, NAN), (1, 1, -INF), (0, 1, 0), (1, 0.0, 0),
                 (1e200, 1, 0), (1, 1e-200, 0)):
        with pytest.raises(ValueError):
            SI(*args)
    for args in ((NAN, 1), (1, INF), (0, 1), (1, -0.0)):
        with pytest.raises(ValueError):
            CO(*args)
    for g in (NAN, INF, 0.0, -1.0, 1e308 * 10):
        with pytest.raises(ValueError):
            RB(g)
    SI(-1, -2, -3)                                          # signs are fine
    # a parameter assigned later is checked when the program is compiled
    mod = S(C(3), RB(0.5), C(4, padding=0))
    mod.mods[1].gamma = -1.0
    with pytest.raises(ValueError):
        Plan(mod, 4, 4)
    bad = SI()
    bad.b = 0.0
    with pytest.raises(ValueError):
        compile_program(S(bad), 4, 4)


def test_structure_key_carries_the_constants():
    build = lambda act: S(C(3), act, C(4, padding=0))                            # noqa: E731
    k1 = build(SI(1, 2, 0.3))._structure_key()
    assert ("sin", *SI(1, 2, 0.3).constants()) in k1
    assert k1 == build(SI(1, 2, 0.3))._structure_key() != build(SI(1, 2.5, 0.3))._structure_key()
    assert build(CO(1, 2))._structure_key() == build(SI(1, 2, math.pi / 2))._structure_key()
    model = build(SI(1, 2, 0.3))
    plan = model._plan(4, 4)
    assert model._plan(4, 4) is plan and plan.pair_ops[1].consts == SI(1, 2, 0.3).constants()
    model.mods[1].b = 2.5                                   # through __setattr__: a new key
    plan2 = model._plan(4, 4)
    assert plan2 is not plan and plan2.pair_ops[1].consts == SI(1, 2.5, 0.3).constants()
    model.mods[1].phase = 1.0
    assert model._plan(4, 4).pair_ops[1].consts == SI(1, 2.5, 1.0).constants()
    model.mods[1].b, model.mods[1].phase = 2.0, 0.3         # back: the first plan is reused
    assert model._plan(4, 4) is plan
    rb = build(RB(0.5))
    p1 = rb._plan(4, 4)
    rb.mods[1].gamma = 0.25
    assert rb._plan(4, 4) is not p1 and rb._plan(4, 4).pair_ops[1].consts == (1.0, 0.25, 0.0, 0.5)


# ------------------------------------------------------------------------------------
# the lowering: one sequential model, one residual model, one pooled model
# ------------------------------------------------------------------------------------
def seq_net():
    return S(C(3), SI(1.5, 2, 0.3), C(3), RB(0.5), C(4, padding=0))


def res_net():
    return S(C(3), m.Sum([S(), S(C(3), CO(1, 2))]), C(4, padding=0))


def pooled_net():
    return S(C(3), SI(1.5, 2, 0.3), A(2), C(3, var_bias=0.1), RB(0.5), G(), C(1))


def test_lowering_of_the_sequential_model():
    model = seq_net()
    prog, v0, vf = compile_program(model, 4, 4)
    assert [o.kind for o in prog.ops] == ["conv", "sin", "conv", "sin", "conv"]
    assert [o.consts for o in prog.ops if o.kind == "sin"] == \
        [SI(1.5, 2, 0.3).constants(), (1.0, 0.5, 0.0, 1.0)]
    assert prog.ops[0].consts is None and prog.ops[1].smh is None
    plan = Plan(model, 4, 4)
    assert [(o.kind, o.pre, o.post) for o in plan.pair_ops] == [
        ("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_NONE), ("sin", N.CGP_PRE_NONE, N.CGP_POST_NONE),
        ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE), ("sin", N.CGP_PRE_NONE, N.CGP_POST_NONE),
        ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]
    srcs = {o.src for o in plan.pair_ops if o.kind == "sin"}
    assert plan.need_var == srcs == plan.ntk_need_var() and plan.pool is None
    assert [s.fn for s in plan.layer_list()[0]] == ["conv", "sin", "conv", "sin", "conv"]
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["conv", "sin_ntk", "conv", "conv", "sin_ntk", "conv", "conv"]
    assert steps[1].theta == steps[1].src == steps[0].dst and steps[1].var == steps[0].dst[1]
    assert steps[1].dst_theta == ("T", steps[1].op.dst) and steps[3].src == steps[1].dst_theta
    assert kbuf == ("K", vf) and tbuf == ("T", vf)
    # before any conv Θ = 0: the forward-only launch
    prog2, v0, vf = compile_program(S(RB(), C(4, padding=0)), 4, 4)
    steps2, kbuf, tbuf = ntk_steps(prog2, v0, vf)
    assert [s.fn for s in steps2] == ["sin", "conv"]
    assert steps2[0].theta is None and steps2[0].dst_theta is None and tbuf == ("K", vf)
    # the buffer lifetimes: the same reads and writes as the erf twin's
    twin = ntk_steps(*compile_program(S(C(3), m.Erf(), C(3), m.Erf(), C(4, padding=0)), 4, 4))[0]
    assert [(s.reads(), s.writes()) for s in steps] == [(s.reads(), s.writes()) for s in twin]
    # on position-pair maps (position_covariance / ntk_maps of a model without a pool)
    bs = pool_steps(prog, *compile_program(model, 4, 4)[1:], body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "sin", "conv", "sin", "conv"]
    ns = pool_ntk_steps(prog, *compile_program(model, 4, 4)[1:], body=True)
    assert [s.fn for s in ns.steps] == ["moments", "conv", "sin_ntk", "conv_ntk", "sin_ntk",
                                        "conv_ntk"]
    assert all(s.post == N.CGP_COV_NONE for s in ns.steps)  # never a conv's post-stage
    assert ns.steps[2].theta == ns.steps[2].src             # Θ is K's buffer after the first conv


def test_lowering_of_the_residual_model():
    plan = Plan(res_net(), 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "conv", "sin", "add", "conv"]
    # rule 2: the identity skip becomes the addend of the block's last op
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "sin", "conv"]
    op = plan.pair_ops[2]
    assert op.addend == plan.pair_ops[0].dst and op.consts == (0.5, 2.0, -1.0, 2.0)
    steps, kbuf, tbuf = ntk_steps(plan.prog, plan.v0, plan.vf)
    assert [s.fn for s in steps] == ["conv", "conv", "conv", "sin_ntk", "axpby", "axpby", "conv",
                                     "conv"]
    bs = pool_steps(plan.prog, plan.v0, plan.vf, body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "conv", "sin", "conv"]
    assert bs.steps[3].addend == bs.steps[1].dst and bs.self_var == frozenset()
    ns = pool_ntk_steps(plan.prog, plan.v0, plan.vf, body=True)
    assert [s.fn for s in ns.steps] == ["moments", "conv", "conv_ntk", "sin_ntk", "conv_ntk"]
    st = ns.steps[3]
    # both addends ride on the launch: K of the skip, and its Θ (the first conv's K buffer)
    assert st.addend == ("K", bs.steps[1].dst) and st.addend_theta == ("K", bs.steps[1].dst)
    assert st.dst_theta == ("T", st.dst[1]) and st.var == bs.steps[3].var


def test_lowering_of_the_pooled_model():
    """upstream and downstream of an AvgPool2d: each a launch of its own, counted in need_var
    like a nonlinearity, the one downstream in self_var"""
    plan = Plan(pooled_net(), 4, 4)
    ps = plan.pool
    assert [o.kind for o in plan.prog.ops] == ["conv", "sin", "avgpool", "conv", "sin", "pool",
                                               "conv"]
    v = [o.dst for o in plan.prog.ops]
    assert [s.fn for s in ps.steps] == ["moments", "conv", "sin", "avgpool", "conv", "sin",
                                        "pool", "conv"]
    g1, g2 = ps.steps[2], ps.steps[5]
    assert (g1.src, g1.var, g1.dst, g1.addend) == (v[0], v[0], v[1], None)
    assert (g2.src, g2.var, g2.dst, g2.addend) == (v[3], v[3], v[4], None)
    assert g1.op.consts == SI(1.5, 2, 0.3).constants() and g2.op.consts == (1.0, 0.5, 0.0, 1.0)
    assert ps.need_var == {v[0], v[3]} and ps.self_var == {v[3]} and ps.self_last == 4
    assert plan.need_var == {v[0], v[3]} == plan.ntk_need_var()
    for fused in (True, False):
        ns = plan.pool_ntk(False, fused, 8)
        conv2 = ["conv_ntk"] if fused else ["conv", "conv"]
        assert [s.fn for s in ns.steps] == ["moments", "conv", "sin_ntk", "avgpool", "avgpool"] \
            + conv2 + ["sin_ntk", "pool", "pool"] + conv2
        assert all(s.post == N.CGP_COV_NONE for s in ns.steps)
        a2 = [s for s in ns.steps if s.fn == "sin_ntk"][1]
        assert a2.theta == ("T", v[3]) and a2.dst_theta == ("T", v[4]) and a2.var == v[3]
    # Θ = None upstream: the forward-only launch of the same entry point
    ns = pool_ntk_steps(*compile_program(S(RB(), C(3), G(), C(1)), 4, 4))
    assert [s.fn for s in ns.steps][:3] == ["moments", "sin", "conv"]


def test_a_model_without_the_modules_compiles_to_the_same_program():
    model = S(C(3), R(), m.Sum([S(), S(C(3), m.Erf())]), m.Gelu(), C(3), m.LeakyReLU(0.2),
              C(4, padding=0))
    plan = Plan(model, 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "relu", "conv", "erf", "add", "gelu",
                                               "conv", "abrelu", "conv"]
    assert [(o.kind, o.post) for o in plan.pair_ops] == [
        ("conv", N.CGP_POST_RELU), ("conv", 0), ("erf", 0), ("gelu", 0), ("conv", 0),
        ("abrelu", 0), ("conv", 0)]
    assert all(o.consts is None for o in plan.prog.ops)
    assert [s.fn for s in plan.layer_list()[0]] == ["conv", "conv", "erf", "gelu", "conv",
                                                    "abrelu", "conv"]
    steps, _, _ = ntk_steps(plan.prog, plan.v0, plan.vf)
    assert [s.fn for s in steps] == ["conv", "relu_ntk", "conv", "conv", "erf_ntk", "axpby",
                                     "axpby", "gelu_ntk", "conv", "conv", "abrelu_ntk", "conv",
                                     "conv"]
    twin = Plan(S(C(3), R(), A(2), C(3, var_bias=0.1), R(), G(), C(1)), 4, 4)
    assert [s.fn for s in twin.pool.steps] == ["moments", "conv", "avgpool", "conv", "nonlin",
                                               "pool", "conv"]
    assert not any("sin" in s.fn for s in twin.pool_ntk(False, True, 8).steps)
    # the records of the other nonlinearities are filled as before
    assert [k for k, v in P.NONLIN_CALLS.items() if v[3] is not None] == ["abrelu", "sin"]
    op = plan.prog.ops[7]
    assert dict(P.NONLIN_CALLS["abrelu"][3](op)) == dict(zip("smh", op.smh))
    assert P.NONLIN_CALLS["abrelu"][4](op) == (op.smh[2],)


def test_after_the_global_pool_is_rejected():
    for act in (SI, CO, RB):
        with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
            Plan(S(C(3), SI(), G(), act()), 4, 4)
        assert str(e.value) == P.SIN_RULE_GLOBAL
    assert "Rbf" in P.SIN_RULE_GLOBAL and P.POOL_RULES["sin"] == P.SIN_RULE_GLOBAL
    assert P.SIN_RULE_GLOBAL not in (P.GELU_RULE_GLOBAL, P.ABRELU_RULE_GLOBAL, P.POOL_RULE_NONLIN)
    with pytest.raises(NotImplementedError) as e:
        pool_ntk_steps(*compile_program(S(C(3), G(), RB()), 4, 4))
    assert str(e.value) == P.SIN_RULE_GLOBAL
    # the other rules hold with the module in the model
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), SI(), G(), R()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
        S(C(3), RB(), G()).ntk(x)
    assert str(e.value) == P.POOL_RULE_NTK


def test_models_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(C(3), RB(), C(4, padding=0)).double()
    plan = model._plan(4, 4)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    # at a geometry the whole-network kernel has (the reference ConvNet's), the op is the reason
    big = S(C(3), SI(), C(28, padding=0)).double()
    with pytest.raises(Unsupported) as e:
        NetPlan(big._plan(28, 28), 8)
    assert str(e.value) == "op sin"
    # the variance chain has no record for it: it declines instead of raising
    assert plan._var_chain({plan.vf}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {"cgp_sin_args_size", "cgp_sin_f64", "cgp_sin_f32", "cgp_var_sin_f64",
               "cgp_var_sin_f32", "cgp_sin_cov_args_size", "cgp_sin_cov_f64", "cgp_sin_cov_f32"}


def test_abi_and_symbols():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    assert lib.cgp_sin_args_size() == ctypes.sizeof(N.SinArgs) == ctypes.sizeof(N.ErfArgs) + 32
    assert lib.cgp_sin_cov_args_size() == ctypes.sizeof(N.SinCovArgs) == \
        ctypes.sizeof(N.ABReluCovArgs) + 8
    assert [f[0] for f in N.SinArgs._fields_] == \
        [f[0] for f in N.ErfArgs._fields_] + ["A", "B", "C", "D"]
    assert [f[0] for f in N.SinCovArgs._fields_] == \
        [f[0] for f in N.ABReluCovArgs._fields_][:-3] + ["A", "B", "C", "D"]
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    syms = set(re.findall(r"\b(cgp_(?:var_)?sin_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if re.match(r"cgp_(var_)?sin_", s)}
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
    assert "typedef struct cgp_sin_args" in txt and "typedef struct cgp_sin_cov_args" in txt
    assert "#define CGP_ABI_VERSION 12" in txt


def sin_args(**kw):
    a = N.SinArgs()
    a.xy, a.theta, a.out_xy, a.out_theta, a.xx, a.yy = 64, 128, 192, 256, 320, 384
    a.nmaps, a.n1, a.n2, a.hw = 6, 3, 2, 4
    a.A, a.B, a.C, a.D = 0.5, 0.5, 1.0, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# constants the entry points refuse: (fields, the message)
BAD_CONSTS = [(dict(A=NAN), b"not finite"), (dict(B=INF), b"not finite"),
              (dict(C=NAN), b"not finite"), (dict(D=-INF), b"not finite"),
              (dict(A=0.0), b"A > 0"), (dict(A=-0.5), b"A > 0"), (dict(B=0.0), b"A > 0"),
              (dict(B=-2.0), b"A > 0"), (dict(C=1.0000001), b"A > 0"), (dict(C=-2.0), b"A > 0")]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_sin_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed); cgp_erf_*'s, and
    last the constants (so every call below that reaches them has valid maps and sizes)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_sin_{sfx}")
    args = sin_args
    assert fn(None, None) == 1001
    for field in ("xy", "out_xy", "out_theta", "xx", "yy"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"sin" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    for kw in (dict(theta=None), dict(theta=None, out_theta=None)):
        assert fn(ctypes.byref(args(nmaps=5, **kw)), None) == 1001
        assert b"nmaps inconsistent" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(yy=None, same=1, n2=3, nmaps=9)), None) == 1001
    assert b"yy is NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(same=1)), None) == 1001           # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    for kw in (dict(nmaps=1 << 31, n1=1 << 16, n2=1 << 15), dict(nmaps=0, n1=0), dict(hw=0),
               dict(hw=-1)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(hw=2049)), None) == 1001          # larger than one chunk
    assert b"too large" in lib.cgp_last_error()
    for kw, msg in BAD_CONSTS:
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert msg in lib.cgp_last_error(), kw


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_var_sin_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_var_sin_{sfx}")
    k4 = (0.5, 0.5, 1.0, 0.5)
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] = None
        assert fn(p[0], p[1], 2, 2, 4, 0, *k4, p[2], p[3], None) == 1001
        assert b"var_sin" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    assert fn(64, 128, 2, 3, 4, 1, *k4, 192, 256, None) == 1001    # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    for n1, n2, hw in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4)):
        assert fn(64, 128, n1, n2, hw, 0, *k4, 192, 256, None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    for kw, msg in BAD_CONSTS:
        c = dict(zip("ABCD", k4), **kw)
        assert fn(64, 128, 2, 2, 4, 0, c["A"], c["B"], c["C"], c["D"], 192, 256, None) == 1001
        assert msg in lib.cgp_last_error(), kw


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_sin_cov_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_sin_cov_{sfx}")

    def args(**kw):
        a = N.SinCovArgs()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        a.npairs, a.h, a.w = 3, 4, 4
        a.A, a.B, a.C, a.D = 1.0, 0.5, 0.0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert fn(None, None) == 1001
    for field in ("in_", "out", "xx", "yy", "pair_i", "pair_j"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"sin_cov" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    # with theta the second output is needed, and is a buffer of its own
    assert fn(ctypes.byref(args(theta=512)), None) == 1001
    assert b"NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(theta=512, out_theta=128)), None) == 1001
    assert b"one buffer" in lib.cgp_last_error()
    for kw in (dict(npairs=0), dict(npairs=-1), dict(npairs=1 << 31), dict(h=0), dict(w=0),
               dict(h=-4), dict(h=256, w=256), dict(h=182, w=182)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert b"bad sizes" in lib.cgp_last_error()
    for kw, msg in BAD_CONSTS:
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert msg in lib.cgp_last_error(), kw
    assert fn(ctypes.byref(args(theta=512, out_theta=640, D=NAN)), None) == 1001
    assert b"not finite" in lib.cgp_last_error()
    # pairs·elements past what one launch counts in int32 blocks: the grid is sized in 64 bits
    assert fn(ctypes.byref(args(npairs=(1 << 31) - 1, h=181, w=181)), None) == 1001
    assert b"elements" in lib.cgp_last_error()


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_model_without_gpu_raises_like_relu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device") as relu:
        S(C(3), R(), C(4, padding=0))(x)
    with pytest.raises(RuntimeError, match="HIP device") as sin:
        seq_net()(x)
    assert str(sin.value) == str(relu.value)
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
