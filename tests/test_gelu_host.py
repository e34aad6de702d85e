"""CPU-only tests of the GELU nonlinearity: the closed forms against a numerical integral,
the test-time oracle against itself (autograd Θ vs the stepwise recursion), the lowering of
cnn_gp.Gelu (program, fusion, NTK steps, the pooled launch list, the whole-network path
declining), and the host side of cgp_gelu_* / cgp_var_gelu_* / cgp_gelu_cov_*."""
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
from cnn_gp.program import Plan, compile_program, ntk_steps, pool_steps

from conftest import ROOT
import gelu_oracle as GO

m = cnn_gp
S, C, R, E, GE, G, A = (m.Sequential, m.Conv2d, m.ReLU, m.Erf, m.Gelu, m.GlobalAvgPool,
                        m.AvgPool2d)


# ------------------------------------------------------------------------------------
# the formulas
# ------------------------------------------------------------------------------------
def _integrals(v1, v2, rho, n):
    """E[φ(u1)φ(u2)] and E[φ'(u1)φ'(u2)], φ(x) = x·Φ(x), φ'(x) = Φ(x) + x·pdf(x), by the
    trapezoid rule with n points per axis on [-12, 12]² over two independent standard
    normals z: u1 = √v1·z1, u2 = √v2·(ρ·z1 + √(1 - ρ²)·z2) -- regular at |ρ| = 1."""
    z = np.linspace(-12.0, 12.0, n)
    h = z[1] - z[0]
    w = np.full(n, h)
    w[0] = w[-1] = h / 2
    w = w * np.exp(-z * z / 2) / math.sqrt(2 * math.pi)
    z1, z2 = np.meshgrid(z, z, indexing="ij")
    u1 = math.sqrt(v1) * z1
    u2 = math.sqrt(v2) * (rho * z1 + math.sqrt(max(0.0, 1 - rho * rho)) * z2)
    cdf = lambda a: 0.5 * (1 + torch.erf(torch.from_numpy(a / math.sqrt(2))).numpy())   # noqa
    pdf = lambda a: np.exp(-a * a / 2) / math.sqrt(2 * math.pi)                         # noqa
    ww = np.outer(w, w)
    k = float(np.sum(ww * (u1 * cdf(u1)) * (u2 * cdf(u2))))
    kd = float(np.sum(ww * (cdf(u1) + u1 * pdf(u1)) * (cdf(u2) + u2 * pdf(u2))))
    return k, kd


# (v1, v2, rho): v <= 5; rho = 1 with v1 = v2 (the variance form's point), rho near -1
QUAD_POINTS = [(0.05, 0.05, 1.0), (1.0, 1.0, 1.0), (5.0, 5.0, 1.0), (3.0, 3.0, -0.999),
               (0.5, 5.0, -0.999), (0.05, 3.0, 0.0), (1.0, 0.7, 0.5), (5.0, 0.3, 0.95),
               (2.0, 5.0, -0.6), (5.0, 5.0, 0.999), (0.7, 0.05, -0.3)]


def test_closed_form_matches_integration():
    """K' and κ̇ against the trapezoid integral of x·Φ(x) and of Φ(x) + x·pdf(x), which
    shares no code with the closed forms.  The integrand is analytic with Gaussian decay, so
    the rule converges geometrically: 241 and 321 points per axis (h = 0.1, 0.075) must agree
    to 1e-12, which shows the integral converged.  Bound 5e-12 absolute, about ten times the
    3.8e-13 (K') and 1.6e-13 (κ̇) that a 4801-point rule measured over v <= 5, ρ in [-0.999, 1].
    Measured here over QUAD_POINTS: K' 4.5e-14, κ̇ 9.4e-15; the two resolutions differ by
    2.9e-14 at most (the rounding of sums of 10^5 terms of values up to 7)."""
    worst_k = worst_kd = worst_res = 0.0
    for v1, v2, rho in QUAD_POINTS:
        k1, kd1 = _integrals(v1, v2, rho, 241)
        k2, kd2 = _integrals(v1, v2, rho, 321)
        worst_res = max(worst_res, abs(k1 - k2), abs(kd1 - kd2))
        c = rho * math.sqrt(v1 * v2)
        k, kd = GO.gelu_pair(*(torch.tensor(a, dtype=torch.float64) for a in (c, v1, v2)))
        worst_k = max(worst_k, abs(float(k) - k2))
        worst_kd = max(worst_kd, abs(float(kd) - kd2))
    print(f"closed form vs integral: K' {worst_k:.2e}, kdot {worst_kd:.2e} abs; "
          f"241 vs 321 points {worst_res:.2e}")
    assert worst_res < 1e-12
    assert worst_k < 5e-12 and worst_kd < 5e-12


def test_kdot_is_the_derivative_of_the_pair_form():
    """κ̇ = ∂K'/∂c at fixed variances, by autograd through the closed form itself"""
    rng = np.random.default_rng(5)
    v1, v2 = (torch.from_numpy(5 * rng.random(64)) for _ in range(2))
    c = (torch.from_numpy(rng.uniform(-1, 1, 64)) * torch.sqrt(v1 * v2)).requires_grad_()
    k, kd = GO.gelu_pair(c, v1, v2)
    g, = torch.autograd.grad(k.sum(), c)
    assert float((g - kd.detach()).abs().max()) < 1e-14


def test_variance_formula_is_the_pair_formula_on_the_diagonal():
    v = torch.tensor([0.0, 1e-6, 0.05, 0.5, 1.0, 3.0, 5.0, 40.0], dtype=torch.float64)
    k, kd = GO.gelu_pair(v, v, v)
    assert float(((GO.gelu_var(v) - k).abs() / (1 + k.abs())).max()) < 1e-15
    assert float((kd - GO.gelu_var_kdot(v)).abs().max()) < 1e-15
    assert float(k[0]) == 0.0 and float(kd[0]) == 0.25              # Φ(0)²
    # the overridden κ̇ is the partial derivative at fixed variances, not dv'/dv
    vv = v[2:].clone().requires_grad_()
    dv, = torch.autograd.grad(GO.gelu_var(vv).sum(), vv)
    assert float((dv - GO.gelu_var_kdot(v[2:])).abs().min()) > 1e-3
    # the same through the walk of a model: on identical images the overridden entries (the
    # variance stream) are the pair stream's, evaluated as same=False
    model = S(GE())
    x = np.random.default_rng(0).standard_normal((4, 3, 1, 1))
    kxx = GO.kernel(model, x)
    assert np.max(np.abs(kxx - GO.kernel(model, x, x, False, False))) < 1e-15
    assert np.max(np.abs(np.diag(kxx) - GO.kernel(model, x, x, True, True))) == 0.0
    assert np.max(np.abs(np.diag(kxx) - GO.gelu_var(torch.from_numpy((x * x).mean(1).ravel()))
                         .numpy())) == 0.0
    assert kxx.min() < 0 < kxx.max()                                # K' takes both signs


# ------------------------------------------------------------------------------------
# the oracle against itself
# ------------------------------------------------------------------------------------
def small_nets():
    return {
        "pure": S(C(3, var_bias=0.2), GE(), m.Sum([S(), S(C(3, var_weight=1.5), GE(), C(3))]),
                  GE(), C(6, padding=0)),
        "mixed": S(C(3, var_bias=0.1), R(), C(3), GE(), C(6, padding=0)),
    }


def images(seed=3, side=6):
    rng = np.random.default_rng(seed)
    return (rng.random((4, 2, side, side), dtype=np.float32).astype(np.float64),
            rng.random((3, 2, side, side), dtype=np.float32).astype(np.float64))


def masked_err(got, ref):
    """max |got - ref| / max |ref| over the entries where neither is NaN"""
    keep = ~(np.isnan(ref) | np.isnan(got))
    assert keep.any()
    return float(np.max(np.abs(got[keep] - ref[keep])) / np.max(np.abs(ref[keep])))


@pytest.mark.parametrize("name", ["pure", "mixed"])
def test_oracle_autograd_matches_stepwise(name):
    model = small_nets()[name].double()
    X, Z = images()
    k, th = GO.ntk_autograd(model, X, Z)
    sk, sth = GO.ntk_stepwise(model, X, Z, False, False)
    assert masked_err(k, sk) < 1e-12 and masked_err(th, sth) < 1e-12
    assert not np.isnan(th).any()
    assert masked_err(GO.kernel(model, X, Z, False, False), sk) < 1e-12
    # identical images: the overrides of same=True against autograd through same=False
    k, th = GO.ntk_autograd(model, X, X)
    sk, sth = GO.ntk_stepwise(model, X)
    if name == "mixed":
        # the ReLU map is singular at rho = 1 under same=False (ntk_oracle.ntk): masked
        idx = np.arange(len(X))
        k[idx, idx] = th[idx, idx] = np.nan
    else:
        assert not np.isnan(th).any()
    assert not np.isnan(th[~np.eye(len(X), dtype=bool)]).any()
    assert masked_err(k, sk) < 1e-12 and masked_err(th, sth) < 1e-12
    if name != "mixed":
        k, th = GO.ntk_autograd(model, X, X, diag=True)
        sk, sth = GO.ntk_stepwise(model, X, X, True, True)
        assert masked_err(k, sk) < 1e-12 and masked_err(th, sth) < 1e-12


def test_pooled_oracle_matches_the_layer_oracle():
    """a dense readout reads the p = p entries only: the walk on position-pair maps and the
    layer walk are two routes to one K"""
    body = lambda: [C(3, var_bias=0.1), GE(), C(3, var_weight=1.5), GE()]       # noqa: E731
    X, Z = images(side=4)
    head = C(4, padding=0, var_bias=0.2)
    want = GO.kernel(S(*body(), head).double(), X, Z, False, False)
    s = GO.position_covariance(S(*body()).double(), X, Z, False)
    got = head.var_weight / 16 * np.einsum("ijabab->ij", s) + head.var_bias
    assert masked_err(got, want) < 1e-13
    kxx = GO.kernel(S(*body(), head).double(), X)
    sxx = GO.position_covariance(S(*body()).double(), X)
    assert masked_err(head.var_weight / 16 * np.einsum("ijabab->ij", sxx) + head.var_bias,
                      kxx) < 1e-13


# ------------------------------------------------------------------------------------
# the package surface and the lowering
# ------------------------------------------------------------------------------------
def head_net():
    return S(C(3), GE(), C(4, padding=0))


def test_gelu_is_exported():
    assert "Gelu" in cnn_gp.__all__ and "Gelu" in cnn_gp.kernels.__all__
    assert issubclass(cnn_gp.Gelu, cnn_gp.NNGPKernel) and cnn_gp.Gelu().layers() == 0
    assert head_net().layers() == 2


def test_gelu_lowering_and_fusion():
    model = head_net()
    prog, v0, vf = compile_program(model, 4, 4)
    assert [o.kind for o in prog.ops] == ["conv", "gelu", "conv"]
    plan = Plan(model, 4, 4)
    kinds = [(o.kind, o.pre, o.post) for o in plan.pair_ops]
    assert kinds == [("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_NONE),
                     ("gelu", N.CGP_PRE_NONE, N.CGP_POST_NONE),
                     ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]
    gelu = plan.pair_ops[1]
    assert gelu.addend is None and gelu.src in plan.need_var and gelu.src in plan.ntk_need_var()
    assert plan.pool is None
    # rule 2: the identity skip of a residual block becomes the addend of its last op
    block = S(C(3), m.Sum([S(), S(C(3), GE())]), C(4, padding=0))
    plan = Plan(block, 4, 4)
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "gelu", "conv"]
    assert plan.pair_ops[2].addend == plan.pair_ops[0].dst
    # a gelu is never a conv's pre- or post-stage, with fusion on or off
    assert [o.kind for o in Plan(model, 4, 4, enable_fusion=False).pair_ops] == \
        ["conv", "gelu", "conv"]


def test_a_model_without_gelu_compiles_to_the_same_program():
    """the ops of a ReLU / Erf network name no gelu anywhere"""
    model = S(C(3), R(), m.Sum([S(), S(C(3), E())]), C(4, padding=0))
    plan = Plan(model, 4, 4)
    assert [o.kind for o in plan.prog.ops] == ["conv", "relu", "conv", "erf", "add", "conv"]
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "erf", "conv"]
    steps, _, _ = ntk_steps(plan.prog, plan.v0, plan.vf)
    assert not any("gelu" in s.fn for s in steps)


def test_gelu_models_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = head_net().double()
    plan = model._plan(4, 4)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    with pytest.raises(Unsupported):
        NetPlan(plan, 8)
    # at a geometry the whole-network kernel has (the reference ConvNet's), the op is the reason
    big = S(C(3), GE(), C(28, padding=0)).double()
    with pytest.raises(Unsupported) as e:
        NetPlan(big._plan(28, 28), 8)
    assert str(e.value) == "op gelu"
    NetPlan(S(C(3), R(), C(28, padding=0)).double()._plan(28, 28), 8)     # the ReLU twin lowers
    # the variance chain has no gelu record: it declines instead of raising
    assert plan._var_chain({plan.vf}, set(), torch.device("cpu")) is None
    # image_variances declines before touching a device for anything but device images
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


def test_gelu_ntk_steps():
    """Θ of the first conv's output is its K' buffer, so the gelu after it already carries Θ
    ("gelu_ntk"); a Gelu before any conv has Θ = 0 and is the plain forward pass ("gelu")"""
    prog, v0, vf = compile_program(head_net(), 4, 4)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["conv", "gelu_ntk", "conv", "conv"]
    assert steps[1].theta == steps[1].src == steps[0].dst and steps[1].var == steps[0].dst[1]
    assert steps[1].dst_theta == ("T", steps[1].op.dst) and steps[3].src == steps[1].dst_theta
    assert kbuf == ("K", vf) and tbuf == ("T", vf)
    prog, v0, vf = compile_program(S(GE(), C(4, padding=0)), 4, 4)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["gelu", "conv"]
    assert steps[0].theta is None and steps[0].dst_theta is None and tbuf == ("K", vf)
    # the erf steps' buffer lifetimes: the same reads and writes as the erf twin's
    for act in (E, GE):
        prog, v0, vf = compile_program(S(C(3), act(), C(3), act(), C(4, padding=0)), 4, 4)
        st = ntk_steps(prog, v0, vf)[0]
        if act is E:
            twin = [(s.reads(), s.writes()) for s in st]
    assert [(s.reads(), s.writes()) for s in st] == twin


def test_gelu_pool_steps():
    """a gelu upstream and downstream of an AvgPool2d: each a launch of its own, counted in
    need_var like a nonlinearity, the one downstream in self_var"""
    model = S(C(3), GE(), A(2), C(3, var_bias=0.1), GE(), G(), C(1))
    plan = Plan(model, 4, 4)
    ps = plan.pool
    assert [o.kind for o in plan.prog.ops] == ["conv", "gelu", "avgpool", "conv", "gelu", "pool",
                                               "conv"]
    v = [o.dst for o in plan.prog.ops]
    assert [s.fn for s in ps.steps] == ["moments", "conv", "gelu", "avgpool", "conv", "gelu",
                                        "pool", "conv"]
    g1, g2 = ps.steps[2], ps.steps[5]
    assert (g1.src, g1.var, g1.dst, g1.addend) == (v[0], v[0], v[1], None)
    assert (g2.src, g2.var, g2.dst, g2.addend) == (v[3], v[3], v[4], None)
    assert ps.need_var == {v[0], v[3]} and ps.self_var == {v[3]} and ps.self_last == 4
    assert ps.avgpooled == set(v[2:]) and ps.pooled == set(v[5:])
    assert ps.maps == {plan.v0} | set(v[:5]) and ps.scalars == set(v[5:])
    # rule 2 on the pooled path: the skip becomes the gelu launch's addend
    body = S(C(3), m.Sum([S(), S(C(3), GE())]))
    bs = pool_steps(*compile_program(body, 4, 4), body=True)
    assert [s.fn for s in bs.steps] == ["moments", "conv", "conv", "gelu"]
    assert bs.steps[3].addend == bs.steps[1].dst and bs.self_var == frozenset()
    # a ReLU twin keeps its launch list: no gelu step appears without a Gelu
    twin = Plan(S(C(3), R(), A(2), C(3, var_bias=0.1), R(), G(), C(1)), 4, 4).pool
    assert [s.fn for s in twin.steps] == ["moments", "conv", "avgpool", "conv", "nonlin", "pool",
                                          "conv"]


def test_gelu_after_the_global_pool_is_rejected():
    with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
        Plan(S(C(3), GE(), G(), GE()), 4, 4)
    assert str(e.value) == P.GELU_RULE_GLOBAL and "Gelu" in str(e.value)
    assert P.GELU_RULE_GLOBAL != P.POOL_RULE_NONLIN
    # the other rules hold with a Gelu in the model
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), GE(), G(), R()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), GE(), G(), G()), 4, 4)
    assert str(e.value) == P.POOL_RULE_ONE


def test_ntk_of_a_pooled_model_with_a_gelu_keeps_its_message():
    x = torch.ones(2, 1, 4, 4)
    corr = m.CorrelatedConv2d(4, padding=0, lengthscale=1.)
    for model, rule in ((S(C(3), GE(), G()), P.POOL_RULE_NTK),
                        (S(C(3), GE(), A(2), G()), P.AVGPOOL_RULE_NTK),
                        (S(C(3), GE(), corr), P.CORRCONV_RULE_NTK)):
        with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
            model.ntk(x)
        assert str(e.value) == rule


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {"cgp_gelu_args_size", "cgp_gelu_f64", "cgp_gelu_f32", "cgp_var_gelu_f64",
               "cgp_var_gelu_f32", "cgp_gelu_cov_args_size", "cgp_gelu_cov_f64",
               "cgp_gelu_cov_f32"}


def test_gelu_abi_and_symbols():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    assert lib.cgp_gelu_args_size() == ctypes.sizeof(N.GeluArgs) == ctypes.sizeof(N.ErfArgs)
    assert lib.cgp_gelu_cov_args_size() == ctypes.sizeof(N.GeluCovArgs) == 88
    assert [f[0] for f in N.GeluArgs._fields_] == [f[0] for f in N.ErfArgs._fields_]
    assert [f[0] for f in N.GeluCovArgs._fields_] == \
        [f[0] for f in N.CovNonlinArgs._fields_ if f[0] != "kind"]
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    syms = set(re.findall(r"\b(cgp_(?:var_)?gelu_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if "gelu" in s}
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s


def gelu_args(**kw):
    a = N.GeluArgs()
    a.xy, a.theta, a.out_xy, a.out_theta, a.xx, a.yy = 64, 128, 192, 256, 320, 384
    a.nmaps, a.n1, a.n2, a.hw = 6, 3, 2, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_gelu_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_gelu_{sfx}")
    args = gelu_args
    assert fn(None, None) == 1001
    for field in ("xy", "out_xy", "out_theta", "xx", "yy"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"gelu" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    # the forward-only form (theta NULL) passes the NULL check whatever out_theta is: the
    # next check is what rejects these
    for kw in (dict(theta=None), dict(theta=None, out_theta=None)):
        assert fn(ctypes.byref(args(nmaps=5, **kw)), None) == 1001
        assert b"nmaps inconsistent" in lib.cgp_last_error()
    # yy may be NULL only for same and diag
    assert fn(ctypes.byref(args(yy=None, same=1, n2=3, nmaps=9)), None) == 1001
    assert b"yy is NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(yy=None, diag=1, n2=3, nmaps=3)), None) == 1001
    assert b"yy is NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(yy=None, same=1, diag=1, n2=3, nmaps=3, hw=4096)), None) == 1001
    assert b"too large" in lib.cgp_last_error()                    # past the yy check
    assert fn(ctypes.byref(args(same=1)), None) == 1001           # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(diag=1, nmaps=3)), None) == 1001  # diag with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(nmaps=5)), None) == 1001          # nmaps != n1 n2
    assert b"nmaps inconsistent" in lib.cgp_last_error()
    for kw in (dict(nmaps=1 << 31, n1=1 << 16, n2=1 << 15), dict(nmaps=0, n1=0), dict(hw=0),
               dict(hw=-1)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(n2=0, nmaps=6)), None) == 1001
    assert fn(ctypes.byref(args(hw=2049)), None) == 1001          # larger than one chunk
    assert b"too large" in lib.cgp_last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_var_gelu_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_var_gelu_{sfx}")
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] = None
        assert fn(p[0], p[1], 2, 2, 4, 0, p[2], p[3], None) == 1001
        assert b"var_gelu" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    assert fn(64, 128, 2, 3, 4, 1, 192, 256, None) == 1001        # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    for n1, n2, hw in ((0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4)):
        assert fn(64, 128, n1, n2, hw, 0, 192, 256, None) == 1001
        assert b"bad sizes" in lib.cgp_last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_gelu_cov_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_gelu_cov_{sfx}")

    def args(**kw):
        a = N.GeluCovArgs()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        a.npairs, a.h, a.w = 3, 4, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert fn(None, None) == 1001
    for field in ("in_", "out", "xx", "yy", "pair_i", "pair_j"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"gelu_cov" in lib.cgp_last_error() and b"NULL" in lib.cgp_last_error()
    # sizes out of range: no pairs, too many, an empty map, (h·w)² past 2^30
    for kw in (dict(npairs=0), dict(npairs=-1), dict(npairs=1 << 31), dict(h=0), dict(w=0),
               dict(h=-4), dict(h=256, w=256), dict(h=182, w=182)):
        assert fn(ctypes.byref(args(**kw)), None) == 1001, kw
        assert b"bad sizes" in lib.cgp_last_error()
    # pairs·elements past what one launch counts in int32 blocks
    assert fn(ctypes.byref(args(npairs=(1 << 31) - 1, h=181, w=181)), None) == 1001
    assert b"elements" in lib.cgp_last_error()


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_gelu_model_without_gpu_raises_like_erf():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device") as erf:
        S(C(3), E(), C(4, padding=0))(x)
    with pytest.raises(RuntimeError, match="HIP device") as gelu:
        head_net()(x)
    assert str(gelu.value) == str(erf.value)
    with pytest.raises(RuntimeError, match="HIP device"):
        head_net().ntk(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        S(C(3), GE(), G())(x)


def test_gelu_model_empty_batches():
    model = head_net()
    x0, x = torch.zeros(0, 1, 4, 4), torch.ones(3, 1, 4, 4)
    assert tuple(model(x0).shape) == (0, 0)
    assert tuple(model(x0, x, False).shape) == (0, 3)
    assert tuple(model(x, x0, False).shape) == (3, 0)
    assert tuple(model(x0, x0, True, True).shape) == (0,)
    k, th = model.ntk(x0, x, False, return_nngp=True)
    assert tuple(k.shape) == tuple(th.shape) == (0, 3)
