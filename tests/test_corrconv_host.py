"""CPU-only tests of convs with correlated weights: the module's constructor rules, the
oracle (tests/corrconv_oracle.py) against a closed form and random finite networks that
share none of its code, the lowering of cnn_gp.CorrelatedConv2d (program op, pool_steps
launch lists, the rejections, the other paths declining) and the host side of
cgp_corrconv_*."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import program as P
from cnn_gp.program import Plan, compile_program, pool_steps

import avgpool_oracle as AO
import corrconv_oracle as CO
from test_pool_host import check_lifetimes

m = cnn_gp
C, R, S, G, A, CC = m.Conv2d, m.ReLU, m.Sequential, m.GlobalAvgPool, m.AvgPool2d, \
    m.CorrelatedConv2d


# ------------------------------------------------------------------------------------
# 1. the module
# ------------------------------------------------------------------------------------
def test_exports_and_helpers():
    for name in ("CorrelatedConv2d", "rbf_corr", "band_corr"):
        assert name in cnn_gp.__all__ and name in cnn_gp.kernels.__all__
    assert issubclass(CC, cnn_gp.NNGPKernel) and CC(3, lengthscale=1.).layers() == 1
    assert S(C(3), R(), CC(3, lengthscale=1.), G()).layers() == 2
    r = m.rbf_corr(4, 1.5)
    assert r.dtype == np.float64 and r.shape == (4, 4)
    a = np.arange(4)
    np.testing.assert_allclose(r, np.exp(-(a[:, None] - a[None, :]) ** 2 / (2 * 1.5 ** 2)),
                               rtol=1e-15)
    np.testing.assert_array_equal(m.rbf_corr(3, 0), np.eye(3))
    np.testing.assert_array_equal(m.rbf_corr(3, float("inf")), np.ones((3, 3)))
    b = m.band_corr(5, 1)
    assert b.dtype == np.float64
    a = np.arange(5)
    np.testing.assert_array_equal(b, (np.abs(a[:, None] - a[None, :]) <= 1) * 1.0)
    np.testing.assert_array_equal(m.band_corr(3, 0), np.eye(3))
    np.testing.assert_array_equal(m.band_corr(3, 2), np.ones((3, 3)))
    assert np.linalg.eigvalsh(m.band_corr(5, 1)).min() < 0            # not PSD: documented
    for bad in (lambda: m.rbf_corr(0, 1.), lambda: m.rbf_corr(3, -1.),
                lambda: m.rbf_corr(3, float("nan")), lambda: m.band_corr(0, 1),
                lambda: m.band_corr(3, -1)):
        with pytest.raises(ValueError):
            bad()


def test_constructor_rules():
    mod = CC(3, lengthscale=0)
    assert mod.corr_rows == mod.corr_cols == ((1., 0., 0.), (0., 1., 0.), (0., 0., 1.))
    mod = CC(2, lengthscale=float("inf"))
    assert mod.corr_rows == mod.corr_cols == ((1., 1.), (1., 1.))
    rr, rc = m.rbf_corr(3, 1.), m.band_corr(3, 1)
    mod = CC(3, stride=2, padding=0, dilation=2, var_weight=2., var_bias=.5, weight_corr=(rr, rc))
    assert mod.corr_rows == tuple(map(tuple, rr.tolist())) and mod.lengthscale is None
    assert mod.corr_cols == tuple(map(tuple, rc.tolist()))
    assert all(type(v) is float for row in mod.corr_rows for v in row)
    assert (mod.kernel_size, mod.stride, mod.padding, mod.dilation) == (3, 2, 0, 2)
    assert not list(mod.buffers())                                   # R is not a buffer
    # lists work as array-likes; the stored tuples do not alias the argument
    lst = [[1., .5], [.5, 1.]]
    mod = CC(2, weight_corr=(lst, lst))
    lst[0][1] = 7.
    assert mod.corr_rows == ((1., .5), (.5, 1.))
    # the padding rules are Conv2d's
    for k, d in ((3, 1), (2, 1), (4, 2), (5, 3)):
        a, b = CC(k, dilation=d, lengthscale=1.), C(k, dilation=d)
        assert (a.padding, a.kernel_has_row_of_zeros) == (b.padding, b.kernel_has_row_of_zeros)
        ga, gb = P.corrconv_geometry(a), P.conv_geometry(b)
        assert (ga.taps, ga.offset, ga.stride, ga.dilation, ga.extent) == \
            (gb.taps, gb.offset, gb.stride, gb.dilation, gb.extent)
        assert CO.tap_offset(a) == ga.offset
        assert P.conv_out_hw(a, 9, 8) == P.conv_out_hw(b, 9, 8)
    assert "lengthscale=1.0" in repr(CC(3, lengthscale=1)) and "weight_corr" in repr(mod)
    # the scale is var_weight/k² in double, not rounded to float32
    assert P.corrconv_geometry(CC(3, var_weight=1., lengthscale=1.)).weight == 1. / 9
    assert P.conv_geometry(C(3, var_weight=1.)).weight == float(np.float32(1. / 9))


def test_constructor_errors():
    eye = np.eye(3)
    for kw, msg in ((dict(), "exactly one"),
                    (dict(weight_corr=(eye, eye), lengthscale=1.), "exactly one"),
                    (dict(weight_corr=eye[0]), "pair"),
                    (dict(weight_corr=(eye, np.eye(2))), r"R_cols has shape \(2, 2\)"),
                    (dict(weight_corr=(np.ones((3, 2)), eye)), r"R_rows has shape \(3, 2\)"),
                    (dict(weight_corr=(eye, np.triu(np.ones((3, 3))))), "R_cols is not symmetric"),
                    (dict(weight_corr=(np.full((3, 3), np.nan), eye)), "R_rows has entries"),
                    (dict(weight_corr=(eye, np.full((3, 3), np.inf))), "R_cols has entries"),
                    (dict(lengthscale=-1.), "non-negative")):
        with pytest.raises(ValueError, match=msg):
            CC(3, **kw)
    with pytest.raises(ValueError, match="at least 1"):
        CC(0, lengthscale=1.)


def test_structure_key_follows_every_argument():
    base = dict(kernel_size=3, stride=1, padding="same", dilation=1, var_weight=1., var_bias=0.)
    rr = m.rbf_corr(3, 1.)
    key = lambda **kw: S(CC(**{**base, "weight_corr": (rr, rr), **kw}))._structure_key()   # noqa
    k0 = key()
    assert k0 == key()
    seen = {k0}
    for kw in (dict(kernel_size=2, weight_corr=(np.eye(2), np.eye(2))), dict(stride=2),
               dict(padding=0), dict(padding=1), dict(dilation=2), dict(var_weight=2.),
               dict(var_bias=.1), dict(weight_corr=None, lengthscale=1.),
               dict(weight_corr=None, lengthscale=2.), dict(weight_corr=(rr, np.eye(3)))):
        k = key(**kw)
        assert k not in seen, kw
        seen.add(k)
    r2 = rr.copy()
    r2[0, 2] = r2[2, 0] = 0.25                                       # one entry of R
    assert key(weight_corr=(r2, rr)) not in seen and key(weight_corr=(rr, r2)) not in seen
    assert key(weight_corr=(r2, rr)) != key(weight_corr=(rr, r2))
    # an attribute assigned later is seen as well (the plan cache's key)
    model = S(CC(3, lengthscale=1.), G())
    k1 = model._structure_key()
    model.mods[0].var_bias = .3
    assert model._structure_key() != k1
    assert model._plan(4, 4).prog.ops[0].geom.bias == .3


# ------------------------------------------------------------------------------------
# 2. the oracle without pair maps
# ------------------------------------------------------------------------------------
def random_corr(rng, k):
    r = rng.standard_normal((k, k))
    return (r + r.T) / 2


def test_single_readout_is_a_quadratic_form():
    """CorrelatedConv2d(H, padding=0) on raw images:
    K_ij = (w/k²)·mean_c x_i[c]ᵀ (R_rows ⊗ R_cols) y_j[c] + b"""
    rng = np.random.default_rng(3)
    k, w, b = 4, 1.7, 0.3
    rr, rc = random_corr(rng, k), random_corr(rng, k)
    X, Z = rng.standard_normal((3, 2, k, k)), rng.standard_normal((2, 2, k, k))
    model = S(CC(k, padding=0, var_weight=w, var_bias=b, weight_corr=(rr, rc)))
    kron = np.kron(rr, rc)
    quad = lambda x, y: np.einsum("icp,pq,jcq->ij", x.reshape(len(x), 2, -1), kron,      # noqa
                                  y.reshape(len(y), 2, -1)) / 2 * (w / k ** 2) + b
    np.testing.assert_allclose(CO.kernel(model, X, Z, False), quad(X, Z), rtol=1e-12)
    np.testing.assert_allclose(CO.kernel(model, X), quad(X, X), rtol=1e-12)
    np.testing.assert_allclose(CO.kernel(model, X, X, True, True), np.diag(quad(X, X)),
                               rtol=1e-12)


def test_oracle_special_cases():
    rng = np.random.default_rng(5)
    s = rng.standard_normal((2, 6, 5, 6, 5))
    # R = I is Conv2d (weights exact in float32), with stride, dilation and the even kernel
    for kw in (dict(kernel_size=3, var_weight=2.25, var_bias=.1),
               dict(kernel_size=3, stride=2, padding=0, dilation=2, var_weight=2.25),
               dict(kernel_size=2, var_weight=2.), dict(kernel_size=4, var_weight=4., stride=2)):
        np.testing.assert_allclose(CO.corrconv_map(s, CC(lengthscale=0, **kw)),
                                   AO.conv_map(s, C(**kw)), rtol=1e-13, atol=1e-13)
    # R = ones with stride k and no padding is AvgPool2d, var_weight k² making up the scale
    for k in (2, 3):
        got = CO.corrconv_map(s, CC(k, stride=k, padding=0, var_weight=1. / k ** 2,
                                    lengthscale=float("inf")))
        np.testing.assert_allclose(got, AO.avgpool_map(s, k, k), rtol=1e-13, atol=1e-14)


def test_oracle_matches_random_finite_networks():
    """CorrelatedConv2d (RBF, PSD), ReLU, dense readout, sampled with torch on the CPU: the
    hidden layer's filter taps are drawn with the correlation R_rows ⊗ R_cols (Cholesky
    factors on both axes).  The ReLU's pre-activation is exactly Gaussian given the inputs,
    so E_W[f(x)·f(y)] equals the kernel at any width; its variance has δ ≠ δ' terms of the
    input's self map, which only the diagonal of the self stream gives.  Width, draws, batch
    and the bound are tests/test_avgpool_host.py's: 5 standard errors from the sample
    itself."""
    width, draws, batch = 64, 4000, 500
    l1 = dict(var_weight=1.3, var_bias=0.2)
    l2 = dict(var_weight=0.9, var_bias=0.1)
    ls = 1.2
    model = S(CC(3, lengthscale=ls, **l1), R(), C(5, padding=0, **l2))
    rng = np.random.default_rng(15)
    X = rng.standard_normal((4, 3, 5, 5))
    ref = CO.kernel(model, X)
    np.testing.assert_allclose(CO.kernel(model, X[:2], X[2:], False), ref[:2, 2:], rtol=1e-13)
    np.testing.assert_allclose(CO.kernel(model, X, X, True, True), np.diag(ref), rtol=1e-13)
    # independent taps give another kernel: the test can tell the two apart
    indep = CO.kernel(S(CC(3, lengthscale=0, **l1), R(), C(5, padding=0, **l2)), X)
    assert np.max(np.abs(indep - ref) / np.abs(ref)) > 0.2

    chol = torch.from_numpy(np.linalg.cholesky(m.rbf_corr(3, ls)))
    gen = torch.Generator().manual_seed(16)
    x = torch.from_numpy(X)
    cin = X.shape[1]
    prods = []
    for _ in range(draws // batch):
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)    # noqa: E731
        w1 = torch.einsum("ia,ocab,jb->ocij", chol, rn(batch * width, cin, 3, 3), chol) \
            * (l1["var_weight"] / (9 * cin)) ** 0.5
        b1 = rn(batch * width) * l1["var_bias"] ** 0.5
        w2 = rn(batch, width, 5, 5) * (l2["var_weight"] / (25 * width)) ** 0.5
        b2 = rn(batch) * l2["var_bias"] ** 0.5
        a = F.relu(F.conv2d(x, w1, b1, padding=1))                     # [4, batch·width, 5, 5]
        f = F.conv2d(a, w2, b2, groups=batch).reshape(4, batch)
        prods.append(f[:, None, :] * f[None, :, :])
    prods = torch.cat(prods, dim=2).numpy()                            # [4, 4, draws]
    est = prods.mean(axis=2)
    se = prods.std(axis=2, ddof=1) / np.sqrt(draws)
    zscore = np.abs(est - ref) / se
    print(f"finite networks with CorrelatedConv2d: worst |z| = {zscore.max():.2f} standard "
          f"errors, relative standard error {np.max(se / np.abs(ref)):.3f}")
    assert np.all(zscore < 5), zscore


# ------------------------------------------------------------------------------------
# 3. lowering
# ------------------------------------------------------------------------------------
def steps_of(model, h, w, body=False):
    prog, v0, vf = compile_program(model, h, w)
    return pool_steps(prog, v0, vf, body=body), prog, v0, vf


def test_compile_program_emits_corrconv():
    rr, rc = m.rbf_corr(3, 1.), m.band_corr(3, 1)
    mod = CC(3, stride=2, padding=0, dilation=2, var_weight=1.8, var_bias=.5, weight_corr=(rr, rc))
    prog, v0, vf = compile_program(S(C(3), mod), 9, 7)
    assert [o.kind for o in prog.ops] == ["conv", "corrconv"]
    op = prog.ops[1]
    g = op.geom
    assert op.src == prog.ops[0].dst and op.shape_in == (9, 7) and op.shape_out == (3, 2)
    assert isinstance(g, P.CorrGeom) and isinstance(g, P.ConvGeom)
    assert (g.taps, g.offset, g.stride, g.dilation, g.extent) == (3, 0, 2, 2, 3)
    assert g.weight == 1.8 / 9 and g.bias == .5
    assert g.corr_rows == mod.corr_rows and g.corr_cols == mod.corr_cols
    with pytest.raises(RuntimeError, match="produces an empty output"):
        compile_program(S(CC(5, padding=0, lengthscale=1.)), 4, 4)


def test_fusion_never_crosses_a_corrconv():
    cc = lambda: CC(3, lengthscale=1.)                                           # noqa: E731
    prog, v0, vf = compile_program(S(cc(), R(), cc(), m.Sum([S(cc()), S(C(3))])), 4, 4)
    ops = P.fuse(prog, v0, vf, True)
    assert [o.kind for o in ops] == [o.kind for o in prog.ops] == \
        ["corrconv", "relu", "corrconv", "corrconv", "conv", "add"]
    assert all(o.post == N.CGP_POST_NONE and o.addend is None and o.pre == N.CGP_PRE_NONE
               for o in ops)


def test_pool_steps_hidden_layer_with_a_relu():
    model = S(C(3, var_bias=.1), R(), CC(3, lengthscale=1., var_bias=.2), R(), G(),
              C(1, var_weight=2.))
    ps, prog, v0, vf = steps_of(model, 6, 5)
    ops = prog.ops
    assert [s.fn for s in ps.steps] == ["moments", "conv", "corrconv", "nonlin", "pool", "conv"]
    conv, corr, relu = ps.steps[1:4]
    assert conv.post == N.CGP_COV_RELU and conv.var == ops[0].dst           # upstream: fused
    assert corr.src == ops[1].dst and corr.dst == ops[2].dst and corr.op.geom is ops[2].geom
    assert corr.post == N.CGP_COV_NONE and corr.var is None and corr.addend is None
    assert relu.post == N.CGP_COV_RELU and relu.src == relu.var == ops[2].dst
    assert ps.need_var == {ops[0].dst, ops[2].dst}
    assert ps.self_var == {ops[2].dst} and ps.self_last == 2
    assert ps.avgpooled == {o.dst for o in ops[2:]}
    assert ps.pooled == ps.scalars == {ops[4].dst, vf}
    assert check_lifetimes(ps) == 2 * 30 ** 2
    assert corr.free == [ops[1].dst]
    # a conv downstream keeps its ReLU as a launch of its own, as after an AvgPool2d
    ps, prog, *_ = steps_of(S(CC(3, lengthscale=1.), C(3), R(), G()), 4, 4)
    assert [s.fn for s in ps.steps] == ["moments", "corrconv", "conv", "nonlin", "pool"]
    assert ps.self_var == {prog.ops[1].dst} and ps.self_last == 2


def test_pool_steps_readout():
    model = S(C(3), R(), CC(4, padding=0, weight_corr=(m.band_corr(4, 1),) * 2, var_bias=.1))
    plan = Plan(model, 4, 4)
    ps = plan.pool
    assert ps is not None and plan.final_hw == (1, 1)
    assert [s.fn for s in ps.steps] == ["moments", "conv", "corrconv"]
    assert not ps.pooled and not ps.scalars and ps.final in ps.maps and ps.elems(ps.final) == 1
    assert not ps.self_var and ps.self_last == -1 and ps.need_var == {plan.prog.ops[0].dst}
    assert check_lifetimes(ps) == 2 * 16 ** 2
    # a body for position_covariance
    body = Plan(S(C(3), CC(2, lengthscale=.5), R()), 6, 5)
    assert body.final_hw == (6, 5) and body.body_steps().final == body.vf
    assert [s.fn for s in body.body_steps().steps] == ["moments", "conv", "corrconv", "nonlin"]
    assert body.body_steps().self_var == {body.prog.ops[1].dst}


def test_pool_steps_in_a_sum_branch():
    model = S(C(3), m.Sum([S(CC(3, lengthscale=1.)), S(R(), C(3))]), R(), G())
    ps, prog, v0, vf = steps_of(model, 4, 4)
    ops = prog.ops
    assert [o.kind for o in ops] == ["conv", "corrconv", "relu", "conv", "add", "relu", "pool"]
    # the Sum stays a launch: no conv takes the correlated branch as its addend
    assert [s.fn for s in ps.steps] == ["moments", "conv", "corrconv", "nonlin", "conv", "axpby",
                                        "nonlin", "pool"]
    assert all(s.addend is None for s in ps.steps)
    axpby = ps.steps[5]
    assert axpby.terms == [(None, ops[1].dst), (None, ops[3].dst)] and axpby.dst == ops[4].dst
    assert ps.need_var == {ops[0].dst, ops[4].dst}
    assert ps.self_var == {ops[4].dst} and ps.self_last == 5
    assert ps.avgpooled == {ops[1].dst, ops[4].dst, ops[5].dst, vf}
    check_lifetimes(ps)


def test_rejections():
    cc = lambda **kw: CC(1, lengthscale=1., **kw)                                # noqa: E731
    for model in (S(C(3), G(), cc()), S(CC(3, lengthscale=1.), G(), C(1), cc())):
        with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
            Plan(model, 4, 4)
        assert str(e.value) == P.CORRCONV_RULE_GLOBAL and "CorrelatedConv2d" in str(e.value)
    x = torch.ones(2, 1, 4, 4)
    for model in (S(C(3), R(), CC(3, lengthscale=1.), G()),
                  S(CC(3, lengthscale=1.), R(), A(2), CC(2, padding=0, lengthscale=1.))):
        with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
            model.ntk(x)
        assert str(e.value) == P.CORRCONV_RULE_NTK and "CorrelatedConv2d" in str(e.value)
        with pytest.raises(NotImplementedError) as e:
            model.ntk(x[:0])
        assert str(e.value) == P.CORRCONV_RULE_NTK
    assert len({P.CORRCONV_RULE_NTK, P.AVGPOOL_RULE_NTK, P.POOL_RULE_NTK}) == 3
    assert P.CORRCONV_RULE_GLOBAL != P.AVGPOOL_RULE_GLOBAL
    # the existing rules hold with the module in the model
    with pytest.raises(NotImplementedError) as e:
        Plan(S(CC(3, lengthscale=1.), G(), R()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN


def test_other_paths_decline():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(C(3), R(), CC(4, padding=0, lengthscale=1.)).double()
    plan = model._plan(4, 4)
    assert plan.pool is not None and plan.final_hw == (1, 1)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    for body in (S(R(), CC(4, padding=0, lengthscale=1.)), S(R(), CC(3, lengthscale=1.), G())):
        with pytest.raises(Unsupported, match="op corrconv"):
            NetPlan(body.double()._plan(4, 4), 8)
    assert plan._var_chain({plan.prog.ops[0].dst}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


def test_empty_batches_and_a_final_value_that_is_not_1x1():
    model = S(CC(3, lengthscale=1.), R())
    x0, x = torch.zeros(0, 1, 4, 4), torch.ones(3, 1, 4, 4)
    assert Plan(model, 4, 4).pool is not None
    assert tuple(model(x0, x, False).shape) == (0, 3)
    assert tuple(model(x0).shape) == (0, 0)
    assert tuple(model.position_covariance(x0, x, False).shape) == (0, 3, 4, 4, 4, 4)
    readout = S(CC(4, padding=0, lengthscale=1.))
    assert tuple(readout(x, x0, False).shape) == (3, 0)
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="4x4 per pair, not 1x1"):
            model(x)
    else:
        with pytest.raises(RuntimeError, match="HIP device"):
            model(x)


def test_a_model_without_the_module_compiles_as_before():
    plan = Plan(S(C(3), R(), C(5, padding=0)), 5, 5)
    assert plan.pool is None and [o.kind for o in plan.prog.ops] == ["conv", "relu", "conv"]
    assert [(o.kind, o.pre, o.post) for o in plan.pair_ops] == \
        [("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_RELU), ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]
    # rule 2 still folds a Sum of convs into an addend
    plan = Plan(S(C(3), m.Sum([S(), S(R(), C(3))])), 4, 4)
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv"]
    assert plan.pair_ops[1].addend == plan.prog.ops[0].dst
    ps = Plan(S(C(3), R(), A(2), C(3), R(), G()), 4, 4).pool
    assert [s.fn for s in ps.steps] == ["moments", "conv", "avgpool", "conv", "nonlin", "pool"]
    assert all(type(o.geom) in (P.ConvGeom, P.PoolGeom, type(None))
               for o in Plan(S(C(3), A(2), G()), 4, 4).prog.ops)


# ------------------------------------------------------------------------------------
# 4. ABI and the entry point's argument checks
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {"cgp_corrconv_args_size", "cgp_corrconv_f64", "cgp_corrconv_f32"}


def test_corrconv_abi():
    from conftest import ROOT
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    assert "#define CGP_ABI_VERSION 12" in txt
    syms = set(re.findall(r"\b(cgp_corrconv_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if s.startswith("cgp_corrconv_")}
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert lib.cgp_corrconv_args_size() == ctypes.sizeof(N.CorrConvArgs) == 88
    fields = [f[0] for f in N.CorrConvArgs._fields_]
    assert fields == ["in_", "out", "corr_rows", "corr_cols", "npairs", "h", "w", "ho", "wo",
                      "taps", "offset", "stride", "dilation", "weight", "bias"]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_point_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    EINVAL = 1001
    fn = getattr(lib, f"cgp_corrconv_{sfx}")
    assert fn(None, None) == EINVAL and b"NULL" in lib.cgp_last_error()

    def args(**kw):
        a = N.CorrConvArgs()
        a.in_, a.out, a.corr_rows, a.corr_cols = 64, 128, 192, 256
        a.npairs, a.h, a.w, a.ho, a.wo = 6, 7, 6, 4, 3
        a.taps, a.offset, a.stride, a.dilation = 3, -1, 2, 1
        a.weight, a.bias = 1. / 9, .1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    item = 8 if sfx == "f64" else 4
    # a w x w block of sums and both tables above 64 KB: by the block, and by the tables
    wide = 91 if sfx == "f64" else 128
    assert wide ** 2 * item + 2 * 9 * item > 64 * 1024
    taps = 60 if sfx == "f64" else 88
    assert 2 * taps ** 2 * item + 40 ** 2 * item > 64 * 1024 > 40 ** 2 * item
    for kw, msg in ((dict(in_=None), b"NULL"), (dict(out=None), b"NULL"),
                    (dict(corr_rows=None), b"NULL"), (dict(corr_cols=None), b"NULL"),
                    (dict(out=64), b"must not be in"),
                    (dict(npairs=0), b"bad sizes"), (dict(npairs=1 << 31), b"bad sizes"),
                    (dict(h=0), b"bad sizes"), (dict(w=-1), b"bad sizes"),
                    (dict(ho=0), b"bad sizes"), (dict(wo=0), b"bad sizes"),
                    (dict(h=200, w=200, ho=99, wo=99), b"bad sizes"),   # (h w)² above 2^30
                    (dict(taps=0), b"bad geometry"), (dict(stride=0), b"bad geometry"),
                    (dict(dilation=0), b"bad geometry"), (dict(taps=-2), b"bad geometry"),
                    (dict(dilation=1 << 30), b"bad geometry"),
                    (dict(offset=-(1 << 24)), b"bad geometry"),
                    (dict(ho=5), b"all miss"),          # the last row's first tap is row 7
                    (dict(wo=5), b"all miss"),
                    (dict(offset=-3), b"all miss"),     # the first output's taps end at -1
                    (dict(h=4, w=wide, ho=2, wo=(wide + 1) // 2), b"of LDS"),
                    (dict(h=40, w=40, taps=taps, offset=0, stride=1, ho=1, wo=1), b"of LDS")):
        assert fn(ctypes.byref(args(**kw)), None) == EINVAL, kw
        assert msg in lib.cgp_last_error(), (kw, lib.cgp_last_error())
