"""CPU-only tests of windowed average pooling: the three-stream oracle
(tests/avgpool_oracle.py) against the existing pooled oracle, random finite networks and a
closed form that share none of its code; the lowering of cnn_gp.AvgPool2d (program op,
pool_steps launch lists, the self-pass fields, the rejections, the whole-network path
declining); and the host side of cgp_covmap_avgpool_* / cgp_covmap_diag_*.

The entry points are named cgp_covmap_*, not cgp_cov_*: tests/test_pool_host.py pins the
cgp_cov_ family of include/cnngp.h to its ten symbols."""
import ctypes
import math
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
import pool_oracle as PO
from test_pool_host import check_lifetimes

m = cnn_gp
C, R, E, S, G, A = m.Conv2d, m.ReLU, m.Erf, m.Sequential, m.GlobalAvgPool, m.AvgPool2d

F32_TINY = float(np.finfo(np.float32).tiny)


# ------------------------------------------------------------------------------------
# 1. the three-stream walk reproduces the closed variance recursion
# ------------------------------------------------------------------------------------
def unpooled_bodies():
    return {
        "chain": [C(3, var_bias=0.1), R(), C(3, stride=2, var_weight=1.5), R(), C(3)],
        "resnet": [C(3), m.resnet_block(), R()],
        "erf": [C(3, var_bias=0.2), E(), C(3, var_weight=1.5), E()],
    }


@pytest.mark.parametrize("name", list(unpooled_bodies()))
def test_oracle_equals_the_existing_one_without_avgpool(name):
    body = unpooled_bodies()[name]
    rng = np.random.default_rng(11)
    X, Z = rng.random((3, 2, 5, 4)), rng.random((2, 2, 5, 4))
    for args in ((X,), (X, Z, False, False), (X[:2], Z, False, True), (X, X, True, True)):
        np.testing.assert_allclose(AO.kernel(S(*body, G()), *args),
                                   PO.kernel(S(*body, G()), *args), rtol=1e-13)
        np.testing.assert_allclose(AO.position_covariance(S(*body), *args),
                                   PO.position_covariance(S(*body), *args), rtol=1e-13,
                                   atol=1e-300)


# ------------------------------------------------------------------------------------
# 2. random finite networks
# ------------------------------------------------------------------------------------
def test_oracle_matches_random_finite_networks():
    """conv, AvgPool2d(2), ReLU, conv, GlobalAvgPool with bias variances, sampled with torch
    on the CPU.  The one nonlinearity sits after the pool: its pre-activation, a window mean
    of the first layer's, is exactly Gaussian given the inputs, so E_W[f(x)·f(y)] equals the
    kernel at any width -- and its variance is the one the closed recursion cannot give.
    Finite network and bound as tests/test_pool_host.py: 5 standard errors, estimated from
    the sample itself."""
    width, draws, batch = 64, 4000, 500
    l1 = dict(var_weight=1.3, var_bias=0.2)
    l2 = dict(var_weight=0.9, var_bias=0.1)
    model = S(C(3, **l1), A(2), R(), C(3, **l2), G())
    rng = np.random.default_rng(15)
    X = rng.standard_normal((4, 3, 6, 4))
    ref = AO.kernel(model, X)
    np.testing.assert_allclose(AO.kernel(model, X[:2], X[2:], False), ref[:2, 2:], rtol=1e-13)
    np.testing.assert_allclose(AO.kernel(model, X, X, True, True), np.diag(ref), rtol=1e-13)

    gen = torch.Generator().manual_seed(16)
    x = torch.from_numpy(X)
    cin = X.shape[1]
    prods = []
    for _ in range(draws // batch):
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)    # noqa: E731
        w1 = rn(batch * width, cin, 3, 3) * (l1["var_weight"] / (9 * cin)) ** 0.5
        b1 = rn(batch * width) * l1["var_bias"] ** 0.5
        w2 = rn(batch, width, 3, 3) * (l2["var_weight"] / (9 * width)) ** 0.5
        b2 = rn(batch) * l2["var_bias"] ** 0.5
        a = F.relu(F.avg_pool2d(F.conv2d(x, w1, b1, padding=1), 2))    # [4, batch·width, 3, 2]
        z = F.conv2d(a, w2, b2, padding=1, groups=batch)               # [4, batch, 3, 2]
        f = z.mean(dim=(2, 3))                                         # [4, batch]
        prods.append(f[:, None, :] * f[None, :, :])
    prods = torch.cat(prods, dim=2).numpy()                            # [4, 4, draws]
    est = prods.mean(axis=2)
    se = prods.std(axis=2, ddof=1) / np.sqrt(draws)
    zscore = np.abs(est - ref) / se
    print(f"finite networks with AvgPool2d: worst |z| = {zscore.max():.2f} standard errors, "
          f"relative standard error {np.max(se / np.abs(ref)):.3f}")
    assert np.all(zscore < 5), zscore


# ------------------------------------------------------------------------------------
# 3. a closed form: linear up to the pool, then one ReLU formula
# ------------------------------------------------------------------------------------
def relu_formula(c, v1, v2):
    """the reference's ReLU covariance (kernels.py:146-152) of scalars"""
    t = v1 * v2 + F32_TINY
    cos = min(1.0, max(-1.0, c / math.sqrt(t)))
    return (math.sqrt(max(t - c * c, 0.0)) + (math.pi - math.acos(cos)) * c) / (2 * math.pi)


@pytest.mark.parametrize("h,w,k,s", [(6, 5, 2, 2), (7, 6, 3, 2)], ids=["k2s2_6x5", "k3s2_7x6"])
def test_oracle_matches_the_linear_closed_form_with_one_relu(h, w, k, s):
    """conv, AvgPool2d, ReLU, GlobalAvgPool.  The pooled pre-activation at P is the window
    mean of the conv's, so c[P, Q] = k⁻⁴·Σ_{δ, δ'} cov(z_i[P·s + δ], z_j[Q·s + δ']) with
    cov(z_i[p], z_j[q]) = bias + (weight/C)·Σ_taps Σ_c x_i[c, p + tap]·x_j[c, q + tap] (zero
    padded), v_i[P] = c_ii[P, P], and K_ij is the mean over (P, Q) of the ReLU formula of
    (c, v_i[P], v_j[Q]) -- plain loops over taps and windows, no pair map anywhere.
    6x5 with k = s = 2 drops a column; 7x6 with k = 3, s = 2 has overlapping windows."""
    conv = C(3, var_weight=1.7, var_bias=0.3)
    g = P.conv_geometry(conv)
    rng = np.random.default_rng(8)
    X, Z = rng.standard_normal((2, 2, h, w)), rng.standard_normal((2, 2, h, w))
    ho, wo = (h - k) // s + 1, (w - k) // s + 1

    def at(img, r, c):
        return img[:, r, c] if 0 <= r < h and 0 <= c < w else np.zeros(img.shape[0])

    def zcov(xi, xj, p, q):
        acc = 0.0
        for a in range(g.taps):
            for b in range(g.taps):
                da, db = g.offset + a * g.dilation, g.offset + b * g.dilation
                acc += np.mean(at(xi, p[0] + da, p[1] + db) * at(xj, q[0] + da, q[1] + db))
        return g.weight * acc + g.bias

    def ccov(xi, xj, pp, qq):
        acc = 0.0
        for a in range(k):
            for b in range(k):
                for a2 in range(k):
                    for b2 in range(k):
                        acc += zcov(xi, xj, (pp[0] * s + a, pp[1] * s + b),
                                    (qq[0] * s + a2, qq[1] * s + b2))
        return acc / k ** 4

    cells = [(r, c) for r in range(ho) for c in range(wo)]

    def var_map(img):
        return {pp: ccov(img, img, pp, pp) for pp in cells}

    def kern(xi, xj, vi, vj, same_image):
        tot = 0.0
        for pp in cells:
            for qq in cells:
                if same_image and pp == qq:
                    tot += vi[pp] / 2                          # kernels.py:155-162
                else:
                    tot += relu_formula(ccov(xi, xj, pp, qq), vi[pp], vj[qq])
        return tot / len(cells) ** 2

    vx, vz = [var_map(x) for x in X], [var_map(z) for z in Z]
    model = S(conv, A(k, s), R(), G())
    want_xz = np.array([[kern(X[i], Z[j], vx[i], vz[j], False) for j in range(2)]
                        for i in range(2)])
    np.testing.assert_allclose(AO.kernel(model, X, Z, False), want_xz, rtol=1e-12)
    want_xx = np.array([[kern(X[i], X[j], vx[i], vx[j], i == j) for j in range(2)]
                        for i in range(2)])
    np.testing.assert_allclose(AO.kernel(model, X), want_xx, rtol=1e-12)


# ------------------------------------------------------------------------------------
# 4. the pool over the whole map
# ------------------------------------------------------------------------------------
def test_whole_map_avgpool_then_global_is_global():
    rng = np.random.default_rng(12)
    X, Z = rng.random((3, 2, 5, 5)), rng.random((2, 2, 5, 5))
    body = [C(3, var_bias=0.1), R(), C(3)]
    for args in ((X,), (X, Z, False, False), (X, X, True, True)):
        np.testing.assert_allclose(AO.kernel(S(*body, A(5), G()), *args),
                                   AO.kernel(S(*body, G()), *args), rtol=1e-13)
    s = rng.random((2, 4, 4, 4, 4))
    np.testing.assert_array_equal(AO.avgpool_map(s, 1, 1), s)
    np.testing.assert_allclose(AO.avgpool_map(s, 4, 4)[:, 0, 0, 0, 0], s.mean(axis=(1, 2, 3, 4)),
                               rtol=1e-13)


# ------------------------------------------------------------------------------------
# 5. host logic: the module, the program op, the launch lists
# ------------------------------------------------------------------------------------
def test_avgpool_is_exported():
    assert "AvgPool2d" in cnn_gp.__all__ and "AvgPool2d" in cnn_gp.kernels.__all__
    assert issubclass(A, cnn_gp.NNGPKernel) and A(2).layers() == 0
    assert (A(2).kernel_size, A(2).stride) == (2, 2) and (A(3, 2).kernel_size, A(3, 2).stride) \
        == (3, 2)
    assert S(C(3), R(), A(2), C(3), G()).layers() == 2
    assert "kernel_size=3, stride=2" in repr(A(3, stride=2))


def test_compile_program_emits_avgpool():
    prog, v0, vf = compile_program(S(C(3), A(2), R(), A(3, 2)), 9, 7)
    assert [o.kind for o in prog.ops] == ["conv", "avgpool", "relu", "avgpool"]
    a, _, b = prog.ops[1:]
    assert a.shape_in == (9, 7) and a.shape_out == (4, 3) == prog.shapes[a.dst]   # floor
    assert (a.geom.taps, a.geom.stride) == (2, 2) and a.src == prog.ops[0].dst
    assert b.shape_in == (4, 3) and b.shape_out == (1, 1) and (b.geom.taps, b.geom.stride) == (3, 2)
    assert compile_program(S(A(2, 1)), 5, 4)[0].ops[0].shape_out == (4, 3)
    for model, hw in ((S(A(5)), (4, 6)), (S(A(2), A(2), A(2)), (4, 4)), (S(A(3, 7)), (7, 2))):
        with pytest.raises(RuntimeError, match="AvgPool2d.*produces an empty output"):
            compile_program(model, *hw)
    with pytest.raises(RuntimeError, match="produces an empty output"):   # conv_out_hw's kind
        compile_program(S(C(5, padding=0)), 4, 4)
    # a model without the module compiles to the program it compiled to before
    plan = Plan(S(C(3), R(), C(5, padding=0)), 5, 5)
    assert plan.pool is None and all(o.kind != "avgpool" for o in plan.prog.ops)
    ps = Plan(S(C(3), R(), G()), 5, 5).pool
    assert not ps.avgpooled and not ps.self_var and ps.self_last == -1


def test_fusion_never_crosses_an_avgpool():
    """rule 1 (conv -> relu), rule 2 (a Sum as an addend) and rule 3 (relu -> conv) each
    with an AvgPool2d in between"""
    prog, v0, vf = compile_program(
        S(C(3), A(2), R(), A(1), C(3), m.Sum([S(A(1)), S(C(3), A(1))])), 4, 4)
    ops = P.fuse(prog, v0, vf, True)
    assert [o.kind for o in ops] == [o.kind for o in prog.ops] == \
        ["conv", "avgpool", "relu", "avgpool", "conv", "avgpool", "conv", "avgpool", "add"]
    assert all(o.post == N.CGP_POST_NONE and o.addend is None for o in ops)
    assert all(o.pre == N.CGP_PRE_NONE for o in ops[1:]) and ops[0].pre == N.CGP_PRE_MOMENTS


def steps_of(model, h, w, body=False):
    prog, v0, vf = compile_program(model, h, w)
    return pool_steps(prog, v0, vf, body=body), prog, v0, vf


def test_pool_steps_chain():
    model = S(C(3, var_bias=0.1), R(), C(3), R(), A(2), C(3), R(), A(2), G(),
              C(1, var_weight=2., var_bias=0.3))
    ps, prog, v0, vf = steps_of(model, 8, 8)
    # upstream of the first pool the ReLUs ride on their convs; downstream the conv's output
    # is a buffer of its own, whose diagonal the ReLU reads
    assert [s.fn for s in ps.steps] == ["moments", "conv", "conv", "avgpool", "conv", "nonlin",
                                        "avgpool", "pool", "conv"]
    ops = prog.ops
    assert [s.post for s in ps.steps[1:3]] == [N.CGP_COV_RELU] * 2
    conv3, relu3 = ps.steps[4:6]
    assert conv3.post == N.CGP_COV_NONE and conv3.var is None and conv3.dst == ops[5].dst
    assert relu3.post == N.CGP_COV_RELU and relu3.src == relu3.var == ops[5].dst
    assert relu3.dst == ops[6].dst
    assert (ps.steps[3].op.geom.taps, ps.steps[3].op.geom.stride) == (2, 2)
    assert ps.need_var == {ops[0].dst, ops[2].dst, ops[5].dst}
    assert ps.self_var == {ops[5].dst} and ps.self_last == 4
    assert ps.avgpooled == {o.dst for o in ops[4:]}
    assert ps.pooled == ps.scalars == {ops[8].dst, vf}
    assert [ps.shapes[s.dst] for s in ps.steps] == [(8, 8)] * 3 + [(4, 4)] * 3 + [(2, 2)] + \
        [(1, 1)] * 2
    assert ps.elems(ops[4].dst) == 256 and ps.elems(ops[7].dst) == 16 and ps.elems(vf) == 1
    # the fullest launch is a conv on the un-pooled maps; a pool's is 64² + 16²
    assert check_lifetimes(ps) == 2 * 64 ** 2
    assert ps.steps[3].free == [ops[3].dst]


def test_pool_steps_without_a_nonlinearity_after_the_pool():
    for model in (S(C(3), R(), A(2), C(3), G()), S(C(3), R(), A(2), G()), S(A(2), C(3), G())):
        ps, prog, v0, vf = steps_of(model, 4, 4)
        assert not ps.self_var and ps.self_last == -1 and ps.avgpooled
        assert ps.need_var <= {prog.ops[0].dst}
        check_lifetimes(ps)


def test_pool_steps_avgpool_in_a_sum_branch():
    model = S(C(3), m.Sum([S(A(2), C(3)), S(R(), C(3, stride=2), R())]), R(), G())
    ps, prog, v0, vf = steps_of(model, 6, 6)
    # branch 1: pool, conv; branch 2: standalone ReLU (the conv output also feeds branch 1),
    # conv with its ReLU -- upstream of every pool on ITS path, so still fused -- which also
    # takes the Sum as its addend (rule 2); the ReLU after the Sum reads a self variance
    assert [s.fn for s in ps.steps] == ["moments", "conv", "avgpool", "conv", "nonlin", "conv",
                                        "nonlin", "pool"]
    ops = prog.ops
    fused = ps.steps[5]
    assert fused.post == N.CGP_COV_RELU and fused.addend == ps.steps[3].dst
    assert fused.var == ops[4].dst and fused.var not in ps.avgpooled
    last = ps.steps[6]
    assert last.var == last.src == fused.dst and last.var in ps.avgpooled
    assert ps.self_var == {fused.dst} and ps.self_last == 5
    assert ps.need_var == {ops[0].dst, ops[4].dst, fused.dst}
    assert ps.avgpooled == {ops[1].dst, ops[2].dst, fused.dst, ops[7].dst, vf}
    # the conv output (36²) lives beside the pooled branch (9² twice) and the ReLU's map
    assert check_lifetimes(ps) == 2 * 36 ** 2 + 81
    assert ps.steps[4].free == [ops[0].dst]


def test_dense_readout_and_body_steps():
    """no GlobalAvgPool: the plan's launch list ends in a map, 1x1 for forward"""
    model = S(C(3), R(), A(2), C(3), R(), C(4, padding=0))
    plan = Plan(model, 8, 8)
    ps = plan.pool
    assert ps is not None and plan.final_hw == (1, 1)
    assert [s.fn for s in ps.steps] == ["moments", "conv", "avgpool", "conv", "nonlin", "conv"]
    assert not ps.pooled and not ps.scalars and ps.final in ps.maps and ps.elems(ps.final) == 1
    assert ps.self_var == {plan.prog.ops[3].dst} and ps.self_last == 3
    check_lifetimes(ps)
    body = Plan(S(C(3), A(2), R()), 6, 5)
    assert body.final_hw == (3, 2) and body.body_steps().final == body.vf
    assert [s.fn for s in body.body_steps().steps] == ["moments", "conv", "avgpool", "nonlin"]
    assert body.body_steps().self_var == {body.prog.ops[1].dst}


# ------------------------------------------------------------------------------------
# the rejections
# ------------------------------------------------------------------------------------
def test_avgpool_after_the_global_pool_is_rejected():
    for model in (S(C(3), G(), A(1)), S(C(3), A(2), G(), C(1), A(1))):
        with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
            Plan(model, 4, 4)
        assert str(e.value) == P.AVGPOOL_RULE_GLOBAL and "AvgPool2d" in str(e.value)


def test_existing_pool_rules_hold_with_an_avgpool():
    with pytest.raises(NotImplementedError) as e:
        Plan(S(C(3), A(2), G(), R()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN
    with pytest.raises(NotImplementedError) as e:            # one path without the global pool
        Plan(S(C(3), A(4), m.Sum([S(G()), S()])), 4, 4)
    assert str(e.value) == P.POOL_RULE_ONE
    # without a GlobalAvgPool anywhere that rule does not apply
    assert Plan(S(C(3), A(4), m.Sum([S(C(1)), S()])), 4, 4).pool is not None


def test_ntk_of_a_model_with_an_avgpool_is_rejected():
    x = torch.ones(2, 1, 4, 4)
    for model in (S(C(3), R(), A(2), G()), S(C(3), A(2), R(), C(2, padding=0))):
        with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
            model.ntk(x)
        assert str(e.value) == P.AVGPOOL_RULE_NTK and "AvgPool2d" in str(e.value)
        with pytest.raises(NotImplementedError):
            model.ntk(x[:0])
    assert P.AVGPOOL_RULE_NTK != P.POOL_RULE_NTK


def test_a_final_value_that_is_not_1x1():
    """with an AvgPool2d and no GlobalAvgPool: forward's existing error; the plan itself
    compiles, position_covariance needs it"""
    model = S(C(3), A(2), R())
    x0, x = torch.zeros(0, 1, 4, 4), torch.ones(3, 1, 4, 4)
    assert Plan(model, 4, 4).pool is not None
    assert tuple(model(x0, x, False).shape) == (0, 3)
    assert tuple(model.position_covariance(x0, x, False).shape) == (0, 3, 2, 2, 2, 2)
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="2x2 per pair, not 1x1"):
            model(x)
    else:
        with pytest.raises(RuntimeError, match="HIP device"):
            model(x)


def test_models_with_an_avgpool_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(C(3), R(), A(2), G()).double()
    plan = model._plan(4, 4)
    assert plan.pool is not None and plan.final_hw == (1, 1)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    with pytest.raises(Unsupported, match="op avgpool"):
        NetPlan(S(R(), A(2), G()).double()._plan(4, 4), 8)
    with pytest.raises(Unsupported, match="op avgpool"):
        NetPlan(S(R(), A(4)).double()._plan(4, 4), 8)
    assert plan._var_chain({plan.prog.ops[0].dst}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


def test_structure_key_follows_the_window():
    model = S(C(3), A(2), G())
    k0 = model._structure_key()
    assert model._plan(8, 8).prog.ops[1].shape_out == (4, 4)
    model.mods[1].kernel_size = 3
    k1 = model._structure_key()
    assert k1 != k0 and model._plan(8, 8).prog.ops[1].shape_out == (3, 3)
    model.mods[1].stride = 1
    assert model._structure_key() not in (k0, k1)
    assert model._plan(8, 8).prog.ops[1].shape_out == (6, 6)
    assert S(C(3), A(2), G())._structure_key() != S(C(3), A(2, 1), G())._structure_key()


# ------------------------------------------------------------------------------------
# ABI and the entry points' argument checks
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {"cgp_covmap_avgpool_args_size", "cgp_covmap_avgpool_f64", "cgp_covmap_avgpool_f32",
               "cgp_covmap_diag_f64", "cgp_covmap_diag_f32"}


def test_avgpool_abi():
    from conftest import ROOT
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    assert "#define CGP_ABI_VERSION 12" in txt
    syms = set(re.findall(r"\b(cgp_covmap_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if s.startswith("cgp_covmap_")}
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert lib.cgp_covmap_avgpool_args_size() == ctypes.sizeof(N.CovAvgPoolArgs) == 48


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_covmap_entry_points_reject_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    EINVAL = 1001
    pool, diag = getattr(lib, f"cgp_covmap_avgpool_{sfx}"), getattr(lib, f"cgp_covmap_diag_{sfx}")
    assert pool(None, None) == EINVAL and b"NULL" in lib.cgp_last_error()

    def args(**kw):
        a = N.CovAvgPoolArgs()
        a.in_, a.out = 64, 128
        a.npairs, a.h, a.w, a.ho, a.wo, a.k, a.stride = 6, 7, 6, 3, 2, 3, 2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    item = 8 if sfx == "f64" else 4
    too_wide = 91 if sfx == "f64" else 128                      # w² · itemsize above 64 KB
    assert too_wide ** 2 * item + 16 > 64 * 1024 >= (too_wide - 1) ** 2 * item + 16
    for kw, msg in ((dict(in_=None), b"NULL"), (dict(out=None), b"NULL"),
                    (dict(out=64), b"must not be in"),
                    (dict(npairs=0), b"bad sizes"), (dict(npairs=1 << 31), b"bad sizes"),
                    (dict(h=0), b"bad sizes"), (dict(w=-1), b"bad sizes"),
                    (dict(ho=0), b"bad sizes"), (dict(wo=0), b"bad sizes"),
                    (dict(h=200, w=200, ho=99, wo=99), b"bad sizes"),   # (h w)² above 2^30
                    (dict(k=0), b"bad geometry"), (dict(stride=0), b"bad geometry"),
                    (dict(k=-2), b"bad geometry"),
                    (dict(k=7, ho=1, wo=1), b"does not fit"),           # k > w
                    (dict(h=6, w=7, k=7, ho=1, wo=1), b"does not fit"),  # k > h
                    (dict(ho=4), b"output size"), (dict(wo=3), b"output size"),
                    (dict(ho=2), b"output size"), (dict(stride=1), b"output size"),
                    (dict(h=4, w=too_wide, k=2, ho=2, wo=(too_wide - 2) // 2 + 1), b"of LDS")):
        assert pool(ctypes.byref(args(**kw)), None) == EINVAL, kw
        assert msg in lib.cgp_last_error(), (kw, lib.cgp_last_error())

    good = [64, 128, 6, 5, 4, 192, None]
    for k in (0, 1, 5):
        bad = list(good)
        bad[k] = None
        assert diag(*bad) == EINVAL and b"NULL" in lib.cgp_last_error()
    for k, v in ((2, 0), (2, 1 << 31), (3, 0), (4, 0), (3, -3), (3, 1 << 14)):
        bad = list(good)
        bad[k] = v
        assert diag(*bad) == EINVAL and b"bad sizes" in lib.cgp_last_error(), (k, v)
