"""CPU-only tests of global average pooling: the package surface, the lowering of
cnn_gp.GlobalAvgPool (program op, pool_steps launch lists, the rejections, the whole-network
path declining), the host side of cgp_cov_*, and the test-time oracle (tests/pool_oracle.py)
against two things that do not share its code: random finite networks and a closed form."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import program as P
from cnn_gp.program import Plan, compile_program, pool_steps

import pool_oracle as PO

m = cnn_gp
C, R, E, S, G = m.Conv2d, m.ReLU, m.Erf, m.Sequential, m.GlobalAvgPool


# ------------------------------------------------------------------------------------
# the package surface and the program op
# ------------------------------------------------------------------------------------
def test_pool_is_exported():
    assert "GlobalAvgPool" in cnn_gp.__all__ and "GlobalAvgPool" in cnn_gp.kernels.__all__
    assert issubclass(G, cnn_gp.NNGPKernel) and G().layers() == 0
    assert S(C(3), R(), G()).layers() == 1
    assert callable(cnn_gp.NNGPKernel.position_covariance)
    model = S(C(3), G())
    assert model.set_pool_workspace(1 << 20) is model
    assert all(mod._cgp_pool_ws == 1 << 20 for mod in model.modules())
    assert model.set_pool_workspace(None)._cgp_pool_ws is None


def test_compile_program_emits_pool():
    prog, v0, vf = compile_program(S(C(3), R(), G()), 5, 4)
    assert [o.kind for o in prog.ops] == ["conv", "relu", "pool"]
    pool = prog.ops[-1]
    assert pool.shape_in == (5, 4) and pool.shape_out == (1, 1) and prog.shapes[vf] == (1, 1)
    assert pool.src == prog.ops[1].dst and pool.dst == vf
    # a model without the module compiles to the program it compiled to before
    plan = Plan(S(C(3), R(), C(5, padding=0)), 5, 5)
    assert plan.pool is None and all(o.kind != "pool" for o in plan.prog.ops)


def steps_of(model, h, w, body=False):
    prog, v0, vf = compile_program(model, h, w)
    return pool_steps(prog, v0, vf, body=body), prog, v0, vf


def check_lifetimes(ps):
    """every buffer is written once, read only while live, freed right after its last
    reader, and the final value is never freed; returns the peak in elements per pair"""
    live, peak = set(), 0
    for idx, st in enumerate(ps.steps):
        assert st.dst not in live
        assert all(b in live for b in st.reads()), (idx, st.fn)
        live.add(st.dst)
        peak = max(peak, sum(ps.elems(b) for b in live))
        later = {b for s in ps.steps[idx + 1:] for b in s.reads()} | {ps.final}
        assert set(st.free) == {b for b in live if b not in later}, (idx, st.fn)
        live -= set(st.free)
    assert live == {ps.final}
    assert peak == ps.peak
    return peak


def test_pool_steps_chain():
    ps, prog, v0, vf = steps_of(S(C(3, var_bias=0.1), R(), C(3, stride=2), R(), G()), 6, 5)
    assert [s.fn for s in ps.steps] == ["moments", "conv", "conv", "pool"]
    assert [s.post for s in ps.steps[1:3]] == [N.CGP_COV_RELU, N.CGP_COV_RELU]
    # the fused ReLU reads the variances of the conv's own output
    assert [s.var for s in ps.steps[1:3]] == [prog.ops[0].dst, prog.ops[2].dst]
    assert ps.need_var == {prog.ops[0].dst, prog.ops[2].dst}
    assert ps.maps == {v0, prog.ops[1].dst, prog.ops[3].dst} and ps.scalars == {vf}
    assert ps.final == vf and ps.pooled == {vf}
    assert ps.shapes[prog.ops[3].dst] == (3, 3) and ps.elems(prog.ops[3].dst) == 81
    assert ps.elems(v0) == 900 and ps.elems(vf) == 1
    # two maps live at a conv: input and output
    assert check_lifetimes(ps) == 900 + 900
    assert ps.steps[1].free == [v0]


def test_pool_steps_resnet_block():
    body = S(C(3), m.resnet_block(), m.resnet_block(stride=2, projection_shortcut=True,
                                                    multiplier=2), R(), G())
    ps, prog, v0, vf = steps_of(body, 6, 6)
    # the identity block opens with a standalone ReLU (its input also feeds the skip); the
    # skip is the last conv's addend; the projection block's ReLU feeds two convs
    assert [s.fn for s in ps.steps] == ["moments", "conv", "nonlin", "conv", "conv", "nonlin",
                                        "conv", "conv", "conv", "nonlin", "pool"]
    first_block_out = ps.steps[4]
    assert first_block_out.addend == ps.steps[1].dst and first_block_out.post == N.CGP_COV_NONE
    assert ps.steps[3].post == N.CGP_COV_RELU
    proj, a, b = ps.steps[6:9]
    assert proj.src == a.src == ps.steps[5].dst and proj.op.geom.taps == 1
    assert b.addend == proj.dst and b.src == a.dst
    assert all(s.post == N.CGP_COV_RELU for s in (ps.steps[2], ps.steps[5], ps.steps[9]))
    assert ps.scalars == {vf} and len(ps.maps) == 10
    # three 6x6 maps live inside the identity block: the skip, a conv's input and its output
    assert check_lifetimes(ps) == 3 * 36 ** 2


def test_pool_steps_mixture_and_readout():
    mix = m.Mixture([S(R(), C(3)), S(E(), C(3, var_bias=0.2)), S()],
                    torch.tensor([0.3, -0.5, 0.1]))
    ps, prog, v0, vf = steps_of(S(C(3), mix, G(), C(1, var_weight=2., var_bias=.3)), 4, 4)
    assert [s.fn for s in ps.steps] == ["moments", "conv", "nonlin", "conv", "nonlin", "conv",
                                        "axpby", "pool", "conv"]
    assert [ps.steps[k].post for k in (2, 4)] == [N.CGP_COV_RELU, N.CGP_COV_ERF]
    ax = ps.steps[6]
    assert [b for _, b in ax.terms] == [ps.steps[3].dst, ps.steps[5].dst, ps.steps[1].dst]
    np.testing.assert_allclose(sum(c for c, _ in ax.terms), 1.0, rtol=1e-6)
    # the readout after the pool is a conv on 1x1 values: a scalar buffer, no variances
    pool, readout = ps.steps[7:]
    assert ps.scalars == {pool.dst, readout.dst} == ps.pooled and readout.dst == vf
    assert readout.var is None and readout.post == N.CGP_COV_NONE and readout.src == pool.dst
    assert ps.shapes[pool.dst] == ps.shapes[vf] == (1, 1)
    assert all(s.dst in ps.maps for s in ps.steps[:7])
    assert ps.need_var == {ps.steps[1].dst}
    check_lifetimes(ps)


def test_pool_steps_sum_of_pooled_branches():
    """the one pool may sit in each branch: the values merge after it as scalars"""
    model = S(C(3), m.Sum([S(R(), G()), S(C(3), G(), C(1, var_bias=0.5))]))
    ps, prog, v0, vf = steps_of(model, 4, 4)
    assert [s.fn for s in ps.steps] == ["moments", "conv", "nonlin", "pool", "conv", "pool",
                                        "conv"]
    assert ps.steps[-1].addend == ps.steps[3].dst        # rule 2 on the 1x1 readout
    assert len(ps.scalars) == 3 and vf in ps.scalars
    check_lifetimes(ps)


def test_body_steps_have_no_pool():
    ps, prog, v0, vf = steps_of(S(C(3), R()), 4, 3, body=True)
    assert [s.fn for s in ps.steps] == ["moments", "conv"] and ps.final in ps.maps
    assert not ps.scalars and not ps.pooled
    check_lifetimes(ps)
    with pytest.raises(ValueError, match="GlobalAvgPool"):
        steps_of(S(C(3), G()), 4, 3, body=True)
    assert Plan(S(C(3), R()), 4, 3).body_steps().final == vf


# ------------------------------------------------------------------------------------
# the rejections
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [R, E])
def test_nonlinearity_after_the_pool_is_rejected(act):
    with pytest.raises(NotImplementedError, match="downstream of a GlobalAvgPool") as e:
        Plan(S(C(3), R(), G(), act()), 4, 4)
    assert str(e.value) == P.POOL_RULE_NONLIN and "self-covariances" in str(e.value)


@pytest.mark.parametrize("model", [
    S(C(3), G(), G()),                                              # two on one path
    S(C(1), m.Sum([S(G()), S()])),                                  # one path without (1x1 maps)
    S(m.Sum([S(C(1), G()), S(C(1))]), G()),                         # none and two
], ids=["twice", "skip_around", "branch_then_again"])
def test_paths_must_pass_exactly_one_pool(model):
    with pytest.raises(NotImplementedError, match="exactly one") as e:
        Plan(model, 1, 1)
    assert str(e.value) == P.POOL_RULE_ONE


def test_conv_after_the_pool_must_stay_1x1():
    with pytest.raises(NotImplementedError, match="must keep the value 1x1"):
        Plan(S(C(3), G(), C(1, padding=1)), 4, 4)
    assert Plan(S(C(3), G(), C(3)), 4, 4).pool is not None     # "same" padding stays 1x1


def test_ntk_of_a_pooled_model_is_rejected():
    model = S(C(3), R(), G())
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(NotImplementedError, match="neural tangent kernel") as e:
        model.ntk(x)
    assert str(e.value) == P.POOL_RULE_NTK
    with pytest.raises(NotImplementedError):
        model.ntk(x[:0])


def test_pooled_models_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(C(3), R(), G()).double()
    plan = model._plan(4, 4)
    assert plan.pool is not None and plan.final_hw == (1, 1)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    with pytest.raises(Unsupported):
        NetPlan(plan, 8)
    with pytest.raises(Unsupported, match="op pool"):      # no conv geometry to decline first
        NetPlan(S(R(), G()).double()._plan(4, 4), 8)
    assert plan._var_chain({plan.prog.ops[0].dst}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


def test_pooled_model_without_gpu_and_empty_batches():
    model = S(C(3), R(), G())
    x0, x = torch.zeros(0, 1, 4, 4), torch.ones(3, 1, 4, 4)
    assert tuple(model(x0).shape) == (0, 0)
    assert tuple(model(x0, x, False).shape) == (0, 3)
    assert tuple(model(x0, x0, True, True).shape) == (0,)
    body = S(C(3, stride=2), R())
    assert tuple(body.position_covariance(x0, x, False).shape) == (0, 3, 2, 2, 2, 2)
    assert tuple(body.position_covariance(x0, x0, True, True).shape) == (0, 2, 2, 2, 2)
    with pytest.raises(ValueError, match="GlobalAvgPool"):
        model.position_covariance(x)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            model(x)
        with pytest.raises(RuntimeError, match="HIP device"):
            body.position_covariance(x)


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
def test_pool_abi():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    assert lib.cgp_cov_conv_args_size() == ctypes.sizeof(N.CovConvArgs)
    assert lib.cgp_cov_nonlin_args_size() == ctypes.sizeof(N.CovNonlinArgs)
    import re
    from conftest import ROOT
    import os
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    syms = set(re.findall(r"\b(cgp_cov_[a-z0-9_]+)\s*\(", txt))
    assert syms == {s for s in N.SIGNATURES if s.startswith("cgp_cov_")} and len(syms) == 10
    assert "#define CGP_ABI_VERSION 12" in txt
    for name, val in (("NONE", 0), ("RELU", 1), ("ERF", 2)):
        assert f"#define CGP_COV_{name} {val}" in txt and getattr(N, f"CGP_COV_{name}") == val


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_cov_entry_points_reject_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    EINVAL = 1001
    conv, nonlin = getattr(lib, f"cgp_cov_conv_{sfx}"), getattr(lib, f"cgp_cov_nonlin_{sfx}")
    mom, pool = getattr(lib, f"cgp_cov_moments_{sfx}"), getattr(lib, f"cgp_cov_pool_{sfx}")
    assert conv(None, None) == EINVAL and nonlin(None, None) == EINVAL

    def cargs(**kw):
        a = N.CovConvArgs()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        a.npairs, a.h, a.w, a.ho, a.wo = 6, 5, 4, 5, 4
        a.taps, a.offset, a.stride, a.dilation, a.weight = 3, -1, 1, 1, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, msg in ((dict(in_=None), b"NULL"), (dict(out=None), b"NULL"),
                    (dict(out=64), b"must not be in"), (dict(npairs=0), b"bad sizes"),
                    (dict(h=0), b"bad sizes"), (dict(wo=0), b"bad sizes"),
                    (dict(h=200, w=200), b"bad sizes"),           # (h w)^2 above 2^30
                    (dict(taps=0), b"bad geometry"), (dict(stride=0), b"bad geometry"),
                    (dict(dilation=0), b"bad geometry"), (dict(post=3), b"not a nonlinearity"),
                    (dict(post=1, xx=None), b"needs xx"), (dict(post=2, pair_j=None), b"needs xx"),
                    (dict(h=100, w=100, taps=7), b"of LDS")):
        assert conv(ctypes.byref(cargs(**kw)), None) == EINVAL, kw
        assert msg in lib.cgp_last_error(), (kw, lib.cgp_last_error())

    def nargs(**kw):
        a = N.CovNonlinArgs()
        a.in_, a.out, a.xx, a.yy, a.pair_i, a.pair_j = 64, 128, 192, 256, 320, 384
        a.npairs, a.h, a.w, a.kind = 6, 5, 4, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for field in ("in_", "out", "xx", "yy", "pair_i", "pair_j"):
        assert nonlin(ctypes.byref(nargs(**{field: None})), None) == EINVAL, field
        assert b"NULL" in lib.cgp_last_error()
    for kw, msg in ((dict(kind=0), b"neither"), (dict(kind=3), b"neither"),
                    (dict(npairs=1 << 31), b"bad sizes"), (dict(w=0), b"bad sizes")):
        assert nonlin(ctypes.byref(nargs(**kw)), None) == EINVAL, kw
        assert msg in lib.cgp_last_error()

    good = [64, 128, 192, 256, 6, 2, 5, 4, 320, None]
    for k in (0, 1, 2, 3, 8):
        bad = list(good)
        bad[k] = None
        assert mom(*bad) == EINVAL and b"NULL" in lib.cgp_last_error()
    for k, v in ((4, 0), (5, 0), (6, 0), (7, 0), (6, 1 << 14)):
        bad = list(good)
        bad[k] = v
        assert mom(*bad) == EINVAL and b"bad sizes" in lib.cgp_last_error()
    assert pool(None, 2, 4, 64, None) == EINVAL and pool(64, 2, 4, None, None) == EINVAL
    assert pool(64, 0, 4, 128, None) == EINVAL and pool(64, 2, 0, 128, None) == EINVAL


# ------------------------------------------------------------------------------------
# the oracle's definition
# ------------------------------------------------------------------------------------
def test_oracle_matches_random_finite_networks():
    """conv, ReLU, conv, pool with bias variances, sampled with torch on the CPU.  One
    nonlinearity deep, the first layer's pre-activations are exactly Gaussian given the
    inputs, so E_W[f(x)·f(y)] equals the kernel at any width.  Finite network, in the
    reference's conventions: W1 ~ N(0, var_weight/(k²·C)), b1 ~ N(0, var_bias) per channel,
    a = relu(z1) (no sqrt 2), W2 ~ N(0, var_weight/(k²·width)), f = the mean over positions
    of one output channel.  Bound: 5 standard errors, estimated from the sample itself
    (measured: every entry within 1.8)."""
    width, draws, batch = 64, 4000, 500
    l1 = dict(var_weight=1.3, var_bias=0.2)
    l2 = dict(var_weight=0.9, var_bias=0.1)
    model = S(C(3, **l1), R(), C(3, **l2), G())
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4, 3, 5, 4))
    ref = PO.kernel(model, X)                                      # all 16 pairs, same
    np.testing.assert_allclose(PO.kernel(model, X[:2], X[2:], False), ref[:2, 2:], rtol=1e-13)
    np.testing.assert_allclose(PO.kernel(model, X, X, True, True), np.diag(ref), rtol=1e-13)

    gen = torch.Generator().manual_seed(6)
    x = torch.from_numpy(X)
    cin = X.shape[1]
    prods = []
    for _ in range(draws // batch):
        rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)    # noqa: E731
        w1 = rn(batch * width, cin, 3, 3) * (l1["var_weight"] / (9 * cin)) ** 0.5
        b1 = rn(batch * width) * l1["var_bias"] ** 0.5
        w2 = rn(batch, width, 3, 3) * (l2["var_weight"] / (9 * width)) ** 0.5
        b2 = rn(batch) * l2["var_bias"] ** 0.5
        a = F.relu(F.conv2d(x, w1, b1, padding=1))                 # [4, batch·width, 5, 4]
        z = F.conv2d(a, w2, b2, padding=1, groups=batch)           # [4, batch, 5, 4]
        f = z.mean(dim=(2, 3))                                     # [4, batch]
        prods.append(f[:, None, :] * f[None, :, :])
    prods = torch.cat(prods, dim=2).numpy()                        # [4, 4, draws]
    est = prods.mean(axis=2)
    se = prods.std(axis=2, ddof=1) / np.sqrt(draws)
    zscore = np.abs(est - ref) / se
    print(f"finite networks: worst |z| = {zscore.max():.2f} standard errors, "
          f"relative standard error {np.max(se / np.abs(ref)):.3f}")
    assert np.all(zscore < 5), zscore


def test_oracle_matches_the_linear_closed_form():
    """conv, pool: K_ij = bias + (weight/C)·Σ_{a,b,c} A_i[c, a, b]·A_j[c, a, b] with
    A_i[c, a, b] the mean over output pixels p of the zero-padded x_i[c, p·s + off + (a, b)·d]
    -- computed from the images with plain loops, no pair map anywhere"""
    rng = np.random.default_rng(8)
    X, Z = rng.standard_normal((3, 2, 5, 4)), rng.standard_normal((2, 2, 5, 4))
    for conv in (C(3, var_weight=1.7, var_bias=0.3), C(3, stride=2, var_bias=0.1),
                 C(2), C(3, dilation=2), C(4, padding=0, var_weight=0.5)):
        g = P.conv_geometry(conv)
        ho, wo = P.conv_out_hw(conv, 5, 4)

        def window_means(imgs):
            out = np.zeros((len(imgs), imgs.shape[1], g.taps, g.taps))
            for a in range(g.taps):
                for b in range(g.taps):
                    for r in range(ho):
                        for c in range(wo):
                            ir = r * g.stride + g.offset + a * g.dilation
                            ic = c * g.stride + g.offset + b * g.dilation
                            if 0 <= ir < 5 and 0 <= ic < 4:
                                out[:, :, a, b] += imgs[:, :, ir, ic]
            return out / (ho * wo)

        ax, az = window_means(X), window_means(Z)
        want = g.bias + g.weight / X.shape[1] * np.einsum("icab,jcab->ij", ax, az)
        got = PO.kernel(S(conv, G()), X, Z, False)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
        want_xx = g.bias + g.weight / X.shape[1] * np.einsum("icab,jcab->ij", ax, ax)
        np.testing.assert_allclose(PO.kernel(S(conv, G()), X), want_xx, rtol=1e-12, atol=1e-14)


def test_oracle_diagonal_is_the_layer_recursion():
    """S[i, j, p, p] of a body is the pair map the reference's recursion carries: the
    position-pair oracle against erf_oracle's walk of the same modules"""
    import erf_oracle as EO
    body = S(C(3, var_bias=0.1), R(), C(3, stride=2), E(), C(3))
    rng = np.random.default_rng(9)
    X, Z = rng.random((3, 2, 6, 5)), rng.random((2, 2, 6, 5))
    for args in ((X,), (X, Z, False, False), (X[:2], Z, False, True), (X, X, True, True)):
        s = PO.position_covariance(body, *args)
        x = torch.as_tensor(args[0])
        y, same, diag = (x, True, False) if len(args) == 1 else \
            (torch.as_tensor(args[1]), args[2], args[3])
        kp = EO._walk(body, (bool(same), bool(diag)) + EO._moments(x, y, diag))
        assert s.shape[-4:] == (3, 3, 3, 3)
        np.testing.assert_allclose(np.einsum("...abab->...ab", s),
                                   kp[2].reshape(s.shape[:-2]).numpy(), rtol=1e-12)
