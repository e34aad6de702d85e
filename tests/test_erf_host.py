"""CPU-only tests of the erf nonlinearity: the closed forms against Gauss-Hermite
quadrature, the test-time oracle against itself (autograd Θ vs the stepwise recursion), the
lowering of cnn_gp.Erf (program, fusion, NTK steps, the whole-network path declining), and
the host side of cgp_erf_* / cgp_var_erf_*."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp.program import Plan, compile_program, ntk_steps

import erf_oracle as EO


# ------------------------------------------------------------------------------------
# the formulas
# ------------------------------------------------------------------------------------
def test_closed_form_matches_quadrature():
    """K' = E[erf(u1) erf(u2)] and κ̇ = E[erf'(u1) erf'(u2)] for (u1, u2) ~ N(0, [[v1, c],
    [c, v2]]), by a 200 x 200 Gauss-Hermite rule -- independent of any formula.  Measured:
    2.8e-16 absolute on K', 1.3e-15 relative on κ̇ (3.4e-13 / 3.6e-11 at 128 nodes, so 200
    it is)."""
    t, w = np.polynomial.hermite.hermgauss(200)
    z1, z2 = np.meshgrid(math.sqrt(2) * t, math.sqrt(2) * t, indexing="ij")
    ww = np.outer(w, w) / math.pi
    erf = lambda a: torch.erf(torch.from_numpy(a)).numpy()                     # noqa: E731
    derf = lambda a: 2 / math.sqrt(math.pi) * np.exp(-a * a)                   # noqa: E731
    worst_k = worst_kd = 0.0
    for v1 in (0.05, 0.5, 1, 3):
        for v2 in (0.05, 0.7, 3):
            for rho in (-0.9, -0.3, 0, 0.5, 0.95):
                c = rho * math.sqrt(v1 * v2)
                u1 = math.sqrt(v1) * z1
                u2 = math.sqrt(v2) * (rho * z1 + math.sqrt(1 - rho * rho) * z2)
                qk = float(np.sum(ww * erf(u1) * erf(u2)))
                qkd = float(np.sum(ww * derf(u1) * derf(u2)))
                k, kd = EO.erf_pair(*(torch.tensor(a, dtype=torch.float64) for a in (c, v1, v2)))
                worst_k = max(worst_k, abs(float(k) - qk))
                worst_kd = max(worst_kd, abs(float(kd) - qkd) / qkd)
    print(f"closed form vs quadrature: K' {worst_k:.2e} abs, kdot {worst_kd:.2e} rel")
    assert worst_k < 1e-13 and worst_kd < 1e-13


def test_variance_formula_is_the_pair_formula_on_the_diagonal():
    v = torch.tensor([0.0, 1e-6, 0.05, 0.5, 1.0, 3.0, 40.0], dtype=torch.float64)
    k, kd = EO.erf_pair(v, v, v)
    assert float((EO.erf_var(v) - k).abs().max()) < 1e-15
    assert float((kd - (4 / math.pi) / torch.sqrt(1 + 4 * v)).abs().max()) < 1e-15
    assert float(k[0]) == 0.0 and float(kd[0]) == 4 / math.pi
    # the same through the walk of a model: on identical images the overridden entries (the
    # variance stream) are the pair stream's, evaluated as same=False
    model = cnn_gp.Sequential(cnn_gp.Erf())
    x = np.random.default_rng(0).random((4, 3, 1, 1))
    kxx = EO.kernel(model, x)
    assert np.max(np.abs(kxx - EO.kernel(model, x, x, False, False))) < 1e-15
    assert np.max(np.abs(np.diag(kxx) - EO.kernel(model, x, x, True, True))) == 0.0
    assert np.max(np.abs(np.diag(kxx) - EO.erf_var(torch.from_numpy((x * x).mean(1).ravel()))
                         .numpy())) == 0.0


# ------------------------------------------------------------------------------------
# networks
# ------------------------------------------------------------------------------------
def small_nets():
    m = cnn_gp
    return {
        "convnet": m.Sequential(m.Conv2d(3, var_bias=0.2), m.Erf(), m.Conv2d(3, var_weight=1.5),
                                m.Erf(), m.Conv2d(6, padding=0)),
        "residual": m.Sequential(m.Conv2d(3), m.Sum([m.Sequential(), m.Sequential(
            m.Erf(), m.Conv2d(3), m.Erf(), m.Conv2d(3))]), m.Erf(), m.Conv2d(6, padding=0)),
        "mixed": m.Sequential(m.Conv2d(3, var_bias=0.1), m.ReLU(), m.Conv2d(3), m.Erf(),
                              m.Conv2d(6, padding=0)),
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


@pytest.mark.parametrize("name", ["convnet", "residual", "mixed"])
def test_oracle_autograd_matches_stepwise(name):
    model = small_nets()[name].double()
    X, Z = images()
    k, th = EO.ntk_autograd(model, X, Z)
    sk, sth = EO.ntk_stepwise(model, X, Z, False, False)
    assert masked_err(k, sk) < 1e-12 and masked_err(th, sth) < 1e-12
    assert not np.isnan(th).any()
    assert masked_err(EO.kernel(model, X, Z, False, False), sk) < 1e-12
    # identical images: the overrides of same=True against autograd through same=False
    k, th = EO.ntk_autograd(model, X, X)
    sk, sth = EO.ntk_stepwise(model, X)
    if name == "mixed":
        # the ReLU map is singular at rho = 1 under same=False (ntk_oracle.ntk): masked
        idx = np.arange(len(X))
        k[idx, idx] = th[idx, idx] = np.nan
    else:
        assert not np.isnan(th).any()
    assert not np.isnan(th[~np.eye(len(X), dtype=bool)]).any()
    assert masked_err(k, sk) < 1e-12 and masked_err(th, sth) < 1e-12
    if name != "mixed":
        k, th = EO.ntk_autograd(model, X, X, diag=True)
        sk, sth = EO.ntk_stepwise(model, X, X, True, True)
        assert masked_err(k, sk) < 1e-12 and masked_err(th, sth) < 1e-12


# ------------------------------------------------------------------------------------
# the package surface
# ------------------------------------------------------------------------------------
def head_net():
    m = cnn_gp
    return m.Sequential(m.Conv2d(3), m.Erf(), m.Conv2d(4, padding=0))


def test_erf_is_exported():
    assert "Erf" in cnn_gp.__all__ and "Erf" in cnn_gp.kernels.__all__
    assert issubclass(cnn_gp.Erf, cnn_gp.NNGPKernel) and cnn_gp.Erf().layers() == 0
    assert head_net().layers() == 2


def test_erf_lowering_and_fusion():
    model = head_net()
    prog, v0, vf = compile_program(model, 4, 4)
    assert [o.kind for o in prog.ops] == ["conv", "erf", "conv"]
    plan = Plan(model, 4, 4)
    kinds = [(o.kind, o.pre, o.post) for o in plan.pair_ops]
    assert kinds == [("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_NONE),
                     ("erf", N.CGP_PRE_NONE, N.CGP_POST_NONE),
                     ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]
    erf = plan.pair_ops[1]
    assert erf.addend is None and erf.src in plan.need_var and erf.src in plan.ntk_need_var()
    # rule 2: the identity skip of a residual block becomes the addend of its last op
    m = cnn_gp
    block = m.Sequential(m.Conv2d(3), m.Sum([m.Sequential(), m.Sequential(m.Conv2d(3), m.Erf())]),
                         m.Conv2d(4, padding=0))
    plan = Plan(block, 4, 4)
    assert [o.kind for o in plan.pair_ops] == ["conv", "conv", "erf", "conv"]
    assert plan.pair_ops[2].addend == plan.pair_ops[0].dst


def test_erf_models_decline_the_whole_network_path():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = head_net().double()
    plan = model._plan(4, 4)
    assert model._net_plan(plan, 8) is None and model._net_plan(plan, 4) is None
    with pytest.raises(Unsupported):
        NetPlan(plan, 8)
    # the variance chain has no erf record: it declines instead of raising
    assert plan._var_chain({plan.vf}, set(), torch.device("cpu")) is None
    # image_variances declines before touching a device for anything but device images
    assert model.image_variances(torch.ones(2, 1, 4, 4, dtype=torch.float64)) is None


def test_erf_ntk_steps():
    """Θ of the first conv's output is its K' buffer, so the erf after it already carries Θ
    ("erf_ntk"); an Erf before any conv has Θ = 0 and is the plain forward pass ("erf")"""
    prog, v0, vf = compile_program(head_net(), 4, 4)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["conv", "erf_ntk", "conv", "conv"]
    assert steps[1].theta == steps[1].src == steps[0].dst
    assert steps[1].dst_theta == ("T", steps[1].op.dst) and steps[3].src == steps[1].dst_theta
    assert kbuf == ("K", vf) and tbuf == ("T", vf)
    m = cnn_gp
    prog, v0, vf = compile_program(m.Sequential(m.Erf(), m.Conv2d(4, padding=0)), 4, 4)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["erf", "conv"]
    assert steps[0].theta is None and steps[0].dst_theta is None and tbuf == ("K", vf)


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
def test_erf_abi():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    assert lib.cgp_erf_args_size() == ctypes.sizeof(N.ErfArgs)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_erf_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_erf_{sfx}")
    assert fn(None, None) == 1001

    def args(**kw):
        a = N.ErfArgs()
        a.xy, a.theta, a.out_xy, a.out_theta, a.xx, a.yy = 64, 128, 192, 256, 320, 384
        a.nmaps, a.n1, a.n2, a.hw = 6, 3, 2, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for field in ("xy", "out_xy", "out_theta", "xx", "yy"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"NULL" in lib.cgp_last_error()
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
    assert fn(ctypes.byref(args(nmaps=1 << 31, n1=1 << 16, n2=1 << 15)), None) == 1001
    assert fn(ctypes.byref(args(hw=0)), None) == 1001
    assert fn(ctypes.byref(args(hw=4096)), None) == 1001          # larger than one chunk
    assert b"too large" in lib.cgp_last_error()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_var_erf_rejects_bad_arguments_on_host(sfx):
    lib = N.load()
    fn = getattr(lib, f"cgp_var_erf_{sfx}")
    for k in range(4):
        p = [64, 128, 192, 256]
        p[k] = None
        assert fn(p[0], p[1], 2, 2, 4, 0, p[2], p[3], None) == 1001
        assert b"NULL" in lib.cgp_last_error()
    assert fn(64, 128, 2, 3, 4, 1, 192, 256, None) == 1001        # same with n1 != n2
    assert fn(64, 128, 2, 2, 0, 0, 192, 256, None) == 1001


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_erf_model_without_gpu_raises_like_relu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    m = cnn_gp
    x = torch.ones(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="HIP device") as relu:
        m.Sequential(m.Conv2d(3), m.ReLU(), m.Conv2d(4, padding=0))(x)
    with pytest.raises(RuntimeError, match="HIP device") as erf:
        head_net()(x)
    assert str(erf.value) == str(relu.value)
    with pytest.raises(RuntimeError, match="HIP device"):
        head_net().ntk(x)


def test_erf_model_empty_batches():
    model = head_net()
    x0, x = torch.zeros(0, 1, 4, 4), torch.ones(3, 1, 4, 4)
    assert tuple(model(x0).shape) == (0, 0)
    assert tuple(model(x0, x, False).shape) == (0, 3)
    assert tuple(model(x, x0, False).shape) == (3, 0)
    assert tuple(model(x0, x0, True, True).shape) == (0,)
    k, th = model.ntk(x0, x, False, return_nngp=True)
    assert tuple(k.shape) == tuple(th.shape) == (0, 3)
