"""CPU-only tests of the neural tangent kernel: the test-time autograd oracle against the
reference's fixture (tests/golden/ntk_e2e.npz), the launch list of program.ntk_steps
interpreted with torch float64 ops against both, and the host side of cgp_relu_ntk_* and
NNGPKernel.ntk."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp.program import compile_program, ntk_steps
from oracle import specs

from conftest import GOLDEN
import configs_util
import ntk_oracle
from ntk_oracle import run_steps

CONFIGS = ["mnist_paper_convnet_gp", "mnist_paper_residual_cnn_gp", "mnist_as_tf", "cifar10"]
NETS = CONFIGS + ["mixture_big", "mixture_small"]
RTOL = 1e-12          # test_oracle_golden.py's bound for the fp64 oracle


def golden():
    return np.load(os.path.join(GOLDEN, "ntk_e2e.npz"))


def product_model(name):
    if name.startswith("mixture_"):
        return configs_util.mixture_nets()[name[len("mixture_"):]][0].double()
    return configs_util.model(name).double()


def rel_err(got, ref):
    """largest |got - ref| / |ref| over the entries where ref is not NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    assert got.shape == ref.shape
    keep = ~np.isnan(ref)
    assert keep.any() and np.all(np.isfinite(got[keep]))
    return float(np.max(np.abs(got[keep] - ref[keep]) / np.abs(ref[keep])))


def all_modes(fn, z, name):
    """fn(x, y, same, diag) -> (K, Θ) against every array of network `name` in the fixture;
    returns the largest relative error."""
    X, Z = z[name + "_X"], z[name + "_Z"]
    errs = []
    k, th = fn(X, Z, False, False)
    errs += [rel_err(k, z[name + "_Kxz"]), rel_err(th, z[name + "_Txz"])]
    k, th = fn(X, X, False, False)            # the fixture's diagonal is NaN
    errs += [rel_err(k, z[name + "_Kxx"]), rel_err(th, z[name + "_Txx"])]
    k, th = fn(X[:3], Z, False, True)
    errs += [rel_err(k, z[name + "_Kxzdiag"]), rel_err(th, z[name + "_Txzdiag"])]
    k, th = fn(X, X, True, True)
    errs += [rel_err(k, z[name + "_Kdiag"]), rel_err(th, z[name + "_Tdiag"])]
    k, th = fn(X, None, None, False)          # same: off-diagonal and diagonal together
    errs += [rel_err(k, z[name + "_Kxx"]), rel_err(th, z[name + "_Txx"]),
             rel_err(np.diag(k), z[name + "_Kdiag"]), rel_err(np.diag(th), z[name + "_Tdiag"])]
    return max(errs)


def test_fixture_holds_every_network():
    z = golden()
    for name in NETS:
        for key in ("X", "Z", "Kxz", "Txz", "Kxx", "Txx", "Kxzdiag", "Txzdiag", "Kdiag", "Tdiag"):
            assert z[f"{name}_{key}"].dtype == np.float64, (name, key)
        assert z[name + "_X"].shape[0] == 5 and z[name + "_Z"].shape[0] == 3
        np.testing.assert_array_equal(z[name + "_X"], z[name + "_X"].astype(np.float32))
        assert np.all(np.isnan(np.diag(z[name + "_Txx"])))


@pytest.mark.parametrize("name", NETS)
def test_oracle_reproduces_fixture(name):
    z = golden()
    spec = specs.CONFIGS[name]() if name in CONFIGS else configs_util.spec_of(product_model(name))
    err = all_modes(lambda *a: ntk_oracle.ntk(spec, *a), z, name)
    print(f"{name}: oracle vs reference {err:.2e}")
    assert err < RTOL


@pytest.mark.parametrize("name", NETS)
def test_ntk_steps_reproduce_fixture(name):
    z = golden()
    model = product_model(name)
    err = all_modes(lambda *a: run_steps(model, *a), z, name)
    print(f"{name}: ntk_steps vs reference {err:.2e}")
    assert err < RTOL


def small_nets():
    m = cnn_gp
    return {
        # the reference README's example network
        "readme": (m.Sequential(m.Conv2d(kernel_size=3), m.ReLU(),
                                m.Conv2d(kernel_size=3, stride=2), m.ReLU(),
                                m.Conv2d(kernel_size=14, padding=0)), 28),
        # an even, dilated "same" kernel (zero first row and column, kernels.py:73-84)
        "dilated": (m.Sequential(m.Conv2d(2, dilation=2, var_bias=0.1), m.ReLU(),
                                 m.Conv2d(3, var_weight=1.5), m.ReLU(),
                                 m.Conv2d(14, padding=0)), 14),
    }


@pytest.mark.parametrize("name", ["readme", "dilated"])
def test_ntk_steps_match_oracle(name):
    model, side = small_nets()[name]
    model = model.double()
    spec = configs_util.spec_of(model)
    rng = np.random.default_rng(5)
    X = rng.random((4, 2, side, side), dtype=np.float32).astype(np.float64)
    Z = rng.random((3, 2, side, side), dtype=np.float32).astype(np.float64)
    for args in ((X, Z, False, False), (X[:3], Z, False, True), (X, X, True, True),
                 (X, None, None, False)):
        k, th = run_steps(model, *args)
        rk, rth = ntk_oracle.ntk(spec, *args)
        assert rel_err(k, rk) < RTOL and rel_err(th, rth) < RTOL, (name, args[2:])


def test_ntk_steps_lowering():
    """zero Θ costs nothing: the first conv's Θ is its K, a ReLU before any conv is the plain
    op, and a model without a Conv2d has Θ = 0"""
    m = cnn_gp
    model = m.Sequential(m.ReLU(), m.Conv2d(3), m.ReLU(), m.Conv2d(3), m.ReLU(),
                         m.Conv2d(6, padding=0))
    prog, v0, vf = compile_program(model, 6, 6)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["relu", "conv", "relu_ntk", "conv", "conv", "relu_ntk",
                                     "conv", "conv"]
    assert steps[2].theta == steps[2].src == steps[1].dst       # Θ aliases K' of conv 1
    assert steps[4].bias == 0.0 and steps[4].addend == steps[3].dst
    assert steps[4].op.geom.bias == steps[3].bias
    assert kbuf == ("K", vf) and tbuf == ("T", vf)
    prog, v0, vf = compile_program(m.Sequential(m.ReLU(), m.Sum([m.Sequential(), m.ReLU()])),
                                   1, 1)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert tbuf is None and [s.fn for s in steps] == ["relu", "relu", "axpby"]
    # a plain Sum with one term whose Θ is not zero passes that buffer on
    model = m.Sequential(m.Sum([m.Sequential(), m.Conv2d(3)]), m.Conv2d(4, padding=0))
    prog, v0, vf = compile_program(model, 4, 4)
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    assert [s.fn for s in steps] == ["conv", "axpby", "conv", "conv"]
    assert steps[3].src == steps[0].dst


# ------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------
def test_abi_version_and_struct():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12
    assert lib.cgp_abi_version() == 12
    assert lib.cgp_relu_ntk_args_size() == ctypes.sizeof(N.ReluNtkArgs)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_relu_ntk_rejects_bad_arguments_on_host(sfx):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    fn = getattr(lib, f"cgp_relu_ntk_{sfx}")
    assert fn(None, None) == 1001

    def args(**kw):
        a = N.ReluNtkArgs()
        a.xy, a.theta, a.out_xy, a.out_theta, a.xx, a.yy = 64, 128, 192, 256, 320, 384
        a.nmaps, a.n1, a.n2, a.hw = 6, 3, 2, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for field in ("xy", "theta", "out_xy", "out_theta", "xx", "yy"):
        assert fn(ctypes.byref(args(**{field: None})), None) == 1001, field
        assert b"NULL" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(same=1)), None) == 1001          # same with n1 != n2
    assert b"n1 == n2" in lib.cgp_last_error()
    assert fn(ctypes.byref(args(diag=1, nmaps=3)), None) == 1001  # diag with n1 != n2
    assert fn(ctypes.byref(args(nmaps=5)), None) == 1001          # nmaps != n1 n2
    assert fn(ctypes.byref(args(nmaps=1 << 31, n1=1 << 16, n2=1 << 15)), None) == 1001
    assert fn(ctypes.byref(args(hw=0)), None) == 1001
    assert fn(ctypes.byref(args(hw=4096)), None) == 1001          # larger than one chunk


# ------------------------------------------------------------------------------------
# NNGPKernel.ntk / ntk_kern without a GPU
# ------------------------------------------------------------------------------------
def test_ntk_without_gpu_raises_like_forward():
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    model = small_nets()["readme"][0]
    x = torch.rand(2, 1, 28, 28)
    with pytest.raises(RuntimeError) as fwd:
        model(x)
    with pytest.raises(RuntimeError) as ntk:
        model.ntk(x)
    assert str(ntk.value) == str(fwd.value)


def test_ntk_empty_batch_and_argument_rules():
    model = small_nets()["readme"][0]
    x0, x = torch.zeros(0, 1, 28, 28), torch.rand(3, 1, 28, 28)
    assert tuple(model.ntk(x0).shape) == (0, 0)
    assert tuple(model.ntk(x0, x, False).shape) == (0, 3)
    assert tuple(model.ntk(x, x0, False).shape) == (3, 0)
    assert tuple(model.ntk(x0, x0, True, True).shape) == (0,)
    k, th = model.ntk(x0, x, False, return_nngp=True)
    assert tuple(k.shape) == tuple(th.shape) == (0, 3) and th.dtype == x.dtype
    with pytest.raises(AssertionError):
        model.ntk(x, x[:2], False, True)              # diag with unequal lengths
    with pytest.raises(TypeError):
        model.ntk(x0.half())
    assert "ntk_kern" in cnn_gp.__all__ and cnn_gp.ntk_kern is cnn_gp.gram.ntk_kern
