"""GPU tests of the neural tangent kernel: cgp_relu_ntk_* alone, NNGPKernel.ntk against the
reference's fixture (tests/golden/ntk_e2e.npz) and the test-time autograd oracle, and the
Gram builds over ntk_kern.

Tolerances on Θ are the project's end-to-end bounds for K: float64 with the
op-by-op ReLU 1e-10 relative, float64 closed form 1e-8, float32 against the float64
fixture on the same float32-representable images 2e-5; the op alone in float64 1e-12."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp.kernel_save_tools import save_K

from conftest import GOLDEN
import configs_util
import ntk_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
RTOL64 = {"exact": 1e-10, "fast": 1e-8}
RTOL32 = 2e-5
NETS = ["mnist_paper_convnet_gp", "mnist_paper_residual_cnn_gp", "mnist_as_tf", "cifar10",
        "mixture_big", "mixture_small"]
F32_TINY = float(np.finfo(np.float32).tiny)


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def rel_err(got, ref):
    """largest |got - ref| / |ref| over the entries where ref is not NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    keep = ~np.isnan(ref)
    assert np.all(np.isfinite(got[keep]))
    return float(np.max(np.abs(got[keep] - ref[keep]) / np.maximum(np.abs(ref[keep]), 1e-300)))


# ------------------------------------------------------------------------------------
# a. the op alone
# ------------------------------------------------------------------------------------
def patches(n1, n2, hw, same, diag, seed, np_dt):
    """Valid covariance patches as relu_ops.npz's generator builds them (Grams of random
    feature vectors, 10% of the x pixels all-zero), |rho| <= 0.98 off the diagonal; Θ is
    standard normal.  Arrays already rounded to np_dt."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n1, hw, 5))
    a[rng.random((n1, hw)) < 0.1] = 0.0
    b = a if same else rng.standard_normal((n2, hw, 5))
    xx, yy = (a * a).sum(-1), (b * b).sum(-1)
    if diag:
        xy = (a * b).sum(-1)
        lim = 0.98 * np.sqrt(xx * yy)
    else:
        xy = np.einsum("ipf,jpf->ijp", a, b)
        lim = 0.98 * np.sqrt(xx[:, None] * yy[None])
    xy = np.clip(xy, -lim, lim)
    if same and not diag:
        idx = np.arange(n1)
        xy[idx, idx] = xx                       # a Gram of one set: rho = 1 on the diagonal
    if same and diag:
        xy = xx.copy()
    theta = rng.standard_normal(xy.shape)
    return tuple(np.ascontiguousarray(v.reshape(-1, hw).astype(np_dt))
                 for v in (xy, theta, xx, yy))


def relu_ntk(xy, theta, xx, yy, n1, n2, same, diag, flags, dt, inplace=False):
    hw = xy.shape[1]
    c, th, vx, vy = (dev(v, dt) for v in (xy, theta, xx, yy))
    oc, oth = (c, th) if inplace else (torch.empty_like(c), torch.empty_like(th))
    a = N.ReluNtkArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(c), N.ptr(th), N.ptr(oc), N.ptr(oth)
    a.xx, a.yy = N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2 = xy.shape[0], n1, n2
    a.hw, a.same, a.diag, a.flags = hw, int(same), int(diag), flags
    sfx = "f64" if dt == torch.float64 else "f32"
    N.check(getattr(N.load(), f"cgp_relu_ntk_{sfx}")(ctypes.byref(a), stream()), "cgp_relu_ntk")
    torch.cuda.synchronize()
    return oc.cpu().numpy(), oth.cpu().numpy()


def relu_plain(xy, xx, yy, n1, n2, same, diag, flags, dt):
    c, vx, vy = (dev(v, dt) for v in (xy, xx, yy))
    out = torch.empty_like(c)
    r = N.ReluArgs()
    r.xy, r.out, r.xx, r.yy = N.ptr(c), N.ptr(out), N.ptr(vx), N.ptr(vy)
    r.nmaps, r.n1, r.n2 = xy.shape[0], n1, n2
    r.hw, r.same, r.diag, r.flags = xy.shape[1], int(same), int(diag), flags
    sfx = "f64" if dt == torch.float64 else "f32"
    N.check(getattr(N.load(), f"cgp_relu_{sfx}")(ctypes.byref(r), stream()), "cgp_relu")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def kdot_ref(xy, xx, yy, n1, n2, same, diag):
    """float64 numpy κ̇ = (π - θ)/2π, 1/2 where the reference overrides the ReLU"""
    xy, xx, yy = (np.asarray(v, dtype=np.float64) for v in (xy, xx, yy))
    hw = xy.shape[1]
    if diag:
        t = xx * yy + F32_TINY
        kd = (np.pi - np.arccos(np.clip(xy / np.sqrt(t), -1, 1))) / (2 * np.pi)
        if same:
            kd[:] = 0.5
        return kd
    t = xx[:, None] * yy[None] + F32_TINY
    c = xy.reshape(n1, n2, hw)
    kd = (np.pi - np.arccos(np.clip(c / np.sqrt(t), -1, 1))) / (2 * np.pi)
    if same:
        idx = np.arange(n1)
        kd[idx, idx] = 0.5
    return kd.reshape(-1, hw)


# (n1, n2, hw, same, diag): one map of one pixel; a partial chunk; ragged last chunks (784
# pixels: 2 maps of a 2048-element chunk, 136 maps); cifar10's 1x1 tail; same; diag; both
OP_CASES = [(1, 1, 1, 0, 0), (3, 2, 49, 0, 0), (17, 8, 784, 0, 0), (17, 8, 1, 0, 0),
            (5, 5, 196, 1, 0), (6, 6, 100, 0, 1), (4, 4, 25, 1, 1)]


@pytest.mark.parametrize("mode", ["fast", "exact"])
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_relu_ntk_op(case, dtn, mode):
    """K' bit-equal to cgp_relu_*, Θ' against float64 numpy, Θ/2 exactly where the reference
    overrides, in-place bit-equal to out-of-place.

    Bounds on Θ' = Θ·κ̇ (relative; Θ is an input, so they are κ̇'s).  float64: 1e-12, the
    fused-stage bound.  float32: with |rho| <= 0.98 the computed rho carries at most
    ~2.1e-7 relative (t: half an ulp halved by the root, the hardware rsq one ulp, the
    product half an ulp), which dθ/drho = 1/sqrt(1 - rho²) <= 5.03 turns into 1.0e-6 of θ;
    acosf adds up to 4 ulp of θ <= π (1.5e-6), the float π 8.7e-8; κ̇ >= (π - acos(-0.98))/2π,
    i.e. π - θ >= 0.2003, so at most (1.0e-6 + 1.5e-6 + 0.1e-6 + an ulp)/0.2003 = 1.4e-5
    relative, within the project's float32 bound 2e-5."""
    n1, n2, hw, same, diag = case
    dt, np_dt = (torch.float64, np.float64) if dtn == "f64" else (torch.float32, np.float32)
    flags = N.CGP_FLAG_EXACT_RELU if mode == "exact" else 0
    xy, theta, xx, yy = patches(n1, n2, hw, same, diag, 100 + hw + n1, np_dt)
    k, th = relu_ntk(xy, theta, xx, yy, n1, n2, same, diag, flags, dt)
    np.testing.assert_array_equal(k, relu_plain(xy, xx, yy, n1, n2, same, diag, flags, dt))
    ref = theta.astype(np.float64) * kdot_ref(xy, xx, yy, n1, n2, same, diag)
    err = rel_err(th, ref)
    print(f"relu_ntk {dtn} {mode} {case}: theta rel err {err:.2e}")
    assert err < (1e-12 if dtn == "f64" else 2e-5)
    if same:
        sel = np.arange(n1) * (n2 + 1) if not diag else np.arange(n1)
        np.testing.assert_array_equal(th[sel], theta[sel] / 2)
        np.testing.assert_array_equal(k[sel], xx / 2)
    ki, thi = relu_ntk(xy, theta, xx, yy, n1, n2, same, diag, flags, dt, inplace=True)
    np.testing.assert_array_equal(ki, k)
    np.testing.assert_array_equal(thi, th)


def test_relu_ntk_theta_aliasing_xy():
    """the first ReLU after a conv reads Θ from the K buffer itself (theta == xy)"""
    n1, n2, hw = 5, 3, 49
    xy, _, xx, yy = patches(n1, n2, hw, 0, 0, 7, np.float64)
    c, vx, vy = dev(xy), dev(xx), dev(yy)
    oc, oth = torch.empty_like(c), torch.empty_like(c)
    a = N.ReluNtkArgs()
    a.xy = a.theta = N.ptr(c)
    a.out_xy, a.out_theta, a.xx, a.yy = N.ptr(oc), N.ptr(oth), N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2, a.hw = n1 * n2, n1, n2, hw
    N.check(N.load().cgp_relu_ntk_f64(ctypes.byref(a), stream()), "cgp_relu_ntk")
    torch.cuda.synchronize()
    k, th = relu_ntk(xy, xy, xx, yy, n1, n2, 0, 0, 0, torch.float64)
    np.testing.assert_array_equal(oc.cpu().numpy(), k)
    np.testing.assert_array_equal(oth.cpu().numpy(), th)


# ------------------------------------------------------------------------------------
# b. end to end against the reference's fixture
# ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "ntk_e2e.npz"))


def product_model(name):
    if name.startswith("mixture_"):
        return configs_util.mixture_nets()[name[len("mixture_"):]][0]
    return configs_util.model(name)


def e2e_errors(model, z, name, dt):
    """relative errors of Θ (and K) in every call form against network `name`'s arrays"""
    X, Z = dev(z[name + "_X"], dt), dev(z[name + "_Z"], dt)
    errs = {}
    with torch.no_grad():
        k, th = model.ntk(X, Z, False, False, return_nngp=True)
        errs["Kxz"], errs["Txz"] = rel_err(k.cpu(), z[name + "_Kxz"]), \
            rel_err(th.cpu(), z[name + "_Txz"])
        th = model.ntk(X).cpu().numpy()
        errs["Txx"] = rel_err(th, z[name + "_Txx"])
        errs["Txx_diag"] = rel_err(np.diag(th), z[name + "_Tdiag"])
        errs["Tdiag"] = rel_err(model.ntk(X, diag=True).cpu(), z[name + "_Tdiag"])
        errs["Txzdiag"] = rel_err(model.ntk(X[:3], Z, False, True).cpu(), z[name + "_Txzdiag"])
    return errs


@pytest.mark.parametrize("mode", ["fast", "exact", "f32"])
@pytest.mark.parametrize("name", NETS)
def test_ntk_e2e_fixture(fixture, name, mode):
    dt = torch.float32 if mode == "f32" else torch.float64
    model = product_model(name).to(DEV, dt)
    model.set_exact_relu(mode == "exact")
    errs = e2e_errors(model, fixture, name, dt)
    print(f"ntk e2e {name} {mode}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    tol = RTOL32 if mode == "f32" else RTOL64[mode]
    assert max(errs.values()) < tol, errs


# ------------------------------------------------------------------------------------
# c. a small strided network at 10x10: tile shapes, tiles of a larger call, symmetry
# ------------------------------------------------------------------------------------
def strided_net():
    m = cnn_gp
    return m.Sequential(m.Conv2d(3, var_bias=0.2), m.ReLU(), m.Conv2d(3, stride=2), m.ReLU(),
                        m.Conv2d(2, dilation=2, var_weight=1.5), m.ReLU(),
                        m.Conv2d(5, padding=0))


@pytest.fixture(scope="module")
def strided_case():
    """17 + 9 images at 10x10 and the oracle's Θ for the 17x9 block, computed once"""
    rng = np.random.default_rng(31)
    X = rng.random((17, 2, 10, 10), dtype=np.float32).astype(np.float64)
    Z = rng.random((9, 2, 10, 10), dtype=np.float32).astype(np.float64)
    model = strided_net().double()
    k, th = ntk_oracle.ntk(configs_util.spec_of(model), X, Z, False, False)
    return X, Z, k, th


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (17, 8)])
def test_ntk_tile_shapes_against_oracle(strided_case, shape):
    X, Z, k_ref, th_ref = strided_case
    a, b = shape
    model = strided_net().double().to(DEV).set_exact_relu(True)
    with torch.no_grad():
        k, th = model.ntk(dev(X[:a]), dev(Z[:b]), False, False, return_nngp=True)
    assert tuple(th.shape) == shape
    assert rel_err(k.cpu(), k_ref[:a, :b]) < RTOL64["exact"]
    assert rel_err(th.cpu(), th_ref[:a, :b]) < RTOL64["exact"]


def test_ntk_tile_of_larger_call_and_symmetry(strided_case):
    X, Z, _, _ = strided_case
    model = strided_net().double().to(DEV)
    Xd, Zd = dev(X), dev(Z)
    with torch.no_grad():
        full = model.ntk(Xd, Zd, False, False)
        part = model.ntk(Xd[3:11], Zd[2:7], False, False)
        assert torch.equal(full[3:11, 2:7], part)          # a pair depends on its images only
        txx = model.ntk(Xd)
        off = model.ntk(Xd[:6], Xd[6:], False, False)
    assert torch.equal(txx[:6, 6:], off)
    t = txx.cpu().numpy()
    assert np.max(np.abs(t - t.T) / np.abs(t)) < 1e-13
    assert np.all(np.diag(t) > 0)


# ------------------------------------------------------------------------------------
# d. return_nngp: K is the layer path's forward
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mnist_paper_convnet_gp", "mnist_as_tf"])
def test_ntk_return_nngp_is_forward(fixture, name):
    model = product_model(name).to(DEV, torch.float64)
    X, Z = dev(fixture[name + "_X"]), dev(fixture[name + "_Z"])
    with torch.no_grad():
        for args in ((X, Z, False, False), (X,), (X[:3], Z, False, True)):
            k, th = model.ntk(*args, return_nngp=True)
            assert torch.equal(th, model.ntk(*args))
            fused = model(*args)                             # whole-network kernel (default)
            model.set_fused_network(False)
            model.set_fusion(False)
            assert torch.equal(k, model(*args))              # the same launches, op by op
            model.set_fusion(True)
            layer = model(*args)
            model.set_fused_network(True)
            assert torch.equal(k, layer)                     # fusion changes no arithmetic
            assert rel_err(k.cpu(), fused.cpu()) < 1e-12


def test_ntk_not_1x1_and_no_conv():
    m = cnn_gp
    x = torch.rand(3, 1, 6, 6, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="not 1x1"):
        m.Sequential(m.Conv2d(3), m.ReLU()).double().ntk(x)
    x1 = torch.rand(3, 2, 1, 1, dtype=torch.float64, device=DEV)
    k, th = m.Sequential(m.ReLU()).ntk(x1, return_nngp=True)     # no Conv2d: Θ = 0
    assert torch.equal(th, torch.zeros_like(k)) and torch.equal(k, m.Sequential(m.ReLU())(x1))
    k, th = m.Sequential(m.Conv2d(1, var_bias=0.5)).ntk(x1, return_nngp=True)
    assert torch.equal(k, th) and k.data_ptr() != th.data_ptr()   # one conv: Θ = K
    assert m.Sequential(m.Conv2d(1)).ntk(x1.cpu()).device.type == "cpu"


# ------------------------------------------------------------------------------------
# e. Gram builds
# ------------------------------------------------------------------------------------
def test_gram_matrix_ntk(fixture):
    name = "mnist_paper_residual_cnn_gp"
    model = product_model(name).to(DEV, torch.float64)
    X = dev(fixture[name + "_X"])
    with torch.no_grad():
        ref = model.ntk(X)
    g = gram.gram_matrix(model, X, batch_size=2, ntk=True)
    iu = np.triu_indices(5)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], ref.cpu().numpy()[iu])
    assert torch.isnan(g[2, 0]) and torch.isnan(g[4, 1])        # tiles below the diagonal
    gz = gram.gram_matrix(model, X, dev(fixture[name + "_Z"]), batch_size=2, ntk=True)
    assert rel_err(gz.cpu(), fixture[name + "_Txz"]) < RTOL64["fast"]
    assert not torch.equal(g, gram.gram_matrix(model, X, batch_size=2))


class MemH5:
    def __init__(self):
        self.d = {}

    def keys(self):
        return self.d.keys()

    def create_dataset(self, name, shape, dtype, fillvalue, chunks, maxshape):
        self.d[name] = np.full(shape, fillvalue, dtype=dtype)
        return self.d[name]


def test_save_K_with_ntk_kern(fixture):
    from torch.utils.data import TensorDataset
    name = "mixture_small"
    model = product_model(name).to(DEV, torch.float64)
    X = torch.from_numpy(fixture[name + "_X"])
    ds = TensorDataset(X, torch.zeros(len(X), dtype=torch.int64))
    nngp = gram.model_kern(model)

    def kern(x, x2, same, diag):
        return nngp(x, x2, same).cpu().numpy()

    f, g = MemH5(), MemH5()
    save_K(f, gram.ntk_kern(model), "K", ds, None, False, 2, print_interval=1e9)
    save_K(g, kern, "K", ds, None, False, 2, print_interval=1e9)
    np.testing.assert_array_equal(np.isnan(f.d["K"]), np.isnan(g.d["K"]))
    assert np.isnan(f.d["K"]).any()
    with torch.no_grad():
        ref = model.ntk(X.to(DEV)).cpu().numpy().astype(np.float32)
    keep = ~np.isnan(f.d["K"][0])
    np.testing.assert_array_equal(f.d["K"][0][keep], ref[keep])
    save_K(f, gram.ntk_kern(model), "Kd", ds, None, True, 2, print_interval=1e9)
    np.testing.assert_array_equal(f.d["Kd"][0], np.diag(ref))
