"""GPU tests of the erf nonlinearity: cgp_erf_* / cgp_var_erf_* alone, networks with
cnn_gp.Erf through forward and ntk against the test-time oracle (tests/erf_oracle.py), the
Gram builds on an erf model, and that a ReLU-only model still makes the launches it made
before Erf existed.

Tolerances are the project's own (tests/test_gpu_ntk.py): the op alone in float64 1e-12,
float64 end to end 1e-10, float32 against the float64 oracle on float32-representable
images 2e-5.  Inputs in [0, 1) use the relative error; signed inputs use
max|got - ref| / max|ref|, because erf kernels cross zero."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp.kernel_save_tools import save_K

import configs_util
import erf_oracle as EO
import net_zoo

pytestmark = pytest.mark.gpu

DEV = "cuda"
OP_TOL = {"f64": 1e-12, "f32": 2e-5}
NET_TOL = {"f64": 1e-10, "f32": 2e-5}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def max_err(got, ref):
    """max|got - ref| / max|ref| over the entries where ref is not NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    keep = ~np.isnan(ref)
    assert keep.any() and np.all(np.isfinite(got[keep]))
    return float(np.max(np.abs(got[keep] - ref[keep])) / np.max(np.abs(ref[keep])))


# ------------------------------------------------------------------------------------
# a. the op alone
# ------------------------------------------------------------------------------------
def patches(n1, n2, hw, same, diag, seed, np_dt, zero_frac=0.1):
    """Random valid patches: v in (0, 3], |rho| <= 0.98, signed c; ``zero_frac`` of the x
    pixels have zero variance (then c = 0 in their pairs).  With same, yy = xx and the
    i = j pairs hold c = v; Θ is standard normal.  Arrays already rounded to np_dt."""
    rng = np.random.default_rng(seed)
    xx = 3.0 * (1.0 - rng.random((n1, hw)))
    xx[rng.random((n1, hw)) < zero_frac] = 0.0
    yy = xx if same else 3.0 * (1.0 - rng.random((n2, hw)))
    if diag:
        rho = rng.uniform(-0.98, 0.98, (n1, hw))
        xy = rho * np.sqrt(xx * yy)
    else:
        rho = rng.uniform(-0.98, 0.98, (n1, n2, hw))
        xy = rho * np.sqrt(xx[:, None] * yy[None])
    if same and not diag:
        idx = np.arange(n1)
        xy[idx, idx] = xx
    if same and diag:
        xy = xx.copy()
    theta = rng.standard_normal(xy.shape)
    addend = rng.standard_normal(xy.shape)
    return tuple(np.ascontiguousarray(v.reshape(-1, hw).astype(np_dt))
                 for v in (xy, theta, xx, yy, addend))


def run_erf(xy, theta, xx, yy, n1, n2, same, diag, dtn, addend=None, inplace=False,
            alias=False):
    """cgp_erf_*: theta None is the forward-only form; ``alias`` passes xy itself as theta;
    ``inplace`` writes over the inputs.  Returns (K', Θ' or None) as numpy arrays."""
    dt = TORCH_DT[dtn]
    c, vx, vy = dev(xy, dt), dev(xx, dt), dev(yy, dt)
    th = c if alias else (None if theta is None else dev(theta, dt))
    ad = None if addend is None else dev(addend, dt)
    oc = c if inplace else torch.empty_like(c)
    oth = None if th is None else (th if inplace and not alias else torch.empty_like(c))
    a = N.ErfArgs()
    a.xy, a.theta, a.out_xy, a.out_theta = N.ptr(c), N.ptr(th), N.ptr(oc), N.ptr(oth)
    a.addend, a.xx, a.yy = N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.nmaps, a.n1, a.n2 = xy.shape[0], n1, n2
    a.hw, a.same, a.diag = xy.shape[1], int(same), int(diag)
    N.check(getattr(N.load(), f"cgp_erf_{dtn}")(ctypes.byref(a), stream()), "cgp_erf")
    torch.cuda.synchronize()
    return oc.cpu().numpy(), None if oth is None else oth.cpu().numpy()


def run_var_erf(xx, yy, same, dtn):
    dt = TORCH_DT[dtn]
    vx, vy = dev(xx, dt), dev(yy, dt)
    ox, oy = torch.empty_like(vx), torch.empty_like(vy)
    N.call(f"cgp_var_erf_{dtn}", N.ptr(vx), N.ptr(vy), xx.shape[0], yy.shape[0], xx.shape[1],
           int(same), N.ptr(ox), N.ptr(oy), stream())
    torch.cuda.synchronize()
    return ox.cpu().numpy(), oy.cpu().numpy()


def op_ref(xy, theta, xx, yy, same, diag):
    """float64 oracle (K', Θ', xx', yy') of one erf step on [n][hw] arrays"""
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))[:, None, None, :]  # noqa
    c, th, vx, vy = t(xy), t(theta), t(xx), t(yy)
    _, _, k, vx2, vy2 = EO._erf((bool(same), bool(diag), c, vx, vy))
    kd = EO.erf_kdot(c, vx, vy, bool(same), bool(diag))
    flat = lambda a: a.reshape(-1, xy.shape[1]).numpy()                         # noqa: E731
    return flat(k), flat(th * kd), flat(vx2), flat(vy2)


# (n1, n2, hw, same, diag): a partial chunk of maps in the last workgroup; the i = j
# overrides; the diag pair indexing without and with same; the final 1x1 map; 784 pixels
# (2 maps of a 2048-element chunk) with an odd map in the last chunk
OP_CASES = [(5, 3, 49, 0, 0), (4, 4, 49, 1, 0), (6, 6, 25, 0, 1), (6, 6, 25, 1, 1),
            (5, 3, 1, 0, 0), (7, 1, 784, 0, 0)]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: "-".join(map(str, c)))
def test_erf_op(case, dtn):
    """K', Θ' and the variance maps against the float64 oracle, and every calling form
    bit-equal to the plain one.

    float32 bound (inputs are float32-representable, so only the arithmetic errs).  With
    P = (1 + 2v1)(1 + 2v2), D = P - 4c² is summed from terms of total magnitude <= P + 4c²
    in about 5 roundings of 2⁻²⁴ each; v <= 3 and |rho| <= 0.98 give (P + 4c²)/(P - 4c²) <=
    (49 + 34.6)/(49 - 34.6) = 5.8, so |δD|/D <= 5·6e-8·5.8 = 1.7e-6.  κ̇ = (4/π)/√D takes
    half of that plus the root's and the division's roundings: 1.0e-6 relative.  K' =
    (2/π)atan(t), t = 2c/√D: |δK'| = (2/π)|δt|/(1 + t²) with |δt| <= |t|(0.87e-6 + 2·6e-8)
    and |t|/(1 + t²) <= 1/2, i.e. 3.2e-7, plus atanf's ~2 ulp of a value below π/2 (2.4e-7)
    and the product's: under 6e-7 absolute against max|ref| ~ 0.6.  Both sit well inside the
    project's float32 bound 2e-5, which is asserted; measured values are printed."""
    n1, n2, hw, same, diag = case
    xy, theta, xx, yy, addend = patches(n1, n2, hw, same, diag, 200 + hw + n1, NP_DT[dtn])
    rk, rth, rvx, rvy = op_ref(xy, theta, xx, yy, same, diag)
    tol = OP_TOL[dtn]

    k0, none = run_erf(xy, None, xx, yy, n1, n2, same, diag, dtn)
    assert none is None
    k, th = run_erf(xy, theta, xx, yy, n1, n2, same, diag, dtn)
    np.testing.assert_array_equal(k, k0)                    # one device function for K'
    vx, vy = run_var_erf(xx, yy, same, dtn)
    errs = dict(K=max_err(k, rk), T=max_err(th, rth), xx=max_err(vx, rvx), yy=max_err(vy, rvy))
    print(f"erf op {dtn} {case}: " + " ".join(f"{n}={e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) < tol, errs
    if same:
        np.testing.assert_array_equal(vy, vx)
        sel = np.arange(n1) if diag else np.arange(n1) * (n2 + 1)
        np.testing.assert_array_equal(k[sel], vx)           # K' = v'[i], the same bits
        want = theta[sel].astype(np.float64) * (4 / math.pi) \
            / np.sqrt(1 + 4 * xx.astype(np.float64))
        assert max_err(th[sel], want) < tol
    # zero-variance pixels of an overridden pair: c = v = 0 gives 0 and Θ·4/π, no NaN
    assert np.all(np.isfinite(k)) and np.all(np.isfinite(th))
    if same:
        z = xx == 0
        assert z.any() or hw == 1
        np.testing.assert_array_equal(k[sel][z], 0)
        assert np.all(np.abs(th[sel][z] - theta[sel][z].astype(np.float64) * (4 / math.pi))
                      <= tol * np.abs(theta[sel][z]))

    # in place; theta aliasing xy; the addend (a separate rounding, on K' only)
    ki, thi = run_erf(xy, theta, xx, yy, n1, n2, same, diag, dtn, inplace=True)
    np.testing.assert_array_equal(ki, k)
    np.testing.assert_array_equal(thi, th)
    ki, _ = run_erf(xy, None, xx, yy, n1, n2, same, diag, dtn, inplace=True)
    np.testing.assert_array_equal(ki, k)
    ka, tha = run_erf(xy, None, xx, yy, n1, n2, same, diag, dtn, alias=True)
    kx, thx = run_erf(xy, xy, xx, yy, n1, n2, same, diag, dtn)
    np.testing.assert_array_equal(ka, k)
    np.testing.assert_array_equal(kx, k)
    np.testing.assert_array_equal(tha, thx)
    kai, thai = run_erf(xy, None, xx, yy, n1, n2, same, diag, dtn, alias=True, inplace=True)
    np.testing.assert_array_equal(kai, k)
    np.testing.assert_array_equal(thai, thx)
    kd, thd = run_erf(xy, theta, xx, yy, n1, n2, same, diag, dtn, addend=addend)
    np.testing.assert_array_equal(kd, k + addend)
    np.testing.assert_array_equal(thd, th)
    kd0, _ = run_erf(xy, None, xx, yy, n1, n2, same, diag, dtn, addend=addend)
    np.testing.assert_array_equal(kd0, kd)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_erf_op_all_zero(dtn):
    """v = c = 0 everywhere, no override in play: K' = 0 and Θ' = Θ·4/π"""
    n1, n2, hw = 3, 2, 10
    zeros = lambda n: np.zeros((n, hw), dtype=NP_DT[dtn])                       # noqa: E731
    theta = np.random.default_rng(1).standard_normal((n1 * n2, hw)).astype(NP_DT[dtn])
    k, th = run_erf(zeros(n1 * n2), theta, zeros(n1), zeros(n2), n1, n2, 0, 0, dtn)
    np.testing.assert_array_equal(k, 0)
    assert rel_err(th, theta.astype(np.float64) * (4 / math.pi)) < OP_TOL[dtn]
    vx, vy = run_var_erf(zeros(n1), zeros(n2), 0, dtn)
    np.testing.assert_array_equal(vx, 0)
    np.testing.assert_array_equal(vy, 0)


# ------------------------------------------------------------------------------------
# b. networks
# ------------------------------------------------------------------------------------
def nets(side):
    """name -> (fresh float32-built model, pure): ``pure`` networks hold no ReLU, so the
    autograd Θ is valid on every pair"""
    m = cnn_gp
    C, E, R, S = m.Conv2d, m.Erf, m.ReLU, m.Sequential
    t = lambda *v: torch.tensor(v, dtype=torch.float32)                         # noqa: E731

    def convnet(b):
        return S(C(3, var_bias=2 * b), E(), C(3, var_weight=1.5, var_bias=b), E(), C(3), E(),
                 C(side, padding=0, var_bias=b))

    return {
        "convnet_bias": (convnet(0.1), True),
        "convnet_nobias": (convnet(0.0), True),
        "identity_block": (S(C(3, var_bias=0.1), m.Sum([S(), S(E(), C(3), E(), C(3))]), E(),
                             C(side, padding=0)), True),
        # resnet_block(stride=2, projection_shortcut=True) with Erf
        "projection_block": (S(C(3), E(), m.Sum([C(1, stride=2),
                                                 S(C(3, stride=2), E(), C(3))]),
                               E(), C(4, padding=0)), True),
        "mixture": (S(C(3), m.Mixture([S(E(), C(3, var_bias=0.2)), S(R(), C(3))], t(0.3, -0.5)),
                      E(), C(side, padding=0)), False),
        "alternating": (S(C(3, var_bias=0.1), R(), C(3), E(), C(3, var_weight=2.0), R(), C(3),
                          E(), C(side, padding=0)), False),
        "head_only": (S(E(), C(side, padding=0, var_bias=0.3)), True),
    }


NET_NAMES = list(nets(8))
SIZES = [(8, 1), (7, 3)]
MODES = ["xx", "xz", "same_diag", "xz_diag"]


def images(side, channels, signed=False):
    rng = np.random.default_rng(10 * side + channels)
    draw = (lambda n: rng.standard_normal((n, channels, side, side)).astype(np.float32)) \
        if signed else (lambda n: rng.random((n, channels, side, side), dtype=np.float32))
    return draw(5).astype(np.float64), draw(3).astype(np.float64)


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:3], Z, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def reference(name, side, channels, signed=False):
    """mode -> (K, Θ) from the float64 oracle, computed once per network and size.  K from
    the walk; Θ by autograd where it is valid on every entry (no ReLU), stepwise otherwise."""
    model, pure = nets(side)[name]
    model = model.double()
    X, Z = images(side, channels, signed)
    out = {}
    for mode in MODES:
        args = mode_args(X, Z, mode)
        k = EO.kernel(model, *args)
        if pure:
            th = EO.ntk_autograd(model, args[0], None if mode == "xx" else args[1],
                                 diag=mode.endswith("diag"))[1]
            assert not np.isnan(th).any()
        else:
            sk, th = EO.ntk_stepwise(model, *args)
            assert max_err(sk, k) < 1e-13
        out[mode] = (k, th)
    return out


def check_network(name, side, channels, dtn, signed=False):
    ref = reference(name, side, channels, signed)
    model = nets(side)[name][0].to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(side, channels, signed))
    err = max_err if signed else rel_err
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(X, Z, mode)
            rk, rth = ref[mode]
            fwd = model(*args)
            k, th = model.ntk(*args, return_nngp=True)
            assert tuple(fwd.shape) == rk.shape
            errs["K_" + mode] = err(fwd.cpu(), rk)
            errs["T_" + mode] = err(th.cpu(), rth)
            # one device function per stream: K of the NTK run is forward's K
            assert max_err(k.cpu(), fwd.cpu().numpy()) < 1e-12, mode
            if mode == "xx":
                kxx, txx = fwd.cpu().numpy(), th.cpu().numpy()
            if mode == "same_diag":
                assert max_err(fwd.cpu(), np.diag(kxx)) < 1e-12
                assert max_err(th.cpu(), np.diag(txx)) < 1e-12
    assert np.max(np.abs(txx - txx.T)) <= 1e-13 * np.max(np.abs(txx))
    assert np.max(np.abs(kxx - kxx.T)) <= 1e-13 * np.max(np.abs(kxx))
    print(f"erf net {name} {side}x{side}x{channels} {dtn}{' signed' if signed else ''}: "
          + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs
    return kxx


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", NET_NAMES)
def test_erf_network(name, size, dtn):
    check_network(name, size[0], size[1], dtn)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_erf_network_signed_inputs(dtn):
    """standard normal images: the erf kernel goes negative, which no ReLU network's does"""
    kxx = check_network("convnet_nobias", 7, 3, dtn, signed=True)
    assert kxx.min() < 0 < kxx.max()


def test_erf_ignores_exact_relu_and_fusion():
    model = nets(8)["identity_block"][0].to(DEV, torch.float64)
    X = dev(images(8, 1)[0])
    with torch.no_grad():
        k = model(X)
        assert torch.equal(model.set_exact_relu(True)(X), k)
        model.set_exact_relu(False)
        assert torch.equal(model.set_fusion(False)(X), k)      # fusion changes no arithmetic
        assert torch.equal(model.set_fused_network(False)(X), k)


@pytest.mark.parametrize("act", ["ReLU", "Erf"])
def test_ntk_without_a_conv_returns_forwards_K(act):
    """A model without a Conv2d has Θ = 0 and its ntk K IS forward's, bit for bit, on
    whichever path forward runs (a ReLU-only model at 1x1 runs the whole-network kernel,
    whose fp64 ReLU is an ulp away from cgp_relu_* on some of these 576 pairs)."""
    model = cnn_gp.Sequential(getattr(cnn_gp, act)())
    x = torch.from_numpy(np.random.default_rng(11).random((24, 2, 1, 1))).to(DEV)
    z = torch.from_numpy(np.random.default_rng(12).random((24, 2, 1, 1))).to(DEV)
    with torch.no_grad():
        for args in ((x,), (x, z, False, False), (x, x, True, True)):
            k, th = model.ntk(*args, return_nngp=True)
            assert torch.equal(k, model(*args))
            assert torch.equal(th, torch.zeros_like(k))


# ------------------------------------------------------------------------------------
# c. Gram builds
# ------------------------------------------------------------------------------------
class MemH5:
    def __init__(self):
        self.d = {}

    def keys(self):
        return self.d.keys()

    def create_dataset(self, name, shape, dtype, fillvalue, chunks, maxshape):
        self.d[name] = np.full(shape, fillvalue, dtype=dtype)
        return self.d[name]


@pytest.fixture(scope="module")
def gram_case():
    model = nets(8)["projection_block"][0].to(DEV, torch.float64)
    X = torch.from_numpy(np.random.default_rng(4).random((10, 2, 8, 8), dtype=np.float32)
                         .astype(np.float64))
    with torch.no_grad():
        k, th = model.ntk(X.to(DEV), return_nngp=True)
    return model, X, k.cpu().numpy(), th.cpu().numpy()


def test_erf_gram_matrix(gram_case):
    model, X, k, th = gram_case
    assert model.image_variances(X.to(DEV)) is None          # declines: the per-tile fallback
    iu = np.triu_indices(10)
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], k[iu])
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4, ntk=True)
    np.testing.assert_array_equal(g.cpu().numpy()[iu], th[iu])


def test_erf_save_K(gram_case):
    from torch.utils.data import TensorDataset
    model, X, k, th = gram_case
    ds = TensorDataset(X, torch.zeros(len(X), dtype=torch.int64))
    f = MemH5()
    nngp = gram.model_kern(model)
    save_K(f, lambda x, x2, same, diag: nngp(x, x2, same).cpu().numpy(), "K", ds, None, False,
           4, print_interval=1e9)
    save_K(f, gram.ntk_kern(model), "T", ds, None, False, 4, print_interval=1e9)
    for key, ref in (("K", k), ("T", th)):
        keep = ~np.isnan(f.d[key][0])
        assert keep[np.triu_indices(10)].all()
        np.testing.assert_array_equal(f.d[key][0][keep], ref.astype(np.float32)[keep])
    save_K(f, gram.ntk_kern(model), "Td", ds, None, True, 4, print_interval=1e9)
    np.testing.assert_array_equal(f.d["Td"][0], np.diag(th).astype(np.float32))


# ------------------------------------------------------------------------------------
# d. a ReLU-only model is untouched
# ------------------------------------------------------------------------------------
def recorded_calls(model, x, monkeypatch):
    """the names N.check sees (every library call goes through it) during model(x)"""
    seen = []
    real = N.check

    def check(rc, what):
        seen.append(what)
        return real(rc, what)

    with torch.no_grad():
        model(x)                                # plans, recipes and uploads built
        monkeypatch.setattr(N, "check", check)
        model(x)
        monkeypatch.setattr(N, "check", real)
    torch.cuda.synchronize()
    return seen


# recorded on the commit before Erf existed, N = 4, float64: the whole-network path
# (default) and the layer path (set_fused_network(False))
_VR, _AX = "cgp_var_relu_f64", "cgp_axpby_f64"
PARENT_CALLS = {
    ("in7", "net"): ["cgp_var_chain", "cgp_rsqrt_batch_f64", "cgp_net", "cgp_net"],
    ("in7", "layer"): ["cgp_moments_var", "cgp_conv", _VR, "cgp_conv", _VR, "cgp_conv", _AX, _AX,
                       _VR, "cgp_conv", _VR, "cgp_conv", _AX, _AX, _VR] + ["cgp_conv"] * 7,
    ("mnist_paper_convnet_gp", "net"): ["cgp_var_chain", "cgp_rsqrt_batch_f64", "cgp_net"],
    ("mnist_paper_convnet_gp", "layer"): ["cgp_moments_var"] + ["cgp_conv", _VR] * 7
    + ["cgp_conv"] * 9,
}


@pytest.mark.parametrize("path", ["net", "layer"])
@pytest.mark.parametrize("name", ["in7", "mnist_paper_convnet_gp"])
def test_relu_only_model_makes_the_same_calls(name, path, monkeypatch):
    if name == "in7":
        net = net_zoo.zoo()[name]
        model, shape = net.build(), (4, net.channels, net.side, net.side)
    else:
        model, shape = configs_util.model(name).double(), (4, 1, 28, 28)
    model = model.to(DEV).set_fused_network(path == "net")
    # numpy draws: torch's global generators stay where they were for the tests after this
    x = dev(np.random.default_rng(0).random(shape))
    assert recorded_calls(model, x, monkeypatch) == PARENT_CALLS[name, path]
