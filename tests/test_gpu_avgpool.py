"""GPU tests of windowed average pooling: cgp_covmap_avgpool_* and cgp_covmap_diag_* alone,
networks with cnn_gp.AvgPool2d through forward and position_covariance against the test-time
oracle (tests/avgpool_oracle.py), chunking (of the self pass as well), the tie of the self
pass to the layer path's variance pipeline, and the Gram builds.

Tolerances are those of tests/test_gpu_pool.py: an op alone 1e-12 in float64, a network
1e-10, float32 against the float64 oracle on float32-representable inputs 2e-5; errors are
max|got - ref| / max|ref|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp.kernel_save_tools import save_K
from cnn_gp.program import Plan

import avgpool_oracle as AO

pytestmark = pytest.mark.gpu

DEV = "cuda"
OP_TOL = {"f64": 1e-12, "f32": 2e-5}
NET_TOL = {"f64": 1e-10, "f32": 2e-5}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}

m = cnn_gp
C, R, E, S, G, A = m.Conv2d, m.ReLU, m.Erf, m.Sequential, m.GlobalAvgPool, m.AvgPool2d


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


# ------------------------------------------------------------------------------------
# a. the entry points alone
# ------------------------------------------------------------------------------------
def run_avgpool(s, k, stride, dtn):
    """cgp_covmap_avgpool_* on maps [P, H, W, H, W] in the oracle's layout"""
    dt = TORCH_DT[dtn]
    h, w = s.shape[1:3]
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    sd = dev(AO.to_device_layout(s), dt)
    out = torch.full((len(s), (ho * wo) ** 2), float("nan"), dtype=dt, device=DEV)
    a = N.CovAvgPoolArgs()
    a.in_, a.out, a.npairs = N.ptr(sd), N.ptr(out), len(s)
    a.h, a.w, a.ho, a.wo, a.k, a.stride = h, w, ho, wo, k, stride
    N.check(getattr(N.load(), f"cgp_covmap_avgpool_{dtn}")(ctypes.byref(a), stream()),
            "cgp_covmap_avgpool")
    torch.cuda.synchronize()
    return AO.from_device_layout(out.cpu().numpy(), ho, wo)


# (h, w, k, stride): a dropped column, overlapping windows, a 1x1 output, the identity, a
# w x w block of 289 > 256 elements (the kernel loops), and the flagship's 28x28.  Pair
# counts 1, 5, 9: a workgroup holds several row pairs of a small map and meets a remainder
AVG_GEOMETRIES = [(4, 4, 2, 2), (6, 5, 2, 2), (7, 6, 3, 2), (5, 5, 5, 5), (6, 6, 1, 1),
                  (17, 17, 2, 2), (28, 28, 2, 2)]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("geom", AVG_GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_covmap_avgpool(geom, dtn):
    h, w, k, stride = geom
    rng = np.random.default_rng(1000 * h + 10 * w + k)
    worst = 0.0
    for pairs in ((3,) if h == 28 else (1, 5, 9)):
        s = rng.standard_normal((pairs, h, w, h, w)).astype(NP_DT[dtn]).astype(np.float64)
        got = run_avgpool(s, k, stride, dtn)
        ref = AO.avgpool_map(s, k, stride)
        assert got.shape == ref.shape
        worst = max(worst, max_err(got, ref))
        if (k, stride) == (1, 1):
            np.testing.assert_array_equal(got, s)                   # the identity, bit for bit
        if pairs > 1:
            # a pair's result depends on that pair alone: the grid and the pair count move
            np.testing.assert_array_equal(run_avgpool(s[1:], k, stride, dtn), got[1:])
    print(f"covmap_avgpool {dtn} {geom}: {worst:.2e}")
    assert worst < OP_TOL[dtn]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_covmap_diag(dtn):
    """a scattered, non-monotone pair_i on a non-square map; images no pair names keep their
    contents"""
    dt = TORCH_DT[dtn]
    h, w, n = 5, 3, 8
    pair_i = np.array([4, 0, 6, 2])
    rng = np.random.default_rng(21)
    s = rng.standard_normal((len(pair_i), h, w, h, w)).astype(NP_DT[dtn])
    sd = dev(AO.to_device_layout(s), dt)
    out = torch.full((n, h, w), -7.0, dtype=dt, device=DEV)
    di = torch.as_tensor(pair_i).to(DEV, torch.int32)
    N.call(f"cgp_covmap_diag_{dtn}", N.ptr(sd), N.ptr(di), len(pair_i), h, w, N.ptr(out), stream())
    torch.cuda.synchronize()
    want = np.full((n, h, w), -7.0, dtype=NP_DT[dtn])
    want[pair_i] = s[:, np.arange(h)[:, None], np.arange(w)[None, :],
                     np.arange(h)[:, None], np.arange(w)[None, :]]
    np.testing.assert_array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------
# b. networks through forward and position_covariance
# ------------------------------------------------------------------------------------
def pooled_nets():
    """name -> (model, image side lengths)"""
    t = lambda *v: torch.tensor(v, dtype=torch.float32)                          # noqa: E731
    l1, l2 = dict(var_weight=1.3, var_bias=0.2), dict(var_weight=0.9, var_bias=0.1)
    conv = lambda: C(3, var_weight=1.7, var_bias=0.3)                            # noqa: E731
    return {
        # the CPU tests' nets
        "finite": (S(C(3, **l1), A(2), R(), C(3, **l2), G()), (8, 6)),
        "closed_k2": (S(conv(), A(2), R(), G()), (8, 6)),
        "closed_k3s2": (S(conv(), A(3, 2), R(), G()), (8, 6)),
        "whole_map": (S(C(3, var_bias=0.1), R(), C(3), A(6), G()), (6, 6)),
        "myrtle": (S(C(3, var_bias=0.1), R(), C(3), R(), A(2), C(3, var_weight=1.5), R(), A(2),
                     G(), C(1, var_weight=2., var_bias=0.3)), (8, 6)),
        "resnet": (S(C(3), A(2), m.resnet_block(),
                     m.resnet_block(stride=2, projection_shortcut=True, multiplier=2), R(), G()),
                   (8, 6)),
        "erf": (S(C(3, var_bias=0.2), E(), A(2), C(3, var_weight=1.5), E(), G()), (8, 6)),
        "mixture": (S(C(3), m.Mixture([S(R(), A(2), C(3), R()), S(A(2), E(), C(3, var_bias=0.2))],
                                      t(0.3, -0.5)), G()), (8, 6)),
        "dense": (S(C(3, var_bias=0.1), R(), A(2), C(3), R(), C(4, padding=0, var_bias=0.2)),
                  (8, 8)),
    }


NET_NAMES = list(pooled_nets())
MODES = ["xx", "xz", "same_diag", "xz_diag"]


def images(h, w):
    rng = np.random.default_rng(10 * h + w)
    draw = lambda n: rng.random((n, 2, h, w), dtype=np.float32).astype(np.float64)   # noqa
    return draw(5), draw(3)


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:3], Z, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def net_reference(name):
    model, hw = pooled_nets()[name]
    X, Z = images(*hw)
    return {mode: AO.kernel(model.double(), *mode_args(X, Z, mode)) for mode in MODES}


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", NET_NAMES)
def test_network_with_avgpool(name, dtn):
    ref = net_reference(name)
    model, hw = pooled_nets()[name]
    model = model.to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(*hw))
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            k = model(*mode_args(X, Z, mode))
            assert tuple(k.shape) == ref[mode].shape and k.dtype == X.dtype
            errs[mode] = max_err(k.cpu(), ref[mode])
            if mode == "xx":
                kxx = k
                assert torch.equal(k, k.T)                       # mirrored, bit for bit
            if mode == "same_diag":
                assert torch.equal(k, torch.diagonal(kxx))       # the pairs (i, i) of xx
        assert torch.equal(model(X, X.clone(), True), kxx)
    print(f"avgpool net {name} {dtn}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs


def pooled_body():
    return S(C(3, var_bias=0.1), R(), A(2), C(3, var_weight=1.5), R())


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_position_covariance_of_a_body_with_avgpool(dtn):
    X, Z = images(8, 6)
    body = pooled_body().to(DEV, TORCH_DT[dtn])
    Xd, Zd = dev(X, TORCH_DT[dtn]), dev(Z, TORCH_DT[dtn])
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            s = body.position_covariance(*mode_args(Xd, Zd, mode))
            ref = AO.position_covariance(pooled_body().double(), *mode_args(X, Z, mode))
            assert tuple(s.shape) == ref.shape and ref.shape[-4:] == (4, 3, 4, 3)
            errs[mode] = max_err(s.cpu(), ref)
            if mode == "xx":
                assert torch.equal(s, s.permute(1, 0, 4, 5, 2, 3))     # S_ji[q, p] = S_ij[p, q]
                sxx = s
            if mode == "same_diag":
                assert torch.equal(s, sxx[torch.arange(5), torch.arange(5)])
    print(f"avgpool body {dtn}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs


# ------------------------------------------------------------------------------------
# c. chunking
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_chunking_changes_no_bit(dtn):
    """one or two pairs per chunk, which chunks the self pass over the 5 (and 3) images too"""
    dt = TORCH_DT[dtn]
    model = pooled_nets()["myrtle"][0].to(DEV, dt)
    body = pooled_body().to(DEV, dt)
    X, Z = (dev(a, dt) for a in images(8, 6))
    with torch.no_grad():
        whole = model(X, Z, False), model(X), body.position_covariance(X, Z, False), \
            body.position_covariance(X)
        for pairs in (1, 2):
            seen = []
            real = N.check

            def check(rc, what):
                seen.append(what)
                return real(rc, what)
            N.check = check
            try:
                per_pair = model._plan(8, 6).pool.peak * X.element_size()
                model.set_pool_workspace(pairs * per_pair + per_pair // 2)
                parts = [model(X, Z, False), model(X)]
                # self passes over x and z, then 15 pairs; a self pass over x, then 15 pairs
                chunks = lambda n: -(-n // pairs)                                # noqa: E731
                assert seen.count("cgp_cov_moments") == chunks(5) + chunks(3) + 2 * chunks(15) \
                    + chunks(5)
                assert seen.count("cgp_cov_pool") == 2 * chunks(15)
                assert seen.count("cgp_covmap_diag") == chunks(5) + chunks(3) + chunks(5)
                per_pair = body._plan(8, 6).body_steps().peak * X.element_size()
                body.set_pool_workspace(pairs * per_pair + per_pair // 2)
                parts += [body.position_covariance(X, Z, False), body.position_covariance(X)]
            finally:
                N.check = real
            for got, want in zip(parts, whole):
                assert torch.equal(got, want), pairs
        model.set_pool_workspace(None)
        assert torch.equal(model(X, Z, False), whole[0])


# ------------------------------------------------------------------------------------
# d. the tie to the existing variance pipeline
# ------------------------------------------------------------------------------------
def test_no_self_pass_without_a_nonlinearity_after_the_pool(monkeypatch):
    """the variance maps such a model reads are run_variances' own"""
    model = S(C(3, var_bias=0.1), R(), C(3), R(), A(2), C(3), G()).to(DEV, torch.float64)
    X, Z = images(8, 6)
    ps = model._plan(8, 6).pool
    assert not ps.self_var and ps.self_last == -1 and ps.need_var

    def refuse(*a, **kw):
        raise AssertionError("the self pass ran")
    monkeypatch.setattr(Plan, "run_self_variances", refuse)
    with torch.no_grad():
        k = model(dev(X), dev(Z), False)
    assert max_err(k.cpu(), AO.kernel(model, X, Z, False)) < NET_TOL["f64"]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_self_pass_diagonal_is_the_variance_pipeline(dtn):
    """upstream of every pool both routes exist: the diagonal the self pass extracts of such
    a value equals run_variances' map of it bit for bit.  6x6 images: no conv here has a
    compile-time instantiation in cgp_conv_*, whose generic kernel sums in the order the
    position-pair conv follows (tests/test_gpu_pool.py)."""
    dt = TORCH_DT[dtn]
    body = S(C(3, var_bias=0.1), R(), C(3, var_weight=1.5), A(2), R()).to(DEV, dt)
    X = dev(images(6, 6)[0], dt)
    n, c, h, w = X.shape
    plan = body._plan(h, w)
    ps = plan.pool
    conv2 = plan.prog.ops[2].dst                       # upstream of the pool, a launch's output
    assert ps.self_var == {plan.prog.ops[3].dst} and conv2 not in ps.avgpooled
    var0 = torch.empty((2 * n, h, w), dtype=dt, device=DEV)
    N.call(f"cgp_moments_var_{dtn}", N.ptr(X), N.ptr(X), n, n, c, h * w, N.ptr(var0[:n]),
           N.ptr(var0[n:]), stream())
    var = plan.run_variances(var0[:n], var0[n:], n, n, True, stream(),
                             need=set(ps.need_var - ps.self_var) | {conv2})
    assert set(var) == set(ps.need_var - ps.self_var) | {conv2}      # nothing past the pool
    side = {v: pair[0] for v, pair in var.items() if v != conv2}
    got = plan.run_self_variances(X, side, stream(), ps, None, want={conv2})
    torch.cuda.synchronize()
    assert set(got) == {conv2} and tuple(got[conv2].shape) == (n, 6, 6)
    assert torch.equal(got[conv2], var[conv2][0])
    # and the pass the model itself makes: the pooled value's variances against the oracle's
    own = plan.run_self_variances(X, side, stream(), ps, 4 * ps.peak * X.element_size())
    sxx = AO.position_covariance(S(*list(body.mods)[:4]), X.cpu().numpy())
    want = np.stack([AO.diag(sxx[i, i][None])[0] for i in range(n)])
    assert max_err(own[plan.prog.ops[3].dst].cpu(), want) < NET_TOL[dtn]


# ------------------------------------------------------------------------------------
# e. Gram builds
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
    model = pooled_nets()["myrtle"][0].to(DEV, torch.float64)
    X = torch.from_numpy(np.random.default_rng(4).random((6, 2, 8, 6), dtype=np.float32)
                         .astype(np.float64))
    with torch.no_grad():
        k = model(X.to(DEV))
    return model, X, k.cpu().numpy()


def test_gram_matrix_with_avgpool(gram_case):
    model, X, k = gram_case
    assert model.image_variances(X.to(DEV)) is None          # declines: the per-tile fallback
    g = gram.gram_matrix(model, X.to(DEV), batch_size=4).cpu().numpy()
    iu = np.triu_indices(6)
    np.testing.assert_array_equal(g[iu], k[iu])


def test_save_K_with_avgpool(gram_case):
    from torch.utils.data import TensorDataset
    model, X, k = gram_case
    ds = TensorDataset(X, torch.zeros(len(X), dtype=torch.int64))
    f = MemH5()
    nngp = gram.model_kern(model)
    save_K(f, lambda x, x2, same, diag: nngp(x, x2, same).cpu().numpy(), "K", ds, None, False,
           4, print_interval=1e9)
    keep = ~np.isnan(f.d["K"][0])
    assert keep[np.triu_indices(6)].all() and not keep.all()     # NaN below the diagonal tiles
    np.testing.assert_array_equal(f.d["K"][0][keep], k.astype(np.float32)[keep])
