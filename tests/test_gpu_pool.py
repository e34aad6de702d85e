"""GPU tests of global average pooling: each cgp_cov_* entry point alone, networks with
cnn_gp.GlobalAvgPool through forward and position_covariance against the test-time oracle
(tests/pool_oracle.py), the tie of the position-pair path to the golden-pinned layer path,
chunking, and the Gram builds on a pooled model.

Tolerances are the project's own (tests/test_gpu_erf.py): the op alone in float64 1e-12,
float64 end to end 1e-10, float32 against the float64 oracle on float32-representable inputs
2e-5; errors are max|got - ref| / max|ref|, because erf makes entries cross zero."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp import program as P
from cnn_gp.kernel_save_tools import save_K

import pool_oracle as PO

pytestmark = pytest.mark.gpu

DEV = "cuda"
OP_TOL = {"f64": 1e-12, "f32": 2e-5}
NET_TOL = {"f64": 1e-10, "f32": 2e-5}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}

m = cnn_gp
C, R, E, S, G = m.Conv2d, m.ReLU, m.Erf, m.Sequential, m.GlobalAvgPool


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


# ------------------------------------------------------------------------------------
# a. each entry point alone
# ------------------------------------------------------------------------------------
def pair_case(kind):
    """kind -> (n1, n2, pair_i, pair_j, same): every pair of a 3 x 2 tile, the upper
    triangle of a same tile of 3, the diagonal pairs of 3 + 3 images, or one pair"""
    if kind == "all":
        i, j = PO.pair_lists(3, 2, False, False)
        return 3, 2, i, j, False
    if kind == "triu":
        i, j = np.triu_indices(3)
        return 3, 3, i, j, True
    if kind == "diag":
        return 3, 3, np.arange(3), np.arange(3), False
    return 1, 1, np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), False


@functools.lru_cache(maxsize=None)
def op_inputs(h, w, kind, dtn):
    """images (float32-representable), their position-pair moments and variance maps rounded
    to the compute type; the oracle starts from the rounded arrays.

    Four channels, not fewer: the oracle's ReLU is the reference's formula, whose acos and
    sqrt(t - c²) each lose eps/sin(theta) near |rho| = 1 (csrc/cgp_common.h), and pixels p of
    x and q of y correlate through their channel vectors alone.  With C channels in [0, 1)
    the smallest of n angles is about n^(-1/(C-1)): 614 656 pixel pairs of one 28x28 pair
    come within 5e-6 of parallel at C = 2 (the oracle is then good to 3e-12 only, measured)
    and within 0.01 at C = 4 (1e-14), which keeps the oracle an order inside the bounds."""
    n1, n2, pi, pj, same = pair_case(kind)
    rng = np.random.default_rng(100 * h + w + len(kind))
    x = rng.random((n1, 4, h, w), dtype=np.float32).astype(np.float64)
    y = x if same else rng.random((n2, 4, h, w), dtype=np.float32).astype(np.float64)
    rnd = lambda a: a.astype(NP_DT[dtn]).astype(np.float64)                      # noqa: E731
    s0 = rnd(PO.moments(x, y, pi, pj))
    return x, y, pi, pj, same, s0, rnd(PO.variances(x)), rnd(PO.variances(y))


def idx32(a):
    return torch.as_tensor(np.asarray(a)).to(DEV, torch.int32)


def run_moments(x, y, pi, pj, dtn):
    dt = TORCH_DT[dtn]
    xd, yd, di, dj = dev(x, dt), dev(y, dt), idx32(pi), idx32(pj)
    h, w = x.shape[2:]
    out = torch.empty((len(pi), (h * w) ** 2), dtype=dt, device=DEV)
    N.call(f"cgp_cov_moments_{dtn}", N.ptr(xd), N.ptr(yd), N.ptr(di), N.ptr(dj), len(pi),
           x.shape[1], h, w, N.ptr(out), stream())
    torch.cuda.synchronize()
    return PO.from_device_layout(out.cpu().numpy(), h, w)


def run_conv(s, mod, pi, pj, dtn, post=N.CGP_COV_NONE, xx=None, yy=None, addend=None, same=False,
             flags=0, rc=0, onto_addend=False):
    """cgp_cov_conv_*; ``onto_addend`` writes the result over the addend (out == addend)"""
    dt = TORCH_DT[dtn]
    h, w = s.shape[1:3]
    ho, wo = P.conv_out_hw(mod, h, w)
    g = P.conv_geometry(mod)
    sd, di, dj = dev(PO.to_device_layout(s), dt), idx32(pi), idx32(pj)
    ad = None if addend is None else dev(PO.to_device_layout(addend), dt)
    vx = None if xx is None else dev(xx, dt)
    vy = None if yy is None else dev(yy, dt)
    out = ad if onto_addend else torch.empty((len(pi), (ho * wo) ** 2), dtype=dt, device=DEV)
    a = N.CovConvArgs()
    a.in_, a.out, a.addend, a.xx, a.yy = N.ptr(sd), N.ptr(out), N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.pair_i, a.pair_j, a.npairs = N.ptr(di), N.ptr(dj), len(pi)
    a.h, a.w, a.ho, a.wo = h, w, ho, wo
    a.taps, a.offset, a.stride, a.dilation = g.taps, g.offset, g.stride, g.dilation
    a.post, a.same, a.flags, a.weight, a.bias = post, int(same), flags, g.weight, g.bias
    got = getattr(N.load(), f"cgp_cov_conv_{dtn}")(ctypes.byref(a), stream())
    assert got == rc, N.load().cgp_last_error()
    torch.cuda.synchronize()
    return PO.from_device_layout(out.cpu().numpy(), ho, wo)


def run_nonlin(s, kind, xx, yy, pi, pj, dtn, addend=None, same=False, flags=0, inplace=False):
    dt = TORCH_DT[dtn]
    h, w = s.shape[1:3]
    sd, di, dj = dev(PO.to_device_layout(s), dt), idx32(pi), idx32(pj)
    ad = None if addend is None else dev(PO.to_device_layout(addend), dt)
    vx, vy = dev(xx, dt), dev(yy, dt)
    out = sd if inplace else torch.empty_like(sd)
    a = N.CovNonlinArgs()
    a.in_, a.out, a.addend, a.xx, a.yy = N.ptr(sd), N.ptr(out), N.ptr(ad), N.ptr(vx), N.ptr(vy)
    a.pair_i, a.pair_j, a.npairs = N.ptr(di), N.ptr(dj), len(pi)
    a.h, a.w, a.kind, a.same, a.flags = h, w, kind, int(same), flags
    N.check(getattr(N.load(), f"cgp_cov_nonlin_{dtn}")(ctypes.byref(a), stream()),
            "cgp_cov_nonlin")
    torch.cuda.synchronize()
    return PO.from_device_layout(out.cpu().numpy(), h, w)


def run_pool(flat, dtn):
    sd = dev(flat, TORCH_DT[dtn])
    out = torch.empty(flat.shape[0], dtype=sd.dtype, device=DEV)
    N.call(f"cgp_cov_pool_{dtn}", N.ptr(sd), flat.shape[0], flat.shape[1], N.ptr(out), stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# H != W catches transposed indices; 28x28 is 2048-element chunks that straddle nothing,
# 33x31 a w x w block of 961 > 256 elements (the conv loops) and (h w)² odd
SHAPES = [(5, 4, "all"), (5, 4, "triu"), (5, 4, "diag"), (7, 7, "all"), (7, 7, "triu"),
          (7, 7, "diag"), (28, 28, "one"), (33, 31, "one")]
ids = lambda c: "-".join(map(str, c))                                            # noqa: E731


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_cov_moments(case, dtn):
    h, w, kind = case
    x, y, pi, pj, same, _, vx, _ = op_inputs(h, w, kind, dtn)
    got = run_moments(x, y, pi, pj, dtn)
    err = max_err(got, PO.moments(x, y, pi, pj))
    print(f"cov_moments {dtn} {case}: {err:.2e}")
    assert err < OP_TOL[dtn]
    if same:
        # the p = q entries of a self pair are the per-image variances, bit for bit
        # (cgp_moments_var_*'s, the maps the layer path starts from)
        xd = dev(x, TORCH_DT[dtn])
        var = torch.empty((2 * len(x), h, w), dtype=xd.dtype, device=DEV)
        N.call(f"cgp_moments_var_{dtn}", N.ptr(xd), N.ptr(xd), len(x), len(x), x.shape[1], h * w,
               N.ptr(var[:len(x)]), N.ptr(var[len(x):]), stream())
        diag = np.einsum("mabab->mab", got)[pi == pj]
        np.testing.assert_array_equal(diag, var[:len(x)].cpu().numpy())


def nonlin_ref(kind, s, xx, yy, pi, pj, same):
    return (PO.relu_map if kind == N.CGP_COV_RELU else PO.erf_map)(s, xx, yy, pi, pj, same)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_cov_nonlin(case, dtn):
    h, w, kind = case
    x, y, pi, pj, same, s0, vx, vy = op_inputs(h, w, kind, dtn)
    rng = np.random.default_rng(7)
    addend = rng.standard_normal(s0.shape).astype(NP_DT[dtn]).astype(np.float64)
    for nl in (N.CGP_COV_RELU, N.CGP_COV_ERF):
        ref = nonlin_ref(nl, s0, vx, vy, pi, pj, same)
        got = run_nonlin(s0, nl, vx, vy, pi, pj, dtn, same=same)
        err = max_err(got, ref)
        print(f"cov_nonlin {dtn} {case} kind {nl}: {err:.2e}")
        assert err < OP_TOL[dtn]
        np.testing.assert_array_equal(
            run_nonlin(s0, nl, vx, vy, pi, pj, dtn, same=same, inplace=True), got)
        gadd = run_nonlin(s0, nl, vx, vy, pi, pj, dtn, same=same, addend=addend)
        np.testing.assert_array_equal(gadd, (got.astype(NP_DT[dtn])
                                             + addend.astype(NP_DT[dtn])).astype(np.float64))
        if nl == N.CGP_COV_RELU:
            exact = run_nonlin(s0, nl, vx, vy, pi, pj, dtn, same=same,
                               flags=N.CGP_FLAG_EXACT_RELU)
            assert max_err(exact, ref) < OP_TOL[dtn]
            assert max_err(exact, got) < 2 * OP_TOL[dtn]     # both are within OP_TOL of ref
            if kind != "one":
                assert not np.array_equal(exact, got)        # the flag selects another form
        if same:
            self_pq = np.einsum("mabab->mab", got)[pi == pj]
            want = vx / 2 if nl == N.CGP_COV_RELU else PO.erf_var(vx)
            assert max_err(self_pq, want) < OP_TOL[dtn]
            # p != q of a self pair takes the ordinary map, which differs from the override
            off = got[pi == pj][:, 0, 0, 0, 1]
            assert np.all(np.abs(off - self_pq[:, 0, 0]) > 1e-4)


GEOMETRIES = {
    "same3": (5, 4, lambda: C(3, var_weight=1.3, var_bias=0.2)),
    "stride2": (7, 7, lambda: C(3, stride=2, var_bias=0.1)),
    "even": (5, 4, lambda: C(2, var_bias=0.1)),
    "dilation2": (7, 7, lambda: C(3, dilation=2, var_weight=0.7)),
    "valid_to_1x1": (7, 7, lambda: C(7, padding=0, var_bias=0.3)),
    "valid4": (5, 4, lambda: C(4, padding=0)),               # 2x1 output
    "28x28": (28, 28, lambda: C(3, var_bias=0.1)),
    "33x31": (33, 31, lambda: C(3, var_bias=0.1)),
}


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_cov_conv(name, dtn):
    """the stencil alone, with each post-nonlinearity and with an addend, on every pair list"""
    h, w, make = GEOMETRIES[name]
    mod = make()
    worst = 0.0
    for kind in (("one",) if h > 7 else ("all", "triu", "diag")):
        x, y, pi, pj, same, s0, vx, vy = op_inputs(h, w, kind, dtn)
        lin = PO.conv_map(s0, mod)
        rnd = lambda a: a.astype(NP_DT[dtn]).astype(np.float64)                  # noqa: E731
        ox, oy = rnd(PO.conv_var(vx, mod)), rnd(PO.conv_var(vy, mod))
        addend = rnd(np.random.default_rng(3).standard_normal(lin.shape))
        for post in (N.CGP_COV_NONE, N.CGP_COV_RELU, N.CGP_COV_ERF):
            ref = lin if post == N.CGP_COV_NONE else nonlin_ref(post, lin, ox, oy, pi, pj, same)
            kw = {} if post == N.CGP_COV_NONE else dict(xx=ox, yy=oy)
            got = run_conv(s0, mod, pi, pj, dtn, post=post, same=same, **kw)
            assert got.shape == ref.shape
            worst = max(worst, max_err(got, ref))
            gadd = run_conv(s0, mod, pi, pj, dtn, post=post, same=same, addend=addend, **kw)
            np.testing.assert_array_equal(gadd, (got.astype(NP_DT[dtn])
                                                 + addend.astype(NP_DT[dtn])).astype(np.float64))
            np.testing.assert_array_equal(
                run_conv(s0, mod, pi, pj, dtn, post=post, same=same, addend=addend,
                         onto_addend=True, **kw), gadd)
            if post == N.CGP_COV_RELU:
                exact = run_conv(s0, mod, pi, pj, dtn, post=post, same=same,
                                 flags=N.CGP_FLAG_EXACT_RELU, **kw)
                worst = max(worst, max_err(exact, ref))
    print(f"cov_conv {dtn} {name}: {worst:.2e}")
    assert worst < OP_TOL[dtn]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_cov_pool(dtn):
    rng = np.random.default_rng(2)
    for pairs, n in ((5, 1), (3, 400), (2, 1023 * 1023), (7, 2049)):
        flat = rng.standard_normal((pairs, n)).astype(NP_DT[dtn])
        got = run_pool(flat, dtn)
        ref = flat.astype(np.float64).mean(axis=1)
        # double accumulation: float32 results are the correctly rounded means, up to the
        # reorder of a double sum
        tol = 1e-12 if dtn == "f64" else 1e-7
        assert np.max(np.abs(got - ref)) < tol * max(1.0, np.max(np.abs(ref))) + tol
        np.testing.assert_array_equal(run_pool(flat, dtn), got)          # run to run
        np.testing.assert_array_equal(run_pool(flat[1:], dtn), got[1:])  # pair by pair


def test_cov_argument_errors_with_device_pointers():
    x, y, pi, pj, same, s0, vx, vy = op_inputs(5, 4, "all", "f64")
    lib = N.load()
    sd = dev(PO.to_device_layout(s0))
    a = N.CovConvArgs()
    a.in_ = a.out = N.ptr(sd)
    a.npairs, a.h, a.w, a.ho, a.wo = len(pi), 5, 4, 5, 4
    a.taps, a.offset, a.stride, a.dilation, a.weight = 3, -1, 1, 1, 1.0
    assert lib.cgp_cov_conv_f64(ctypes.byref(a), stream()) == 1001
    assert b"must not be in" in lib.cgp_last_error()
    b = N.CovNonlinArgs()
    b.in_ = b.out = N.ptr(sd)
    b.npairs, b.h, b.w, b.kind = len(pi), 5, 4, N.CGP_COV_RELU
    assert lib.cgp_cov_nonlin_f64(ctypes.byref(b), stream()) == 1001     # no variances
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sd.cpu().numpy(), PO.to_device_layout(s0))


# ------------------------------------------------------------------------------------
# b. networks through forward
# ------------------------------------------------------------------------------------
def bodies():
    t = lambda *v: torch.tensor(v, dtype=torch.float32)                          # noqa: E731
    return {
        "chain": [C(3, var_bias=0.1), R(), C(3, var_weight=1.5), R(), C(3, var_bias=0.2), R()],
        "resnet": [C(3), m.resnet_block(),
                   m.resnet_block(stride=2, projection_shortcut=True, multiplier=2), R()],
        "mixture": [C(3), m.Mixture([S(R(), C(3)), S(E(), C(3, var_bias=0.2)), S()],
                                    t(0.3, -0.5, 0.1)), R()],
        "erf": [C(3, var_bias=0.2), E(), C(3, var_weight=1.5), E()],
    }


def pooled_nets():
    nets = {k: S(*v, G()) for k, v in bodies().items()}
    nets["readout"] = S(C(3), R(), C(3), G(), C(1, var_weight=2., var_bias=.3))
    return nets


NET_NAMES = list(pooled_nets())
MODES = ["xx", "xz", "same_diag", "xz_diag"]


def images(h, w):
    rng = np.random.default_rng(10 * h + w)
    draw = lambda n: rng.random((n, 2, h, w), dtype=np.float32).astype(np.float64)   # noqa
    return draw(4), draw(3)


def mode_args(X, Z, mode):
    return {"xx": (X,), "xz": (X, Z, False, False), "same_diag": (X, X, True, True),
            "xz_diag": (X[:3], Z, False, True)}[mode]


@functools.lru_cache(maxsize=None)
def net_reference(name):
    model = pooled_nets()[name].double()
    X, Z = images(6, 5)
    return {mode: PO.kernel(model, *mode_args(X, Z, mode)) for mode in MODES}


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", NET_NAMES)
def test_pooled_network(name, dtn):
    ref = net_reference(name)
    model = pooled_nets()[name].to(DEV, TORCH_DT[dtn])
    X, Z = (dev(a, TORCH_DT[dtn]) for a in images(6, 5))
    errs = {}
    with torch.no_grad():
        for mode in MODES:
            k = model(*mode_args(X, Z, mode))
            assert tuple(k.shape) == ref[mode].shape and k.dtype == X.dtype
            assert k.device == X.device
            errs[mode] = max_err(k.cpu(), ref[mode])
            if mode == "xx":
                kxx = k
                assert torch.equal(k, k.T)                       # mirrored, bit for bit
            if mode == "same_diag":
                assert torch.equal(k, torch.diagonal(kxx))       # the pairs (i, i) of xx
        # y given explicitly with same=True is the same tile; CPU inputs come back on the CPU
        assert torch.equal(model(X, X.clone(), True), kxx)
        kc = model(X.cpu(), Z.cpu(), False)
        assert kc.device.type == "cpu" and torch.equal(kc, model(X, Z, False).cpu())
        if name == "chain":
            ke = model.set_exact_relu(True)(X, Z, False)
            assert max_err(ke.cpu(), ref["xz"]) < NET_TOL[dtn]
            assert not torch.equal(ke, model.set_exact_relu(False)(X, Z, False))
    print(f"pooled net {name} {dtn}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < NET_TOL[dtn], errs


# ------------------------------------------------------------------------------------
# c. the tie to the existing path
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bodies()))
def test_position_covariance_ties_to_the_layer_path(name):
    """position_covariance against the oracle; its [.., p, p] entries through a dense
    readout against the existing forward of body + Conv2d(H, padding=0); and, on a same
    tile, its i = j, p = q entries against the layer path's variance maps bit for bit.
    6x6 images: no conv here has a compile-time instantiation in cgp_conv_*, whose generic
    kernel sums in the order the position-pair conv follows."""
    X, Z = images(6, 6)
    body = S(*bodies()[name]).to(DEV, torch.float64)
    Xd, Zd = dev(X), dev(Z)
    with torch.no_grad():
        for mode in MODES:
            args = mode_args(Xd, Zd, mode)
            s = body.position_covariance(*args)
            ref = PO.position_covariance(body, *mode_args(X, Z, mode))
            assert tuple(s.shape) == ref.shape
            assert max_err(s.cpu(), ref) < NET_TOL["f64"], mode
            ho = s.shape[-1]
            dense = C(ho, padding=0, var_weight=1.7, var_bias=0.2).to(DEV, torch.float64)
            g = P.conv_geometry(dense)
            want = g.weight * torch.einsum("...abab->...", s) + g.bias
            full = S(body, dense)
            for fused in (True, False):
                k = full.set_fused_network(fused)(*args)
                assert max_err(k.cpu(), want.cpu().numpy()) < NET_TOL["f64"], (mode, fused)
            if mode == "xx":
                assert torch.equal(s, s.permute(1, 0, 4, 5, 2, 3))     # S_ji[q, p] = S_ij[p, q]
                sxx = s
            if mode == "same_diag":
                assert torch.equal(s, sxx[torch.arange(4), torch.arange(4)])
        # the layer path's variance maps of the body's output
        n, c, h, w = Xd.shape
        plan = body._plan(h, w)
        var0 = torch.empty((2 * n, h, w), dtype=Xd.dtype, device=DEV)
        N.call("cgp_moments_var_f64", N.ptr(Xd), N.ptr(Xd), n, n, c, h * w, N.ptr(var0[:n]),
               N.ptr(var0[n:]), stream())
        var = plan.run_variances(var0[:n], var0[n:], n, n, True, stream(), need={plan.vf})
        diag = torch.einsum("iiabab->iab", sxx)
        assert torch.equal(diag, var[plan.vf][0])


def test_1x1_input_pooled_equals_unpooled():
    """on 1x1 images a position-pair map is the pair map and the pool is the identity"""
    layers = lambda: [C(1, var_bias=0.1), R(), C(1, var_weight=1.5), R(), C(1)]   # noqa: E731
    rng = np.random.default_rng(3)
    X, Z = dev(rng.random((5, 3, 1, 1))), dev(rng.random((4, 3, 1, 1)))
    plain = S(*layers()).to(DEV, torch.float64).set_fused_network(False)
    with torch.no_grad():
        for pooled in (S(*layers(), G()), S(*layers()[:4], G(), C(1))):
            pooled = pooled.to(DEV, torch.float64)
            for args in ((X,), (X, Z, False, False), (X, X, True, True), (X[:4], Z, False, True)):
                assert max_err(pooled(*args).cpu(), plain(*args).cpu().numpy()) < NET_TOL["f64"]


# ------------------------------------------------------------------------------------
# d. chunking
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_chunking_changes_no_bit(dtn):
    dt = TORCH_DT[dtn]
    model = pooled_nets()["resnet"].to(DEV, dt)
    rng = np.random.default_rng(5)
    X, Z = dev(rng.random((5, 2, 6, 5)), dt), dev(rng.random((3, 2, 6, 5)), dt)
    per_pair = model._plan(6, 5).pool.peak * X.element_size()
    with torch.no_grad():
        whole = model(X, Z, False), model(X)
        # 15 pairs each (5 x 3, and the upper triangle of 5 x 5) in chunks of 4: 4, 4, 4, 3
        model.set_pool_workspace(4 * per_pair + per_pair // 2)
        seen = []
        real = N.check

        def check(rc, what):
            seen.append(what)
            return real(rc, what)
        N.check = check
        try:
            parts = model(X, Z, False), model(X)
        finally:
            N.check = real
        assert seen.count("cgp_cov_pool") == 8 and seen.count("cgp_cov_moments") == 8
        assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1])
        model.set_pool_workspace(per_pair)                       # one pair per chunk
        assert torch.equal(model(X, Z, False), whole[0])
        model.set_pool_workspace(per_pair - 1)
        with pytest.raises(RuntimeError, match=f"{per_pair} bytes.*workspace of {per_pair - 1}"):
            model(X, Z, False)
        model.set_pool_workspace(None)
        assert torch.equal(model(X, Z, False), whole[0])


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
    model = pooled_nets()["chain"].to(DEV, torch.float64)
    X = torch.from_numpy(np.random.default_rng(4).random((5, 2, 6, 5), dtype=np.float32)
                         .astype(np.float64))
    with torch.no_grad():
        k = model(X.to(DEV))
    return model, X, k.cpu().numpy()


def test_pooled_gram_matrix(gram_case):
    model, X, k = gram_case
    assert model.image_variances(X.to(DEV)) is None          # declines: the per-tile fallback
    g = gram.gram_matrix(model, X.to(DEV), batch_size=2).cpu().numpy()
    iu = np.triu_indices(5)
    np.testing.assert_array_equal(g[iu], k[iu])


def test_pooled_save_K(gram_case):
    from torch.utils.data import TensorDataset
    model, X, k = gram_case
    ds = TensorDataset(X, torch.zeros(len(X), dtype=torch.int64))
    f = MemH5()
    nngp = gram.model_kern(model)
    save_K(f, lambda x, x2, same, diag: nngp(x, x2, same).cpu().numpy(), "K", ds, None, False,
           2, print_interval=1e9)
    keep = ~np.isnan(f.d["K"][0])
    assert keep[np.triu_indices(5)].all() and not keep.all()     # NaN below the diagonal tiles
    np.testing.assert_array_equal(f.d["K"][0][keep], k.astype(np.float32)[keep])
