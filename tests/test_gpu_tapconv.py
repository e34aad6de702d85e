"""GPU tests of convs whose taps carry individual weights: the entry points
bit for bit against the numpy emulation of their contract and against the reference's
goldens, then forward, ntk, the position-pair paths and the plumbing of a model whose
Conv2d.kernel buffers were edited."""
import os
import re

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import kernels as KM
from cnn_gp import program as P
from cnn_gp.program import Plan

from conftest import GOLDEN
import configs_util
import tapconv_nets as TN
import tapconv_oracle as TO

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
C, R, S = cnn_gp.Conv2d, cnn_gp.ReLU, cnn_gp.Sequential
G = np.load(os.path.join(GOLDEN, "tapconv.npz"))
N_OPS = len([k for k in G.files if re.fullmatch(r"op\d+_par", k)])
MODES = ("Kxx", "Kxz", "Kxdiag", "Kxzdiag")
NP = {"f64": np.float64, "f32": np.float32}
# the project's own tolerances (tests/test_gpu_parity.py)
TOL_EXACT, TOL_CLOSED, TOL_F32 = 1e-10, 1e-8, 2e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))


def run_tapconv(inp, tab, offset, stride=1, dilation=1, bias=0.0, addend=None, max_groups=0):
    """cgp_tapconv_* on numpy maps [m, h, w] in their dtype; the table rounded once to it"""
    sfx = "f64" if inp.dtype == np.float64 else "f32"
    ke = tab.shape[0]
    m, h, w = inp.shape
    ho, wo = (TO.out_size(n, ke, offset, stride, dilation) for n in (h, w))
    x, t = dev(inp), dev(np.asarray(tab, np.float64).astype(inp.dtype))
    out = torch.empty((m, ho, wo), dtype=x.dtype, device=DEV)
    ad = None if addend is None else dev(addend)
    a = N.TapConvArgs()
    a.in_, a.out, a.table, a.addend = N.ptr(x), N.ptr(out), N.ptr(t), N.ptr(ad)
    a.nmaps, a.h, a.w, a.ho, a.wo = m, h, w, ho, wo
    a.extent, a.offset, a.stride, a.dilation = ke, offset, stride, dilation
    a.max_groups, a.bias = max_groups, bias
    N.check(getattr(N.load(), f"cgp_tapconv_{sfx}")(a, stream()), "cgp_tapconv")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_tapconv_cov(s, tab, offset, stride=1, dilation=1, bias=0.0, addend=None):
    """cgp_tapconv_cov_* on position-pair maps in the oracles' layout [m, pr, pc, qr, qc]"""
    from pool_oracle import from_device_layout, to_device_layout
    sfx = "f64" if s.dtype == np.float64 else "f32"
    ke = tab.shape[0]
    m, h, w = s.shape[:3]
    ho, wo = (TO.out_size(n, ke, offset, stride, dilation) for n in (h, w))
    x, t = dev(to_device_layout(s)), dev(np.asarray(tab, np.float64).astype(s.dtype))
    out = torch.empty((m, ho, ho, wo, wo), dtype=x.dtype, device=DEV)
    ad = None if addend is None else dev(to_device_layout(addend))
    a = N.TapConvCovArgs()
    a.in_, a.out, a.table, a.addend = N.ptr(x), N.ptr(out), N.ptr(t), N.ptr(ad)
    a.npairs, a.h, a.w, a.ho, a.wo = m, h, w, ho, wo
    a.extent, a.offset, a.stride, a.dilation, a.bias = ke, offset, stride, dilation, bias
    N.check(getattr(N.load(), f"cgp_tapconv_cov_{sfx}")(a, stream()), "cgp_tapconv_cov")
    torch.cuda.synchronize()
    return from_device_layout(out.cpu().numpy(), ho, wo)


def op_case(n):
    k, s, pad, d, vb = G[f"op{n}_par"]
    k, s, pad, d = int(k), int(s), int(pad), int(d)
    tab = G[f"op{n}_tab"]
    padding = d * (k // 2) if pad < 0 else pad
    return tab, -padding, s, d, float(vb), G[f"op{n}_in"], G[f"op{n}_out"]


def golden_model(name, side, dtype):
    model, which = TN.build(cnn_gp, name, side)
    tables = [G[f"{name}_{side}_tab{i}"] for i in range(len(which))]
    return TN.set_tables(cnn_gp, model.to(dtype), which, tables).to(DEV)


def tapped(k=3, seed=0, **kw):
    """a Conv2d whose buffer holds a random non-negative table"""
    c = C(k, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        c.kernel.copy_(torch.rand(c.kernel.shape, generator=g) * (2.0 / c.kernel[0, 0].numel()))
    return c


def images(n, side, seed, channels=2):
    return np.random.default_rng(seed).random((n, channels, side, side), dtype=np.float32) \
        .astype(np.float64)


# ------------------------------------------------------------------------------------
# 1. the entry points against the emulation of their contract, and against the reference
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_entry_point_on_the_op_cases(sfx):
    """bit for bit against numpy in the contract's order; against the reference within the
    bound of a dot product summed in another order, (ke² + 2)·u·(Σ|W||in| + |b|)"""
    u = 2.0 ** -53 if sfx == "f64" else 2.0 ** -24
    for n in range(N_OPS):
        tab, off, s, d, vb, inp, ref = op_case(n)
        x = inp.astype(NP[sfx])
        got = run_tapconv(x, tab, off, s, d, vb)
        assert np.array_equal(got, TO.tapconv(x, tab, off, s, d, vb)), n
        mag = TO.tapconv(inp.astype(np.float64), np.abs(tab), off, s, d, abs(vb))
        assert np.all(np.abs(got - ref) <= (tab.size + 2) * u * mag), n
        ad = np.random.default_rng(n).random(got.shape).astype(NP[sfx])
        got = run_tapconv(x, tab, off, s, d, vb, addend=ad)
        assert np.array_equal(got, TO.tapconv(x, tab, off, s, d, vb, addend=ad)), n


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("geom", [(3, -1, 1, 1, 7), (4, 0, 2, 1, 8), (7, 0, 1, 1, 7),
                                  (5, -4, 1, 2, 9), (3, -1, 2, 1, 28)],
                         ids=["same3_49outputs", "stride2_3x3outputs_split", "readout_split",
                              "dilated", "stride2_28"])
def test_map_counts_and_the_grid_cap_change_no_bit(sfx, geom):
    """nmaps of 1, of a prime above any chunk (a chunk holds at most 64 maps) and of a count
    that makes each of 3 workgroups walk at least three chunks; capped and uncapped grids
    agree bit for bit with each other and with the emulation"""
    ke, off, s, d, side = geom
    rng = np.random.default_rng(ke * 100 + side)
    tab = rng.random((ke, ke)) - 0.3
    tab[0, 0] = 0.0
    for m in (1, 67, 3 * 3 * 64 + 5):
        x = rng.random((m, side, side)).astype(NP[sfx])
        want = TO.tapconv(x, tab, off, s, d, 0.25)
        free = run_tapconv(x, tab, off, s, d, 0.25)
        capped = run_tapconv(x, tab, off, s, d, 0.25, max_groups=3)
        assert np.array_equal(free, capped) and np.array_equal(free, want), m
        assert np.array_equal(run_tapconv(x, tab, off, s, d, 0.25, max_groups=1), want), m


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("k,kw,side", [(3, {}, 28), (7, {}, 28), (4, {}, 14),
                                       (3, dict(stride=2), 14), (28, dict(padding=0), 28),
                                       (5, dict(dilation=2, padding=1), 14)])
def test_a_constant_table_agrees_with_the_box_kernel(sfx, k, kw, side):
    """within ke²·eps relative: the box kernel multiplies once, after its window sums"""
    conv = C(k, var_weight=1.7, var_bias=0.3, **kw)
    plan = Plan(S(conv), side, side)
    op = plan.prog.ops[0]
    assert op.kind == "conv"
    x = dev(np.random.default_rng(k).random((5, side, side)).astype(NP[sfx]))
    out = torch.empty((5, *op.shape_out), dtype=x.dtype, device=DEV)
    N.check(getattr(N.load(), f"cgp_conv_{sfx}")(Plan._conv_args(op, x, out, 5, 5, 1), stream()),
            "cgp_conv")
    g = P.tap_geometry(conv)
    got = run_tapconv(x.cpu().numpy(), np.array(g.table), g.offset, g.stride, g.dilation, g.bias)
    eps = np.finfo(NP[sfx]).eps
    assert rel(got, out.cpu().numpy()) <= g.extent ** 2 * eps


# ------------------------------------------------------------------------------------
# 2. forward and ntk against the reference's goldens and the oracle
# ------------------------------------------------------------------------------------
def call_mode(f, mode, X, Z):
    return {"Kxx": lambda: f(X), "Kxz": lambda: f(X, Z, False, False),
            "Kxdiag": lambda: f(X, X, True, True),
            "Kxzdiag": lambda: f(X[:3], Z, False, True)}[mode]()


@pytest.mark.parametrize("side", TN.SIDES)
@pytest.mark.parametrize("name", TN.NETS)
def test_forward_against_the_reference(name, side):
    for dtn, tdt, exact, tol in (("f64", torch.float64, True, TOL_EXACT),
                                 ("f64", torch.float64, False, TOL_CLOSED),
                                 ("f32", torch.float32, False, TOL_F32)):
        model = golden_model(name, side, tdt).set_exact_relu(exact)
        assert any(o.kind == "tapconv" for o in model._plan(side, side).prog.ops)
        X, Z = dev(G[f"X_{side}"]).to(tdt), dev(G[f"Z_{side}"]).to(tdt)
        for mode in MODES:
            with torch.no_grad():
                got = call_mode(model, mode, X, Z).cpu().numpy()
            ref = G[f"{name}_{side}_{dtn}_{mode}"]
            assert got.dtype == ref.dtype and got.shape == ref.shape
            assert rel(got, ref) < tol, (dtn, exact, mode, rel(got, ref))


@pytest.mark.parametrize("name", TN.NETS)
def test_ntk_against_the_oracle(name):
    model = golden_model(name, 8, torch.float64).set_exact_relu(True)
    Xn, Zn = G["X_8"].astype(np.float64), G["Z_8"].astype(np.float64)
    X, Z = dev(Xn), dev(Zn)
    for args, nargs in (((X,), (Xn,)), ((X, Z, False, False), (Xn, Zn, False, False)),
                        ((X, X, True, True), (Xn, Xn, True, True)),
                        ((X[:3], Z, False, True), (Xn[:3], Zn, False, True))):
        k, th = model.ntk(*args, return_nngp=True)
        ko, to = TO.ntk(model.cpu(), *nargs)
        model.to(DEV)
        assert rel(k.cpu().numpy(), ko) < 1e-8 and rel(th.cpu().numpy(), to) < 1e-8
        with torch.no_grad():
            assert torch.equal(k, model(*args))


# ------------------------------------------------------------------------------------
# 3. position-pair maps
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("geom", [(3, -1, 1, 1, 6), (5, -2, 2, 1, 8), (3, -2, 1, 2, 7),
                                  (6, 0, 1, 1, 6), (3, -1, 1, 1, 1)],
                         ids=["same3", "stride2", "dilated", "readout", "one_element"])
def test_cov_entry_point_bit_for_bit(sfx, geom):
    ke, off, s, d, side = geom
    rng = np.random.default_rng(ke * 10 + side)
    tab = rng.random((ke, ke)) - 0.3
    tab[-1, 0] = 0.0
    x = rng.random((5, side, side, side, side)).astype(NP[sfx])
    want = TO.tapconv_cov(x, tab, off, s, d, 0.5)
    assert np.array_equal(run_tapconv_cov(x, tab, off, s, d, 0.5), want)
    ad = rng.random(want.shape).astype(NP[sfx])
    assert np.array_equal(run_tapconv_cov(x, tab, off, s, d, 0.0, addend=ad),
                          TO.tapconv_cov(x, tab, off, s, d, 0.0, addend=ad))
    # the P = Q, U = V entries are the layer entry point on the maps' diagonals, bit for bit
    diag = np.ascontiguousarray(np.einsum("mabab->mab", x))
    assert np.array_equal(np.einsum("mabab->mab", want), run_tapconv(diag, tab, off, s, d, 0.5))


def tapped_body():
    return S(tapped(3, 1, var_bias=0.1), R(), tapped(4, 2, var_bias=0.2), R(),
             tapped(3, 3, stride=2, var_bias=0.1))


def test_position_covariance_of_a_tapped_body():
    body = tapped_body().double().to(DEV).set_exact_relu(True)
    Xn, Zn = images(3, 8, 1), images(2, 8, 2)
    X, Z = dev(Xn), dev(Zn)
    s = body.position_covariance(X, Z, False, False)
    assert rel(s.cpu().numpy(), TO.position_covariance(body.cpu(), Xn, Zn, False, False)) < 1e-8
    body.to(DEV)
    # chunked pair lists: one pair at a time gives the same bits
    ps = body._plan(8, 8).body_steps()
    body.set_pool_workspace(ps.peak * 8)
    assert torch.equal(body.position_covariance(X, Z, False, False), s)
    body.set_pool_workspace(None)
    # through a dense readout the [i, j, p, p] entries give forward
    readout = tapped(4, 4, padding=0, var_bias=0.3).double()
    full = S(*body.mods, readout).to(DEV).set_exact_relu(True)
    with torch.no_grad():
        k = full(X, Z, False, False).cpu().numpy()
    maps = np.einsum("ijabab->ijab", s.cpu().numpy()).reshape(6, 4, 4)
    via = TO.conv_var(maps, readout.cpu()).reshape(3, 2)
    assert rel(via, k) < 1e-10
    # on a same tile the i = j, p = q entries are run_variances' maps, bit for bit
    sx = body.position_covariance(X)
    plan = body._plan(8, 8)
    with torch.cuda.device(DEV):
        var = KM._variances(plan, X, X, True, stream(), {plan.vf})
    torch.cuda.synchronize()
    sx = sx.cpu().numpy()[np.arange(3), np.arange(3)]
    assert np.array_equal(np.einsum("iabab->iab", sx), var[plan.vf][0].cpu().numpy())


def pooled_model():
    return S(tapped(3, 5, var_bias=0.1), R(), cnn_gp.AvgPool2d(2), tapped(3, 6, var_bias=0.1),
             R(), cnn_gp.GlobalAvgPool(), C(1, var_bias=0.05))


def corr_model():
    return S(tapped(3, 7, var_bias=0.1), R(),
             cnn_gp.CorrelatedConv2d(3, var_bias=0.1, lengthscale=1.0), R(),
             tapped(8, 8, padding=0, var_bias=0.1))


@pytest.mark.parametrize("build", [pooled_model, corr_model], ids=["pooled", "corrconv"])
def test_pooled_and_correlated_models_against_the_oracle(build):
    model = build().double().to(DEV).set_exact_relu(True)
    Xn, Zn = images(3, 8, 3), images(2, 8, 4)
    X, Z = dev(Xn), dev(Zn)
    for args, nargs in (((X, Z, False, False), (Xn, Zn, False, False)), ((X,), (Xn,)),
                        ((X[:2], Z, False, True), (Xn[:2], Zn, False, True))):
        with torch.no_grad():
            k = model(*args)
        km, tm = model.ntk_maps(*args, return_nngp=True)
        ko, to = TO.ntk_maps(model.cpu(), *nargs)
        model.to(DEV)
        assert torch.equal(k, km)
        assert rel(k.cpu().numpy(), ko) < 1e-8 and rel(tm.cpu().numpy(), to) < 1e-8
    body = S(*model.mods[:4]).to(DEV).set_exact_relu(True)
    s, th = body.position_ntk(X, Z, False, False, return_nngp=True)
    so, tho = TO.position_ntk(body.cpu(), Xn, Zn, False, False)
    assert rel(s.cpu().numpy(), so) < 1e-8 and rel(th.cpu().numpy(), tho) < 1e-8


# ------------------------------------------------------------------------------------
# 4. plumbing
# ------------------------------------------------------------------------------------
def test_an_in_place_edit_changes_the_next_forward():
    model = S(C(3, var_bias=0.1), R(), C(8, padding=0)).double().to(DEV).set_exact_relu(True)
    Xn = images(4, 8, 5)
    X = dev(Xn)
    with torch.no_grad():
        k0 = model(X).cpu().numpy()
        model.mods[0].kernel[0, 0, 1, 1] *= 4.0
        k1 = model(X).cpu().numpy()
    assert model._plan(8, 8).prog.ops[0].kind == "tapconv"
    assert rel(k1, TO.kernel(model.cpu(), Xn)) < 1e-10
    assert np.min(np.abs(k1 - k0) / np.abs(k0)) > 1e-3


def test_gram_matrix_equals_tile_by_tile_forward():
    from cnn_gp.gram import gram_matrix
    model = S(tapped(3, 9, var_bias=0.1), R(), tapped(3, 10), R(),
              C(8, padding=0)).double().to(DEV)
    X, Z = dev(images(7, 8, 6)), dev(images(5, 8, 7))
    assert model.image_variances(X) is None            # the per-tile forward fallback
    kxx = gram_matrix(model, X, batch_size=3)
    kxz = gram_matrix(model, X, Z, batch_size=3)
    with torch.no_grad():
        for i0 in range(0, 7, 3):
            for j0 in range(0, 5, 3):
                assert torch.equal(kxz[i0:i0 + 3, j0:j0 + 3],
                                   model(X[i0:i0 + 3], Z[j0:j0 + 3], False, False))
            assert torch.equal(kxx[i0:i0 + 3, i0:i0 + 3], model(X[i0:i0 + 3]))
            for j0 in range(i0 + 3, 7, 3):
                assert torch.equal(kxx[i0:i0 + 3, j0:j0 + 3],
                                   model(X[i0:i0 + 3], X[j0:j0 + 3], False, False))


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


# the call lists tests/test_gpu_erf.py recorded for this model before any of the additions
_VR = "cgp_var_relu_f64"
BOX_CALLS = {
    "net": ["cgp_var_chain", "cgp_rsqrt_batch_f64", "cgp_net"],
    "layer": ["cgp_moments_var"] + ["cgp_conv", _VR] * 7 + ["cgp_conv"] * 9,
}


@pytest.mark.parametrize("path", ["net", "layer"])
def test_a_box_model_makes_the_same_calls(path, monkeypatch):
    model = configs_util.model("mnist_paper_convnet_gp").double().to(DEV)
    model.set_fused_network(path == "net")
    x = dev(np.random.default_rng(0).random((4, 1, 28, 28)))
    seen = recorded_calls(model, x, monkeypatch)
    assert seen == BOX_CALLS[path] and not any("tapconv" in s for s in seen)
    # the same model with one table tapered: its convs run as cgp_tapconv / cgp_conv launches
    with torch.no_grad():
        model.mods[0].kernel.mul_(cnn_gp.gaussian_taps(7, 2.0).to(DEV).reshape(1, 1, 7, 7))
    seen = recorded_calls(model, x, monkeypatch)
    assert seen.count("cgp_tapconv") == 2 and "cgp_net" not in seen
