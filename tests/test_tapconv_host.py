"""CPU tests of convs whose taps carry individual weights: the test-side
oracle against the reference's goldens and against itself, the public surface, the lowering
of an edited kernel buffer and the ABI of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import program as P
from cnn_gp.program import Plan

from conftest import GOLDEN, ROOT
import tapconv_nets as TN
import tapconv_oracle as TO

C, R, S = cnn_gp.Conv2d, cnn_gp.ReLU, cnn_gp.Sequential
G = np.load(os.path.join(GOLDEN, "tapconv.npz"))
N_OPS = len([k for k in G.files if re.fullmatch(r"op\d+_par", k)])
MODES = ("Kxx", "Kxz", "Kxdiag", "Kxzdiag")


def golden_model(name, side, dtype=torch.float64):
    model, which = TN.build(cnn_gp, name, side)
    tables = [G[f"{name}_{side}_tab{i}"] for i in range(len(which))]
    return TN.set_tables(cnn_gp, model.to(dtype), which, tables)


def call_mode(f, mode, X, Z):
    return {"Kxx": lambda: f(X), "Kxz": lambda: f(X, Z, False, False),
            "Kxdiag": lambda: f(X, X, True, True),
            "Kxzdiag": lambda: f(X[:3], Z, False, True)}[mode]()


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - b) / np.abs(b)))


def tapped(k=3, seed=0, **kw):
    """a Conv2d whose buffer holds a random non-negative table"""
    c = C(k, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        c.kernel.copy_(torch.rand(c.kernel.shape, generator=g) * 0.3)
    return c


# ------------------------------------------------------------------------------------
# 1. the oracle
# ------------------------------------------------------------------------------------
def test_the_goldens_cover_the_stated_geometries():
    assert N_OPS >= 40
    pars = np.array([G[f"op{n}_par"][:4] for n in range(N_OPS)])
    assert set(pars[:, 0]) >= {1, 2, 3, 4, 5, 7, 28} and set(pars[:, 1]) == {1, 2}
    assert set(pars[:, 2]) == {-1, 0, 1} and set(pars[:, 3]) == {1, 2}
    assert {G[f"op{n}_in"].shape[-1] for n in range(N_OPS)} >= {7, 8, 14, 28}
    tabs = [G[f"op{n}_tab"] for n in range(N_OPS)]
    assert any((t < 0).any() for t in tabs) and any((t == 0).any() for t in tabs)
    # an even "same" buffer whose first row and column were written
    assert any(t.shape[0] == G[f"op{n}_par"][0] + 1 and (t[0] != 0).any() and (t[:, 0] != 0).any()
               for n, t in enumerate(tabs))
    for name in TN.NETS:
        for side in TN.SIDES:
            for dt in ("f64", "f32"):
                assert all((G[f"{name}_{side}_{dt}_{m}"] > 0).all() for m in MODES)


@pytest.mark.parametrize("n", range(N_OPS))
def test_oracle_reproduces_the_op_goldens(n):
    k, s, pad, d, vb = G[f"op{n}_par"]
    k, s, pad, d = int(k), int(s), int(pad), int(d)
    mod = C(k, stride=s, padding="same" if pad < 0 else pad, dilation=d, var_bias=vb).double()
    tab = G[f"op{n}_tab"]
    with torch.no_grad():
        mod.kernel.copy_(torch.from_numpy(tab).double().reshape(mod.kernel.shape))
    got = TO.conv_var(G[f"op{n}_in"].astype(np.float64), mod)
    ref = G[f"op{n}_out"]
    # the bound of a dot product summed in another order: (ke² + 2)·eps·(Σ|W||in| + |b|)
    mag = TO.tapconv(G[f"op{n}_in"].astype(np.float64), np.abs(tab), -int(mod.padding), s, d,
                     abs(vb))
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 1e-13 * mag)
    assert np.all(np.abs(got - ref) <= (tab.size + 2) * 2.0 ** -53 * mag)


@pytest.mark.parametrize("side", TN.SIDES)
@pytest.mark.parametrize("name", TN.NETS)
def test_oracle_reproduces_the_end_to_end_goldens(name, side):
    model = golden_model(name, side)
    X, Z = G[f"X_{side}"], G[f"Z_{side}"]
    for mode in MODES:
        got = call_mode(lambda *a: TO.kernel(model, *a), mode, X, Z)
        assert rel(got, G[f"{name}_{side}_f64_{mode}"]) < 1e-13, mode


@pytest.mark.parametrize("name", TN.NETS)
def test_oracle_stepwise_ntk_agrees_with_autograd(name):
    model = golden_model(name, 8)
    X, Z = G["X_8"], G["Z_8"]
    for args in ((X,), (X, Z, False, False), (X, X, True, True), (X[:3], Z, False, True)):
        k, th = TO.ntk(model, *args)
        ka, ta = TO.ntk_autograd(model, *args)
        assert rel(k, ka) < 1e-12 and rel(th, ta) < 1e-12
        assert np.all(th > k)


@pytest.mark.parametrize("name", ["chain", "even4", "mixed"])
def test_oracle_position_covariance_holds_the_layer_maps(name):
    """through a dense readout the [i, j, p, p] entries are the layer path's pair maps: the
    position-pair walk reproduces the layer recursion's kernel and Θ"""
    model = golden_model(name, 8)
    X, Z = G["X_8"][:3], G["Z_8"][:2]
    for args in ((X,), (X, Z, False, False), (X[:2], Z, False, True)):
        k, th = TO.ntk(model, *args)
        km, tm = TO.ntk_maps(model, *args)
        assert rel(km, k) < 1e-12 and rel(tm, th) < 1e-12
    body = S(*model.mods[:-1])
    s = TO.position_covariance(body, X, Z, False, False)
    maps = TO.layer_run(body, X, Z, False, False)[0].reshape(3, 2, *s.shape[2:4])
    assert rel(np.einsum("ijabab->ijab", s), maps) < 1e-12


# ------------------------------------------------------------------------------------
# 2. the public surface
# ------------------------------------------------------------------------------------
def test_tap_weights_and_gaussian_taps():
    assert "gaussian_taps" in cnn_gp.__all__ and "gaussian_taps" in cnn_gp.kernels.__all__
    for k, kw in ((3, {}), (4, {}), (4, dict(padding=0)), (5, dict(var_weight=2.79 * 25))):
        box = C(k, **kw)
        for tw in (None, torch.ones(k, k), np.ones((k, k)), [[1.0] * k] * k,
                   cnn_gp.gaussian_taps(k, float("inf")), 3.0 * torch.ones(k, k)):
            c = C(k, tap_weights=tw, **kw)
            assert c.kernel.dtype == box.kernel.dtype and torch.equal(c.kernel, box.kernel)
            assert "taps=custom" not in repr(c)
    g = cnn_gp.gaussian_taps(3, 1.0)
    assert g.dtype == torch.float64 and tuple(g.shape) == (3, 3)
    want = np.exp(-np.array([[2, 1, 2], [1, 0, 1], [2, 1, 2]]) / 2.0)
    assert np.allclose(g.numpy(), want, rtol=1e-15)
    g4 = cnn_gp.gaussian_taps(4, 2.0).numpy()           # the centre is between the taps
    assert np.allclose(g4[0, 0], np.exp(-(1.5 ** 2 * 2) / 8)) and np.allclose(g4, g4[::-1, ::-1])
    c = C(3, var_weight=1.8, tap_weights=g)
    assert np.allclose(c.kernel[0, 0].numpy(), 1.8 * want / want.sum(), rtol=1e-6)
    assert abs(float(c.kernel.sum()) - 1.8) < 1e-6 and "taps=custom" in repr(c)
    # an even "same" kernel keeps its zero first row and column
    c = C(4, var_weight=2.0, tap_weights=cnn_gp.gaussian_taps(4, 1.0))
    kern = c.kernel[0, 0]
    assert tuple(kern.shape) == (5, 5) and not kern[0].any() and not kern[:, 0].any()
    assert abs(float(kern.sum()) - 2.0) < 1e-6 and (kern[1:, 1:] > 0).all()
    # the reference's positional surface is unchanged: tap_weights is the last keyword
    assert C(3, 1, "same", 1, 1., 0., 1, 1).kernel_size == 3
    for bad, msg in ((torch.ones(2, 2), "3x3"), (-torch.ones(3, 3), "non-negative"),
                     (torch.zeros(3, 3), "positive sum"),
                     (torch.full((3, 3), float("nan")), "finite"), ("abc", "tap_weights")):
        with pytest.raises(ValueError, match=msg):
            C(3, tap_weights=bad)
    for args, msg in (((0, 1.0), "k"), ((2.5, 1.0), "k"), ((3, 0.0), "lengthscale"),
                      ((3, -1.0), "lengthscale"), ((3, float("nan")), "lengthscale"),
                      ((3, "x"), "lengthscale")):
        with pytest.raises(ValueError, match=msg):
            cnn_gp.gaussian_taps(*args)


def test_a_wrong_shape_and_a_non_finite_entry_raise():
    c = C(3)
    c.kernel = torch.ones(1, 1, 5, 5) * 0.1
    c.kernel[0, 0, 2, 2] = 0.3
    with pytest.raises(NotImplementedError, match=r"\(1, 1, 5, 5\)"):
        Plan(S(c), 6, 6)
    c = C(3)
    c.kernel[0, 0, 1, 1] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        Plan(S(c), 6, 6)


# ------------------------------------------------------------------------------------
# 3. the lowering
# ------------------------------------------------------------------------------------
def _box_models():
    from cnn_gp import Sum, resnet_block
    return [S(C(3), R(), C(5, padding=0)), S(C(4), R(), C(3, stride=2), R(), C(3, padding=0)),
            S(C(3), Sum([S(), S(R(), C(3))]), R(), C(6, padding=0)),
            S(C(3), resnet_block(), R(), C(6, padding=0))]


def test_a_box_model_compiles_as_before():
    """kinds, geometries and step lists hold no tapconv, and equal those of the same model
    whose buffers were rebuilt by the constructor's own formula (a box written in place)"""
    for n, model in enumerate(_box_models()):
        plan = Plan(model, 6, 6)
        assert all(o.kind != "tapconv" and not isinstance(o.geom, P.TapGeom)
                   for o in plan.prog.ops + plan.pair_ops)
        for ntk in (False, True):
            steps = plan.layer_list(ntk)[0]
            assert all(st.fn != "tapconv" for st in steps)
        twin = _box_models()[n]
        for m in twin.modules():
            if isinstance(m, C):
                with torch.no_grad():
                    m.kernel.copy_(m.kernel.clone())
        p2 = Plan(twin, 6, 6)
        strip = lambda ops: [(o.kind, o.dst, o.src, o.geom, o.pre, o.post, o.addend,  # noqa: E731
                              tuple(o.terms)) for o in ops]
        assert strip(plan.prog.ops) == strip(p2.prog.ops)
        assert strip(plan.pair_ops) == strip(p2.pair_ops)
        key = lambda lst: [(s.fn, s.dst, s.src, s.addend, s.bias, s.theta, s.dst_theta,  # noqa: E731
                            tuple(s.free)) for s in lst[0]]
        assert key(plan.layer_list()) == key(p2.layer_list())
        assert key(plan.layer_list(True)) == key(p2.layer_list(True))
    plan = Plan(S(C(3), R(), C(5, padding=0)), 5, 5)
    assert [(o.kind, o.pre, o.post) for o in plan.pair_ops] == \
        [("conv", N.CGP_PRE_MOMENTS, N.CGP_POST_RELU), ("conv", N.CGP_PRE_NONE, N.CGP_POST_NONE)]


@pytest.mark.parametrize("k,kw,ke,off", [(3, {}, 3, -1), (4, {}, 5, -2), (4, dict(padding=1), 4, -1),
                                         (3, dict(dilation=2, stride=2, var_bias=0.5), 3, -2),
                                         (2, {}, 3, -1)])
def test_an_edited_buffer_lowers_to_tapconv(k, kw, ke, off):
    c = tapped(k, seed=k, **kw)
    assert "taps=custom" in repr(c)
    with pytest.raises(NotImplementedError, match="constant"):
        P.conv_geometry(c)
    plan = Plan(S(c, R(), C(3)), 8, 8)
    op = plan.prog.ops[0]
    assert [o.kind for o in plan.prog.ops] == ["tapconv", "relu", "conv"]
    g = op.geom
    assert type(g) is P.TapGeom
    assert (g.extent, g.offset, g.stride, g.dilation, g.bias) == \
        (ke, off, kw.get("stride", 1), kw.get("dilation", 1), kw.get("var_bias", 0.0))
    assert isinstance(g.table, tuple) and all(isinstance(r, tuple) and len(r) == ke and
                                              all(type(v) is float for v in r) for r in g.table)
    assert np.array_equal(np.array(g.table), c.kernel[0, 0].double().numpy())
    assert op.shape_out == P.conv_out_hw(c, 8, 8)
    # the ReLU beside a tapconv is its own launch, folded into the box conv after it; the
    # moments are not folded into a tapconv
    assert [(o.kind, o.pre, o.post) for o in plan.pair_ops] == \
        [("tapconv", N.CGP_PRE_NONE, N.CGP_POST_NONE), ("conv", N.CGP_PRE_RELU, N.CGP_POST_NONE)]
    assert not plan.moments_fused and plan.pool is None
    plan = Plan(S(C(3), R(), tapped(k, **kw), R()), 8, 8)
    assert [o.kind for o in plan.pair_ops] == ["conv", "tapconv", "relu"]
    assert plan.pair_ops[0].post == N.CGP_POST_RELU


def test_step_lists_of_a_tapped_model():
    from cnn_gp import Sum
    model = S(tapped(3, var_bias=0.1), Sum([S(), S(R(), tapped(3, 1))]), R(),
              tapped(6, 2, padding=0, var_bias=0.2))
    plan = Plan(model, 6, 6)
    steps, k, th = plan.layer_list()
    assert [s.fn for s in steps] == ["tapconv", "relu", "tapconv", "axpby", "relu", "tapconv"]
    assert all(s.addend is None for s in steps) and th is None
    assert [s.bias for s in steps if s.fn == "tapconv"] == [0.1, 0.0, 0.2]
    steps, k, th = plan.layer_list(ntk=True)
    fns = [(s.fn, s.dst[0], s.bias, None if s.addend is None else s.addend[0]) for s in steps]
    assert fns == [("tapconv", "K", 0.1, None),                       # Θ' is this K' buffer
                   ("relu_ntk", "K", None, None),
                   ("tapconv", "K", 0.0, None), ("tapconv", "T", 0.0, "K"),
                   ("axpby", "K", None, None), ("axpby", "T", None, None),
                   ("relu_ntk", "K", None, None),
                   ("tapconv", "K", 0.2, None), ("tapconv", "T", 0.0, "K")]
    assert steps[1].theta == steps[0].dst and th == ("T", plan.vf)


def test_the_fast_paths_decline():
    from cnn_gp.netplan import NetPlan, Unsupported
    model = S(tapped(3), R(), C(28, padding=0)).double()
    plan = model._plan(28, 28)
    with pytest.raises(Unsupported, match="op tapconv"):
        NetPlan(plan, 8)
    assert model._net_plan(plan, 8) is None
    assert plan._var_chain({plan.prog.ops[0].dst}, set(), torch.device("cpu")) is None
    assert model.image_variances(torch.ones(2, 1, 28, 28, dtype=torch.float64)) is None
    box = S(C(3), R(), C(28, padding=0)).double()
    assert box._net_plan(box._plan(28, 28), 8) is not None


def test_every_edit_of_a_buffer_drops_the_plans():
    model = S(C(3), R(), C(6, padding=0))
    conv = model.mods[0]
    skey = model._structure_key()
    p0 = model._plan(6, 6)
    assert model._plan(6, 6) is p0 and p0.prog.ops[0].kind == "conv"
    conv.kernel[0, 0, 1, 1] *= 2.0                       # in place
    p1 = model._plan(6, 6)
    assert p1 is not p0 and p1.prog.ops[0].kind == "tapconv" and model._plan(6, 6) is p1
    conv.kernel.data = conv.kernel.data * 0.5            # .data =
    p2 = model._plan(6, 6)
    assert p2 is not p1 and p2.prog.ops[0].geom.table[1][1] == 0.5 * p1.prog.ops[0].geom.table[1][1]
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["0.kernel"][0, 0, 0, 2] = 0.75
    model.load_state_dict(sd)                            # load_state_dict
    p3 = model._plan(6, 6)
    assert p3 is not p2 and p3.prog.ops[0].geom.table[0][2] == 0.75
    conv.kernel = torch.full((1, 1, 3, 3), 1.0 / 9)      # assignment: the box again
    p4 = model._plan(6, 6)
    assert p4 is not p3 and p4.prog.ops[0].kind == "conv"
    assert model._structure_key() == skey                # host attributes only: unchanged
    wv = model._weights_version()
    conv.kernel.add_(0.0)
    assert model._weights_version() != wv


def test_pool_rules_and_position_pair_lists():
    from cnn_gp import AvgPool2d, GlobalAvgPool
    A, GP = AvgPool2d, GlobalAvgPool
    with pytest.raises(NotImplementedError, match="must keep the value 1x1"):
        Plan(S(C(3), R(), GP(), tapped(3, padding=2)), 6, 6)
    plan = Plan(S(tapped(3), R(), A(2), tapped(3, 1), R(), GP(), tapped(3, 2, var_bias=0.3)), 8, 8)
    ps = plan.pool
    assert [s.fn for s in ps.steps] == ["moments", "tapconv", "nonlin", "avgpool", "tapconv",
                                        "nonlin", "pool", "tapconv"]
    ops = plan.prog.ops
    # upstream of the AvgPool2d the variances come from run_variances, downstream from the
    # self pass, where the tapconv is one more step of the list
    assert ps.need_var == {ops[0].dst, ops[3].dst} and ps.self_var == {ops[3].dst}
    assert ps.self_last == 4 and ps.scalars == {ops[5].dst, ops[6].dst}
    ns = plan.pool_ntk(False, True, 8)
    fns = [(s.fn, s.dst[0], s.bias, None if s.addend is None else s.addend[0]) for s in ns.steps]
    assert fns == [("moments", "K", None, None), ("tapconv", "K", 0.0, None),
                   ("nonlin_ntk", "K", None, None),
                   ("avgpool", "K", None, None), ("avgpool", "T", None, None),
                   ("tapconv", "K", 0.0, None), ("tapconv", "T", 0.0, "K"),
                   ("nonlin_ntk", "K", None, None),
                   ("pool", "K", None, None), ("pool", "T", None, None),
                   ("tapconv", "K", 0.3, None), ("tapconv", "T", 0.0, "K")]
    assert ns.final_theta == ("T", plan.vf)
    body = Plan(S(tapped(3), R(), tapped(3, 1)), 6, 6).body_steps()
    assert [s.fn for s in body.steps] == ["moments", "tapconv", "nonlin", "tapconv"]
    assert not body.self_var


# ------------------------------------------------------------------------------------
# 4. ABI and the entry points' argument checks
# ------------------------------------------------------------------------------------
NEW_SYMBOLS = {"cgp_tapconv_args_size", "cgp_tapconv_f64", "cgp_tapconv_f32",
               "cgp_tapconv_cov_args_size", "cgp_tapconv_cov_f64", "cgp_tapconv_cov_f32"}


def test_tapconv_abi():
    lib = N.load()
    assert N.CGP_ABI_VERSION == 12 and lib.cgp_abi_version() == 12
    txt = open(os.path.join(ROOT, "include", "cnngp.h")).read()
    assert "#define CGP_ABI_VERSION 12" in txt
    syms = set(re.findall(r"\b(cgp_tapconv_[a-z0-9_]+)\s*\(", txt))
    assert syms == NEW_SYMBOLS == {s for s in N.SIGNATURES if "tapconv" in s}
    assert not any(s.startswith(("cgp_cov_", "cgp_covmap_")) for s in NEW_SYMBOLS)
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert lib.cgp_tapconv_args_size() == ctypes.sizeof(N.TapConvArgs) == 88
    assert lib.cgp_tapconv_cov_args_size() == ctypes.sizeof(N.TapConvCovArgs) == 80
    assert [f[0] for f in N.TapConvArgs._fields_] == \
        ["in_", "out", "addend", "table", "nmaps", "h", "w", "ho", "wo", "extent", "offset",
         "stride", "dilation", "max_groups", "reserved", "bias"]
    assert [f[0] for f in N.TapConvCovArgs._fields_] == \
        ["in_", "out", "addend", "table", "npairs", "h", "w", "ho", "wo", "extent", "offset",
         "stride", "dilation", "bias"]


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("cov", [False, True])
def test_entry_points_reject_bad_arguments_on_host(sfx, cov):
    """argument checks return CGP_EINVAL before any HIP call (no GPU needed)"""
    lib = N.load()
    EINVAL = 1001
    fn = getattr(lib, f"cgp_tapconv_{'cov_' if cov else ''}{sfx}")
    assert fn(None, None) == EINVAL and b"NULL" in lib.cgp_last_error()
    count = "npairs" if cov else "nmaps"

    def args(**kw):
        a = (N.TapConvCovArgs if cov else N.TapConvArgs)()
        a.in_, a.out, a.table = 64, 128, 192
        a.h, a.w, a.ho, a.wo = 7, 6, 4, 3
        a.extent, a.offset, a.stride, a.dilation = 3, -1, 2, 1
        a.bias = .1
        setattr(a, count, 6)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    item = 8 if sfx == "f64" else 4
    cases = [(dict(in_=None), b"NULL"), (dict(out=None), b"NULL"), (dict(table=None), b"NULL"),
             (dict(out=64), b"must not be in"), ({count: 0}, b"bad sizes"),
             (dict(h=0), b"bad sizes"), (dict(w=-1), b"bad sizes"), (dict(ho=0), b"bad sizes"),
             (dict(wo=0), b"bad sizes"),
             (dict(extent=0), b"bad geometry"), (dict(stride=0), b"bad geometry"),
             (dict(dilation=0), b"bad geometry"), (dict(dilation=1 << 30), b"bad geometry"),
             (dict(offset=-(1 << 24)), b"bad geometry"),
             (dict(ho=5), b"inconsistent"), (dict(wo=2), b"inconsistent"),
             (dict(ho=3), b"inconsistent"), (dict(extent=9, offset=0), b"inconsistent"),
             # a padding beyond the taps' span: F.conv2d's size, but the first output row and
             # column have no tap inside the map
             (dict(extent=1, offset=-1, stride=1, ho=9, wo=8), b"all miss")]
    if cov:
        cases += [({count: 1 << 31}, b"bad sizes"),
                  (dict(h=200, w=200, ho=100, wo=100), b"bad sizes"),     # (h w)² above 2^30
                  # 3 taps of a w x w block above 64 KB
                  (dict(h=4, w=60 if item == 8 else 80, ho=2, wo=30 if item == 8 else 40),
                   b"of LDS")]
    else:
        cases += [(dict(max_groups=-1), b"max_groups"),
                  # one staged map above 64 KB
                  (dict(h=100, w=100 if item == 8 else 200, extent=1, offset=0, stride=1,
                        ho=100, wo=100 if item == 8 else 200), b"of LDS")]
    for kw, msg in cases:
        assert fn(ctypes.byref(args(**kw)), None) == EINVAL, kw
        assert msg in lib.cgp_last_error(), (kw, lib.cgp_last_error())

