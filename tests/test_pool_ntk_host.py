"""CPU-only tests of the neural tangent kernel on position-pair maps: the test-time oracle
(tests/pool_ntk_oracle.py) pinned to the definition of Θ by finite differences, the lowering
program.pool_ntk_steps, and the host side of ntk_maps / position_ntk."""
import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import program as P
from cnn_gp.program import compile_program, pool_ntk_steps, pool_steps

import pool_ntk_oracle as NO

m = cnn_gp
S, C, R, E, GE, G, A, CC = (m.Sequential, m.Conv2d, m.ReLU, m.Erf, m.Gelu, m.GlobalAvgPool,
                            m.AvgPool2d, m.CorrelatedConv2d)


def nets():
    """name -> (model, (H, W)): a GAP head, a Myrtle-style net with AvgPool2d(2), a corrconv
    readout, erf, gelu, a residual Sum"""
    return {
        "gap": (S(C(3, var_bias=.1), R(), C(3, var_weight=1.5), R(), G()), (5, 4)),
        "myrtle": (S(C(3, var_bias=.1), R(), C(3), R(), A(2), C(3, var_bias=.2), R(), A(2), G(),
                     C(1, var_weight=2., var_bias=.3)), (8, 8)),
        "corr_readout": (S(C(3, var_bias=.1), R(), CC(3, lengthscale=1., var_bias=.1), R(),
                           CC(4, padding=0, lengthscale=1.5, var_weight=1.5, var_bias=.2)),
                         (4, 4)),
        "erf": (S(C(3, var_bias=.2), E(), C(3, var_weight=1.5), E(), G()), (5, 4)),
        "gelu": (S(C(3, var_bias=.2), GE(), C(3, var_weight=1.5), GE(), A(2), C(2, padding=0)),
                 (4, 4)),
        "residual": (S(C(3), m.Sum([S(), S(R(), C(3, var_bias=.1), R(), C(3))]), R(), G()),
                     (5, 4)),
    }


NAMES = list(nets())


def images(hw, n=(2, 3), seed=0):
    rng = np.random.default_rng(seed + 10 * hw[0] + hw[1])
    return tuple(rng.random((k, 4) + hw, dtype=np.float32).astype(np.float64) for k in n)


# ------------------------------------------------------------------------------------
# the oracle against the definition
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_the_derivative_of_the_forward_map(name):
    """Θ = Σ over conv / corrconv outputs of ⟨∂K_final/∂S^l, S^l⟩ at fixed variances, taken as
    the central difference in ε of K_final with every such output's map scaled by (1 ± ε) and
    the variance streams untouched.  same=False and distinct images: the override elements
    have no such derivative.  ε = 1e-5 and 1e-7 relative: truncation is ~ε² and round-off
    ~eps/ε, both near 1e-10, three orders under the bound and far under any structural error
    (a dropped term of the recursion is O(1))."""
    model, hw = nets()[name]
    model = model.double()
    x, y = images(hw)
    k, th = NO.ntk(model, x, y, False, False)
    fd = NO.ntk_by_difference(model, x, y, eps=1e-5)
    err = float(np.max(np.abs(fd - th)) / np.max(np.abs(th)))
    print(f"{name}: recursion vs central difference {err:.2e}")
    assert err < 1e-7
    assert np.all(th > 0) and not np.allclose(th, k)


def test_oracle_without_a_pooling_layer_is_the_layer_oracle():
    """on a model the layer path runs, the maps' 1x1 result is ntk_oracle's stepwise Θ"""
    import ntk_oracle as NT
    model = S(C(3, var_bias=.1), R(), C(3), R(), C(4, padding=0, var_bias=.2)).double()
    x, y = images((4, 4))
    for args in ((x,), (x, y, False, False), (x, x, True, True)):
        k, th = NO.ntk(model, *args)
        rk, rth = NT.run_steps(model, *args)
        assert np.max(np.abs(k - rk)) < 1e-13 * np.max(k)
        assert np.max(np.abs(th - rth)) < 1e-13 * np.max(th)


# ------------------------------------------------------------------------------------
# the lowering
# ------------------------------------------------------------------------------------
def lower(name, **kw):
    model, (h, w) = nets()[name]
    prog, v0, vf = compile_program(model, h, w)
    body = not any(o.kind == "pool" for o in prog.ops)
    return pool_ntk_steps(prog, v0, vf, body=body, **kw), (prog, v0, vf, body)


def check_buffers(ns):
    """every buffer read was written before, is freed after its last reader and not earlier;
    peak is the live total of both streams at the fullest launch"""
    live, peak = set(), 0
    for idx, st in enumerate(ns.steps):
        for b in st.reads():
            assert b in live, (st.fn, b)
        for b in st.writes():
            assert b in ns.shapes
            if st.fn != "accum":
                assert b not in live, (st.fn, b)
            live.add(b)
        peak = max(peak, sum(ns.elems(b) for b in live))
        later = {b for s2 in ns.steps[idx + 1:] for b in s2.reads()}
        keep = {ns.final} | ({ns.final_theta} if ns.final_theta is not None else set())
        for b in st.free:
            assert b in live and b not in later and b not in keep
        live.difference_update(st.free)
        assert not {b for b in live if b not in later and b not in keep}, (idx, live)
    assert ns.final in live and (ns.final_theta is None or ns.final_theta in live)
    assert ns.peak == peak
    return peak


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_steps_structure(name, fused):
    ns, (prog, v0, vf, body) = lower(name, fused=fused)
    fwd = pool_steps(prog, v0, vf, body)
    check_buffers(ns)
    steps = ns.steps
    assert steps[0].fn == "moments" and steps[0].dst == ("K", v0)
    assert ns.final == ("K", vf) and ns.final_theta is not None
    assert ns.need_var == fwd.need_var and ns.forward.self_var == fwd.self_var
    # both streams are live somewhere: the peak exceeds the forward run's
    assert ns.peak > fwd.peak
    # the K stream's buffers carry the forward program's values: every forward buffer is there
    assert {("K", b) for b in fwd.shapes} <= set(ns.shapes)
    assert all(ns.shapes[("K", b)] == fwd.shapes[b] for b in fwd.shapes)
    # Θ = None short cuts: the first conv reads no theta and no step before it has one
    first = next(i for i, st in enumerate(steps) if st.fn in ("conv", "conv_ntk", "corrconv"))
    assert steps[first].theta is None and steps[first].src == ("K", v0)
    assert all(st.theta is None and st.dst[0] == "K" for st in steps[:first + 1])
    fns = [st.fn for st in steps]
    if fused:
        assert "conv_ntk" in fns
    else:
        assert "conv_ntk" not in fns
        # the first conv's Θ is its K buffer: the nonlinearity after it reads one buffer twice
        nl = next(st for st in steps if st.fn == "nonlin_ntk")
        assert nl.theta == nl.src == steps[first].dst
        # every later conv is the sequence: K, then Θ with bias 0 and addend K'
        for a, b in zip(steps, steps[1:]):
            if b.fn == "conv" and b.dst[0] == "T":
                assert a.fn == "conv" and b.bias == 0.0 and b.addend == a.dst
                assert a.bias == a.op.geom.bias and b.op is a.op


def test_first_conv_with_post_stage_is_one_launch_without_theta():
    ns, _ = lower("gap", fused=True)
    st = ns.steps[1]
    assert st.fn == "conv_ntk" and st.theta is None and st.post == N.CGP_COV_RELU
    assert st.dst_theta == ("T", st.dst[1])
    nxt = ns.steps[2]
    assert nxt.fn == "conv_ntk" and nxt.theta == st.dst_theta and nxt.src == st.dst


def test_nonlinearity_on_zero_theta_is_the_forward_launch():
    for nl, fn in ((R(), "nonlin"), (E(), "nonlin"), (GE(), "gelu")):
        prog, v0, vf = compile_program(S(nl, C(3), G()), 4, 4)
        ns = pool_ntk_steps(prog, v0, vf)
        assert [st.fn for st in ns.steps] == ["moments", fn, "conv", "pool", "pool"]
        assert ns.steps[1].theta is None and ns.steps[2].dst == ("K", ns.steps[2].dst[1])
        # the conv's Θ is its K buffer, pooled by a launch of its own
        assert ns.steps[4].src == ns.steps[2].dst and ns.final_theta == ns.steps[4].dst
    prog, v0, vf = compile_program(S(R(), G()), 4, 4)
    ns = pool_ntk_steps(prog, v0, vf)
    assert ns.final_theta is None and all(st.dst[0] == "K" for st in ns.steps)
    prog, v0, vf = compile_program(S(C(3), G()), 4, 4)
    assert pool_ntk_steps(prog, v0, vf, body=False).final_theta == ("T", vf)
    prog, v0, vf = compile_program(S(C(4, padding=0)), 4, 4)
    ns = pool_ntk_steps(prog, v0, vf, body=True)
    assert ns.final_theta == ns.final                        # a single conv: Θ is K's buffer


def test_conv_after_avgpool_keeps_its_nonlinearity_as_a_launch():
    ns, _ = lower("myrtle", fused=True)
    fns = [st.fn for st in ns.steps]
    k = fns.index("avgpool")
    assert fns[k:k + 2] == ["avgpool", "avgpool"]            # the same op on K and on Θ
    after = ns.steps[k + 2:]
    conv = after[0]
    assert conv.fn == "conv_ntk" and conv.post == N.CGP_COV_NONE
    assert after[1].fn == "nonlin_ntk" and after[1].src == conv.dst \
        and after[1].theta == conv.dst_theta
    assert ns.forward.self_var                               # the self pass is the forward's


def test_corrconv_theta_is_bias_zero_then_add():
    ns, _ = lower("corr_readout", fused=True)
    cc = [i for i, st in enumerate(ns.steps) if st.fn == "corrconv"]
    assert len(cc) == 4
    for k_i, t_i in (cc[:2], cc[2:]):
        ks, ts, acc = ns.steps[k_i], ns.steps[t_i], ns.steps[t_i + 1]
        assert ks.bias == ks.op.geom.bias and ts.bias == 0.0 and ts.op is ks.op
        assert acc.fn == "accum" and acc.dst == ts.dst and acc.src == ks.dst


def test_fused_falls_back_to_the_sequence_over_the_lds_cap():
    """7 taps of a 28x28 map in float64: one stream is 43 904 bytes, two are 87 808 > 64 KB"""
    assert P.conv_ntk_fits(7, 28, 1, 8) and not P.conv_ntk_fits(7, 28, 2, 8)
    assert P.conv_ntk_fits(7, 28, 2, 4) and P.conv_ntk_fits(3, 28, 2, 8)
    model = S(C(7, var_bias=.1), R(), C(7), R(), G())
    prog, v0, vf = compile_program(model, 28, 28)
    f64 = [st.fn for st in pool_ntk_steps(prog, v0, vf, fused=True, itemsize=8).steps]
    f32 = [st.fn for st in pool_ntk_steps(prog, v0, vf, fused=True, itemsize=4).steps]
    assert f64 == ["moments", "conv_ntk", "conv", "conv", "nonlin_ntk", "pool", "pool"]
    assert f32 == ["moments", "conv_ntk", "conv_ntk", "pool", "pool"]
    check_buffers(pool_ntk_steps(prog, v0, vf, fused=True, itemsize=8))


def test_forward_rules_still_raise():
    cases = [(S(C(3), G(), R()), P.POOL_RULE_NONLIN), (S(C(3), G(), GE()), P.GELU_RULE_GLOBAL),
             (S(C(3), G(), G()), P.POOL_RULE_ONE), (S(C(3), G(), C(3, padding=2)), P.POOL_RULE_CONV),
             (S(C(3), G(), A(1)), P.AVGPOOL_RULE_GLOBAL),
             (S(C(3), G(), CC(1, lengthscale=0)), P.CORRCONV_RULE_GLOBAL),
             (S(C(1), m.Sum([S(G()), S()])), P.POOL_RULE_ONE)]         # on 1x1 images
    for model, rule in cases:
        h = 1 if model is cases[-1][0] else 4
        prog, v0, vf = compile_program(model, h, h)
        for fused in (True, False):
            with pytest.raises(NotImplementedError) as e:
                pool_ntk_steps(prog, v0, vf, fused=fused)
            assert str(e.value) == rule
        with pytest.raises(NotImplementedError) as e:
            model.ntk_maps(torch.zeros(1, 1, h, h))
        assert str(e.value) == rule
    prog, v0, vf = compile_program(S(C(3), R()), 4, 4)
    with pytest.raises(NotImplementedError):
        pool_ntk_steps(prog, v0, vf, body=False)             # no pool on the path
    prog, v0, vf = compile_program(S(C(3), G()), 4, 4)
    with pytest.raises(ValueError, match="GlobalAvgPool"):
        pool_ntk_steps(prog, v0, vf, body=True)


# ------------------------------------------------------------------------------------
# the public methods without a device
# ------------------------------------------------------------------------------------
def test_model_ntk_points_to_ntk_maps_and_still_raises():
    model = nets()["gap"][0]
    with pytest.raises(NotImplementedError) as e:
        model.ntk(torch.zeros(1, 1, 5, 4))
    assert str(e.value) == P.POOL_RULE_NTK
    assert "ntk_maps" in m.NNGPKernel.ntk.__doc__


def test_empty_batches():
    model, (h, w) = nets()["gap"]
    for dt in (torch.float32, torch.float64):
        x, e = torch.zeros(3, 2, h, w, dtype=dt), torch.zeros(0, 2, h, w, dtype=dt)
        th = model.ntk_maps(x, e, False)
        assert tuple(th.shape) == (3, 0) and th.dtype == dt
        k, th = model.ntk_maps(e, x, False, return_nngp=True)
        assert tuple(k.shape) == tuple(th.shape) == (0, 3) and k is not th
        assert tuple(model.ntk_maps(e).shape) == (0, 0)
        assert tuple(model.ntk_maps(e, e, False, True).shape) == (0,)
    body = S(C(3), R(), C(3, stride=2))
    x, e = torch.zeros(2, 1, 5, 4), torch.zeros(0, 1, 5, 4)
    assert tuple(body.position_ntk(x, e, False).shape) == (2, 0, 3, 2, 3, 2)
    s, th = body.position_ntk(e, e, False, True, return_nngp=True)
    assert tuple(s.shape) == tuple(th.shape) == (0, 3, 2, 3, 2)
    with pytest.raises(ValueError, match="GlobalAvgPool"):
        nets()["gap"][0].position_ntk(x)


def test_device_and_not_1x1_errors():
    """forward's order: no device is reported first, then a final value that is not 1x1"""
    model, (h, w) = nets()["gap"]
    x = torch.zeros(2, 1, 4, 4)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            model.ntk_maps(torch.zeros(2, 1, h, w))
        with pytest.raises(RuntimeError, match="HIP device"):
            S(C(3), R()).position_ntk(x)
        with pytest.raises(RuntimeError, match="HIP device"):
            S(C(3), R(), A(2)).ntk_maps(x)
    else:
        with pytest.raises(RuntimeError, match="2x2 per pair, not 1x1"):
            S(C(3), R(), A(2)).ntk_maps(x)
        with pytest.raises(RuntimeError, match="4x4 per pair, not 1x1"):
            S(C(3), R()).ntk_maps(x)


def test_conv_ntk_entry_point_checks_come_before_any_launch():
    """host pointers that are never read: every check returns before a HIP call"""
    import ctypes
    lib = N.load()
    buf = [(ctypes.c_double * 4)() for _ in range(4)]
    at = lambda k: ctypes.c_void_p(ctypes.addressof(buf[k]))                    # noqa: E731
    a = N.CovConvNtkArgs()
    a.in_, a.theta, a.out, a.out_theta = at(0), at(1), at(2), at(3)
    a.npairs, a.h, a.w, a.ho, a.wo = 1, 28, 28, 28, 28
    a.taps, a.offset, a.stride, a.dilation, a.weight = 7, -3, 1, 1, 1.0
    assert lib.cgp_covntk_conv_f64(ctypes.byref(a), None) == 1001
    msg = lib.cgp_last_error().decode()
    assert "7 taps of a 28x28 block of 2 stream(s) are 87808 bytes" in msg and "65536" in msg
    a.out = a.in_
    assert lib.cgp_covntk_conv_f32(ctypes.byref(a), None) == 1001
    assert b"must not be in" in lib.cgp_last_error()
    a.out, a.post = at(2), 7
    assert lib.cgp_covntk_conv_f32(ctypes.byref(a), None) == 1001
    assert b"not a nonlinearity" in lib.cgp_last_error()
    a.post = N.CGP_COV_GELU
    assert lib.cgp_covntk_conv_f32(ctypes.byref(a), None) == 1001       # no variances
    b = N.CovNonlinNtkArgs()
    b.in_, b.theta, b.out, b.out_theta = at(0), at(0), at(0), at(0)
    b.npairs, b.h, b.w, b.kind = 1, 2, 2, N.CGP_COV_GELU
    assert lib.cgp_covntk_nonlin_f64(ctypes.byref(b), None) == 1001     # no variances
    b.xx = b.yy = b.pair_i = b.pair_j = at(1)
    assert lib.cgp_covntk_nonlin_f64(ctypes.byref(b), None) == 1001
    assert b"one buffer" in lib.cgp_last_error()
    b.out_theta, b.kind = at(2), 4
    assert lib.cgp_covntk_nonlin_f64(ctypes.byref(b), None) == 1001
    assert b"neither ReLU, erf nor GELU" in lib.cgp_last_error()


def test_gram_matrix_rejects_an_unknown_ntk_route():
    from cnn_gp import gram
    with pytest.raises(ValueError, match="maps"):
        gram.gram_matrix(nets()["gap"][0], torch.zeros(2, 1, 5, 4), ntk="map")


def test_native_structs_and_constants():
    assert N.CGP_COV_GELU == 3 and N.CGP_COV_GELU not in (N.CGP_COV_NONE, N.CGP_COV_RELU,
                                                          N.CGP_COV_ERF)
    lib = N.load()                                           # checks both struct sizes
    assert N.CGP_ABI_VERSION == 12 == lib.cgp_abi_version()
    for sfx in ("f64", "f32"):
        assert hasattr(lib, f"cgp_covntk_nonlin_{sfx}") and hasattr(lib, f"cgp_covntk_conv_{sfx}")
