"""CPU-only: the two lists of the layer path (program.layer_steps, ntk_steps), pinned to the
commit before they shared one step record, one scheduling helper and one executor
(Plan.run_layer_steps).  Recorded there, with fusion on and off: the fused op list, the
ntk_steps list, and the buffers its two executors (the forward run's and the NTK run's)
dropped after every step -- their ``last`` / delete logic replayed on the host.  On that commit an NTK step that is
not a conv carried an unused ``bias`` of 0.0 (its record's default); here it is None, as on
every other list, and the literals say so.

Four networks at 6x6:
  chain     fused moments, a ReLU post-stage and a ReLU pre-stage
  residual  a conv addend
  mixed     no fused moments (the input moments are a launch of their own), a three-term
            weighted sum, all four nonlinearities, a ReLU with an addend
  lead      a nonlinearity on Θ = 0, and a sum whose only live Θ term has weight 1: the term's
            buffer is passed on"""
import pytest

import cnn_gp
from cnn_gp.program import Plan

m = cnn_gp
S, C, R, E, GE, AB = m.Sequential, m.Conv2d, m.ReLU, m.Erf, m.Gelu, m.ABReLU


def nets():
    return {
        "chain": S(C(3, var_bias=.1), R(), C(3), R(), C(6, padding=0)),
        "residual": S(C(3, var_bias=.1), R(), m.Sum([S(C(3), R(), C(3)), S()]), R(),
                      C(6, padding=0, var_bias=.2)),
        "mixed": S(m.Mixture([S(C(3), E()), S(C(3, var_bias=.3), AB(.2, 1.5)), S()]),
                   m.Sum([S(GE(), C(3)), S(R())]), R(), C(6, padding=0)),
        "lead": S(R(), m.Sum([S(C(3)), S()]), R(), C(6, padding=0)),
    }


def K(v):
    return ("K", v)


def T(v):
    return ("T", v)


_ = None
W = 0.3333333432674408        # a Mixture's proportion: softmax in float32

# fused ops: (kind, dst, src, pre, pre_var, post, post_var, addend, terms); then the values
# the forward executor dropped after each op
FORWARD = {
    ("chain", True): (
        [("conv", 2, 0, 2, _, 1, 1, _, []),
         ("conv", 4, 2, 0, _, 1, 3, _, []),
         ("conv", 5, 4, 0, _, 0, _, _, [])],
        [[], [2], [4]]),
    ("chain", False): (
        [("conv", 1, 0, 0, _, 0, _, _, []),
         ("relu", 2, 1, 0, _, 0, _, _, []),
         ("conv", 3, 2, 0, _, 0, _, _, []),
         ("relu", 4, 3, 0, _, 0, _, _, []),
         ("conv", 5, 4, 0, _, 0, _, _, [])],
        [[0], [1], [2], [3], [4]]),
    ("residual", True): (
        [("conv", 2, 0, 2, _, 1, 1, _, []),
         ("conv", 4, 2, 0, _, 1, 3, _, []),
         ("conv", 6, 4, 0, _, 0, _, 2, []),
         ("conv", 8, 6, 1, 6, 0, _, _, [])],
        [[], [], [2, 4], [6]]),
    ("residual", False): (
        [("conv", 1, 0, 0, _, 0, _, _, []),
         ("relu", 2, 1, 0, _, 0, _, _, []),
         ("conv", 3, 2, 0, _, 0, _, _, []),
         ("relu", 4, 3, 0, _, 0, _, _, []),
         ("conv", 5, 4, 0, _, 0, _, _, []),
         ("add", 6, _, 0, _, 0, _, _, [(_, 5), (_, 2)]),
         ("relu", 7, 6, 0, _, 0, _, _, []),
         ("conv", 8, 7, 0, _, 0, _, _, [])],
        [[0], [1], [], [3], [4], [2, 5], [6], [7]]),
    ("mixed", True): (
        [("conv", 1, 0, 0, _, 0, _, _, []),
         ("erf", 2, 1, 0, _, 0, _, _, []),
         ("conv", 3, 0, 0, _, 0, _, _, []),
         ("abrelu", 4, 3, 0, _, 0, _, _, []),
         ("add", 5, _, 0, _, 0, _, _, [(W, 2), (W, 4), (W, 0)]),
         ("gelu", 6, 5, 0, _, 0, _, _, []),
         ("conv", 7, 6, 0, _, 0, _, _, []),
         ("relu", 9, 5, 0, _, 0, _, 7, []),
         ("conv", 11, 9, 1, 9, 0, _, _, [])],
        [[], [1], [], [3], [0, 2, 4], [], [6], [5, 7], [9]]),
    ("mixed", False): (
        [("conv", 1, 0, 0, _, 0, _, _, []),
         ("erf", 2, 1, 0, _, 0, _, _, []),
         ("conv", 3, 0, 0, _, 0, _, _, []),
         ("abrelu", 4, 3, 0, _, 0, _, _, []),
         ("add", 5, _, 0, _, 0, _, _, [(W, 2), (W, 4), (W, 0)]),
         ("gelu", 6, 5, 0, _, 0, _, _, []),
         ("conv", 7, 6, 0, _, 0, _, _, []),
         ("relu", 8, 5, 0, _, 0, _, _, []),
         ("add", 9, _, 0, _, 0, _, _, [(_, 7), (_, 8)]),
         ("relu", 10, 9, 0, _, 0, _, _, []),
         ("conv", 11, 10, 0, _, 0, _, _, [])],
        [[], [1], [], [3], [0, 2, 4], [], [6], [5], [7, 8], [9], [10]]),
    ("lead", True): (
        [("relu", 1, 0, 0, _, 0, _, _, []),
         ("conv", 3, 1, 0, _, 0, _, 1, []),
         ("conv", 5, 3, 1, 3, 0, _, _, [])],
        [[0], [1], [3]]),
    ("lead", False): (
        [("relu", 1, 0, 0, _, 0, _, _, []),
         ("conv", 2, 1, 0, _, 0, _, _, []),
         ("add", 3, _, 0, _, 0, _, _, [(_, 2), (_, 1)]),
         ("relu", 4, 3, 0, _, 0, _, _, []),
         ("conv", 5, 4, 0, _, 0, _, _, [])],
        [[0], [], [1, 2], [3], [4]]),
}
FORWARD_PEAK = {("chain", True): 2, ("chain", False): 2, ("residual", True): 3,
                ("residual", False): 3, ("mixed", True): 4, ("mixed", False): 4,
                ("lead", True): 2, ("lead", False): 3}

# ntk_steps (the unfused program, whatever the plan's fusion):
# (fn, dst, src, bias, addend, var, theta, dst_theta, terms); the final K and Θ buffers; the
# buffers the NTK executor dropped after each step; its peak of live maps
NTK = {
    "chain": (
        [("conv", K(1), K(0), 0.1, _, _, _, _, []),
         ("relu_ntk", K(2), K(1), _, _, 1, K(1), T(2), []),
         ("conv", K(3), K(2), 0.0, _, _, _, _, []),
         ("conv", T(3), T(2), 0.0, K(3), _, _, _, []),
         ("relu_ntk", K(4), K(3), _, _, 3, T(3), T(4), []),
         ("conv", K(5), K(4), 0.0, _, _, _, _, []),
         ("conv", T(5), T(4), 0.0, K(5), _, _, _, [])],
        (K(5), T(5)),
        [[K(0)], [K(1)], [K(2)], [T(2)], [K(3), T(3)], [K(4)], [T(4)]], 4),
    "residual": (
        [("conv", K(1), K(0), 0.1, _, _, _, _, []),
         ("relu_ntk", K(2), K(1), _, _, 1, K(1), T(2), []),
         ("conv", K(3), K(2), 0.0, _, _, _, _, []),
         ("conv", T(3), T(2), 0.0, K(3), _, _, _, []),
         ("relu_ntk", K(4), K(3), _, _, 3, T(3), T(4), []),
         ("conv", K(5), K(4), 0.0, _, _, _, _, []),
         ("conv", T(5), T(4), 0.0, K(5), _, _, _, []),
         ("axpby", K(6), _, _, _, _, _, _, [(_, K(5)), (_, K(2))]),
         ("axpby", T(6), _, _, _, _, _, _, [(_, T(5)), (_, T(2))]),
         ("relu_ntk", K(7), K(6), _, _, 6, T(6), T(7), []),
         ("conv", K(8), K(7), 0.2, _, _, _, _, []),
         ("conv", T(8), T(7), 0.0, K(8), _, _, _, [])],
        (K(8), T(8)),
        [[K(0)], [K(1)], [], [], [K(3), T(3)], [K(4)], [T(4)], [K(2), K(5)], [T(2), T(5)],
         [K(6), T(6)], [K(7)], [T(7)]], 6),
    "mixed": (
        [("conv", K(1), K(0), 0.0, _, _, _, _, []),
         ("erf_ntk", K(2), K(1), _, _, 1, K(1), T(2), []),
         ("conv", K(3), K(0), 0.3, _, _, _, _, []),
         ("abrelu_ntk", K(4), K(3), _, _, 3, K(3), T(4), []),
         ("axpby", K(5), _, _, _, _, _, _, [(W, K(2)), (W, K(4)), (W, K(0))]),
         ("axpby", T(5), _, _, _, _, _, _, [(W, T(2)), (W, T(4))]),
         ("gelu_ntk", K(6), K(5), _, _, 5, T(5), T(6), []),
         ("conv", K(7), K(6), 0.0, _, _, _, _, []),
         ("conv", T(7), T(6), 0.0, K(7), _, _, _, []),
         ("relu_ntk", K(8), K(5), _, _, 5, T(5), T(8), []),
         ("axpby", K(9), _, _, _, _, _, _, [(_, K(7)), (_, K(8))]),
         ("axpby", T(9), _, _, _, _, _, _, [(_, T(7)), (_, T(8))]),
         ("relu_ntk", K(10), K(9), _, _, 9, T(9), T(10), []),
         ("conv", K(11), K(10), 0.0, _, _, _, _, []),
         ("conv", T(11), T(10), 0.0, K(11), _, _, _, [])],
        (K(11), T(11)),
        [[], [K(1)], [], [K(3)], [K(0), K(2), K(4)], [T(2), T(4)], [], [K(6)], [T(6)],
         [K(5), T(5)], [K(7), K(8)], [T(7), T(8)], [K(9), T(9)], [K(10)], [T(10)]], 6),
    "lead": (
        [("relu", K(1), K(0), _, _, 0, _, _, []),
         ("conv", K(2), K(1), 0.0, _, _, _, _, []),
         ("axpby", K(3), _, _, _, _, _, _, [(_, K(2)), (_, K(1))]),
         ("relu_ntk", K(4), K(3), _, _, 3, K(2), T(4), []),
         ("conv", K(5), K(4), 0.0, _, _, _, _, []),
         ("conv", T(5), T(4), 0.0, K(5), _, _, _, [])],
        (K(5), T(5)),
        [[K(0)], [], [K(1)], [K(2), K(3)], [K(4)], [T(4)]], 4),
}
CASES = [(name, fusion) for name in nets() for fusion in (True, False)]


def replay(steps, given):
    """(the set dropped after each step, the peak count of live buffers, what is left) of a
    run that holds ``given`` at the start, as the executor does: outputs appear at the step
    that writes them, ``free`` goes after it"""
    live, peak, dropped = set(given), 0, []
    for st in steps:
        assert not live & set(st.writes())
        live |= set(st.writes())
        assert set(st.reads()) <= live and set(st.free) <= live
        peak = max(peak, len(live))
        live -= set(st.free)
        dropped.append(set(st.free))
    return dropped, peak, live


@pytest.mark.parametrize("name,fusion", CASES)
def test_fused_ops_are_the_parents(name, fusion):
    plan = Plan(nets()[name], 6, 6, enable_fusion=fusion)
    assert [(o.kind, o.dst, o.src, o.pre, o.pre_var, o.post, o.post_var, o.addend,
             list(o.terms)) for o in plan.pair_ops] == FORWARD[name, fusion][0]
    assert plan.final_hw == (1, 1)
    assert plan.moments_fused is (fusion and name in ("chain", "residual"))


@pytest.mark.parametrize("name,fusion", CASES)
def test_forward_list_is_the_op_list_with_the_parents_frees(name, fusion):
    plan = Plan(nets()[name], 6, 6, enable_fusion=fusion)
    steps, kbuf, tbuf = plan.layer_list()
    assert plan.layer_list()[0] is steps                     # lowered once per plan
    assert (kbuf, tbuf) == (K(plan.vf), None)
    assert len(steps) == len(plan.pair_ops)
    for st, op in zip(steps, plan.pair_ops):
        assert st.op is op and st.dst == K(op.dst)
        assert st.theta is st.dst_theta is st.addend_theta is None
        assert st.addend == (None if op.addend is None else K(op.addend))
        if op.kind == "conv":
            moments = op.pre == 2                            # CGP_PRE_MOMENTS: reads the images
            assert (st.fn, st.src, st.bias, st.var, st.terms) == \
                ("conv", None if moments else K(op.src), op.geom.bias, None, [])
        elif op.kind == "add":
            assert (st.fn, st.src, st.var, st.terms) == \
                ("axpby", None, None, [(c, K(t)) for c, t in op.terms])
        else:
            assert (st.fn, st.src, st.var, st.terms) == (op.kind, K(op.src), op.src, [])
    dropped, peak, left = replay(steps, [] if plan.moments_fused else [K(plan.v0)])
    assert dropped == [{K(v) for v in vs} for vs in FORWARD[name, fusion][1]]
    assert peak == FORWARD_PEAK[name, fusion] and left == {K(plan.vf)}


@pytest.mark.parametrize("name,fusion", CASES)
def test_ntk_list_is_the_parents(name, fusion):
    plan = Plan(nets()[name], 6, 6, enable_fusion=fusion)
    steps, kbuf, tbuf = plan.layer_list(ntk=True)
    want, final, frees, peak = NTK[name]
    assert [(s.fn, s.dst, s.src, s.bias, s.addend, s.var, s.theta, s.dst_theta, list(s.terms))
            for s in steps] == want
    assert (kbuf, tbuf) == final
    assert all(s.addend_theta is None and s.op is not None for s in steps)
    dropped, live_peak, left = replay(steps, [K(plan.v0)])
    assert dropped == [set(f) for f in frees]
    # run_layer_steps' docstring: 4 live maps on a chain, 6 inside a residual block
    assert live_peak == peak and left == set(final)
    assert plan.ntk_need_var() == {s.var for s in steps if s.var is not None}


def test_the_pinned_networks_cover_the_layer_path():
    fwd = {op[0] for ops, _f in FORWARD.values() for op in ops}
    assert fwd == {"conv", "relu", "erf", "gelu", "abrelu", "add"}
    assert {s[0] for rec in NTK.values() for s in rec[0]} == {
        "conv", "relu", "relu_ntk", "erf_ntk", "gelu_ntk", "abrelu_ntk", "axpby"}
    ops = [op for ops, _f in FORWARD.values() for op in ops]
    assert any(op[3] == 2 for op in ops) and any(op[3] == 1 for op in ops)      # pre stages
    assert any(op[5] == 1 for op in ops)                                        # ReLU post
    assert any(op[0] == "conv" and op[7] is not None for op in ops)             # conv addend
    assert any(op[0] == "relu" and op[7] is not None for op in ops)             # ReLU addend
    assert any(len(op[8]) == 3 for op in ops)
    # lead: Θ of the sum is the conv's K buffer, passed on without a launch
    assert NTK["lead"][0][3][6] == K(2)
