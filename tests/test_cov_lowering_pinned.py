"""CPU-only: the lowering onto position-pair maps (program.pool_steps, pool_ntk_steps), pinned
step by step to what the commit before the two lists shared one record type (Step) and one
scheduling helper gave.  The literals were recorded there; on that commit a forward step had no
``bias`` of its own, and the geometry's (op.geom.bias of a conv or corrconv step, None
elsewhere) was recorded in its place.

Two networks at 6x6 hit every ``fn`` of both lists, a fused addend, the ("pre", d) buffer of
the launch-by-launch sequence, the self pass and "accum"."""
import pytest

import cnn_gp
from cnn_gp.program import compile_program, pool_ntk_steps, pool_steps

m = cnn_gp
S, C, R, E, GE, G, A, CC = (m.Sequential, m.Conv2d, m.ReLU, m.Erf, m.Gelu, m.GlobalAvgPool,
                            m.AvgPool2d, m.CorrelatedConv2d)


def nets():
    """name -> (model, body)"""
    return {
        "residual_gap": (S(C(3, var_bias=.1), R(), A(2), m.Sum([S(C(3), R(), C(3)), S()]), R(),
                           G(), C(1)), False),
        "corr_body": (S(C(3), GE(), CC(3, lengthscale=1.), E(),
                        CC(6, padding=0, lengthscale=1.)), True),
    }


def forward_record(ps):
    return dict(steps=[(st.fn, st.dst, st.src, st.post, st.var, st.addend, st.bias,
                        list(st.terms), list(st.free)) for st in ps.steps],
                peak=ps.peak, self_var=sorted(ps.self_var), self_last=ps.self_last)


def ntk_record(ns):
    return dict(steps=[(st.fn, st.dst, st.src, st.post, st.var, st.addend, st.bias, st.theta,
                        st.dst_theta, st.addend_theta, list(st.terms), list(st.free))
                       for st in ns.steps],
                peak=ns.peak, final=ns.final, final_theta=ns.final_theta)


def K(v):
    return ("K", v)


def T(v):
    return ("T", v)


_ = None
PRE7 = ("pre", 7)

# forward: (fn, dst, src, post, var, addend, bias, terms, free)
# ntk:     (fn, dst, src, post, var, addend, bias, theta, dst_theta, addend_theta, terms, free)
PINNED = {
    ("residual_gap", "forward"): dict(
        steps=[
            ("moments", 0, _, 0, _, _, _, [], []),
            ("conv", 2, 0, 1, 1, _, 0.1, [], [0]),
            ("avgpool", 3, 2, 0, _, _, _, [], [2]),
            ("conv", 4, 3, 0, _, _, 0.0, [], []),
            ("nonlin", 5, 4, 1, 4, _, _, [], [4]),
            ("conv", 7, 5, 0, _, 3, 0.0, [], [3, 5]),
            ("nonlin", 8, 7, 1, 7, _, _, [], [7]),
            ("pool", 9, 8, 0, _, _, _, [], [8]),
            ("conv", 10, 9, 0, _, _, 0.0, [], [9]),
        ],
        peak=2592, self_var=[4, 7], self_last=5),
    ("residual_gap", "ntk_fused"): dict(
        steps=[
            ("moments", K(0), _, 0, _, _, _, _, _, _, [], []),
            ("conv_ntk", K(2), K(0), 1, 1, _, 0.1, _, T(2), _, [], [K(0)]),
            ("avgpool", K(3), K(2), 0, _, _, _, _, _, _, [], [K(2)]),
            ("avgpool", T(3), T(2), 0, _, _, _, _, _, _, [], [T(2)]),
            ("conv_ntk", K(4), K(3), 0, _, _, 0.0, T(3), T(4), _, [], []),
            ("nonlin_ntk", K(5), K(4), 1, 4, _, _, T(4), T(5), _, [], [K(4), T(4)]),
            ("conv_ntk", K(7), K(5), 0, _, K(3), 0.0, T(5), T(7), T(3), [], [K(3), K(5), T(3),
             T(5)]),
            ("nonlin_ntk", K(8), K(7), 1, 7, _, _, T(7), T(8), _, [], [K(7), T(7)]),
            ("pool", K(9), K(8), 0, _, _, _, _, _, _, [], [K(8)]),
            ("pool", T(9), T(8), 0, _, _, _, _, _, _, [], [T(8)]),
            ("conv_ntk", K(10), K(9), 0, _, _, 0.0, T(9), T(10), _, [], [K(9), T(9)]),
        ],
        peak=3888, final=K(10), final_theta=T(10)),
    ("residual_gap", "ntk_unfused"): dict(
        steps=[
            ("moments", K(0), _, 0, _, _, _, _, _, _, [], []),
            ("conv", K(1), K(0), 0, _, _, 0.1, _, _, _, [], [K(0)]),
            ("nonlin_ntk", K(2), K(1), 1, 1, _, _, K(1), T(2), _, [], [K(1)]),
            ("avgpool", K(3), K(2), 0, _, _, _, _, _, _, [], [K(2)]),
            ("avgpool", T(3), T(2), 0, _, _, _, _, _, _, [], [T(2)]),
            ("conv", K(4), K(3), 0, _, _, 0.0, _, _, _, [], []),
            ("conv", T(4), T(3), 0, _, K(4), 0.0, _, _, _, [], []),
            ("nonlin_ntk", K(5), K(4), 1, 4, _, _, T(4), T(5), _, [], [K(4), T(4)]),
            ("conv", K(PRE7), K(5), 0, _, _, 0.0, _, _, _, [], [K(5)]),
            ("conv", T(PRE7), T(5), 0, _, K(PRE7), 0.0, _, _, _, [], [T(5)]),
            ("axpby", K(7), _, 0, _, _, _, _, _, _, [(_, K(PRE7)), (_, K(3))], [K(PRE7), K(3)]),
            ("axpby", T(7), _, 0, _, _, _, _, _, _, [(_, T(PRE7)), (_, T(3))], [T(PRE7), T(3)]),
            ("nonlin_ntk", K(8), K(7), 1, 7, _, _, T(7), T(8), _, [], [K(7), T(7)]),
            ("pool", K(9), K(8), 0, _, _, _, _, _, _, [], [K(8)]),
            ("pool", T(9), T(8), 0, _, _, _, _, _, _, [], [T(8)]),
            ("conv", K(10), K(9), 0, _, _, 0.0, _, _, _, [], [K(9)]),
            ("conv", T(10), T(9), 0, _, K(10), 0.0, _, _, _, [], [T(9)]),
        ],
        peak=3888, final=K(10), final_theta=T(10)),
    ("corr_body", "forward"): dict(
        steps=[
            ("moments", 0, _, 0, _, _, _, [], []),
            ("conv", 1, 0, 0, _, _, 0.0, [], [0]),
            ("gelu", 2, 1, 0, 1, _, _, [], [1]),
            ("corrconv", 3, 2, 0, _, _, 0.0, [], [2]),
            ("nonlin", 4, 3, 2, 3, _, _, [], [3]),
            ("corrconv", 5, 4, 0, _, _, 0.0, [], [4]),
        ],
        peak=2592, self_var=[3], self_last=3),
    # no conv here has a Θ input, a nonlinearity or an addend: both lowerings are one list
    ("corr_body", "ntk_fused"): dict(
        steps=[
            ("moments", K(0), _, 0, _, _, _, _, _, _, [], []),
            ("conv", K(1), K(0), 0, _, _, 0.0, _, _, _, [], [K(0)]),
            ("nonlin_ntk", K(2), K(1), 3, 1, _, _, K(1), T(2), _, [], [K(1)]),
            ("corrconv", K(3), K(2), 0, _, _, 0.0, _, _, _, [], [K(2)]),
            ("corrconv", T(3), T(2), 0, _, _, 0.0, _, _, _, [], [T(2)]),
            ("accum", T(3), K(3), 0, _, _, _, _, _, _, [], []),
            ("nonlin_ntk", K(4), K(3), 2, 3, _, _, T(3), T(4), _, [], [K(3), T(3)]),
            ("corrconv", K(5), K(4), 0, _, _, 0.0, _, _, _, [], [K(4)]),
            ("corrconv", T(5), T(4), 0, _, _, 0.0, _, _, _, [], [T(4)]),
            ("accum", T(5), K(5), 0, _, _, _, _, _, _, [], []),
        ],
        peak=5184, final=K(5), final_theta=T(5)),
}
PINNED["corr_body", "ntk_unfused"] = PINNED["corr_body", "ntk_fused"]


@pytest.mark.parametrize("name", list(nets()))
def test_forward_lowering_is_the_parents(name):
    model, body = nets()[name]
    prog, v0, vf = compile_program(model, 6, 6)
    assert forward_record(pool_steps(prog, v0, vf, body)) == PINNED[name, "forward"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", list(nets()))
def test_two_stream_lowering_is_the_parents(name, fused):
    model, body = nets()[name]
    prog, v0, vf = compile_program(model, 6, 6)
    ns = pool_ntk_steps(prog, v0, vf, body=body, fused=fused, itemsize=8)
    assert ntk_record(ns) == PINNED[name, "ntk_fused" if fused else "ntk_unfused"]
    assert ns.fused is fused
    assert forward_record(ns.forward) == PINNED[name, "forward"]


def test_the_pinned_networks_cover_every_launch():
    fwd = {st[0] for (_n, kind), rec in PINNED.items() if kind == "forward"
           for st in rec["steps"]}
    two = {st[0] for (_n, kind), rec in PINNED.items() if kind != "forward"
           for st in rec["steps"]}
    assert fwd == {"moments", "conv", "nonlin", "gelu", "pool", "avgpool", "corrconv"}
    assert two == fwd - {"gelu", "nonlin"} | {"conv_ntk", "nonlin_ntk", "accum", "axpby"}
    unfused = PINNED["residual_gap", "ntk_unfused"]["steps"]
    assert any(st[1] == K(PRE7) for st in unfused)
    assert any(st[0] == "conv_ntk" and st[5] is not None and st[9] is not None
               for st in PINNED["residual_gap", "ntk_fused"]["steps"])
