"""Networks outside the reference configs that the whole-network kernel (csrc/netfuse.hip)
must run through its op-record interpreter, defined once for the CPU tests
(test_netplan_zoo.py) and the device tests (test_gpu_netfuse_zoo.py).

Every entry names what it is in the zoo for and a predicate over ``NetPlan.stages`` that
says so in code: both test files assert it, so a planner change that lowers a network
differently — and with that loses the coverage — fails there instead of passing on
another path.  The predicates describe the lowering with the first stage on two pairs per
workgroup (netplan.FIRST_PAIRS = "2", the default).
"""
from __future__ import annotations

import collections

import torch

try:
    from cnn_gp import _native as N
except ImportError:        # imported beside the reference's package (golden/make_golden.py):
    N = None               # only the builders are used there

Net = collections.namedtuple("Net", "build channels side purpose feature")

# geometry rows (h, w, ho, wo, taps, stride, offset) of csrc/netfuse.hip's table
ROW_28_TO_14_POINT = (28, 28, 14, 14, 1, 2, 0)
ROW_32_REDUCE = (32, 32, 1, 1, 32, 1, 0)


# -- what a lowered stage holds -----------------------------------------------------------
def _recs(st):
    return [f for f, _ in st.records]


def _convs(st):
    return [f for f in _recs(st) if f["kind"] == N.CGP_NET_CONV]


def _kinds(st):
    return [f["kind"] for f in _recs(st)]


def is_reduction(f):
    h, w, ho, wo, taps, s, off = f["geom"]
    return ho == wo == 1 and off == 0 and taps == h == w


def is_separable(f):
    """a conv that goes through the row-sum scratch: more than 3 taps, not a reduction"""
    h, w, ho, wo, taps, s, off = f["geom"]
    return taps > 3 and not is_reduction(f)


def pairs(net):
    return [st.pairs for st in net.stages]


def dirty_convs(net):
    """separable convs that rewrite their scratch zero rows (no CGP_NET_CODE_HS_CLEAN)"""
    return [f for st in net.stages for f in _convs(st)
            if is_separable(f) and not f["code"] & N.CGP_NET_CODE_HS_CLEAN]


def clean_convs(net):
    return [f for st in net.stages for f in _convs(st)
            if is_separable(f) and f["code"] & N.CGP_NET_CODE_HS_CLEAN]


def sum_pairs(net):
    """CGP_NET_CODE_SUM convs directly followed by their CGP_NET_CODE_FROM_SUM reduction"""
    n = 0
    for st in net.stages:
        r = _recs(st)
        for a, b in zip(r, r[1:]):
            if a["kind"] == b["kind"] == N.CGP_NET_CONV and a["code"] & N.CGP_NET_CODE_SUM \
                    and b["code"] & N.CGP_NET_CODE_FROM_SUM:
                n += 1
    return n


def halo_zeroings(net, stage=None):
    """ops that zero a slot's halo before they write it (cgp_net_op.zero_halo)"""
    sts = net.stages if stage is None else [net.stages[stage]]
    return sum(("zero" in f) + ("zero2" in f) for st in sts for f in _recs(st))


def dual_outputs(net):
    return sum(f.get("dst2", -1) >= 0 for st in net.stages for f in _recs(st))


def linears(net, npairs):
    """LINEAR ops in the stages with ``npairs`` pairs per workgroup"""
    return [f for st in net.stages if st.pairs == npairs for f in _recs(st)
            if f["kind"] == N.CGP_NET_LINEAR]


def head_is_moments_only(net):
    return set(_kinds(net.stages[0])) == {N.CGP_NET_MOMENTS, N.CGP_NET_STORE}


def rows(net):
    return {f["geom"] for st in net.stages for f in _convs(st)}


def ends_in_reduction(net, npairs, side):
    st = net.stages[-1]
    last = _recs(st)[-1]
    return st.pairs == npairs and last["kind"] == N.CGP_NET_CONV and is_reduction(last) and \
        last["geom"][0] == side


def has_addend_conv(net):
    return any(f["add"] >= 0 for st in net.stages for f in _convs(st))


# -- the architectures --------------------------------------------------------------------
def zoo(m=None):
    """name -> Net(build, channels, side, purpose, feature).  ``build()`` returns a fresh
    float64 model (a float32 Mixture logit alone moves the kernel by 3e-8) made from the
    module namespace ``m`` (default: the package under test); ``feature(NetPlan)`` is true
    while the lowering still reaches what ``purpose`` names."""
    if m is None:
        import cnn_gp as m
    C, R, S = m.Conv2d, m.ReLU, m.Sequential

    def blk():
        return m.resnet_block(1, False, 1)

    def pblk(s):
        return m.resnet_block(s, True, 1)

    def ident():
        return S()

    def t(*v):      # created in float32 like the reference's default, cast with the model
        return torch.tensor(v, dtype=torch.float32)

    def mix74():
        return S(C(7, var_bias=.2), R(), C(4, var_weight=2), R(), C(7), R(),
                 C(28, padding=0))

    def mix47sum():
        return S(C(4, var_bias=.2), R(), m.Sum([ident(), S(C(7), R())]),
                 C(4, var_weight=2), R(), C(28, padding=0))

    def to14blocks():
        return S(C(3), pblk(2), blk(), blk(), R(), C(14, padding=0))

    def to16blocks():
        return S(C(3), pblk(1), pblk(2), blk(), R(), C(16, padding=0))

    def in14():
        return S(C(3), blk(), pblk(2), blk(), R(), C(7, padding=0))

    def in16mix3():
        return S(C(3, var_bias=.1),
                 m.Mixture([ident(), S(R(), C(3)), S(R(), C(3, var_bias=.2))], t(.4, -.3, .2)),
                 pblk(2), blk(), R(), C(8, padding=0))

    def in8mix():
        return S(C(3), m.Mixture([ident(), S(R(), C(3))], t(.4, -.3)), R(), C(8, padding=0))

    def in7():
        return S(C(3, var_bias=.1), blk(), blk(), R(), C(7, padding=0))

    def nested():
        return S(C(3),
                 m.Sum([ident(), S(R(), C(3), m.Sum([ident(), S(R(), C(3, var_bias=.2))]))]),
                 R(), C(1, stride=2), R(), C(3), R(), C(14, padding=0))

    def short_tail():
        return S(C(3), R(), C(3, stride=2), R(), C(3, stride=2), R(), C(7, padding=0))

    def red32():
        return S(C(3, var_bias=.3), R(), C(1, var_weight=1.5), R(), C(32, padding=0))

    def only_reduce():
        return S(C(28, padding=0, var_bias=.5))

    def px1():
        return S(C(1), R(), C(1, var_bias=.3))

    def dbl(build):
        return lambda: build().double()

    entries = {
        "mix74": (mix74, 1, 28, "two separable convs that rewrite their scratch zero rows, "
                  "one clean conv, a SUM / FROM_SUM pair",
                  lambda n: len(dirty_convs(n)) >= 2 and len(clean_convs(n)) >= 1
                  and sum_pairs(n) == 1),
        "mix47sum": (mix47sum, 1, 28, "as mix74, with an addend on a separable conv",
                     lambda n: len(dirty_convs(n)) >= 2 and len(clean_convs(n)) >= 1
                     and sum_pairs(n) == 1 and has_addend_conv(n)),
        "to14blocks": (to14blocks, 1, 28, "stages [2, 4]; the 14x14 -> 1 reduction ends the "
                       "4-pair stage; three dual outputs",
                       lambda n: pairs(n) == [2, 4] and ends_in_reduction(n, 4, 14)
                       and dual_outputs(n) >= 3),
        "to16blocks": (to16blocks, 3, 32, "stages [2, 4]; the 16x16 -> 1 reduction ends the "
                       "4-pair stage; halo zeroings in both stages",
                       lambda n: pairs(n) == [2, 4] and ends_in_reduction(n, 4, 16)
                       and halo_zeroings(n, 0) >= 1 and halo_zeroings(n, 1) >= 1),
        "in14": (in14, 1, 14, "stages [2, 4, 16] with a head of MOMENTS + STORE only; halo "
                 "zeroings in the multi-pair stages",
                 lambda n: pairs(n) == [2, 4, 16] and head_is_moments_only(n)
                 and halo_zeroings(n) >= 1),
        "in16mix3": (in16mix3, 2, 16, "stages [2, 4, 16]; two LINEAR ops in the 4-pair stage",
                     lambda n: pairs(n) == [2, 4, 16] and head_is_moments_only(n)
                     and len(linears(n, 4)) >= 2),
        "in8mix": (in8mix, 1, 8, "stages [2, 16]; a LINEAR op in the 16-pair stage",
                   lambda n: pairs(n) == [2, 16] and head_is_moments_only(n)
                   and len(linears(n, 16)) >= 1),
        "in7": (in7, 1, 7, "stages [2, 16] with a head of MOMENTS + STORE only",
                lambda n: pairs(n) == [2, 16] and head_is_moments_only(n)),
        "nested": (nested, 1, 28, "one stage; 14x14 values in reused 28x28 slots with halo "
                   "zeroings; a generic LINEAR; the 1x1 stride-2 conv",
                   lambda n: pairs(n) == [2] and halo_zeroings(n) >= 3
                   and len(linears(n, 2)) >= 1 and ROW_28_TO_14_POINT in rows(n)),
        "short_tail": (short_tail, 1, 28, "a 7x7 tail shorter than MIN_STAGE_OPS stays in "
                       "the head stage",
                       lambda n: pairs(n) == [2] and (7, 7, 1, 1, 7, 1, 0) in rows(n)),
        "red32": (red32, 3, 32, "the 32x32 -> 1 reduction row",
                  lambda n: ROW_32_REDUCE in rows(n)),
        "only_reduce": (only_reduce, 1, 28, "a network that is the moments and one reduction",
                        lambda n: len(n.stages) == 1 and
                        _kinds(n.stages[0]) == [N.CGP_NET_MOMENTS, N.CGP_NET_CONV]),
        "px1": (px1, 4, 1, "1x1 maps", lambda n: rows(n) == {(1, 1, 1, 1, 1, 1, 0)}),
    }
    return {k: Net(dbl(b), c, s, p, f) for k, (b, c, s, p, f) in entries.items()}


NAMES = list(zoo())


def layout(net):
    """the stage layout as text: pairs per workgroup and op kinds of every stage"""
    names = {N.CGP_NET_CONV: "conv", N.CGP_NET_RELU: "relu", N.CGP_NET_MOMENTS: "moments",
             N.CGP_NET_LINEAR: "linear", N.CGP_NET_LOAD: "load", N.CGP_NET_STORE: "store"}
    return " | ".join(f"{st.pairs}: " + " ".join(names[k] for k in _kinds(st))
                      for st in net.stages)
