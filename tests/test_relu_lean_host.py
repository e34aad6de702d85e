"""cgp_net_program_lean (include/cnngp.h): which ReLU sites of a compiled fp64 program run
cap-free and add-free (csrc/netfuse.hip prog_lean, DESIGN §4.1 "Round 8"), and the condition
on the launch's CONV records under which a workgroup takes that lean chain.  Host only: the
library loads without a GPU.

Op numbers below are those of csrc/net_programs.h (op 0 is the MOMENTS op or a LOAD)."""
import ctypes
import importlib
import math

import pytest
import torch

from cnn_gp import _native as N

CONFIGS = ["mnist_paper_convnet_gp", "mnist_paper_residual_cnn_gp", "mnist_as_tf", "cifar10"]


def stage_records(m, side, dt=torch.float64):
    """[(stage, op records with the model's weights and null pointers, flags, itemsize)]"""
    itemsize = torch.tensor([], dtype=dt).element_size()
    net = m._net_plan(m._plan(side, side), itemsize)
    assert net is not None
    return [(st, net._ops_array(st, None), N.CGP_FLAG_NET_DUAL if st.dual else 0, itemsize)
            for st in net.stages]


def program(st, arr, flags, itemsize):
    return N.load().cgp_net_program(ctypes.byref(arr), st.n_ops, st.pairs, flags, st.lds_elems,
                                    itemsize)


def lean(st, arr, flags, itemsize):
    """(return value, capfree, addfree); the counts are -1 where the library wrote none"""
    cap, add = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = N.load().cgp_net_program_lean(ctypes.byref(arr), st.n_ops, st.pairs, flags,
                                       st.lds_elems, itemsize, ctypes.byref(cap),
                                       ctypes.byref(add))
    return rc, cap.value, add.value


def model_lean(m, side):
    """cgp_net_program_lean of every fp64 stage of a model, on the model's own weights"""
    return [lean(*s) for s in stage_records(m, side)]


def config(name, dt=torch.float64):
    cfg = importlib.import_module(f"configs.{name}")
    importlib.reload(cfg)
    return cfg.initial_model.to(dt), 32 if getattr(cfg, "in_channels", 1) == 3 else 28


def convs(arr):
    return [o for o in arr if o.kind == N.CGP_NET_CONV]


# (capfree, addfree) per stage with every CONV record passing the condition.
EXPECTED = {
    # ops 1-7 are conv+ReLU: all cap-free.  Op 1 reads the MOMENTS map (signed images): it
    # keeps its add.  Ops 2-7 read the previous ReLU's output, have no addend and no dst2,
    # and their maps are read only by the next conv as `src` (op 7's, never stored, by the
    # FROM_SUM reduction): add-free, stored halved.
    "mnist_paper_convnet_gp": [(7, 6)],
    # ops 1-9 are conv+ReLU: cap-free.  Ops 1-8 add their own source slot, which starts as
    # the signed MOMENTS map, so the slot never becomes provably non-negative; op 9 reads
    # that slot: no add-free site.
    "mnist_paper_residual_cnn_gp": [(9, 0)],
    # The ResNets' programs keep the default chain only, so no site even where the records
    # pass the condition: their head stage has dual outputs (a second chain beside the
    # default one measured slower on the reference ResNets, whose convs have var_bias = 0 and
    # so never take it) and their other stages run 4 / 16 pairs per workgroup.
    "mnist_as_tf": [(0, 0), (0, 0), (0, 0)],
    "cifar10": [(0, 0), (0, 0), (0, 0)],
}


@pytest.mark.parametrize("name", CONFIGS)
def test_reference_configs_sites(name):
    """Every fp64 stage of the reference configs, with the config's own weights and — for
    the two ResNets, whose convs have var_bias = 0, so that the cap is live and the
    condition fails on their own records — with every conv's bias set to 1."""
    m, side = config(name)
    stages = stage_records(m, side)
    assert len(stages) == len(EXPECTED[name])
    for (st, arr, flags, itemsize), want in zip(stages, EXPECTED[name]):
        pid = program(st, arr, flags, itemsize)
        assert pid > 0
        assert any(o.relu for o in convs(arr))          # every stage has a conv+ReLU
        own_bias = [o.bias for o in convs(arr)]
        got = lean(st, arr, flags, itemsize)
        if min(own_bias) >= 2.0 ** -60:
            assert got == (1,) + want, (name, got)
        else:
            assert name in ("mnist_as_tf", "cifar10") and max(own_bias) == 0.0
            assert got == (0, -1, -1), (name, got)
            for o in convs(arr):
                o.bias = 1.0
            assert lean(st, arr, flags, itemsize) == (1,) + want, name
        assert program(st, arr, flags, itemsize) == pid


def test_convnet_counts():
    """the headline config: 7 cap-free and 6 add-free sites"""
    m, side = config("mnist_paper_convnet_gp")
    assert model_lean(m, side) == [(1, 7, 6)]


def test_condition_on_the_records():
    """bias 0, bias 2^-61, one negative / inf / NaN weight, a weight or bias above 2^60: 0;
    the limits themselves: 1; cgp_net_program returns the same id throughout"""
    m, side = config("mnist_paper_convnet_gp")
    (st, arr, flags, itemsize), = stage_records(m, side)
    pid = program(st, arr, flags, itemsize)
    assert pid > 0 and lean(st, arr, flags, itemsize) == (1, 7, 6)
    own = [(o.weight, o.bias) for o in arr]

    def restore():
        for o, (w, b) in zip(arr, own):
            o.weight, o.bias = w, b

    def check(want):
        assert lean(st, arr, flags, itemsize)[0] == want
        assert program(st, arr, flags, itemsize) == pid

    for b in (0.0, 2.0 ** -61, -1.0, math.inf, math.nan, 2.0 ** 61):
        for o in convs(arr):
            o.bias = b
        check(0)
        restore()
        convs(arr)[2].bias = b                 # one record is enough
        check(0)
        restore()
    for w in (-1.0, -2.0 ** -80, math.inf, -math.inf, math.nan, 2.0 ** 61):
        convs(arr)[3].weight = w
        check(0)
        restore()
    for o in convs(arr):                       # the limits are inside
        o.weight, o.bias = 0.0, 2.0 ** -60
    check(1)
    for o in convs(arr):
        o.weight, o.bias = 2.0 ** 60, 2.0 ** 60
    check(1)
    restore()
    arr[0].weight, arr[0].bias = -1.0, 0.0     # not a CONV record (MOMENTS): not looked at
    check(1)
    restore()
    check(1)
    # NULL count pointers are allowed
    assert N.load().cgp_net_program_lean(ctypes.byref(arr), st.n_ops, st.pairs, flags,
                                         st.lds_elems, itemsize, None, None) == 1


def test_fp32_dual_and_exact_have_no_lean_chain():
    """fp32 records, the records with CGP_FLAG_NET_DUAL (no program matches them then) and
    CGP_FLAG_EXACT_RELU launches (they run the interpreter): 0"""
    m, side = config("mnist_paper_convnet_gp", torch.float32)
    (st, arr, flags, itemsize), = stage_records(m, side, torch.float32)
    assert itemsize == 4 and program(st, arr, flags, itemsize) > 0
    assert lean(st, arr, flags, itemsize) == (0, -1, -1)
    m, side = config("mnist_paper_convnet_gp")
    (st, arr, flags, itemsize), = stage_records(m, side)
    assert flags == 0
    assert lean(st, arr, N.CGP_FLAG_NET_DUAL, itemsize) == (0, -1, -1)
    assert lean(st, arr, N.CGP_FLAG_EXACT_RELU, itemsize) == (0, -1, -1)
    assert lean(st, arr, flags, 4) == (0, -1, -1)
    arr[3].dst += 1                            # no program: 0
    assert program(st, arr, flags, itemsize) == 0
    assert lean(st, arr, flags, itemsize) == (0, -1, -1)
