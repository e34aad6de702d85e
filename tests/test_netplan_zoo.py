"""The lowering of networks outside the reference configs (tests/net_zoo.py), checked on
the CPU: every net's op lists, run by the numpy emulator of csrc/netfuse.hip over the
planned LDS arenas, reproduce the oracle; the library's validator accepts them and holds
no compiled program for them (the op-record interpreter runs them on the device); and two
mutations of the plans show that these inputs do reach the halo zeroing and the zero-row
rewrite — the emulator walks every pair of a tile through one arena per pair slot, so
stale cells of earlier pairs are there to be read, as in a workgroup that walks a second
group."""
import ctypes
import functools

import numpy as np
import pytest

import configs_util
import net_emulator as E
import net_zoo
from cnn_gp import _native as N
from cnn_gp.netplan import NetPlan
from cnn_gp.program import Plan
from oracle import nngp_oracle as O

ZOO = net_zoo.zoo()
RTOL = 1e-13               # test_netplan.py's bound for the reference configs


def plan_of(name, itemsize=8):
    """a fresh NetPlan (the mutation tests edit its records in place)"""
    z = ZOO[name]
    return NetPlan(Plan(z.build(), z.side, z.side), itemsize)


@functools.lru_cache(maxsize=None)
def inputs(name):
    z = ZOO[name]
    rng = np.random.default_rng(sorted(ZOO).index(name))
    X = rng.random((6, z.channels, z.side, z.side))
    Z = rng.random((5, z.channels, z.side, z.side))
    X.setflags(write=False)
    Z.setflags(write=False)
    return X, Z


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(Kxx, Kxz) of the oracle, computed once per net and left unchanged"""
    X, Z = inputs(name)
    spec = configs_util.spec_of(ZOO[name].build())
    kxx, kxz = O.kernel(spec, X), O.kernel(spec, X, Z, False, False)
    kxx.setflags(write=False)
    kxz.setflags(write=False)
    return kxx, kxz


@pytest.mark.parametrize("itemsize", [8, 4])
@pytest.mark.parametrize("name", net_zoo.NAMES)
def test_zoo_emulated_plan_matches_oracle(name, itemsize):
    """6 images (same) and 6 x 5: every arena is reused by several pairs"""
    net = plan_of(name, itemsize)
    assert ZOO[name].feature(net), (ZOO[name].purpose, net_zoo.layout(net))
    X, Z = inputs(name)
    kxx, kxz = oracle(name)
    np.testing.assert_allclose(E.kernel(net, X, X, True), kxx, rtol=RTOL)
    np.testing.assert_allclose(E.kernel(net, X, Z, False), kxz, rtol=RTOL)


@pytest.mark.parametrize("itemsize", [8, 4])
@pytest.mark.parametrize("name", net_zoo.NAMES)
def test_zoo_stages_validate_and_have_no_compiled_program(name, itemsize):
    """cgp_net_validate accepts every stage, and cgp_net_program knows none of them: on
    the device the zoo runs in the op-record interpreter"""
    lib = N.load()
    net = plan_of(name, itemsize)
    for st in net.stages:
        arr = net._ops_array(st, None)
        assert lib.cgp_net_validate(ctypes.byref(arr), st.n_ops, st.pairs) == 0
        E.validate(st)
        flags = N.CGP_FLAG_NET_DUAL if st.dual else 0
        assert lib.cgp_net_program(ctypes.byref(arr), st.n_ops, st.pairs, flags,
                                   st.lds_elems, itemsize) == 0


def _relative_shift(a, b):
    return np.abs(a - b) / np.abs(b)


# one net per stage shape whose halo zeroings sit in a stage of that shape; in `nested` a
# 14x14 value takes cells that the same pair's 28x28 maps wrote, so there even the first
# pair needs the zeroing
ZERO_HALO_CASES = [("to16blocks", 2, True), ("nested", 2, False), ("to14blocks", 4, True),
                   ("in14", 16, True)]


@pytest.mark.parametrize("name,npairs,first_exact", ZERO_HALO_CASES)
def test_dropping_halo_zeroings_is_seen_from_the_second_pair_on(name, npairs, first_exact):
    """without the planner's zero / zero2 marks in the stages of ``npairs`` pairs per
    workgroup the first pair, on freshly zeroed arenas, is still right, and a later pair
    of the same arena reads an earlier pair's data as padding: the zoo's inputs reach
    cgp_net_op.zero_halo, and only a walk past the first group can see it"""
    net = plan_of(name)
    dropped = 0
    for st in net.stages:
        if st.pairs == npairs:
            for f, _ in st.records:
                dropped += ("zero" in f) + ("zero2" in f)
                f.pop("zero", None)
                f.pop("zero2", None)
    assert dropped, net_zoo.layout(net)
    X, Z = inputs(name)
    _, kxz = oracle(name)
    shift = _relative_shift(E.kernel(net, X, Z, False), kxz)
    if first_exact:
        assert shift[0, 0] <= RTOL
    assert shift.reshape(-1)[1:].max() > 1e-6, shift.max()


@pytest.mark.parametrize("name", ["mix74", "mix47sum"])
def test_forcing_hs_clean_on_dirty_convs_is_seen(name):
    """CGP_NET_CODE_HS_CLEAN on the convs the planner left dirty: the column pass reads the
    other geometry's row sums where zero rows belong.  Separable convs exist at 28x28 only
    (one pair per workgroup or half), so this mutation has no multi-pair case."""
    net = plan_of(name)
    dirty = net_zoo.dirty_convs(net)
    assert dirty
    for f in dirty:
        f["code"] |= N.CGP_NET_CODE_HS_CLEAN
    X, Z = inputs(name)
    _, kxz = oracle(name)
    assert _relative_shift(E.kernel(net, X, Z, False), kxz).max() > 1e-6
