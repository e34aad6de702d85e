"""Identities of the one element walk (csrc/nonlin_walk.h) that hold by construction: every
nonlinearity's forward-only launch and the K' of its two-stream launch are one map function,
and the position-pair walk over 1x1 maps is the layer-path walk over one-pixel maps.  Bit
patterns are compared, so the planted NaN counts.  Inputs and launches: tools/nonlin_ab.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "tools"))

import nonlin_ab as A  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = pytest.mark.parametrize("kind", A.KINDS)
DTYPES = pytest.mark.parametrize("dtn", ["f32", "f64"])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(A.bits(a), A.bits(b))


@KINDS
@DTYPES
def test_forward_is_the_two_stream_k(kind, dtn):
    """hw = 49: 49 maps, 41 in the first workgroup and 8 in the last; 19 pairs of 5x3 maps:
    two full chunks and a partial one, straddling pairs"""
    n = 7
    for same, diag in ((0, 0), (1, 0), (0, 1), (1, 1)):
        m = A.layer_maps(n, 49, same, diag, dtn)
        for exact in A.exact_modes(kind):
            fwd, none = A.run_layer(kind, dtn, m, n, same, diag, exact=exact)
            two, theta = A.run_layer(kind, dtn, m, n, same, diag, ntk=True, exact=exact)
            assert none is None and theta.shape == fwd.shape
            assert same_bits(fwd, two), (same, diag, exact)
    h, w, nimg, pairs = A.COV_SHAPES[0]
    assert (h, w, len(pairs)) == (5, 3, 19)
    for same in (0, 1):
        m = A.cov_maps(h, w, nimg, pairs, same, dtn)
        for exact in A.exact_modes(kind):
            fwd, _ = A.run_cov(kind, dtn, m, h, w, same, exact=exact)
            two, theta = A.run_cov(kind, dtn, m, h, w, same, ntk=True, exact=exact)
            assert theta.shape == fwd.shape
            assert same_bits(fwd, two), (same, exact)


@KINDS
@DTYPES
def test_one_pixel_position_pair_maps_are_the_layer_path(kind, dtn):
    """h = w = 1 with pair m = (m // n, m % n): the layer path's maps of one pixel"""
    n = 7
    for same in (0, 1):
        m = A.layer_maps(n, 1, same, 0, dtn)
        c = dict(s=m["xy"], theta=m["theta"], xx=m["xx"], yy=m["yy"],
                 pi=np.repeat(np.arange(n, dtype=np.int32), n),
                 pj=np.tile(np.arange(n, dtype=np.int32), n))
        for exact in A.exact_modes(kind):
            for ntk in (False, True):
                layer = A.run_layer(kind, dtn, m, n, same, 0, ntk=ntk, exact=exact)
                cov = A.run_cov(kind, dtn, c, 1, 1, same, ntk=ntk, exact=exact)
                assert same_bits(layer[0], cov[0]), (same, exact, ntk)
                assert not ntk or same_bits(layer[1], cov[1]), (same, exact)
