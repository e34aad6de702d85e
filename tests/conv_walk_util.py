"""Shared by the host and GPU tests of the layer-path conv launch (cgp_conv_* and
cgp_conv_plan_*): the geometry table of csrc/cnngp.hip, the fusion modes, a ConvArgs
builder that needs no device, and the map counts that make a capped grid walk."""
import ctypes

import numpy as np

from cnn_gp import _native as N
from oracle import nngp_oracle as O

# CGP_GEOMETRIES of csrc/cnngp.hip as (side, kernel_size, stride), padding "same": the 18
# shapes the compile-time-geometry kernel is instantiated for
GEOS = [(28, 7, 1), (28, 1, 1), (32, 1, 1), (28, 4, 1), (28, 3, 1), (28, 3, 2), (28, 1, 2),
        (14, 3, 1), (14, 3, 2), (14, 1, 2), (7, 3, 1), (32, 3, 1), (32, 3, 2), (32, 1, 2),
        (16, 3, 1), (16, 3, 2), (16, 1, 2), (8, 3, 1)]

# name -> (pre, post, addend)
GEO_MODES = {"none": (0, 0, 0), "post": (0, 1, 0), "add": (0, 0, 1), "post_add": (0, 1, 1),
             "prerelu_post": (1, 1, 0), "moments": (2, 0, 0), "moments_post": (2, 1, 0)}
# the two fusions launch_geo_mode's switch does not have: the generic kernel takes them
GENERIC_ONLY_MODES = {"prerelu": (1, 0, 0), "prerelu_post_add": (1, 1, 1)}
MODES = dict(GEO_MODES, **GENERIC_ONLY_MODES)

CAP = 3        # the capped grid of the walk tests
EINVAL = 1001


def conv_spec(k, stride=1, dilation=1, padding="same"):
    return dict(kernel_size=k, stride=stride, padding=padding, dilation=dilation,
                var_weight=2.0, var_bias=0.5)


def geometry(h, w, spec):
    """The cgp_conv_args shape fields of the oracle's Conv2d `spec` on an h x w map."""
    g = O.conv_geometry(spec)
    return dict(h=h, w=w, ho=O.conv_out_size(h, g), wo=O.conv_out_size(w, g), taps=g["k"],
                offset=-g["pad"] + (g["d"] if g["zero_row"] else 0), stride=g["s"],
                dilation=g["d"], weight=float(O.conv_weight(spec, np.float64)),
                bias=float(spec.get("var_bias", 0.0)))


FAKE = 64      # a non-NULL pointer for calls that launch nothing


def conv_args(geo, nmaps, n1, n2, mode="none", same=0, diag=0, mpb=0, flags=0, max_groups=0,
              channels=0, ptrs=None):
    """ConvArgs of one launch.  ptrs: name -> device address of the buffers the mode reads
    and writes; None fills them with a fake address (argument checks and plans only)."""
    pre, post, add = MODES[mode]
    need = ["in_", "out"] + (["in_y"] if pre == N.CGP_PRE_MOMENTS else []) \
        + (["pre_xx", "pre_yy"] if pre == N.CGP_PRE_RELU else []) \
        + (["post_xx", "post_yy"] if post else []) + (["addend"] if add else [])
    a = N.ConvArgs()
    for name in need:
        setattr(a, name, FAKE if ptrs is None else ptrs[name])
    a.nmaps, a.n1, a.n2 = nmaps, n1, n2
    a.h, a.w, a.ho, a.wo = geo["h"], geo["w"], geo["ho"], geo["wo"]
    a.taps, a.offset, a.stride, a.dilation = (geo["taps"], geo["offset"], geo["stride"],
                                              geo["dilation"])
    a.weight, a.bias = geo["weight"], geo["bias"]
    a.channels = channels if pre == N.CGP_PRE_MOMENTS else 0
    a.pre, a.post, a.same, a.diag = pre, post, same, diag
    a.maps_per_block, a.flags, a.max_groups = mpb, flags, max_groups
    return a


def plan_rc(a, dtn):
    """(return code, [kernel, maps_per_chunk, chunks, groups]) of cgp_conv_plan_<dtn>"""
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    rc = getattr(N.load(), f"cgp_conv_plan_{dtn}")(ctypes.byref(a), out)
    return rc, list(out)


def plan(a, dtn):
    rc, out = plan_rc(a, dtn)
    N.check(rc, "cgp_conv_plan")
    return out


def _walks(n, mpc, want, cap):
    chunks = -(-n // mpc)
    return chunks >= 17 and chunks % cap == want and (mpc == 1 or n % mpc != 0)


def walk_remainder(mpc, form, cap=CAP):
    """chunks % cap of the walk cases: 2 (with cap 3 the workgroups walk 6, 6 and 5 chunks
    at 17).  A same tile holds a square number of maps, and for some chunk sizes no square
    gives that remainder with a ragged last chunk (one map per chunk: squares are 0 or 1
    mod 3; four: 12t + 5 is no square); such a tile takes the remainder 1, walks of 9, 8
    and 8 at 25 chunks, and its pairs and diag forms carry the other."""
    if form == "same" and not any(_walks(n * n, mpc, 2, cap) for n in range(5, 400)):
        return 1
    return 2


def walk_counts(mpc, form, cap=CAP):
    """(nmaps, n1, n2), the smallest map count of pair form `form` whose chunks of `mpc`
    maps make `cap` workgroups walk unevenly: at least 17 chunks, chunks % cap ==
    walk_remainder(), and a ragged last chunk where a chunk holds more than one map.
      pairs     n1 x n2 with n2 >= 2 not dividing mpc: chunks straddle the rows of the tile
      diag      n pairs (i, i)
      same      an n x n tile"""
    want = walk_remainder(mpc, form, cap)
    for n in range(5, 4000):
        if form == "diag" and _walks(n, mpc, want, cap):
            return n, n, n
        if form == "same" and _walks(n * n, mpc, want, cap):
            return n * n, n, n
        if form == "pairs" and _walks(n, mpc, want, cap):
            for n2 in range(2, n // 2 + 1):
                if n % n2 == 0 and mpc % n2 != 0:
                    return n, n // n2, n2
    raise AssertionError((mpc, form))
