"""The networks and op geometries of the tapconv goldens, written against the constructor
surface the reference and this package share: ``build(lib, name, side)`` makes the network
with either package passed as ``lib`` and names the Conv2d modules whose kernel buffers the
goldens overwrite, in the order of their tables.  tests/golden/
make_golden_tapconv.py runs them through the reference; the tests through this package."""
from __future__ import annotations

import itertools

import numpy as np
import torch

NETS = ("chain", "stride2", "dil2", "even4", "sum", "mixture", "readout", "mixed")
SIDES = (8, 14)
CHANNELS = 2


def build(lib, name, side):
    """(model, indices into model.modules()'s Conv2d list of the tapped convs)"""
    C, R, S = lib.Conv2d, lib.ReLU, lib.Sequential
    if name == "chain":
        return S(C(3, var_weight=2.0, var_bias=0.1), R(), C(3, var_weight=1.5, var_bias=0.2), R(),
                 C(side, padding=0, var_bias=0.05)), (0, 1)
    if name == "stride2":
        return S(C(3, stride=2, var_weight=2.0, var_bias=0.1), R(),
                 C(side // 2, padding=0, var_bias=0.05)), (0,)
    if name == "dil2":
        return S(C(3, dilation=2, var_weight=2.0, var_bias=0.1), R(),
                 C(side, padding=0, var_bias=0.05)), (0,)
    if name == "even4":
        return S(C(4, var_weight=2.0, var_bias=0.1), R(),
                 C(side, padding=0, var_bias=0.05)), (0,)
    if name == "sum":
        return S(C(3, var_weight=2.0, var_bias=0.1),
                 lib.Sum([S(), S(R(), C(3, var_weight=2.0, var_bias=0.1))]), R(),
                 C(side, padding=0, var_bias=0.05)), (0, 1)
    if name == "mixture":
        return S(C(3, var_weight=2.0, var_bias=0.1),
                 lib.Mixture([S(R(), C(3, var_weight=2.0)), S(R(), C(5, var_weight=1.0))],
                             logit_proportions=torch.tensor([0.3, -0.2])), R(),
                 C(side, padding=0, var_bias=0.05)), (0, 1, 2)
    if name == "readout":
        return S(C(3, var_weight=2.0, var_bias=0.1), R(),
                 C(side, padding=0, var_bias=0.05)), (1,)
    if name == "mixed":
        return S(C(3, var_weight=2.0, var_bias=0.1), R(), C(3, var_weight=2.0), R(),
                 C(3, stride=2, var_weight=2.0, var_bias=0.1), R(),
                 C(side // 2, padding=0, var_bias=0.05)), (0, 2)
    raise KeyError(name)


def convs(lib, model):
    return [m for m in model.modules() if isinstance(m, lib.Conv2d)]


def random_table(mod, rng):
    """a non-negative float32 table of the buffer's shape with the box's mean"""
    ke = mod.kernel.shape[-1]
    scale = 2.0 * float(mod.var_weight) / ke ** 2
    return (rng.random((ke, ke), dtype=np.float32) * np.float32(scale)).astype(np.float32)


def set_tables(lib, model, which, tables):
    """overwrite the kernel buffers of the tapped convs, in place, keeping dtype and device"""
    cs = convs(lib, model)
    with torch.no_grad():
        for i, tab in zip(which, tables):
            k = cs[i].kernel
            k.copy_(torch.as_tensor(np.asarray(tab)).to(k.dtype).reshape(k.shape))
    return model


def op_cases():
    """(k, stride, padding, dilation, side, mode): mode 'pos' non-negative, 'mixed' with zero
    and negative entries, 'full' an even "same" buffer with its first row and column written"""
    rng = np.random.default_rng(4321)
    grid = [c for c in itertools.product([1, 2, 3, 4, 5, 7], [1, 2], ["same", 0, 1], [1, 2],
                                         [7, 8, 14, 28])
            # a padding beyond the taps' span leaves border outputs with no tap in the map
            if not (c[2] == 1 and c[3] * (c[0] - 1) < 1)]
    sel = [grid[i] for i in rng.choice(len(grid), size=36, replace=False)]
    cases = [c + (("pos", "mixed")[n % 2],) for n, c in enumerate(sel)]
    cases += [(28, 1, 0, 1, 28, "mixed"), (28, 1, 0, 1, 28, "pos"), (4, 1, "same", 1, 8, "full"),
              (2, 1, "same", 2, 14, "full"), (7, 1, "same", 1, 28, "pos"),
              (3, 1, "same", 1, 28, "mixed"), (3, 2, "same", 1, 14, "pos"),
              (7, 1, "same", 1, 32, "pos"), (6, 2, "same", 1, 14, "full")]
    return cases
