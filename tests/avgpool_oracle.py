"""Test-time oracle of networks with windowed average pooling: float64 numpy on the CPU.

pool_oracle.py carries the per-image variance maps by a recursion of their own, closed
because a conv reads S_xx[p + δ, p + δ] only.  An AvgPool2d averages S over the window of p
times the window of q, so the variance at p reads S_xx[p·s + δ, p·s + δ'] with δ ≠ δ' and the
recursion no longer closes.  This oracle therefore has NO variance recursion.  It carries
three position-pair streams through the module tree, 5-D arrays in pool_oracle's layout
[m, p_row, p_col, q_row, q_col]:

    S_xy  for the requested pairs (i, j)
    S_xx  for the self pairs (i, i) of x
    S_yy  for the self pairs (j, j) of y

and every nonlinearity takes xx = diag(S_xx), yy = diag(S_yy), the p = q entries.  The self
streams run with ``same`` (they are a tile of an image set against itself), so the
nonlinearities' override applies on their diagonals.

    AvgPool2d      S'[P, Q] = k⁻⁴·Σ_{δ, δ' in the k×k window} S[P·s + δ, Q·s + δ'],
                   output floor((H - k)/s) + 1 per side (avgpool_map)
    everything else as pool_oracle (its moments, conv_map, relu_map, erf_map)"""
from __future__ import annotations

import numpy as np

import cnn_gp

from pool_oracle import (moments, conv_map, relu_map, erf_map, pair_lists,  # noqa: F401
                         to_device_layout, from_device_layout)


def avgpool_map(s, k, stride):
    """AvgPool2d(k, stride) on position-pair maps [P, H, W, H, W]: a plain sum over the
    k² x k² offsets of the two windows"""
    h, w = s.shape[1:3]
    ho, wo = (h - k) // stride + 1, (w - k) // stride + 1
    assert ho > 0 and wo > 0
    rows = lambda a: slice(a, a + stride * (ho - 1) + 1, stride)                # noqa: E731
    cols = lambda b: slice(b, b + stride * (wo - 1) + 1, stride)                # noqa: E731
    acc = np.zeros((s.shape[0], ho, wo, ho, wo))
    for a in range(k):
        for b in range(k):
            for a2 in range(k):
                for b2 in range(k):
                    acc += s[:, rows(a), cols(b), rows(a2), cols(b2)]
    return acc / k ** 4


def diag(s):
    """[n, H, W, H, W] self maps -> the [n, H, W] variance maps S[i, p, p]"""
    return np.einsum("mabab->mab", s)


def _walk(mod, st, pairs):
    """st = (S_xy, S_xx, S_yy, pooled); pairs = (pair_i, pair_j, same)"""
    sxy, sxx, syy, pooled = st
    pi, pj, same = pairs
    ax, ay = np.arange(len(sxx)), np.arange(len(syy))
    if isinstance(mod, cnn_gp.Conv2d):
        return conv_map(sxy, mod), conv_map(sxx, mod), conv_map(syy, mod), pooled
    if isinstance(mod, (cnn_gp.ReLU, cnn_gp.Erf)):
        assert not pooled, "a nonlinearity after the global pool has no definition here"
        f = relu_map if isinstance(mod, cnn_gp.ReLU) else erf_map
        xx, yy = diag(sxx), diag(syy)
        return (f(sxy, xx, yy, pi, pj, same), f(sxx, xx, xx, ax, ax, True),
                f(syy, yy, yy, ay, ay, True), False)
    if isinstance(mod, cnn_gp.AvgPool2d):
        assert not pooled
        k, s = int(mod.kernel_size), int(mod.stride)
        return avgpool_map(sxy, k, s), avgpool_map(sxx, k, s), avgpool_map(syy, k, s), False
    if isinstance(mod, cnn_gp.GlobalAvgPool):
        assert not pooled
        mean = lambda a: a.mean(axis=(1, 2, 3, 4), keepdims=True)               # noqa: E731
        return mean(sxy), mean(sxx), mean(syy), True
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _walk(m, st, pairs)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_walk(m, st, pairs) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        assert len({o[3] for o in outs}) == 1
        add = lambda k: sum(c * o[k] for c, o in zip(coef, outs))               # noqa: E731
        return add(0), add(1), add(2), outs[0][3]
    raise TypeError(type(mod).__name__)


def _run(model, x, y, same, diag_):
    x = np.asarray(x, np.float64)
    if y is None:
        assert same is None
        y, same = x, True
    y = np.asarray(y, np.float64)
    pi, pj = pair_lists(len(x), len(y), same, diag_)
    ax, ay = np.arange(len(x)), np.arange(len(y))
    st = (moments(x, y, pi, pj), moments(x, x, ax, ax), moments(y, y, ay, ay), False)
    s, _, _, pooled = _walk(model, st, (pi, pj, bool(same)))
    lead = (len(x),) if diag_ else (len(x), len(y))
    return s, pooled, lead


def kernel(model, x, y=None, same=None, diag=False):
    """K of a model whose final value is 1x1 (through a GlobalAvgPool or a dense readout):
    [N1, N2], or [N1] with diag"""
    s, _, lead = _run(model, x, y, same, diag)
    assert s.shape[1:] == (1, 1, 1, 1)
    return s.reshape(lead)


def position_covariance(model, x, y=None, same=None, diag=False):
    """The map a pool after ``model`` would read: [N1, N2, H', W', H', W'] (diag: [N1, ...])"""
    s, pooled, lead = _run(model, x, y, same, diag)
    assert not pooled
    return s.reshape(lead + s.shape[1:])
