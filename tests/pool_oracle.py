"""Test-time oracle of networks with global average pooling: float64 numpy on the CPU.

The reference has no pooling layer, so the oracle restates the definition itself.  Values
upstream of a GlobalAvgPool are position-pair maps, 5-D arrays per pair list

    S[m, p_row, p_col, q_row, q_col] = cov(pixel p of x_i, pixel q of y_j),  (i, j) = pair m

with the reference's conventions (the ReLU without the sqrt 2, var_weight/k² per tap, one
bias per channel shared by all positions):

    input          S = mean_c x_i[c, p]·y_j[c, q]
    Conv2d         S'[p, q] = weight·Σ_{a,b<taps} S[p·s + off + (a, b)·d, q·s + off + (a, b)·d]
                   + bias, a term zero when either index leaves the map (shifted adds);
                   geometry from program.conv_geometry
    ReLU           the reference's formula (kernels.py:146-152) of (S[p, q], xx_i[p], yy_j[q]);
                   with same, i = j and p = q: xx_i[p]/2
    Erf            erf_oracle's closed form, with the same override (erf_var)
    Sum / Mixture  the (weighted) sum
    GlobalAvgPool  mean over (p, q): a 1x1 map per pair, which linear ops may follow

and the per-image variance maps xx[i, p] = S_xx[i, i, p, p] follow their own recursion
(conv, v/2, erf_var, sums), closed because the variance at p reads S_xx[p + δ, p + δ] only.
With ``same`` every pair (i, j) is evaluated, i > j included: nothing is mirrored."""
from __future__ import annotations

import math

import numpy as np
import torch

import cnn_gp
from cnn_gp.program import conv_geometry, conv_out_hw

import erf_oracle as EO

F32_TINY = float(np.finfo(np.float32).tiny)


def pair_lists(n1, n2, same, diag):
    if diag:
        return np.arange(n1), np.arange(n1)
    i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
    return i.ravel(), j.ravel()


def moments(x, y, pi, pj):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return np.einsum("mchw,mcuv->mhwuv", x[pi], y[pj]) / x.shape[1]


def variances(x):
    x = np.asarray(x, np.float64)
    return (x * x).mean(1)


def _taps(n_in, n_out, g, t):
    """input index of every output index for tap t, and which are inside the map"""
    idx = np.arange(n_out) * g.stride + g.offset + t * g.dilation
    ok = (idx >= 0) & (idx < n_in)
    return np.where(ok, idx, 0), ok


def conv_map(s, mod):
    """Conv2d on position-pair maps [P, H, W, H, W]: shifted adds."""
    g = conv_geometry(mod)
    h, w = s.shape[1:3]
    ho, wo = conv_out_hw(mod, h, w)
    acc = np.zeros((s.shape[0], ho, wo, ho, wo))
    for a in range(g.taps):
        r, rok = _taps(h, ho, g, a)
        for b in range(g.taps):
            c, cok = _taps(w, wo, g, b)
            ok = rok[:, None] & cok[None, :]
            term = s[:, r][:, :, c][:, :, :, r][:, :, :, :, c]
            acc += term * (ok[None, :, :, None, None] & ok[None, None, None, :, :])
    return g.weight * acc + g.bias


def conv_var(v, mod):
    """Conv2d on per-image variance maps [N, H, W]"""
    g = conv_geometry(mod)
    h, w = v.shape[1:]
    ho, wo = conv_out_hw(mod, h, w)
    acc = np.zeros((v.shape[0], ho, wo))
    for a in range(g.taps):
        r, rok = _taps(h, ho, g, a)
        for b in range(g.taps):
            c, cok = _taps(w, wo, g, b)
            acc += v[:, r][:, :, c] * (rok[:, None] & cok[None, :])
    return g.weight * acc + g.bias


def _self_mask(s, pi, pj):
    """[P, H, W, H, W] True where pair m is (i, i) and p = q"""
    h, w = s.shape[1:3]
    eye = np.eye(h * w, dtype=bool).reshape(h, w, h, w)
    return (np.asarray(pi) == np.asarray(pj))[:, None, None, None, None] & eye[None]


def relu_map(s, xx, yy, pi, pj, same):
    v1 = xx[pi][:, :, :, None, None]
    v2 = yy[pj][:, None, None, :, :]
    t = v1 * v2 + F32_TINY                                       # kernels.py:146
    cos = np.clip(s * (1.0 / np.sqrt(t)), -1.0, 1.0)
    sin = np.sqrt(np.clip(t - s * s, 0.0, None))
    out = (sin + (math.pi - np.arccos(cos)) * s) / (2 * math.pi)
    if same:
        out = np.where(_self_mask(s, pi, pj), np.broadcast_to(v1 / 2, s.shape), out)
    return out


def erf_map(s, xx, yy, pi, pj, same):
    v1 = xx[pi][:, :, :, None, None]
    v2 = yy[pj][:, None, None, :, :]
    t = lambda a: torch.from_numpy(np.array(np.broadcast_to(a, s.shape)))  # noqa: E731
    out = EO.erf_pair(t(s), t(v1), t(v2))[0].numpy()
    if same:
        over = EO.erf_var(t(v1)).numpy()
        out = np.where(_self_mask(s, pi, pj), over, out)
    return out


def erf_var(v):
    return EO.erf_var(torch.from_numpy(np.ascontiguousarray(v))).numpy()


def _walk(mod, st, pairs):
    """st = (S, xx, yy, pooled), xx / yy None after the pool; pairs = (pair_i, pair_j, same)"""
    s, xx, yy, pooled = st
    pi, pj, same = pairs
    if isinstance(mod, cnn_gp.Conv2d):
        if pooled:
            return conv_map(s, mod), None, None, True
        return conv_map(s, mod), conv_var(xx, mod), conv_var(yy, mod), False
    if isinstance(mod, (cnn_gp.ReLU, cnn_gp.Erf)):
        assert not pooled, "a nonlinearity after the pool has no definition here"
        if isinstance(mod, cnn_gp.ReLU):
            return relu_map(s, xx, yy, pi, pj, same), xx / 2, yy / 2, False
        return erf_map(s, xx, yy, pi, pj, same), erf_var(xx), erf_var(yy), False
    if isinstance(mod, cnn_gp.GlobalAvgPool):
        assert not pooled
        return s.mean(axis=(1, 2, 3, 4), keepdims=True), None, None, True
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _walk(m, st, pairs)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_walk(m, st, pairs) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        assert len({o[3] for o in outs}) == 1

        def add(k):
            if outs[0][k] is None:
                return None
            return sum(c * o[k] for c, o in zip(coef, outs))
        return add(0), add(1), add(2), outs[0][3]
    raise TypeError(type(mod).__name__)


def _run(model, x, y, same, diag):
    x = np.asarray(x, np.float64)
    if y is None:
        assert same is None
        y, same = x, True
    y = np.asarray(y, np.float64)
    pi, pj = pair_lists(len(x), len(y), same, diag)
    s, _, _, pooled = _walk(model, (moments(x, y, pi, pj), variances(x), variances(y), False),
                            (pi, pj, bool(same)))
    lead = (len(x),) if diag else (len(x), len(y))
    return s, pooled, lead


def kernel(model, x, y=None, same=None, diag=False):
    """K of a model whose every path passes one GlobalAvgPool: [N1, N2], or [N1] with diag"""
    s, pooled, lead = _run(model, x, y, same, diag)
    assert pooled and s.shape[1:] == (1, 1, 1, 1)
    return s.reshape(lead)


def position_covariance(model, x, y=None, same=None, diag=False):
    """The map a pool after ``model`` would read: [N1, N2, H', W', H', W'] (diag: [N1, ...])"""
    s, pooled, lead = _run(model, x, y, same, diag)
    assert not pooled
    return s.reshape(lead + s.shape[1:])


def to_device_layout(s):
    """[P, p_row, p_col, q_row, q_col] -> the library's [P][p_row][q_row][p_col][q_col]"""
    return np.ascontiguousarray(np.transpose(s, (0, 1, 3, 2, 4)))


def from_device_layout(a, h, w):
    return np.transpose(np.asarray(a).reshape(-1, h, h, w, w), (0, 1, 3, 2, 4))
