"""Test-time oracle of the neural tangent kernel on position-pair maps: float64 numpy on the
CPU.  No reference has these networks, so the oracle restates the recursion itself on

    S[m, p_row, p_col, q_row, q_col],  Θ[m, p_row, p_col, q_row, q_col]

per pair list, with Θ = 0 at the input moments:

    Conv2d, CorrelatedConv2d   K' = A(K) + b,   Θ' = A(Θ) + K'   (A without the bias)
    ReLU / Erf / Gelu          K' as forward,   Θ' = Θ·κ̇ of (S[p, q], xx_i[p], yy_j[q]); the
                               layer path's override value where same, i = j and p = q
    AvgPool2d, GlobalAvgPool   the same linear op on both
    Sum / Mixture              the same (weighted) sum on both

The forward maps are those of pool_oracle, avgpool_oracle, corrconv_oracle and gelu_oracle; κ̇
restates ntk_oracle.kdot, erf_oracle.erf_kdot and gelu_oracle.gelu_kdot elementwise.  The
variance streams are the self maps S_xx, S_yy of the images (avgpool_oracle's walk): forward
only, Θ plays no part in them.

``eps`` scales the xy map of every conv / corrconv output by (1 + eps) with the variance
streams untouched: d K_final / d eps at 0 is Σ_l ⟨∂K_final/∂S^l, S^l⟩, the definition of Θ the
finite-difference test pins the recursion to."""
from __future__ import annotations

import math

import numpy as np

import cnn_gp
from cnn_gp.program import conv_geometry

import avgpool_oracle as AO
import corrconv_oracle as CO
import gelu_oracle as GO
import pool_oracle as PO

F32_TINY = PO.F32_TINY


# ------------------------------------------------------------------------------------
# κ̇ on position-pair maps
# ------------------------------------------------------------------------------------
def _bcast(s, xx, yy, pi, pj):
    v1 = np.broadcast_to(xx[pi][:, :, :, None, None], s.shape)
    v2 = np.broadcast_to(yy[pj][:, None, None, :, :], s.shape)
    return v1, v2


def relu_kdot_map(s, xx, yy, pi, pj, same):
    """ntk_oracle.kdot: (π - θ)/2π; 1/2 where the override applies"""
    v1, v2 = _bcast(s, xx, yy, pi, pj)
    t = v1 * v2 + F32_TINY
    kd = (math.pi - np.arccos(np.clip(s * (1.0 / np.sqrt(t)), -1.0, 1.0))) / (2 * math.pi)
    if same:
        kd = np.where(PO._self_mask(s, pi, pj), 0.5, kd)
    return kd


def erf_kdot_map(s, xx, yy, pi, pj, same):
    """erf_oracle.erf_kdot: (4/π)/√D; (4/π)/√(1 + 4v) where the override applies"""
    v1, v2 = _bcast(s, xx, yy, pi, pj)
    kd = (4 / math.pi) / np.sqrt(1 + 2 * (v1 + v2) + 4 * (v1 * v2 - s * s))
    if same:
        kd = np.where(PO._self_mask(s, pi, pj), (4 / math.pi) / np.sqrt(1 + 4 * v1), kd)
    return kd


def gelu_kdot_map(s, xx, yy, pi, pj, same):
    """gelu_oracle.gelu_kdot: gelu_pair's κ̇; gelu_var_kdot where the override applies"""
    v1, v2 = _bcast(s, xx, yy, pi, pj)
    kd = GO.gelu_pair(s, v1, v2)[1]
    if same:
        kd = np.where(PO._self_mask(s, pi, pj), GO.gelu_var_kdot(v1), kd)
    return kd


NONLIN = {
    cnn_gp.ReLU: (PO.relu_map, relu_kdot_map),
    cnn_gp.Erf: (PO.erf_map, erf_kdot_map),
    cnn_gp.Gelu: (GO.gelu_map, gelu_kdot_map),
}


def conv_lin(t, mod):
    """A(t) of a Conv2d or CorrelatedConv2d: the map without the bias (both are affine)"""
    f = CO.corrconv_map if isinstance(mod, cnn_gp.CorrelatedConv2d) else PO.conv_map
    return f(t, mod) - f(np.zeros_like(t), mod)


# ------------------------------------------------------------------------------------
# the walk: st = (S_xy, S_xx, S_yy, pooled, Θ_xy or None for zero)
# ------------------------------------------------------------------------------------
def _walk(mod, st, pairs, eps):
    sxy, sxx, syy, pooled, th = st
    pi, pj, same = pairs
    if isinstance(mod, (cnn_gp.Conv2d, cnn_gp.CorrelatedConv2d)):
        f = CO.corrconv_map if isinstance(mod, cnn_gp.CorrelatedConv2d) else PO.conv_map
        k = f(sxy, mod) * (1.0 + eps)
        t = k if th is None else conv_lin(th, mod) + k
        return k, f(sxx, mod), f(syy, mod), pooled, t
    if type(mod) in NONLIN:
        assert not pooled, "a nonlinearity after the global pool has no definition here"
        fmap, fdot = NONLIN[type(mod)]
        ax, ay = np.arange(len(sxx)), np.arange(len(syy))
        xx, yy = AO.diag(sxx), AO.diag(syy)
        t = None if th is None else th * fdot(sxy, xx, yy, pi, pj, same)
        return (fmap(sxy, xx, yy, pi, pj, same), fmap(sxx, xx, xx, ax, ax, True),
                fmap(syy, yy, yy, ay, ay, True), False, t)
    if isinstance(mod, cnn_gp.AvgPool2d):
        assert not pooled
        k, s = int(mod.kernel_size), int(mod.stride)
        f = lambda a: AO.avgpool_map(a, k, s)                                   # noqa: E731
        return f(sxy), f(sxx), f(syy), False, None if th is None else f(th)
    if isinstance(mod, cnn_gp.GlobalAvgPool):
        assert not pooled
        f = lambda a: a.mean(axis=(1, 2, 3, 4), keepdims=True)                  # noqa: E731
        return f(sxy), f(sxx), f(syy), True, None if th is None else f(th)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _walk(m, st, pairs, eps)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_walk(m, st, pairs, eps) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        assert len({o[3] for o in outs}) == 1
        add = lambda k: sum(c * o[k] for c, o in zip(coef, outs))               # noqa: E731
        live = [c * o[4] for c, o in zip(coef, outs) if o[4] is not None]
        return add(0), add(1), add(2), outs[0][3], sum(live) if live else None
    raise TypeError(type(mod).__name__)


def _run(model, x, y, same, diag, eps=0.0):
    x = np.asarray(x, np.float64)
    if y is None:
        assert same is None
        y, same = x, True
    y = np.asarray(y, np.float64)
    pi, pj = PO.pair_lists(len(x), len(y), same, diag)
    ax, ay = np.arange(len(x)), np.arange(len(y))
    st = (PO.moments(x, y, pi, pj), PO.moments(x, x, ax, ax), PO.moments(y, y, ay, ay), False,
          None)
    k, _, _, pooled, th = _walk(model, st, (pi, pj, bool(same)), eps)
    if th is None:
        th = np.zeros_like(k)
    return k, th, pooled, (len(x),) if diag else (len(x), len(y))


def ntk(model, x, y=None, same=None, diag=False, eps=0.0):
    """(K, Θ) of a model whose final value is 1x1: [N1, N2] each, or [N1] with diag"""
    k, th, _, lead = _run(model, x, y, same, diag, eps)
    assert k.shape[1:] == (1, 1, 1, 1)
    return k.reshape(lead), th.reshape(lead)


def position_ntk(model, x, y=None, same=None, diag=False):
    """(S, Θ) of a body without a GlobalAvgPool: [N1, N2, H', W', H', W'] each (diag: [N1, ...])"""
    k, th, pooled, lead = _run(model, x, y, same, diag)
    assert not pooled
    return k.reshape(lead + k.shape[1:]), th.reshape(lead + th.shape[1:])


def ntk_by_difference(model, x, y, eps=1e-5):
    """Θ from its definition: the central difference in eps of K_final with every conv /
    corrconv output's xy map scaled by (1 ± eps), variances untouched; same=False only (the
    override elements have no such derivative)."""
    kp = ntk(model, x, y, False, False, eps=+eps)[0]
    km = ntk(model, x, y, False, False, eps=-eps)[0]
    return (kp - km) / (2 * eps)


# ------------------------------------------------------------------------------------
# single ops, for the entry points alone
# ------------------------------------------------------------------------------------
KIND_MODS = {"relu": cnn_gp.ReLU, "erf": cnn_gp.Erf, "gelu": cnn_gp.Gelu}


def nonlin_ntk(kind, s, th, xx, yy, pi, pj, same):
    """(map(s), th·κ̇) of cgp_covntk_nonlin_*"""
    fmap, fdot = NONLIN[KIND_MODS[kind]]
    return fmap(s, xx, yy, pi, pj, same), th * fdot(s, xx, yy, pi, pj, same)


def conv_ntk(s, th, mod):
    """(k', t') of cgp_covntk_conv_* without a post-stage; th None for Θ = 0"""
    k = PO.conv_map(s, mod)
    g = conv_geometry(mod)
    return k, k if th is None else (PO.conv_map(th, mod) - g.bias) + k
