"""Test-time oracle of networks with correlated-weight convs: float64 numpy on the CPU.

avgpool_oracle.py's three-stream walk (S_xy, S_xx, S_yy; every nonlinearity reads the p = q
diagonals of the self streams) extended by import with one module:

    CorrelatedConv2d   S'[p, q] = (var_weight/k²) · Σ_{a,b,a',b' < k} R_rows[a, a']·R_cols[b, b']
                                  · S[p·s + off + (a, b)·d, q·s + off + (a', b')·d] + var_bias

a term zero where an index leaves the map, off from Conv2d's padding rules (corrconv_map:
the plain quadruple loop over (a, b, a', b'), no mirror pairing, no separation into a row
and a column pass).  The variance at p reads S_xx[p + δ, p + δ'] with δ ≠ δ', which only the
self stream holds."""
from __future__ import annotations

import numpy as np

import cnn_gp
from cnn_gp.program import conv_out_hw

import avgpool_oracle as AO
from avgpool_oracle import (moments, pair_lists, to_device_layout,  # noqa: F401
                            from_device_layout, diag)


def tap_offset(mod):
    """the first tap's offset: Conv2d.__init__'s padding rules, restated"""
    d = int(mod.dilation)
    if mod._padding_arg == "same":
        k = int(mod.kernel_size)
        return -d * (k // 2) + (d if k % 2 == 0 else 0)
    return -int(mod._padding_arg)


def corrconv_terms(s, k, stride, off, dil, ho, wo, rr, rc):
    """Σ R_rows[a, a']·R_cols[b, b']·S[P·s + off + a·d, U·s + off + b·d, Q·s + off + a'·d,
    V·s + off + b'·d] over the four taps, on [m, H, W, H, W]"""
    h, w = s.shape[1:3]

    def idx(n_in, n_out, t):
        i = np.arange(n_out) * stride + off + t * dil
        ok = (i >= 0) & (i < n_in)
        return np.where(ok, i, 0), ok

    acc = np.zeros((s.shape[0], ho, wo, ho, wo))
    for a in range(k):
        r1, k1 = idx(h, ho, a)
        for b in range(k):
            c1, k2 = idx(w, wo, b)
            for a2 in range(k):
                if rr[a][a2] == 0.0:             # every weight below is zero (a band's rows)
                    continue
                r2, k3 = idx(h, ho, a2)
                for b2 in range(k):
                    c2, k4 = idx(w, wo, b2)
                    wgt = rr[a][a2] * rc[b][b2]
                    if wgt == 0.0:
                        continue
                    term = s[:, r1][:, :, c1][:, :, :, r2][:, :, :, :, c2]
                    ok = (k1[:, None, None, None] & k2[None, :, None, None]
                          & k3[None, None, :, None] & k4[None, None, None, :])
                    acc += wgt * term * ok[None]
    return acc


def corrconv_map(s, mod):
    """CorrelatedConv2d on position-pair maps [m, H, W, H, W]"""
    k = int(mod.kernel_size)
    h, w = s.shape[1:3]
    ho, wo = conv_out_hw(mod, h, w)
    acc = corrconv_terms(s, k, int(mod.stride), tap_offset(mod), int(mod.dilation), ho, wo,
                         mod.corr_rows, mod.corr_cols)
    return float(mod.var_weight) / k ** 2 * acc + float(mod.var_bias)


def _walk(mod, st, pairs):
    if isinstance(mod, cnn_gp.CorrelatedConv2d):
        sxy, sxx, syy, pooled = st
        assert not pooled
        return corrconv_map(sxy, mod), corrconv_map(sxx, mod), corrconv_map(syy, mod), False
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
    return AO._walk(mod, st, pairs)


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
    """K of a model whose final value is 1x1: [N1, N2], or [N1] with diag"""
    s, _, lead = _run(model, x, y, same, diag)
    assert s.shape[1:] == (1, 1, 1, 1)
    return s.reshape(lead)


def position_covariance(model, x, y=None, same=None, diag=False):
    """The map a pool after ``model`` would read: [N1, N2, H', W', H', W'] (diag: [N1, ...])"""
    s, pooled, lead = _run(model, x, y, same, diag)
    assert not pooled
    return s.reshape(lead + s.shape[1:])
