"""Test-time oracle of convs whose taps carry individual weights: numpy on the CPU.

The reference's Conv2d.propagate is F.conv2d with the module's ``kernel`` buffer
(kernels.py:92-98), so a Conv2d here is read the same way, box or not: table = the buffer,
offset = -padding, and

    out[m][oh][ow] = ( Σ_a p_a ) + bias [+ addend]
    p_a            =   Σ_b W[a][b] · in[m][oh·s + off + a·d][ow·s + off + b·d]

in the order include/cnngp.h states for cgp_tapconv_*: W rounded once to the maps' type, every
product rounded, p_a summed left to right, the p_a added top to bottom, then the bias, then the
addend.  ``tapconv`` and ``tapconv_cov`` evaluate that in the input's dtype (the emulation the
entry points are compared with bit for bit; a zero weight is multiplied like any other, which
for finite inputs gives the value of skipping it).  On top of them, in float64:

    kernel / ntk          the layer recursion (K, its variances, Θ stepwise) of Conv2d, ReLU,
                          Sequential, Sum and Mixture: K' = A_W(K) + b, Θ' = A_W(Θ) + K';
                          ReLU and its κ̇ as the reference has them
    ntk_autograd          Θ = Σ_l ⟨∂K_final/∂K_xy^l, K_xy^l⟩ by torch autograd through
                          F.conv2d with the buffer (the scale trick of ntk_oracle)
    position_ntk / ntk_maps / position_covariance
                          the same on position-pair maps, with AvgPool2d, GlobalAvgPool and
                          CorrelatedConv2d from avgpool_oracle / corrconv_oracle
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

import cnn_gp

import avgpool_oracle as AO
import corrconv_oracle as CO
import pool_ntk_oracle as PN
import pool_oracle as PO
from oracle import torch_cpu as T

F32_TINY = PO.F32_TINY


# ------------------------------------------------------------------------------------
# the op, in the contract's order and the input's dtype
# ------------------------------------------------------------------------------------
def out_size(n, extent, offset, stride, dilation):
    """F.conv2d's output size with padding = -offset"""
    return (n - 2 * offset - dilation * (extent - 1) - 1) // stride + 1


def _taps(n_in, n_out, offset, stride, dilation, t):
    idx = np.arange(n_out) * stride + offset + t * dilation
    ok = (idx >= 0) & (idx < n_in)
    return np.where(ok, idx, 0), ok


def tapconv(inp, table, offset, stride=1, dilation=1, bias=0.0, addend=None):
    """cgp_tapconv_* on [m, h, w] maps, every operation rounded in inp.dtype"""
    inp = np.asarray(inp)
    ty = inp.dtype.type
    w_ = np.asarray(table, np.float64).astype(inp.dtype)
    ke = w_.shape[0]
    h, w = inp.shape[1:]
    ho, wo = (out_size(n, ke, offset, stride, dilation) for n in (h, w))
    acc = np.zeros((inp.shape[0], ho, wo), inp.dtype)
    for a in range(ke):
        r, rok = _taps(h, ho, offset, stride, dilation, a)
        pa = np.zeros_like(acc)
        for b in range(ke):
            c, cok = _taps(w, wo, offset, stride, dilation, b)
            term = inp[:, r][:, :, c] * (rok[:, None] & cok[None, :]).astype(inp.dtype)
            pa = pa + w_[a, b] * term
        acc = acc + pa
    out = acc + ty(bias)
    return out if addend is None else out + np.asarray(addend, inp.dtype)


def tapconv_cov(s, table, offset, stride=1, dilation=1, bias=0.0, addend=None):
    """cgp_tapconv_cov_* on position-pair maps [m, p_row, p_col, q_row, q_col] (the oracles'
    layout), every operation rounded in s.dtype"""
    s = np.asarray(s)
    ty = s.dtype.type
    w_ = np.asarray(table, np.float64).astype(s.dtype)
    ke = w_.shape[0]
    h, w = s.shape[1:3]
    ho, wo = (out_size(n, ke, offset, stride, dilation) for n in (h, w))
    acc = np.zeros((s.shape[0], ho, wo, ho, wo), s.dtype)
    for a in range(ke):
        r, rok = _taps(h, ho, offset, stride, dilation, a)
        pa = np.zeros_like(acc)
        for b in range(ke):
            c, cok = _taps(w, wo, offset, stride, dilation, b)
            ok = rok[:, None] & cok[None, :]
            term = s[:, r][:, :, c][:, :, :, r][:, :, :, :, c]
            mask = ok[None, :, :, None, None] & ok[None, None, None, :, :]
            pa = pa + w_[a, b] * (term * mask.astype(s.dtype))
        acc = acc + pa
    out = acc + ty(bias)
    return out if addend is None else out + np.asarray(addend, s.dtype)


# ------------------------------------------------------------------------------------
# a Conv2d as the reference reads it
# ------------------------------------------------------------------------------------
def table_of(mod):
    ke = mod.kernel.shape[-1]
    return mod.kernel.detach().cpu().double().numpy().reshape(ke, ke)


def conv_args(mod):
    return dict(table=table_of(mod), offset=-int(mod.padding), stride=int(mod.stride),
                dilation=int(mod.dilation))


def conv_var(v, mod, bias=None):
    """the Conv2d on [n, h, w] maps"""
    return tapconv(v, bias=float(mod.var_bias) if bias is None else bias, **conv_args(mod))


def conv_cov(s, mod, bias=None):
    """the Conv2d on position-pair maps"""
    return tapconv_cov(s, bias=float(mod.var_bias) if bias is None else bias, **conv_args(mod))


# ------------------------------------------------------------------------------------
# the layer recursion: K, its variances and Θ stepwise, float64
# ------------------------------------------------------------------------------------
def _relu_layer(xy, xx, yy, n1, n2, same, diag):
    """(relu(xy), κ̇) on pair maps [nmaps, h, w] with the reference's overrides"""
    if diag:
        v1, v2, c = xx, yy, xy
    else:
        c = xy.reshape(n1, n2, *xy.shape[1:])
        v1, v2 = xx[:, None], yy[None, :]
    t = v1 * v2 + F32_TINY
    cos = np.clip(c * (1.0 / np.sqrt(t)), -1.0, 1.0)
    sin = np.sqrt(np.clip(t - c * c, 0.0, None))
    th = np.arccos(cos)
    out = (sin + (math.pi - th) * c) / (2 * math.pi)
    kd = (math.pi - th) / (2 * math.pi)
    if same and diag:
        out, kd = xx / 2, np.full_like(kd, 0.5)
    elif same:
        idx = np.arange(n1)
        out[idx, idx], kd[idx, idx] = xx / 2, 0.5
    return out.reshape(xy.shape), kd.reshape(xy.shape)


def _layer_walk(mod, st, info):
    """st = (K, xx, yy, Θ or None for zero) on [nmaps, h, w] / [n, h, w]"""
    k, xx, yy, th = st
    n1, n2, same, diag = info
    if isinstance(mod, cnn_gp.Conv2d):
        k2 = conv_var(k, mod)
        t2 = k2 if th is None else conv_var(th, mod, bias=0.0) + k2
        return k2, conv_var(xx, mod), conv_var(yy, mod), t2
    if isinstance(mod, cnn_gp.ReLU):
        out, kd = _relu_layer(k, xx, yy, n1, n2, same, diag)
        return out, xx / 2, yy / 2, None if th is None else th * kd
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _layer_walk(m, st, info)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_layer_walk(m, st, info) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        add = lambda i: sum(c * o[i] for c, o in zip(coef, outs))               # noqa: E731
        live = [c * o[3] for c, o in zip(coef, outs) if o[3] is not None]
        return add(0), add(1), add(2), sum(live) if live else None
    raise TypeError(type(mod).__name__)


def _inputs(x, y, same):
    x = np.asarray(x, np.float64)
    if y is None:
        assert same is None
        y, same = x, True
    return x, np.asarray(y, np.float64), bool(same)


def layer_run(model, x, y=None, same=None, diag=False):
    """(K, xx, yy, Θ) of the final value: pair maps [nmaps, h, w], variance maps [n, h, w]"""
    x, y, same = _inputs(x, y, same)
    n1, n2 = len(x), len(y)
    if diag:
        xy = (x * y).mean(1)
    else:
        xy = (x[:, None] * y[None]).mean(2).reshape(n1 * n2, *x.shape[2:])
    st = (xy, (x * x).mean(1), (y * y).mean(1), None)
    k, xx, yy, th = _layer_walk(model, st, (n1, n2, same, bool(diag)))
    return k, xx, yy, np.zeros_like(k) if th is None else th


def ntk(model, x, y=None, same=None, diag=False):
    """(K, Θ) of a model whose final value is 1x1, by the layer recursion"""
    k, _, _, th = layer_run(model, x, y, same, diag)
    assert k.shape[1:] == (1, 1)
    shape = (len(x),) if diag else (len(x), len(x if y is None else y))
    return k.reshape(shape), th.reshape(shape)


def kernel(model, x, y=None, same=None, diag=False):
    return ntk(model, x, y, same, diag)[0]


# ------------------------------------------------------------------------------------
# Θ by autograd through the torch ops (ntk_oracle's scale trick over the module tree)
# ------------------------------------------------------------------------------------
def _auto_walk(mod, kp, scales, both):
    if isinstance(mod, cnn_gp.Conv2d):
        same, diag = kp[:2]
        kern = mod.kernel.detach().cpu().double()
        f = lambda t: F.conv2d(t, kern, stride=int(mod.stride), padding=int(mod.padding),  # noqa: E731,E501
                               dilation=int(mod.dilation)) + float(mod.var_bias)
        xy, xx, yy = (f(t) for t in kp[2:])
        s = torch.ones(xy.shape[0], 1, 1, 1, dtype=xy.dtype, requires_grad=True)
        scales.append(s)
        return (same, diag, xy * s, xx * s if both else xx, yy)
    if isinstance(mod, cnn_gp.ReLU):
        return T._relu(kp)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            kp = _auto_walk(m, kp, scales, both)
        return kp
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [None] * len(mod.mods)
        return T._axpy([(c, _auto_walk(m, kp, scales, both)) for c, m in zip(coef, mod.mods)])
    raise TypeError(type(mod).__name__)


def _autograd(model, x, y, same, diag):
    n1, n2 = x.shape[0], y.shape[0]
    if diag:
        xy = (x * y).mean(1, keepdim=True)
    else:
        xy = (x[:, None] * y[None]).mean(2).view(n1 * n2, 1, *x.shape[2:])
    scales = []
    kp = _auto_walk(model, (same, diag, xy, (x * x).mean(1, keepdim=True),
                            (y * y).mean(1, keepdim=True)), scales, same and diag)
    shape = (n1,) if diag else (n1, n2)
    k = kp[2].reshape(shape)
    theta = torch.zeros_like(k)
    for g in torch.autograd.grad(k.sum(), scales) if scales else ():
        theta = theta + g.view(shape)
    return k.detach().numpy(), theta.detach().numpy()


def ntk_autograd(model, x, y=None, same=None, diag=False):
    """(K, Θ) as ntk_oracle.ntk gives them: a same tile takes its diagonal from the diagonal
    mode; same=False pairs of identical images come out NaN"""
    x, y, same = _inputs(x, y, same)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    if same and not diag:
        k, th = _autograd(model, x, x, False, False)
        kd, td = _autograd(model, x, x, True, True)
        idx = np.arange(len(x))
        k[idx, idx], th[idx, idx] = kd, td
        return k, th
    return _autograd(model, x, y, same, bool(diag))


# ------------------------------------------------------------------------------------
# position-pair maps: st = (S_xy, S_xx, S_yy, pooled, Θ_xy or None for zero)
# ------------------------------------------------------------------------------------
def _cov_walk(mod, st, pairs):
    sxy, sxx, syy, pooled, th = st
    pi, pj, same = pairs
    if isinstance(mod, cnn_gp.CorrelatedConv2d):
        k = CO.corrconv_map(sxy, mod)
        t = k if th is None else PN.conv_lin(th, mod) + k
        return k, CO.corrconv_map(sxx, mod), CO.corrconv_map(syy, mod), pooled, t
    if isinstance(mod, cnn_gp.Conv2d):
        k = conv_cov(sxy, mod)
        t = k if th is None else conv_cov(th, mod, bias=0.0) + k
        return k, conv_cov(sxx, mod), conv_cov(syy, mod), pooled, t
    if isinstance(mod, cnn_gp.ReLU):
        assert not pooled
        ax, ay = np.arange(len(sxx)), np.arange(len(syy))
        xx, yy = AO.diag(sxx), AO.diag(syy)
        t = None if th is None else th * PN.relu_kdot_map(sxy, xx, yy, pi, pj, same)
        return (PO.relu_map(sxy, xx, yy, pi, pj, same), PO.relu_map(sxx, xx, xx, ax, ax, True),
                PO.relu_map(syy, yy, yy, ay, ay, True), False, t)
    if isinstance(mod, cnn_gp.AvgPool2d):
        assert not pooled
        f = lambda a: AO.avgpool_map(a, int(mod.kernel_size), int(mod.stride))  # noqa: E731
        return f(sxy), f(sxx), f(syy), False, None if th is None else f(th)
    if isinstance(mod, cnn_gp.GlobalAvgPool):
        assert not pooled
        f = lambda a: a.mean(axis=(1, 2, 3, 4), keepdims=True)                  # noqa: E731
        return f(sxy), f(sxx), f(syy), True, None if th is None else f(th)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _cov_walk(m, st, pairs)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_cov_walk(m, st, pairs) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        assert len({o[3] for o in outs}) == 1
        add = lambda i: sum(c * o[i] for c, o in zip(coef, outs))               # noqa: E731
        live = [c * o[4] for c, o in zip(coef, outs) if o[4] is not None]
        return add(0), add(1), add(2), outs[0][3], sum(live) if live else None
    raise TypeError(type(mod).__name__)


def _cov_run(model, x, y, same, diag):
    x, y, same = _inputs(x, y, same)
    pi, pj = PO.pair_lists(len(x), len(y), same, diag)
    ax, ay = np.arange(len(x)), np.arange(len(y))
    st = (PO.moments(x, y, pi, pj), PO.moments(x, x, ax, ax), PO.moments(y, y, ay, ay), False,
          None)
    k, _, _, pooled, th = _cov_walk(model, st, (pi, pj, same))
    return k, np.zeros_like(k) if th is None else th, pooled, \
        (len(x),) if diag else (len(x), len(y))


def ntk_maps(model, x, y=None, same=None, diag=False):
    """(K, Θ) of a model whose final value is 1x1, carried on position-pair maps"""
    k, th, _, lead = _cov_run(model, x, y, same, diag)
    assert k.shape[1:] == (1, 1, 1, 1)
    return k.reshape(lead), th.reshape(lead)


def position_ntk(model, x, y=None, same=None, diag=False):
    """(S, Θ) of a body without a GlobalAvgPool: [N1, N2, H', W', H', W'] (diag: [N1, ...])"""
    k, th, pooled, lead = _cov_run(model, x, y, same, diag)
    assert not pooled
    return k.reshape(lead + k.shape[1:]), th.reshape(lead + th.shape[1:])


def position_covariance(model, x, y=None, same=None, diag=False):
    return position_ntk(model, x, y, same, diag)[0]
