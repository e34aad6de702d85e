"""Test-time oracle of networks with the GELU nonlinearity: float64 on the CPU.

The reference has no Gelu.  The closed forms (Tsuchida, Pearce et al. 2021) for
φ(x) = x·Φ(x) and (u1, u2) ~ N(0, [[v1, c], [c, v2]]), with P = v1 v2, P1 = (1 + v1)(1 + v2),
Δ = √(P1 − c²), t = c/Δ:

    K'  = E[φ(u1) φ(u2)]   = ((c² + P·Δ²)/(P1·Δ) + c·atan t)/2π + c/4
    κ̇   = E[φ'(u1) φ'(u2)] = (1/Δ² + (1 − P)/P1 + 1)·t/2π + 1/4 + atan(t)/2π = ∂K'/∂c
    v'  = (2v²/((1 + v)·s) + v·atan(v/s))/2π + v/4,  s = √(1 + 2v)   (K' at c = v1 = v2 = v)

are written here without the library's Δ² >= 1 guard, so autograd stays smooth.
tests/test_gelu_host.py checks them against a numerical integral that shares none of this.

Layer path (torch): the walk of erf_oracle.py extended by import with one module; Conv2d,
ReLU and Erf go through erf_oracle's own walk.  Θ comes two ways, as there:

* ``ntk_autograd``: the scale-leaf trick, always run as same=False.  Valid on every pair of a
  network without a ReLU, identical images included (Δ² >= 1 + 2v: the map is smooth at
  rho = 1); with a ReLU the pairs of identical images come out NaN and callers mask them.
* ``ntk_stepwise``: program.ntk_steps launch by launch with torch ops, the overridden pairs
  (same and i = j, or same and diag) with K' = v'[i] and κ̇ at c = v1 = v2 = v.

Pooled path (numpy): the three-stream walk on position-pair maps of avgpool_oracle.py /
corrconv_oracle.py (S_xy, S_xx, S_yy; a nonlinearity reads the p = q diagonals of the self
streams) extended by import in the same way; the override applies where ``same``, i = j and
p = q.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import cnn_gp
from oracle import torch_cpu as T

import corrconv_oracle as CO
import erf_oracle as EO
import ntk_oracle as NT

TWO_PI = 2 * math.pi


# ------------------------------------------------------------------------------------
# the closed forms (torch tensors or numpy arrays of float64: only +, *, /, sqrt, atan)
# ------------------------------------------------------------------------------------
def _fn(a):
    return (torch.sqrt, torch.atan) if isinstance(a, torch.Tensor) else (np.sqrt, np.arctan)


def gelu_pair(c, v1, v2):
    """(K', κ̇) of the GELU map, elementwise, no guard."""
    sqrt, atan = _fn(c)
    p, p1 = v1 * v2, (1 + v1) * (1 + v2)
    d2 = p1 - c * c
    d = sqrt(d2)
    t = c / d
    a = atan(t)
    k = ((c * c + p * d2) / (p1 * d) + c * a) / TWO_PI + c / 4
    kd = (1 / d2 + (1 - p) / p1 + 1) * t / TWO_PI + 0.25 + a / TWO_PI
    return k, kd


def gelu_var(v):
    sqrt, atan = _fn(v)
    s = sqrt(1 + 2 * v)
    return (2 * v * v / ((1 + v) * s) + v * atan(v / s)) / TWO_PI + v / 4


def gelu_var_kdot(v):
    """κ̇ of a pair the library overrides with its own variance: ∂K'/∂c at c = v1 = v2 = v"""
    sqrt, atan = _fn(v)
    s = sqrt(1 + 2 * v)
    return (1 / (1 + 2 * v) + (1 - v) / (1 + v) + 1) * (v / s) / TWO_PI + 0.25 \
        + atan(v / s) / TWO_PI


# ------------------------------------------------------------------------------------
# the layer path
# ------------------------------------------------------------------------------------
def _override(out, over, same, diag, n1):
    """``over`` ([n1, 1, h, w]) written where the reference overrides its ReLU: out is
    [n1, n2, h, w] (or [n1, 1, h, w] with diag)"""
    if not same:
        return out
    if diag:
        return over
    idx = torch.arange(n1)
    out = out.clone()
    out[idx, idx] = over.view(n1, *over.shape[-2:])
    return out


def _gelu(kp):
    """T._relu's counterpart: (same, diag, xy', xx', yy') with the same overrides."""
    same, diag, xy, xx, yy = kp
    out, _ = gelu_pair(*EO._broadcast(xy, xx, yy, diag))
    xx2 = gelu_var(xx)
    out = _override(out, xx2, same, diag, xx.shape[0])
    if not diag:
        out = out.reshape(-1, 1, *out.shape[-2:])
    return (same, diag, out, xx2, xx2 if same else gelu_var(yy))


def gelu_kdot(c, xx, yy, same, diag):
    """κ̇ on pair maps c [nmaps, 1, h, w], gelu_var_kdot where K' is overridden"""
    _, kd = gelu_pair(*EO._broadcast(c, xx, yy, diag))
    return _override(kd, gelu_var_kdot(xx), same, diag, xx.shape[0]).reshape(c.shape)


def _walk(mod, kp, scales=None):
    if isinstance(mod, cnn_gp.Gelu):
        return _gelu(kp)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            kp = _walk(m, kp, scales)
        return kp
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        pr = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [None] * len(mod.mods)
        return T._axpy([(pr[i], _walk(m, kp, scales)) for i, m in enumerate(mod.mods)])
    return EO._walk(mod, kp, scales)          # Conv2d (with its scale leaf), ReLU, Erf


@torch.no_grad()
def kernel(model, x, y=None, same=None, diag=False):
    """K as a float64 numpy array, [N1, N2] or [N1] with diag."""
    x, y, same = EO._inputs(x, y, same)
    kp = _walk(model, (same, bool(diag)) + EO._moments(x, y, diag))
    return kp[2].reshape((len(x),) if diag else (len(x), len(y))).numpy()


def ntk_autograd(model, x, y=None, diag=False):
    """(K, Θ) by autograd with every pair evaluated as same=False (module docstring)."""
    x, y, _ = EO._inputs(x, y, None if y is None else False)
    scales = []
    kp = _walk(model, (False, bool(diag)) + EO._moments(x, y, diag), scales)
    shape = (len(x),) if diag else (len(x), len(y))
    k = kp[2].reshape(shape)
    theta = torch.zeros_like(k)
    if scales:
        for g in torch.autograd.grad(k.sum(), scales):
            theta = theta + g.view(shape)
    return k.detach().numpy(), theta.detach().numpy()


# op kind -> (the step on (same, diag, xy, xx, yy), κ̇, the variance map)
_NONLIN = {
    "relu": (T._relu, NT.kdot, lambda v: v / 2),
    "erf": (EO._erf, EO.erf_kdot, EO.erf_var),
    "gelu": (_gelu, gelu_kdot, gelu_var),
}


def _variances(prog, v0, xx, yy, same):
    var = {v0: (xx, yy)}
    for op in prog.ops:
        if op.kind == "conv":
            var[op.dst] = tuple(NT.conv_t(t, op.geom, op.geom.bias) for t in var[op.src])
        elif op.kind in _NONLIN:
            f = _NONLIN[op.kind][2]
            x2 = f(var[op.src][0])
            var[op.dst] = (x2, x2 if same else f(var[op.src][1]))
        elif op.kind == "add":
            acc = None
            for coef, t in op.terms:
                c = 1.0 if coef is None else coef
                term = tuple(c * m for m in var[t])
                acc = term if acc is None else tuple(a + b for a, b in zip(acc, term))
            var[op.dst] = acc
        else:
            raise AssertionError(op.kind)
    return var


@torch.no_grad()
def ntk_stepwise(model, x, y=None, same=None, diag=False):
    """(K, Θ) of program.ntk_steps, every launch a torch float64 CPU op."""
    from cnn_gp.program import compile_program, ntk_steps
    x, y, same = EO._inputs(x, y, same)
    n1, n2 = len(x), len(y)
    prog, v0, vf = compile_program(model, x.shape[2], x.shape[3])
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    xy, xx, yy = EO._moments(x, y, diag)
    var = _variances(prog, v0, xx, yy, same)
    bufs = {("K", v0): xy}
    for st in steps:
        kind = st.fn[:-4] if st.fn.endswith("_ntk") else st.fn
        if st.fn == "conv":
            out = NT.conv_t(bufs[st.src], st.op.geom, st.bias)
            bufs[st.dst] = out if st.addend is None else out + bufs[st.addend]
        elif kind in _NONLIN:
            step, kdot, _ = _NONLIN[kind]
            vx, vy = var[st.var]
            c = bufs[st.src]
            if st.fn.endswith("_ntk"):
                bufs[st.dst_theta] = bufs[st.theta] * kdot(c, vx, vy, same, diag)
            bufs[st.dst] = step((same, diag, c, vx, vy))[2].reshape(c.shape)
        elif st.fn == "axpby":
            acc = None
            for coef, b in st.terms:
                term = bufs[b] if coef is None else coef * bufs[b]
                acc = term if acc is None else acc + term
            bufs[st.dst] = acc
        else:
            raise AssertionError(st.fn)
    shape = (n1,) if diag else (n1, n2)
    k = bufs[kbuf].reshape(shape)
    th = torch.zeros_like(k) if tbuf is None else bufs[tbuf].reshape(shape)
    return k.numpy(), th.numpy()


# ------------------------------------------------------------------------------------
# the pooled path: position-pair maps [m, p_row, p_col, q_row, q_col]
# ------------------------------------------------------------------------------------
def gelu_map(s, xx, yy, pi, pj, same):
    """GELU of (S[m][p, q], xx[pi[m]][p], yy[pj[m]][q]); with same, i = j and p = q: v'"""
    v1 = np.broadcast_to(xx[pi][:, :, :, None, None], s.shape)
    v2 = np.broadcast_to(yy[pj][:, None, None, :, :], s.shape)
    out = gelu_pair(s, v1, v2)[0]
    if same:
        h, w = s.shape[1:3]
        eye = np.eye(h * w, dtype=bool).reshape(h, w, h, w)
        self_ = (np.asarray(pi) == np.asarray(pj))[:, None, None, None, None] & eye[None]
        out = np.where(self_, gelu_var(v1), out)
    return out


def _walk_maps(mod, st, pairs):
    """st = (S_xy, S_xx, S_yy, pooled); pairs = (pair_i, pair_j, same)"""
    if isinstance(mod, cnn_gp.Gelu):
        sxy, sxx, syy, pooled = st
        pi, pj, same = pairs
        assert not pooled, "a nonlinearity after the global pool has no definition here"
        ax, ay = np.arange(len(sxx)), np.arange(len(syy))
        xx, yy = CO.diag(sxx), CO.diag(syy)
        return (gelu_map(sxy, xx, yy, pi, pj, same), gelu_map(sxx, xx, xx, ax, ax, True),
                gelu_map(syy, yy, yy, ay, ay, True), False)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _walk_maps(m, st, pairs)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_walk_maps(m, st, pairs) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        assert len({o[3] for o in outs}) == 1
        return tuple(sum(c * o[k] for c, o in zip(coef, outs)) for k in range(3)) + (outs[0][3],)
    return CO._walk(mod, st, pairs)           # every other module, one at a time


def _run_maps(model, x, y, same, diag):
    x = np.asarray(x, np.float64)
    if y is None:
        assert same is None
        y, same = x, True
    y = np.asarray(y, np.float64)
    pi, pj = CO.pair_lists(len(x), len(y), same, diag)
    ax, ay = np.arange(len(x)), np.arange(len(y))
    st = (CO.moments(x, y, pi, pj), CO.moments(x, x, ax, ax), CO.moments(y, y, ay, ay), False)
    s, _, _, pooled = _walk_maps(model, st, (pi, pj, bool(same)))
    return s, pooled, (len(x),) if diag else (len(x), len(y))


def pooled_kernel(model, x, y=None, same=None, diag=False):
    """K of a model on position-pair maps whose final value is 1x1: [N1, N2] or [N1]"""
    s, _, lead = _run_maps(model, x, y, same, diag)
    assert s.shape[1:] == (1, 1, 1, 1)
    return s.reshape(lead)


def position_covariance(model, x, y=None, same=None, diag=False):
    """The map a pool after ``model`` would read: [N1, N2, H', W', H', W'] (diag: [N1, ...])"""
    s, pooled, lead = _run_maps(model, x, y, same, diag)
    assert not pooled
    return s.reshape(lead + s.shape[1:])
