"""Test-time oracle of networks with the two-slope ReLU φ(x) = a·min(x, 0) + b·max(x, 0)
(cnn_gp.ABReLU, cnn_gp.LeakyReLU): float64 on the CPU.

The reference has no such module.  For (u1, u2) ~ N(0, [[v1, c], [c, v2]]) with angle θ,
cos θ = c/√(v1 v2), the closed forms are written here from θ,

    K'  = E[φ(u1) φ(u2)]   = (a − b)²·√(v1 v2)·(sin θ + (π − θ) cos θ)/2π + a·b·c
    κ̇   = E[φ'(u1) φ'(u2)] = (a − b)²·(π − θ)/2π + a·b = ∂K'/∂c
    v'  = (a² + b²)/2 · v                                   (K' at θ = 0, c = v1 = v2 = v)

with the reference's guard of the ReLU (t = v1 v2 + float32 tiny under the root, cos θ clamped
to [−1, 1], sin θ·√t = √max(t − c², 0)) so a zero-variance pixel gives 0 and not NaN.  They
share no code with the ReLU oracle; tests/test_abrelu_host.py checks them against an angular
integral that shares none of this.

Layer path (torch): the walk of erf_oracle.py extended by import with one module; every other
leaf goes through gelu_oracle's walk (Conv2d with its scale leaf, ReLU, Erf, Gelu).  Θ comes
two ways, as there:

* ``ntk_autograd``: the scale-leaf trick, always run as same=False; the pairs of identical
  images are singular (θ = 0) and come out NaN or wrong: callers use same=False pairs only.
* ``ntk_stepwise``: program.ntk_steps launch by launch with torch ops, the overridden pairs
  (same and i = j, or same and diag) with K' = h·v[i] and κ̇ = h, h = (a² + b²)/2.

Pooled path (numpy): the five-stream walk on position-pair maps of pool_ntk_oracle.py (S_xy,
S_xx, S_yy, pooled, Θ) extended by import in the same way; the override applies where
``same``, i = j and p = q.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import cnn_gp
from oracle import torch_cpu as T

import avgpool_oracle as AO
import erf_oracle as EO
import gelu_oracle as GO
import ntk_oracle as NT
import pool_ntk_oracle as PN
import pool_oracle as PO

TWO_PI = 2 * math.pi
F32_TINY = float(np.finfo(np.float32).tiny)


def slopes(mod):
    return float(mod.a), float(mod.b)


def tol_factor(a, b):
    """A(a, b) = ((a − b)² + 2|ab|)/(a² + b²): the absolute error of K' is at most
    s·δR + |m|·δc, both maxima at θ = 0, against max|K'| = h·v there.  1 for ab >= 0, at most 3."""
    return ((a - b) ** 2 + 2 * abs(a * b)) / (a * a + b * b)


# ------------------------------------------------------------------------------------
# the closed forms (torch tensors or numpy arrays of float64)
# ------------------------------------------------------------------------------------
def abrelu_pair(c, v1, v2, a, b):
    """(K', κ̇) of the two-slope map, elementwise, from θ."""
    if isinstance(c, torch.Tensor):
        sqrt, acos, clip = torch.sqrt, torch.acos, torch.clamp
    else:
        sqrt, acos, clip = np.sqrt, np.arccos, np.clip
    s, m = (a - b) ** 2, a * b
    t = v1 * v2 + F32_TINY
    theta = acos(clip(c / sqrt(t), -1.0, 1.0))
    root = sqrt(clip(t - c * c, 0.0, None))                 # √t · sin θ
    k = s * (root + (math.pi - theta) * c) / TWO_PI + m * c
    kd = s * (math.pi - theta) / TWO_PI + m
    return k, kd


def abrelu_var(v, a, b):
    return (a * a + b * b) / 2 * v


# ------------------------------------------------------------------------------------
# the layer path
# ------------------------------------------------------------------------------------
def _abrelu(kp, a, b):
    """T._relu's counterpart: (same, diag, xy', xx', yy') with the same overrides."""
    same, diag, xy, xx, yy = kp
    out, _ = abrelu_pair(*EO._broadcast(xy, xx, yy, diag), a, b)
    xx2 = abrelu_var(xx, a, b)
    out = GO._override(out, xx2, same, diag, xx.shape[0])
    if not diag:
        out = out.reshape(-1, 1, *out.shape[-2:])
    return (same, diag, out, xx2, xx2 if same else abrelu_var(yy, a, b))


def abrelu_kdot(c, xx, yy, same, diag, a, b):
    """κ̇ on pair maps c [nmaps, 1, h, w], h = (a² + b²)/2 where K' is overridden"""
    _, kd = abrelu_pair(*EO._broadcast(c, xx, yy, diag), a, b)
    over = torch.full_like(xx, (a * a + b * b) / 2)
    return GO._override(kd, over, same, diag, xx.shape[0]).reshape(c.shape)


def _walk(mod, kp, scales=None):
    if isinstance(mod, cnn_gp.ABReLU):
        return _abrelu(kp, *slopes(mod))
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            kp = _walk(m, kp, scales)
        return kp
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        pr = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [None] * len(mod.mods)
        return T._axpy([(pr[i], _walk(m, kp, scales)) for i, m in enumerate(mod.mods)])
    return GO._walk(mod, kp, scales)          # Conv2d (with its scale leaf), ReLU, Erf, Gelu


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


def _nonlin(op):
    """(the step on (same, diag, xy, xx, yy), κ̇, the variance map) of a nonlinearity op"""
    if op.kind == "abrelu":
        a, b = op.slopes
        return (lambda kp: _abrelu(kp, a, b),
                lambda c, vx, vy, same, diag: abrelu_kdot(c, vx, vy, same, diag, a, b),
                lambda v: abrelu_var(v, a, b))
    return GO._NONLIN[op.kind]


def _variances(prog, v0, xx, yy, same):
    var = {v0: (xx, yy)}
    for op in prog.ops:
        if op.kind == "conv":
            var[op.dst] = tuple(NT.conv_t(t, op.geom, op.geom.bias) for t in var[op.src])
        elif op.kind == "add":
            acc = None
            for coef, t in op.terms:
                c = 1.0 if coef is None else coef
                term = tuple(c * m for m in var[t])
                acc = term if acc is None else tuple(a + b for a, b in zip(acc, term))
            var[op.dst] = acc
        else:
            f = _nonlin(op)[2]
            x2 = f(var[op.src][0])
            var[op.dst] = (x2, x2 if same else f(var[op.src][1]))
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
        if st.fn == "conv":
            out = NT.conv_t(bufs[st.src], st.op.geom, st.bias)
            bufs[st.dst] = out if st.addend is None else out + bufs[st.addend]
        elif st.fn == "axpby":
            acc = None
            for coef, b in st.terms:
                term = bufs[b] if coef is None else coef * bufs[b]
                acc = term if acc is None else acc + term
            bufs[st.dst] = acc
        else:
            assert st.fn in (st.op.kind, st.op.kind + "_ntk"), st.fn
            step, kdot, _ = _nonlin(st.op)
            vx, vy = var[st.var]
            c = bufs[st.src]
            if st.fn.endswith("_ntk"):
                bufs[st.dst_theta] = bufs[st.theta] * kdot(c, vx, vy, same, diag)
            bufs[st.dst] = step((same, diag, c, vx, vy))[2].reshape(c.shape)
    shape = (n1,) if diag else (n1, n2)
    k = bufs[kbuf].reshape(shape)
    th = torch.zeros_like(k) if tbuf is None else bufs[tbuf].reshape(shape)
    return k.numpy(), th.numpy()


def pair_op(xy, theta, xx, yy, same, diag, a, b):
    """float64 (K', Θ', xx', yy') of one step on [n][hw] arrays: cgp_abrelu_* / cgp_var_abrelu_*"""
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))[:, None, None, :]   # noqa
    c, th, vx, vy = t(xy), t(theta), t(xx), t(yy)
    _, _, k, vx2, vy2 = _abrelu((bool(same), bool(diag), c, vx, vy), a, b)
    kd = abrelu_kdot(c, vx, vy, bool(same), bool(diag), a, b)
    flat = lambda v: v.reshape(-1, np.shape(xy)[1]).numpy()                      # noqa: E731
    return flat(k), flat(th * kd), flat(vx2), flat(vy2)


# ------------------------------------------------------------------------------------
# the pooled path: position-pair maps [m, p_row, p_col, q_row, q_col], both streams
# ------------------------------------------------------------------------------------
def abrelu_map(s, xx, yy, pi, pj, same, a, b):
    """(K', κ̇) of (S[m][p, q], xx[pi[m]][p], yy[pj[m]][q]); with same, i = j and p = q: h·v, h"""
    v1, v2 = PN._bcast(s, xx, yy, pi, pj)
    k, kd = abrelu_pair(s, v1, v2, a, b)
    if same:
        mask = PO._self_mask(s, pi, pj)
        k = np.where(mask, abrelu_var(v1, a, b), k)
        kd = np.where(mask, (a * a + b * b) / 2, kd)
    return k, kd


def _walk_maps(mod, st, pairs, eps=0.0):
    """st = (S_xy, S_xx, S_yy, pooled, Θ_xy or None for zero); pairs = (pair_i, pair_j, same)"""
    if isinstance(mod, cnn_gp.ABReLU):
        sxy, sxx, syy, pooled, th = st
        pi, pj, same = pairs
        assert not pooled, "a nonlinearity after the global pool has no definition here"
        a, b = slopes(mod)
        ax, ay = np.arange(len(sxx)), np.arange(len(syy))
        xx, yy = AO.diag(sxx), AO.diag(syy)
        k, kd = abrelu_map(sxy, xx, yy, pi, pj, same, a, b)
        return (k, abrelu_map(sxx, xx, xx, ax, ax, True, a, b)[0],
                abrelu_map(syy, yy, yy, ay, ay, True, a, b)[0], False,
                None if th is None else th * kd)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            st = _walk_maps(m, st, pairs, eps)
        return st
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        outs = [_walk_maps(m, st, pairs, eps) for m in mod.mods]
        coef = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [1.0] * len(outs)
        assert len({o[3] for o in outs}) == 1
        add = lambda k: sum(c * o[k] for c, o in zip(coef, outs))               # noqa: E731
        live = [c * o[4] for c, o in zip(coef, outs) if o[4] is not None]
        return add(0), add(1), add(2), outs[0][3], sum(live) if live else None
    return PN._walk(mod, st, pairs, eps)      # every other module, one at a time


def _run_maps(model, x, y, same, diag):
    x = np.asarray(x, np.float64)
    if y is None:
        assert same is None
        y, same = x, True
    y = np.asarray(y, np.float64)
    pi, pj = PO.pair_lists(len(x), len(y), same, diag)
    ax, ay = np.arange(len(x)), np.arange(len(y))
    st = (PO.moments(x, y, pi, pj), PO.moments(x, x, ax, ax), PO.moments(y, y, ay, ay), False,
          None)
    k, _, _, pooled, th = _walk_maps(model, st, (pi, pj, bool(same)))
    if th is None:
        th = np.zeros_like(k)
    return k, th, pooled, (len(x),) if diag else (len(x), len(y))


def pool_ntk(model, x, y=None, same=None, diag=False):
    """(K, Θ) of a model on position-pair maps whose final value is 1x1: [N1, N2] or [N1]"""
    k, th, _, lead = _run_maps(model, x, y, same, diag)
    assert k.shape[1:] == (1, 1, 1, 1)
    return k.reshape(lead), th.reshape(lead)


def position_ntk(model, x, y=None, same=None, diag=False):
    """(S, Θ) of a body without a GlobalAvgPool: [N1, N2, H', W', H', W'] each (diag: [N1, ...])"""
    k, th, pooled, lead = _run_maps(model, x, y, same, diag)
    assert not pooled
    return k.reshape(lead + k.shape[1:]), th.reshape(lead + th.shape[1:])
