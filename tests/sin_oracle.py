"""Test-time oracle of networks with the sinusoid φ(x) = a·sin(b·x + θ) (cnn_gp.Sin, cnn_gp.Cos,
cnn_gp.Rbf): float64 on the CPU.

The reference has no such module.  For (u1, u2) ~ N(0, [[v1, c], [c, v2]]), the identity
sin P·sin Q = (cos(P − Q) − cos(P + Q))/2 and E cos(g + μ) = cos μ·exp(−Var g/2) give, with
d = v1 + v2 − 2c and s = v1 + v2 + 2c,

    K'  = E[φ(u1) φ(u2)]   = A·(exp(−B·d) − C·exp(−B·s))
    κ̇   = E[φ'(u1) φ'(u2)] = D·(exp(−B·d) + C·exp(−B·s)) = ∂K'/∂c
    v'  = A·(1 − C·exp(−4B·v))                              (K' at c = v1 = v2 = v)
    (A, B, C, D) = (a²/2, b²/2, cos 2θ, a²b²/2);  Rbf(γ): (1, γ, 0, 2γ)

written here without the library's d, s >= 0 guard, so autograd stays smooth.
tests/test_sin_host.py checks them against a Gauss–Hermite quadrature that shares none of this.

Layer path (torch): the walk of erf_oracle.py extended by import with one module; every other
leaf goes through abrelu_oracle's walk (Conv2d with its scale leaf, ReLU, Erf, Gelu, ABReLU).
Θ comes two ways, as there:

* ``ntk_autograd``: the scale-leaf trick, always run as same=False.  The map is smooth
  everywhere, so it is valid on every pair of a network without a ReLU or an ABReLU.
* ``ntk_stepwise``: program.ntk_steps launch by launch with torch ops, the overridden pairs
  (same and i = j, or same and diag) with K' = v'[i] and κ̇ = D·(1 + C·exp(−4B·v)).

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

import abrelu_oracle as AB
import avgpool_oracle as AO
import erf_oracle as EO
import gelu_oracle as GO
import ntk_oracle as NT
import pool_ntk_oracle as PN
import pool_oracle as PO


def constants(a=1.0, b=1.0, phase=0.0):
    """(A, B, C, D) of φ(x) = a·sin(b·x + phase), written from the formulas"""
    return a * a / 2, b * b / 2, math.cos(2 * phase), a * a * b * b / 2


def rbf_constants(gamma):
    return 1.0, gamma, 0.0, 2 * gamma


def consts_of(mod):
    """The constants of a module from its own attributes (not from mod.constants())"""
    if isinstance(mod, cnn_gp.Rbf):
        return rbf_constants(float(mod.gamma))
    return constants(float(mod.a), float(mod.b), float(mod.phase))


# ------------------------------------------------------------------------------------
# the closed forms (torch tensors or numpy arrays of float64)
# ------------------------------------------------------------------------------------
def _exp(a):
    return torch.exp if isinstance(a, torch.Tensor) else np.exp


def sin_pair(c, v1, v2, k4):
    """(K', κ̇) of the sinusoid map, elementwise, no guard."""
    A, B, C, D = k4
    exp = _exp(c)
    ed = exp(-B * (v1 + v2 - 2 * c))
    es = exp(-B * (v1 + v2 + 2 * c))
    return A * (ed - C * es), D * (ed + C * es)


def sin_var(v, k4):
    A, B, C, _ = k4
    return A * (1 - C * _exp(v)(-4 * B * v))


def sin_var_kdot(v, k4):
    """κ̇ of a pair the library overrides with its own variance: ∂K'/∂c at c = v1 = v2 = v"""
    _, B, C, D = k4
    return D * (1 + C * _exp(v)(-4 * B * v))


# ------------------------------------------------------------------------------------
# the layer path
# ------------------------------------------------------------------------------------
def _sin(kp, k4):
    """T._relu's counterpart: (same, diag, xy', xx', yy') with the same overrides."""
    same, diag, xy, xx, yy = kp
    out, _ = sin_pair(*EO._broadcast(xy, xx, yy, diag), k4)
    xx2 = sin_var(xx, k4)
    out = GO._override(out, xx2, same, diag, xx.shape[0])
    if not diag:
        out = out.reshape(-1, 1, *out.shape[-2:])
    return (same, diag, out, xx2, xx2 if same else sin_var(yy, k4))


def sin_kdot(c, xx, yy, same, diag, k4):
    """κ̇ on pair maps c [nmaps, 1, h, w], sin_var_kdot where K' is overridden"""
    _, kd = sin_pair(*EO._broadcast(c, xx, yy, diag), k4)
    return GO._override(kd, sin_var_kdot(xx, k4), same, diag, xx.shape[0]).reshape(c.shape)


def _walk(mod, kp, scales=None):
    if isinstance(mod, cnn_gp.Sin):
        return _sin(kp, consts_of(mod))
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            kp = _walk(m, kp, scales)
        return kp
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        pr = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [None] * len(mod.mods)
        return T._axpy([(pr[i], _walk(m, kp, scales)) for i, m in enumerate(mod.mods)])
    return AB._walk(mod, kp, scales)          # Conv2d (with its scale leaf) and the others


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
    if op.kind == "sin":
        k4 = tuple(op.consts)
        return (lambda kp: _sin(kp, k4),
                lambda c, vx, vy, same, diag: sin_kdot(c, vx, vy, same, diag, k4),
                lambda v: sin_var(v, k4))
    return AB._nonlin(op)


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


def pair_op(xy, theta, xx, yy, same, diag, k4):
    """float64 (K', Θ', xx', yy') of one step on [n][hw] arrays: cgp_sin_* / cgp_var_sin_*"""
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))[:, None, None, :]   # noqa
    c, th, vx, vy = t(xy), t(theta), t(xx), t(yy)
    _, _, k, vx2, vy2 = _sin((bool(same), bool(diag), c, vx, vy), k4)
    kd = sin_kdot(c, vx, vy, bool(same), bool(diag), k4)
    flat = lambda v: v.reshape(-1, np.shape(xy)[1]).numpy()                      # noqa: E731
    return flat(k), flat(th * kd), flat(vx2), flat(vy2)


# ------------------------------------------------------------------------------------
# the pooled path: position-pair maps [m, p_row, p_col, q_row, q_col], both streams
# ------------------------------------------------------------------------------------
def sin_map(s, xx, yy, pi, pj, same, k4):
    """(K', κ̇) of (S[m][p, q], xx[pi[m]][p], yy[pj[m]][q]); with same, i = j and p = q: v' and
    its κ̇"""
    v1, v2 = PN._bcast(s, xx, yy, pi, pj)
    k, kd = sin_pair(s, v1, v2, k4)
    if same:
        mask = PO._self_mask(s, pi, pj)
        k = np.where(mask, sin_var(v1, k4), k)
        kd = np.where(mask, sin_var_kdot(v1, k4), kd)
    return k, kd


def _walk_maps(mod, st, pairs, eps=0.0):
    """st = (S_xy, S_xx, S_yy, pooled, Θ_xy or None for zero); pairs = (pair_i, pair_j, same)"""
    if isinstance(mod, cnn_gp.Sin):
        sxy, sxx, syy, pooled, th = st
        pi, pj, same = pairs
        assert not pooled, "a nonlinearity after the global pool has no definition here"
        k4 = consts_of(mod)
        ax, ay = np.arange(len(sxx)), np.arange(len(syy))
        xx, yy = AO.diag(sxx), AO.diag(syy)
        k, kd = sin_map(sxy, xx, yy, pi, pj, same, k4)
        return (k, sin_map(sxx, xx, xx, ax, ax, True, k4)[0],
                sin_map(syy, yy, yy, ay, ay, True, k4)[0], False,
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
    return AB._walk_maps(mod, st, pairs, eps)     # every other module, one at a time


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


def map_op(s, theta, xx, yy, pi, pj, same, k4):
    """float64 (K', Θ') of one step on position-pair maps [m, h, w, h, w]: cgp_sin_cov_*"""
    k, kd = sin_map(np.asarray(s, np.float64), np.asarray(xx, np.float64),
                    np.asarray(yy, np.float64), pi, pj, same, k4)
    return k, np.asarray(theta, np.float64) * kd
