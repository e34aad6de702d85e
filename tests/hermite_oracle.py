"""Test-time oracle of networks with a Hermite-series nonlinearity (cnn_gp.HermiteNonlin and its
subclasses Tanh, Sigmoid, Softplus, SiLU, GeluTanh): float64 on the CPU.

The reference has no such module.  For (u1, u2) ~ N(0, [[v1, c], [c, v2]]) and ρ = c/√(v1·v2),
Mehler's formula gives, with h_n = He_n/√n! and z ~ N(0, 1),

    K'  = E[φ(u1) φ(u2)]   = Σ_n a_n(v1)·a_n(v2)·ρⁿ      a_n(v)  = E_z[φ(√v·z)·h_n(z)]
    κ̇   = E[φ'(u1) φ'(u2)] = Σ_n a'_n(v1)·a'_n(v2)·ρⁿ    a'_n(v) = E_z[φ'(√v·z)·h_n(z)]
    v'  = Σ_n a_n(v)²                                     (K' at ρ = 1)

and the library truncates each sum at n = order and takes the expectations by a Gauss–Hermite
rule of quad_nodes nodes: that truncated, quadrature-built series is what this module writes
(``series``), from numpy's hermegauss, compressed to |z| <= 12.5 by the substitution z → s·z
(nodes s·z_q, weights s·w_q·exp((1 − s²)·z_q²/2); s = 1 where the rule ends inside already), and
a table h[n][q] of the three-term recurrence h_{n+1} = (z·h_n − √n·h_{n−1})/√(n+1).  ρ is 0 where v1·v2 is not positive and is clamped to
[−1, 1].  ``truth`` shares none of it: a two-dimensional 300 x 300 Gauss–Hermite rule on
u1,2 = √v1,2·(√((1+ρ)/2)·z1 ± √((1−ρ)/2)·z2); ``tail`` is E φ² − Σ_{n<=order} a_n², the bound
on what the truncation drops.  The closed forms of erf and GELU come from erf_oracle.py and
gelu_oracle.py.

Layer path (torch) and pooled path (numpy): the walks of sin_oracle.py, extended by import with
one module in the same way; Θ by ``ntk_stepwise`` (program.ntk_steps launch by launch) and by
the five-stream walk on position-pair maps.
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

PHIS = ("tanh", "sigmoid", "softplus", "silu", "gelu_tanh", "erf", "gelu")
# the library's function ids (CGP_HERMITE_*), written from the header
PHI_ID = {name: k for k, name in enumerate(PHIS)}
PHI_OF_ID = dict(enumerate(PHIS))


def _erf(x):
    flat = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    return torch.erf(torch.from_numpy(flat)).numpy().reshape(np.shape(x))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def phi(name, x, deriv=False):
    """φ(x), or φ'(x), of float64 arrays"""
    x = np.asarray(x, np.float64)
    if name == "tanh":
        t = np.tanh(x)
        return 1 - t * t if deriv else t
    if name == "sigmoid":
        s = _sigmoid(x)
        return s * _sigmoid(-x) if deriv else s
    if name == "softplus":
        return _sigmoid(x) if deriv else np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0)
    if name == "silu":
        s = _sigmoid(x)
        return s * (1 + x * _sigmoid(-x)) if deriv else x * s
    if name == "gelu_tanh":
        k = math.sqrt(2 / math.pi)
        t = np.tanh(k * (x + 0.044715 * x ** 3))
        if deriv:
            return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x)
        return 0.5 * x * (1 + t)
    if name == "erf":
        return 2 / math.sqrt(math.pi) * np.exp(-x * x) if deriv else _erf(x)
    if name == "gelu":
        cdf = 0.5 * (1 + _erf(x / math.sqrt(2)))
        return cdf + x * np.exp(-0.5 * x * x) / math.sqrt(2 * math.pi) if deriv else x * cdf
    raise ValueError(name)


def rule_of(mod):
    """(phi name, order, quad_nodes) of a module from its own attributes (not mod.rule())"""
    return str(mod.phi), int(mod.order), int(mod.quad_nodes)


# ------------------------------------------------------------------------------------
# coefficients and series (numpy float64)
# ------------------------------------------------------------------------------------
_TABLES = {}


def tables(order, nq):
    """(z [nq], w [nq] normalised by √(2π), h [order + 1][nq])"""
    key = (int(order), int(nq))
    if key not in _TABLES:
        z, w = np.polynomial.hermite_e.hermegauss(int(nq))
        s = min(1.0, 12.5 / np.abs(z).max())                 # the rule compressed to |z| <= 12.5
        z, w = s * z, s * w * np.exp((1 - s * s) * z * z / 2) / math.sqrt(2 * math.pi)
        h = np.empty((order + 1, nq))
        h[0] = 1.0
        h[1] = z
        for n in range(1, order):
            h[n + 1] = (z * h[n] - math.sqrt(n) * h[n - 1]) / math.sqrt(n + 1)
        _TABLES[key] = (z, w, h)
    return _TABLES[key]


def coefficients(v, rule, deriv=False):
    """a_n(v) (a'_n with deriv) for n = 0 .. order: [..., order + 1] of v [...]"""
    name, order, nq = rule
    z, w, h = tables(order, nq)
    v = np.asarray(v, np.float64)
    f = phi(name, np.sqrt(np.maximum(v, 0.0))[..., None] * z, deriv) * w
    return f @ h.T


def rho_of(c, v1, v2):
    t = v1 * v2
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(t > 0, c / np.sqrt(np.where(t > 0, t, 1.0)), 0.0)
    return np.clip(rho, -1.0, 1.0)


def _horner(x, y, rho):
    """Σ_n a_n·b_n·ρⁿ from n = order down; x = (a [u1, order + 1], index into u1), y likewise"""
    (a, ia), (b, ib) = x, y
    acc = np.zeros(np.broadcast(ia, ib, rho).shape)
    for n in range(a.shape[-1] - 1, -1, -1):
        acc = acc * rho + a[:, n][ia] * b[:, n][ib]
    return acc


def _indexed(v, rule, deriv=False):
    """the coefficients of the distinct values of v, and each element's row among them: equal
    variances get the same bits whatever the array's shape, and a map broadcast over pairs is
    integrated once per pixel"""
    u, inv = np.unique(v, return_inverse=True)
    return coefficients(u, rule, deriv), inv.reshape(np.shape(v))


def series(c, v1, v2, rule):
    """(K', κ̇) of the truncated series, elementwise over broadcastable float64 arrays"""
    c, v1, v2 = (np.asarray(t, np.float64) for t in (c, v1, v2))
    rho = rho_of(c, v1, v2)
    k = _horner(_indexed(v1, rule), _indexed(v2, rule), rho)
    kd = _horner(_indexed(v1, rule, True), _indexed(v2, rule, True), rho)
    return k, kd


def var(v, rule):
    """v' = Σ a_n(v)²"""
    a = coefficients(v, rule)
    return (a * a).sum(-1)


def var_kdot(v, rule):
    """κ̇ of a pair the library overrides with its own variance: Σ a'_n(v)²"""
    a = coefficients(v, rule, True)
    return (a * a).sum(-1)


# ------------------------------------------------------------------------------------
# the independent truth and the truncation tail
# ------------------------------------------------------------------------------------
def truth(name, v1, v2, rho, deriv=False, nodes=300):
    """E[φ(u1)·φ(u2)] (of φ' with deriv) at scalars (v1, v2, ρ) by a 2-D Gauss–Hermite rule"""
    z, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / math.sqrt(2 * math.pi)
    p, m = math.sqrt((1 + rho) / 2), math.sqrt((1 - rho) / 2)
    u1 = math.sqrt(v1) * (p * z[:, None] + m * z[None, :])
    u2 = math.sqrt(v2) * (p * z[:, None] - m * z[None, :])
    return float(w @ (phi(name, u1, deriv) * phi(name, u2, deriv)) @ w)


def second_moment(name, v, deriv=False, nodes=300):
    """E φ(√v·z)² by a 1-D rule"""
    z, w = np.polynomial.hermite_e.hermegauss(nodes)
    return float((w / math.sqrt(2 * math.pi)) @ phi(name, math.sqrt(v) * z, deriv) ** 2)


def tail(v, rule, deriv=False):
    """t(v) = E φ² − Σ_{n<=order} a_n(v)²: the weight of the dropped terms"""
    a = coefficients(v, rule, deriv)
    return second_moment(rule[0], v, deriv) - float((a * a).sum())


def closed_form(name, c, v1, v2):
    """(K', κ̇) of erf_oracle's / gelu_oracle's closed form on numpy arrays"""
    t = [torch.from_numpy(np.asarray(a, np.float64)) for a in np.broadcast_arrays(c, v1, v2)]
    k, kd = {"erf": EO.erf_pair, "gelu": GO.gelu_pair}[name](*t)
    return k.numpy(), kd.numpy()


# ------------------------------------------------------------------------------------
# torch in, torch out (the layer path's walk runs on tensors)
# ------------------------------------------------------------------------------------
def _np(t):
    return t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def _like(a, ref):
    return torch.from_numpy(np.ascontiguousarray(a)) if isinstance(ref, torch.Tensor) else a


def hermite_pair(c, v1, v2, rule):
    k, kd = series(_np(c), _np(v1), _np(v2), rule)
    return _like(k, c), _like(kd, c)


def hermite_var(v, rule):
    return _like(var(_np(v), rule), v)


def hermite_var_kdot(v, rule):
    return _like(var_kdot(_np(v), rule), v)


# ------------------------------------------------------------------------------------
# the layer path
# ------------------------------------------------------------------------------------
def _hermite(kp, rule):
    """T._relu's counterpart: (same, diag, xy', xx', yy') with the same overrides."""
    same, diag, xy, xx, yy = kp
    out, _ = hermite_pair(*EO._broadcast(xy, xx, yy, diag), rule)
    xx2 = hermite_var(xx, rule)
    out = GO._override(out, xx2, same, diag, xx.shape[0])
    if not diag:
        out = out.reshape(-1, 1, *out.shape[-2:])
    return (same, diag, out, xx2, xx2 if same else hermite_var(yy, rule))


def hermite_kdot(c, xx, yy, same, diag, rule):
    """κ̇ on pair maps c [nmaps, 1, h, w], hermite_var_kdot where K' is overridden"""
    _, kd = hermite_pair(*EO._broadcast(c, xx, yy, diag), rule)
    return GO._override(kd, hermite_var_kdot(xx, rule), same, diag, xx.shape[0]).reshape(c.shape)


def _walk(mod, kp, scales=None):
    if isinstance(mod, cnn_gp.HermiteNonlin):
        return _hermite(kp, rule_of(mod))
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            kp = _walk(m, kp, scales)
        return kp
    if isinstance(mod, (cnn_gp.Sum, cnn_gp.Mixture)):
        pr = mod.proportions() if isinstance(mod, cnn_gp.Mixture) else [None] * len(mod.mods)
        return T._axpy([(pr[i], _walk(m, kp, scales)) for i, m in enumerate(mod.mods)])
    return AB._walk(mod, kp, scales)          # Conv2d and the closed-form nonlinearities


@torch.no_grad()
def kernel(model, x, y=None, same=None, diag=False):
    """K as a float64 numpy array, [N1, N2] or [N1] with diag."""
    x, y, same = EO._inputs(x, y, same)
    kp = _walk(model, (same, bool(diag)) + EO._moments(x, y, diag))
    return kp[2].reshape((len(x),) if diag else (len(x), len(y))).numpy()


def _nonlin(op):
    """(the step on (same, diag, xy, xx, yy), κ̇, the variance map) of a nonlinearity op"""
    if op.kind == "hermite":
        rule = (PHI_OF_ID[op.rule[0]],) + tuple(op.rule[1:])
        return (lambda kp: _hermite(kp, rule),
                lambda c, vx, vy, same, diag: hermite_kdot(c, vx, vy, same, diag, rule),
                lambda v: hermite_var(v, rule))
    return AB._nonlin(op)


def variances(prog, v0, xx, yy, same):
    """value -> (xx, yy) variance maps of every value of the program (torch, [n, 1, h, w])"""
    var_ = {v0: (xx, yy)}
    for op in prog.ops:
        if op.kind == "conv":
            var_[op.dst] = tuple(NT.conv_t(t, op.geom, op.geom.bias) for t in var_[op.src])
        elif op.kind == "add":
            acc = None
            for coef, t in op.terms:
                c = 1.0 if coef is None else coef
                term = tuple(c * m for m in var_[t])
                acc = term if acc is None else tuple(a + b for a, b in zip(acc, term))
            var_[op.dst] = acc
        else:
            f = _nonlin(op)[2]
            x2 = f(var_[op.src][0])
            var_[op.dst] = (x2, x2 if same else f(var_[op.src][1]))
    return var_


@torch.no_grad()
def nonlin_input_variances(model, x):
    """The variance maps every nonlinearity of a layer-path model reads on images x: a list of
    float64 arrays, one per nonlinearity op"""
    from cnn_gp.program import NONLIN_KINDS, compile_program
    x, _, _ = EO._inputs(x, None, None)
    prog, v0, _ = compile_program(model, x.shape[2], x.shape[3])
    _, xx, _ = EO._moments(x, x, True)
    var_ = variances(prog, v0, xx, xx, True)
    return [var_[op.src][0].numpy() for op in prog.ops if op.kind in NONLIN_KINDS]


@torch.no_grad()
def ntk_stepwise(model, x, y=None, same=None, diag=False):
    """(K, Θ) of program.ntk_steps, every launch a torch float64 CPU op."""
    from cnn_gp.program import compile_program, ntk_steps
    x, y, same = EO._inputs(x, y, same)
    n1, n2 = len(x), len(y)
    prog, v0, vf = compile_program(model, x.shape[2], x.shape[3])
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    xy, xx, yy = EO._moments(x, y, diag)
    var_ = variances(prog, v0, xx, yy, same)
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
            vx, vy = var_[st.var]
            c = bufs[st.src]
            if st.fn.endswith("_ntk"):
                bufs[st.dst_theta] = bufs[st.theta] * kdot(c, vx, vy, same, diag)
            bufs[st.dst] = step((same, diag, c, vx, vy))[2].reshape(c.shape)
    shape = (n1,) if diag else (n1, n2)
    k = bufs[kbuf].reshape(shape)
    th = torch.zeros_like(k) if tbuf is None else bufs[tbuf].reshape(shape)
    return k.numpy(), th.numpy()


def pair_op(xy, theta, xx, yy, same, diag, rule):
    """float64 (K', Θ', xx', yy') of one step on [n][hw] arrays: cgp_hermite_* /
    cgp_var_hermite_*"""
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))[:, None, None, :]   # noqa
    c, th, vx, vy = t(xy), t(theta), t(xx), t(yy)
    _, _, k, vx2, vy2 = _hermite((bool(same), bool(diag), c, vx, vy), rule)
    kd = hermite_kdot(c, vx, vy, bool(same), bool(diag), rule)
    flat = lambda v: v.reshape(-1, np.shape(xy)[1]).numpy()                      # noqa: E731
    return flat(k), flat(th * kd), flat(vx2), flat(vy2)


# ------------------------------------------------------------------------------------
# the pooled path: position-pair maps [m, p_row, p_col, q_row, q_col], both streams
# ------------------------------------------------------------------------------------
def hermite_map(s, xx, yy, pi, pj, same, rule):
    """(K', κ̇) of (S[m][p, q], xx[pi[m]][p], yy[pj[m]][q]); with same, i = j and p = q: v' and
    its κ̇"""
    v1, v2 = PN._bcast(s, xx, yy, pi, pj)
    k, kd = series(s, v1, v2, rule)
    if same:
        mask = PO._self_mask(s, pi, pj)
        k = np.where(mask, var(v1, rule), k)
        kd = np.where(mask, var_kdot(v1, rule), kd)
    return k, kd


def _walk_maps(mod, st, pairs, eps=0.0):
    """st = (S_xy, S_xx, S_yy, pooled, Θ_xy or None for zero); pairs = (pair_i, pair_j, same)"""
    if isinstance(mod, cnn_gp.HermiteNonlin):
        sxy, sxx, syy, pooled, th = st
        pi, pj, same = pairs
        assert not pooled, "a nonlinearity after the global pool has no definition here"
        rule = rule_of(mod)
        ax, ay = np.arange(len(sxx)), np.arange(len(syy))
        xx, yy = AO.diag(sxx), AO.diag(syy)
        k, kd = hermite_map(sxy, xx, yy, pi, pj, same, rule)
        return (k, hermite_map(sxx, xx, xx, ax, ax, True, rule)[0],
                hermite_map(syy, yy, yy, ay, ay, True, rule)[0], False,
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


def map_op(s, theta, xx, yy, pi, pj, same, rule):
    """float64 (K', Θ') of one step on position-pair maps [m, h, w, h, w]: cgp_hermite_cov_*"""
    k, kd = hermite_map(np.asarray(s, np.float64), np.asarray(xx, np.float64),
                        np.asarray(yy, np.float64), pi, pj, same, rule)
    return k, np.asarray(theta, np.float64) * kd
