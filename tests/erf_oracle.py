"""Test-time oracle of networks with the erf nonlinearity: torch float64 on the CPU.

The reference has no Erf, so the oracle walks the module tree of a ``cnn_gp`` model itself:
Conv2d, ReLU, Sum and Mixture through oracle/torch_cpu.py's restatements of the reference
(_conv, _relu, _axpy), Erf through the closed form (Williams 1997 in its atan form)

    D = 1 + 2(v1 + v2) + 4(v1 v2 - c²),  K' = (2/π) atan(2c/√D),  κ̇ = ∂K'/∂c = (4/π)/√D
    v' = (2/π) atan(2v/√(1 + 4v))

without the library's D >= 1 guard, so autograd stays smooth.  K comes from the walk.  Θ
comes two ways:

* ``ntk_autograd``: the scale-leaf trick of tests/ntk_oracle.py (a leaf of ones on every
  conv output's xy, K.sum() differentiated in the leaves), always run as same=False so no
  override cuts the graph.  Valid on every pair of a pure-erf network, identical images
  included (erf has no singularity at rho = 1); in a network that also has a ReLU the pairs
  of identical images come out NaN, as ntk_oracle.ntk documents, and callers mask them.
* ``ntk_stepwise``: program.ntk_steps run launch by launch with torch ops, the erf steps
  with the closed-form κ̇ and the overrides (same and i = j, or same and diag: K' = v'[i],
  κ̇ = (4/π)/√(1 + 4v)).  For mixed networks and for same / diag.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import cnn_gp
from oracle import torch_cpu as T

import ntk_oracle as NT


def erf_pair(c, v1, v2):
    """(K', κ̇) of the erf map, elementwise, no guard."""
    s = torch.sqrt(1 + 2 * (v1 + v2) + 4 * (v1 * v2 - c * c))
    return (2 / math.pi) * torch.atan(2 * c / s), (4 / math.pi) / s


def erf_var(v):
    return (2 / math.pi) * torch.atan(2 * v / torch.sqrt(1 + 4 * v))


def _broadcast(xy, xx, yy, diag):
    n1, n2 = xx.shape[0], yy.shape[0]
    if diag:
        return xy, xx, yy
    return (xy.view(n1, n2, *xy.shape[-2:]), xx.view(n1, 1, *xx.shape[-2:]),
            yy.view(1, n2, *yy.shape[-2:]))


def _erf(kp):
    """T._relu's counterpart: (same, diag, xy', xx', yy') with the same overrides."""
    same, diag, xy, xx, yy = kp
    n1 = xx.shape[0]
    out, _ = erf_pair(*_broadcast(xy, xx, yy, diag))
    xx2 = erf_var(xx)
    if same:
        yy2 = xx2
        if diag:
            out = xx2
        else:
            idx = torch.arange(n1)
            out = out.clone()
            out[idx, idx] = xx2.view(n1, *xx2.shape[-2:])
    else:
        yy2 = erf_var(yy)
    if not diag:
        out = out.reshape(-1, 1, *out.shape[-2:])
    return (same, diag, out, xx2, yy2)


def conv_params(mod) -> dict:
    """The spec dict oracle/torch_cpu.py's _conv reads, from a cnn_gp.Conv2d."""
    return dict(kernel_size=mod.kernel_size, stride=mod.stride, dilation=mod.dilation,
                padding=mod._padding_arg, var_weight=mod.var_weight, var_bias=mod.var_bias)


def _walk(mod, kp, scales=None):
    if isinstance(mod, cnn_gp.Conv2d):
        p = conv_params(mod)
        xy, xx, yy = (T._conv(t, p) for t in kp[2:])
        if scales is not None:
            s = torch.ones(xy.shape[0], 1, 1, 1, dtype=xy.dtype, requires_grad=True)
            scales.append(s)
            xy = xy * s
        return kp[:2] + (xy, xx, yy)
    if isinstance(mod, cnn_gp.ReLU):
        return T._relu(kp)
    if isinstance(mod, cnn_gp.Erf):
        return _erf(kp)
    if isinstance(mod, cnn_gp.Sequential):
        for m in mod.mods:
            kp = _walk(m, kp, scales)
        return kp
    if isinstance(mod, cnn_gp.Sum):
        return T._axpy([(None, _walk(m, kp, scales)) for m in mod.mods])
    if isinstance(mod, cnn_gp.Mixture):
        pr = mod.proportions()
        return T._axpy([(pr[i], _walk(m, kp, scales)) for i, m in enumerate(mod.mods)])
    raise TypeError(type(mod).__name__)


def _inputs(x, y, same):
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    if y is None:
        assert same is None
        return x, x, True
    return x, torch.as_tensor(np.asarray(y), dtype=torch.float64), bool(same)


def _moments(x, y, diag):
    n1, n2 = x.shape[0], y.shape[0]
    if diag:
        xy = (x * y).mean(1, keepdim=True)
    else:
        xy = (x[:, None] * y[None]).mean(2).view(n1 * n2, 1, *x.shape[2:])
    return xy, (x * x).mean(1, keepdim=True), (y * y).mean(1, keepdim=True)


@torch.no_grad()
def kernel(model, x, y=None, same=None, diag=False):
    """K as a float64 numpy array, [N1, N2] or [N1] with diag."""
    x, y, same = _inputs(x, y, same)
    kp = _walk(model, (same, bool(diag)) + _moments(x, y, diag))
    return kp[2].reshape((len(x),) if diag else (len(x), len(y))).numpy()


def ntk_autograd(model, x, y=None, diag=False):
    """(K, Θ) by autograd with every pair evaluated as same=False (module docstring)."""
    x, y, _ = _inputs(x, y, None if y is None else False)
    scales = []
    kp = _walk(model, (False, bool(diag)) + _moments(x, y, diag), scales)
    shape = (len(x),) if diag else (len(x), len(y))
    k = kp[2].reshape(shape)
    theta = torch.zeros_like(k)
    if scales:
        for g in torch.autograd.grad(k.sum(), scales):
            theta = theta + g.view(shape)
    return k.detach().numpy(), theta.detach().numpy()


def _variances(prog, v0, xx, yy, same):
    var = {v0: (xx, yy)}
    for op in prog.ops:
        if op.kind == "conv":
            var[op.dst] = tuple(NT.conv_t(t, op.geom, op.geom.bias) for t in var[op.src])
        elif op.kind in ("relu", "erf"):
            f = erf_var if op.kind == "erf" else (lambda v: v / 2)
            x2 = f(var[op.src][0])
            var[op.dst] = (x2, x2 if same else f(var[op.src][1]))
        else:
            acc = None
            for coef, t in op.terms:
                c = 1.0 if coef is None else coef
                term = tuple(c * m for m in var[t])
                acc = term if acc is None else tuple(a + b for a, b in zip(acc, term))
            var[op.dst] = acc
    return var


def erf_kdot(c, xx, yy, same, diag):
    """κ̇ on pair maps c [nmaps, 1, h, w]; (4/π)/√(1 + 4v) where K' is overridden."""
    n1 = xx.shape[0]
    _, kd = erf_pair(*_broadcast(c, xx, yy, diag))
    over = (4 / math.pi) / torch.sqrt(1 + 4 * xx)
    if same:
        if diag:
            kd = over
        else:
            idx = torch.arange(n1)
            kd = kd.clone()
            kd[idx, idx] = over.view(n1, *over.shape[-2:])
    return kd.reshape(c.shape)


@torch.no_grad()
def ntk_stepwise(model, x, y=None, same=None, diag=False):
    """(K, Θ) of program.ntk_steps, every launch a torch float64 CPU op."""
    from cnn_gp.program import compile_program, ntk_steps
    x, y, same = _inputs(x, y, same)
    n1, n2 = len(x), len(y)
    prog, v0, vf = compile_program(model, x.shape[2], x.shape[3])
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    xy, xx, yy = _moments(x, y, diag)
    var = _variances(prog, v0, xx, yy, same)
    bufs = {("K", v0): xy}
    for st in steps:
        if st.fn == "conv":
            out = NT.conv_t(bufs[st.src], st.op.geom, st.bias)
            bufs[st.dst] = out if st.addend is None else out + bufs[st.addend]
        elif st.fn in ("relu", "relu_ntk", "erf", "erf_ntk"):
            vx, vy = var[st.var]
            c = bufs[st.src]
            erf = st.fn.startswith("erf")
            if st.fn.endswith("_ntk"):
                kd = (erf_kdot if erf else NT.kdot)(c, vx, vy, same, diag)
                bufs[st.dst_theta] = bufs[st.theta] * kd
            bufs[st.dst] = (_erf if erf else T._relu)((same, diag, c, vx, vy))[2].reshape(c.shape)
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
