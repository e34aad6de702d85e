"""Test-time oracle of the neural tangent kernel: torch float64 autograd over the oracle's
spec walker (oracle/specs.py, oracle/torch_cpu.py's conv / ReLU / sum restatements).

    Θ = Σ over all Conv2d outputs l of ⟨∂K_final/∂K_xy^l, K_xy^l⟩   at fixed variances

taken by the scale trick tests/golden/make_golden_ntk.py applies to the reference: each
conv output's pair maps are multiplied by a leaf of ones, one entry per pair, and K.sum()
is differentiated in the leaves.  Pairs with rho = 1 (x_i against itself with same=False)
are singular under autograd; same=True runs take them from the diagonal mode instead,
where the ReLU passes xx/2 on and both the xy and the xx stream carry the leaves.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_cpu as T


def _walk(spec, kp, scales, both):
    kind = spec[0]
    if kind == "conv":
        same, diag = kp[:2]
        xy, xx, yy = (T._conv(t, spec[1]) for t in kp[2:])
        s = torch.ones(xy.shape[0], 1, 1, 1, dtype=xy.dtype, requires_grad=True)
        scales.append(s)
        return (same, diag, xy * s, xx * s if both else xx, yy)
    if kind == "relu":
        return T._relu(kp)
    if kind == "seq":
        for m in spec[1]:
            kp = _walk(m, kp, scales, both)
        return kp
    if kind == "sum":
        return T._axpy([(None, _walk(m, kp, scales, both)) for m in spec[1]])
    if kind == "mix":
        lg = torch.tensor(spec[2], dtype=torch.float32).to(kp[2].dtype)
        pr = torch.softmax(lg, dim=0)
        return T._axpy([(pr[i], _walk(m, kp, scales, both)) for i, m in enumerate(spec[1])])
    raise ValueError(kind)


def _autograd(spec, x, y, same, diag):
    n1, n2 = x.shape[0], y.shape[0]
    if diag:
        xy = (x * y).mean(1, keepdim=True)
    else:
        xy = (x[:, None] * y[None]).mean(2).view(n1 * n2, 1, *x.shape[2:])
    xx = (x * x).mean(1, keepdim=True)
    yy = (y * y).mean(1, keepdim=True)
    scales = []
    kp = _walk(spec, (same, diag, xy, xx, yy), scales, same and diag)
    shape = (n1,) if diag else (n1, n2)
    k = kp[2].reshape(shape)
    theta = torch.zeros_like(k)
    if scales:
        for g in torch.autograd.grad(k.sum(), scales):
            theta = theta + g.view(shape)
    return k.detach().numpy(), theta.detach().numpy()


def ntk(spec, x, y=None, same=None, diag=False):
    """(K, Θ) as float64 numpy arrays, [N1, N2] or [N1] with diag.  x, y: [N, C, H, W]
    arrays or CPU tensors.  same=False pairs of identical images come out NaN."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    if y is None:
        assert same is None
        y, same = x, True
    else:
        y = torch.as_tensor(np.asarray(y), dtype=torch.float64)
    same, diag = bool(same), bool(diag)
    if same and not diag:
        k, th = _autograd(spec, x, x, False, False)
        kd, td = _autograd(spec, x, x, True, True)
        idx = np.arange(len(x))
        k[idx, idx], th[idx, idx] = kd, td
        return k, th
    return _autograd(spec, x, y, same, diag)


# ------------------------------------------------------------------------------------
# program.ntk_steps run with torch CPU ops: the recursion itself, launch by launch
# ------------------------------------------------------------------------------------
def conv_t(t, g, bias):
    zero = g.extent > g.taps
    kern = torch.full((1, 1, g.extent, g.extent), g.weight, dtype=t.dtype)
    if zero:
        kern[:, :, 0, :] = 0
        kern[:, :, :, 0] = 0
    pad = -g.offset + (g.dilation if zero else 0)
    return F.conv2d(t, kern, stride=g.stride, padding=pad, dilation=g.dilation) + bias


def variances(prog, v0, xx, yy, same):
    var = {v0: (xx, yy)}
    for op in prog.ops:
        if op.kind == "conv":
            var[op.dst] = tuple(conv_t(t, op.geom, op.geom.bias) for t in var[op.src])
        elif op.kind == "relu":
            x2 = var[op.src][0] / 2
            var[op.dst] = (x2, x2 if same else var[op.src][1] / 2)
        else:
            acc = None
            for coef, t in op.terms:
                c = 1.0 if coef is None else coef
                term = tuple(c * m for m in var[t])
                acc = term if acc is None else tuple(a + b for a, b in zip(acc, term))
            var[op.dst] = acc
    return var


def kdot(c, xx, yy, same, diag):
    """κ̇ = (π - θ)/2π on pair maps c [nmaps, 1, h, w]; 1/2 where the reference overrides"""
    n1, n2 = xx.shape[0], yy.shape[0]
    if diag:
        v1, v2, cc = xx, yy, c
    else:
        cc = c.view(n1, n2, *c.shape[-2:])
        v1, v2 = xx.view(n1, 1, *xx.shape[-2:]), yy.view(1, n2, *yy.shape[-2:])
    t = v1 * v2 + T.F32_TINY
    kd = (math.pi - torch.acos((cc * torch.rsqrt(t)).clamp(-1, 1))) / (2 * math.pi)
    if same:
        if diag:
            kd = torch.full_like(kd, 0.5)
        else:
            idx = torch.arange(n1)
            kd[idx, idx] = 0.5
    return kd.reshape(c.shape)


def run_steps(model, x, y=None, same=None, diag=False, dtype=torch.float64):
    """(K, Θ) of ntk_steps(compile_program(model)) as numpy arrays, every op a torch CPU
    op in ``dtype`` (float32: the reference's own production precision)."""
    from cnn_gp.program import compile_program, ntk_steps
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    if y is None:
        y, same = x, True
    else:
        y = torch.as_tensor(np.asarray(y)).to(dtype)
    n1, n2 = len(x), len(y)
    prog, v0, vf = compile_program(model, x.shape[2], x.shape[3])
    steps, kbuf, tbuf = ntk_steps(prog, v0, vf)
    if diag:
        xy = (x * y).mean(1, keepdim=True)
    else:
        xy = (x[:, None] * y[None]).mean(2).view(n1 * n2, 1, *x.shape[2:])
    var = variances(prog, v0, (x * x).mean(1, keepdim=True), (y * y).mean(1, keepdim=True), same)
    bufs = {("K", v0): xy}
    for st in steps:
        if st.fn == "conv":
            out = conv_t(bufs[st.src], st.op.geom, st.bias)
            bufs[st.dst] = out if st.addend is None else out + bufs[st.addend]
        elif st.fn in ("relu", "relu_ntk"):
            xx, yy = var[st.var]
            c = bufs[st.src]
            if st.fn == "relu_ntk":
                bufs[st.dst_theta] = bufs[st.theta] * kdot(c, xx, yy, same, diag)
            bufs[st.dst] = T._relu((same, diag, c, xx, yy))[2].reshape(c.shape)
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
