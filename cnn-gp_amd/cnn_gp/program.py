"""Compile an NNGP module tree into a fused device program and run it.

The reference evaluates ``Sequential.propagate`` recursively (cnn_gp/kernels.py:184-187),
issuing 3 ``F.conv2d`` + a bias pass per Conv2d and ~14 pointwise ops per ReLU on the
whole [N1·N2, 1, H, W] covariance tensor.  Here the tree is flattened once into SSA form

    v0 = moments(x, y)               kernels.py:44-49
    v  = conv(u, geometry)           kernels.py:92-98
    v  = tapconv(u, geometry, W)     the same with a kernel buffer that is not the constant
                                     box: its own launch on every path
    v  = relu(u)                     kernels.py:134-165
    v  = erf(u)                      Erf (no reference counterpart)
    v  = gelu(u)                     Gelu (no reference counterpart)
    v  = abrelu(u; a, b)             ABReLU / LeakyReLU (no reference counterpart)
    v  = sin(u; A, B, C, D)          Sin / Cos / Rbf (no reference counterpart)
    v  = hermite(u; phi, N, Q)       HermiteNonlin: Tanh, Sigmoid, Softplus, SiLU, GeluTanh (no
                                     reference counterpart)
    v  = add[(coef, u), ...]         Sum (kernels.py:252-254) / Mixture (:220-225)
    v  = pool(u)                     GlobalAvgPool (no reference counterpart; DESIGN §3.3:
                                     such a program runs on position-pair maps, pool_steps)
    v  = avgpool(u, k, stride)       AvgPool2d (no reference counterpart; DESIGN §3.4: on
                                     position-pair maps as well)
    v  = corrconv(u, geom, R)        CorrelatedConv2d (no reference counterpart; DESIGN §3.5:
                                     on position-pair maps as well)

and then split into two device pipelines:

* the VARIANCE pipeline runs every op, unfused, on the per-image maps [xx | yy]
  ((N1 + N2) maps — negligible next to the N1·N2 pair maps) and keeps the variances
  of every value a ReLU, Erf, Gelu, ABReLU or Sin consumes;
* the PAIR pipeline runs on the N1·N2 maps with ops fused so each HBM pass does the
  most work:  [ReLU|moments] → Conv → [ReLU] → [+ addend]  is ONE kernel
  (cgp_conv_*), a ReLU not adjacent to a single-use conv is cgp_relu_* (+ addend),
  an Erf, a Gelu, an ABReLU or a Sin is always its own pass cgp_erf_* / cgp_gelu_* /
  cgp_abrelu_* / cgp_sin_* (+ addend), and only sums that cannot be folded into their producer
  run as cgp_axpby_*.

Fusion changes no arithmetic: each fused stage performs exactly the operations of the
op it replaces (a + b == b + a in IEEE, so folding a Sum into either branch is exact).

Every run on pair maps is lowered once per plan to a list of Step records, each with the
buffers to drop after it: layer_steps (the fused forward run) and ntk_steps (K and Θ through
the unfused program) run in Plan.run_layer_steps; pool_steps and pool_ntk_steps, on
position-pair maps, in Plan.run_cov_steps.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import numpy as np
import torch

from . import _native as N


# ------------------------------------------------------------------------------------
# IR
# ------------------------------------------------------------------------------------
@dataclasses.dataclass
class ConvGeom:
    taps: int
    offset: int
    stride: int
    dilation: int
    weight: float       # the kernel buffer's value (fp32-rounded unless built in fp64)
    bias: float
    extent: int = 0     # the reference kernel's edge (k + 1 for an even "same" kernel)


@dataclasses.dataclass
class PoolGeom:
    """An AvgPool2d's window: kernel_size and stride (no padding)."""
    taps: int
    stride: int


@dataclasses.dataclass
class CorrGeom(ConvGeom):
    """A CorrelatedConv2d: ConvGeom (weight = var_weight/k² in double) plus the two k x k
    tap correlation matrices, tuples of tuples of float."""
    corr_rows: tuple = ()
    corr_cols: tuple = ()


@dataclasses.dataclass
class TapGeom:
    """A Conv2d whose kernel buffer is not the constant box: the buffer's edge
    (k + 1 for an even "same" kernel, whose first row and column are taps like any other
    here), offset = -padding, and the buffer itself as a tuple of tuples of float, read once
    in double."""
    extent: int
    offset: int
    stride: int
    dilation: int
    bias: float
    table: tuple = ()


@dataclasses.dataclass
class Op:
    # 'conv' | 'tapconv' | 'relu' | 'erf' | 'gelu' | 'abrelu' | 'sin' | 'hermite' | 'add' |
    # 'pool' | 'avgpool' | 'corrconv' | 'moments'
    kind: str
    dst: int
    src: Optional[int] = None
    # conv: ConvGeom, tapconv: TapGeom, avgpool: PoolGeom, corrconv: CorrGeom
    geom: Optional[object] = None
    shape_in: tuple = (0, 0)
    shape_out: tuple = (0, 0)
    terms: list = dataclasses.field(default_factory=list)   # add: [(coef|None, value)]
    # fusion (pair pipeline only)
    pre: int = N.CGP_PRE_NONE
    pre_var: Optional[int] = None          # value whose variances feed the PRE ReLU
    post: int = N.CGP_POST_NONE
    post_var: Optional[int] = None
    addend: Optional[int] = None
    # abrelu: the slopes (a, b) and the kernels' constants (s, m, h) =
    # ((a − b)², a·b, (a² + b²)/2), computed in double
    slopes: Optional[tuple] = None
    smh: Optional[tuple] = None
    # sin: the kernels' constants (A, B, C, D) = (a²/2, b²/2, cos 2θ, a²b²/2), computed in double
    consts: Optional[tuple] = None
    # hermite: (function id, order, quad_nodes) of the series (HermiteNonlin.rule)
    rule: Optional[tuple] = None


class Program:
    """Flattened SSA program for one module tree at one input size."""

    def __init__(self):
        self.ops: list[Op] = []
        self.shapes: dict[int, tuple] = {}
        self.n_values = 0

    def new_value(self, shape) -> int:
        v = self.n_values
        self.n_values += 1
        self.shapes[v] = tuple(shape)
        return v


def conv_geometry(mod) -> ConvGeom:
    """Conv2d.__init__'s padding rules (kernels.py:71-88) as tap offsets."""
    k, d, s = int(mod.kernel_size), int(mod.dilation), int(mod.stride)
    pad = int(mod.padding)
    offset = -pad + (d if mod.kernel_has_row_of_zeros else 0)
    kern = mod.kernel.detach().to("cpu", torch.float64).reshape(mod.kernel.shape[-2:])
    w = float(kern[-1, -1])
    want = torch.full_like(kern, w)
    if mod.kernel_has_row_of_zeros:
        want[0, :] = 0.
        want[:, 0] = 0.
    if tuple(mod.kernel.shape[:2]) != (1, 1) or not torch.equal(kern, want):
        # the HIP kernels run the reference's constant box kernel (kernels.py:75-87); a
        # buffer edited to anything else has no device path
        raise NotImplementedError(
            "Conv2d.kernel must be the constant var_weight/k² box (kernels.py:75-87), with "
            "the zero first row and column of an even 'same' kernel; got a buffer of shape "
            f"{tuple(mod.kernel.shape)} that is not")
    return ConvGeom(taps=k, offset=offset, stride=s, dilation=d, weight=w,
                    extent=k + 1 if mod.kernel_has_row_of_zeros else k,
                    bias=float(mod.var_bias))


def tap_geometry(mod) -> TapGeom:
    """The geometry of a Conv2d whose kernel buffer conv_geometry refuses: any finite buffer
    of the buffer's own shape (1, 1, ke, ke), as F.conv2d reads it (kernels.py:92-97).
    NotImplementedError naming the shape for another shape, ValueError for a non-finite
    entry."""
    k = int(mod.kernel_size)
    ke = k + 1 if mod.kernel_has_row_of_zeros else k
    if tuple(mod.kernel.shape) != (1, 1, ke, ke):
        raise NotImplementedError(
            f"Conv2d.kernel must keep its shape (1, 1, {ke}, {ke}) (kernel_size={k}, padding="
            f"{mod._padding_arg!r}); got a buffer of shape {tuple(mod.kernel.shape)}")
    kern = mod.kernel.detach().to("cpu", torch.float64).reshape(ke, ke)
    if not bool(torch.isfinite(kern).all()):
        raise ValueError(f"Conv2d.kernel has a non-finite entry: {kern.tolist()}")
    return TapGeom(extent=ke, offset=-int(mod.padding), stride=int(mod.stride),
                   dilation=int(mod.dilation), bias=float(mod.var_bias),
                   table=tuple(tuple(float(v) for v in row) for row in kern.tolist()))


def conv_out_hw(mod, h: int, w: int):
    """F.conv2d output size for Conv2d `mod` (kernel extent k+1 for even 'same')."""
    k, d, s, p = int(mod.kernel_size), int(mod.dilation), int(mod.stride), int(mod.padding)
    keff = k + 1 if mod.kernel_has_row_of_zeros else k
    ho = (h + 2 * p - d * (keff - 1) - 1) // s + 1
    wo = (w + 2 * p - d * (keff - 1) - 1) // s + 1
    if ho <= 0 or wo <= 0:
        raise RuntimeError(f"Conv2d(kernel_size={k}, stride={s}, padding={p}, dilation={d}) "
                           f"produces an empty output from a {h}x{w} input")
    return ho, wo


def avgpool_out_hw(mod, h: int, w: int):
    """torch.nn.AvgPool2d's output size without padding: floor((h - k)/s) + 1 per side."""
    k, s = int(mod.kernel_size), int(mod.stride)
    if k < 1 or s < 1:
        raise ValueError(f"AvgPool2d(kernel_size={k}, stride={s}): both must be at least 1")
    ho, wo = (h - k) // s + 1, (w - k) // s + 1
    if ho <= 0 or wo <= 0:
        raise RuntimeError(f"AvgPool2d(kernel_size={k}, stride={s}) produces an empty output "
                           f"from a {h}x{w} input")
    return ho, wo


def corrconv_geometry(mod) -> CorrGeom:
    """Conv2d's padding rules as tap offsets (conv_geometry) for a CorrelatedConv2d; the
    scale is var_weight/k² in double."""
    k, d, s = int(mod.kernel_size), int(mod.dilation), int(mod.stride)
    if s < 1 or d < 1:
        raise ValueError(f"CorrelatedConv2d(stride={s}, dilation={d}): both must be at least 1")
    offset = -int(mod.padding) + (d if mod.kernel_has_row_of_zeros else 0)
    return CorrGeom(taps=k, offset=offset, stride=s, dilation=d,
                    weight=float(mod.var_weight) / (k * k), bias=float(mod.var_bias),
                    extent=k + 1 if mod.kernel_has_row_of_zeros else k,
                    corr_rows=mod.corr_rows, corr_cols=mod.corr_cols)


def _emit(prog: Program, mod, v: int) -> int:
    """Append the ops of `mod` applied to value v; return the output value."""
    from . import kernels as K
    if isinstance(mod, K.CorrelatedConv2d):
        h, w = prog.shapes[v]
        ho, wo = conv_out_hw(mod, h, w)
        out = prog.new_value((ho, wo))
        prog.ops.append(Op("corrconv", out, src=v, geom=corrconv_geometry(mod),
                           shape_in=(h, w), shape_out=(ho, wo)))
        return out
    if isinstance(mod, K.Conv2d):
        h, w = prog.shapes[v]
        ho, wo = conv_out_hw(mod, h, w)
        out = prog.new_value((ho, wo))
        # the box first, by conv_geometry's own comparison (its one k x k copy to the host):
        # a model of boxes compiles as it always did.  Any other buffer is a tapconv, which
        # no fast path knows (fuse, NetPlan and _var_chain match "conv")
        try:
            kind, geom = "conv", conv_geometry(mod)
        except NotImplementedError:
            kind, geom = "tapconv", tap_geometry(mod)
        prog.ops.append(Op(kind, out, src=v, geom=geom, shape_in=(h, w), shape_out=(ho, wo)))
        return out
    # one table from module class to elementwise kind (LeakyReLU is an ABReLU; Cos and Rbf
    # are Sins)
    kind = next((k for cls, k in ((K.ReLU, "relu"), (K.Erf, "erf"), (K.Gelu, "gelu"),
                                  (K.ABReLU, "abrelu"), (K.Sin, "sin"),
                                  (K.HermiteNonlin, "hermite"))
                 if isinstance(mod, cls)), None)
    if kind is not None:
        out = prog.new_value(prog.shapes[v])
        consts = dict(slopes=(float(mod.a), float(mod.b)), smh=mod.constants()) \
            if kind == "abrelu" else dict(consts=mod.constants()) if kind == "sin" else \
            dict(rule=mod.rule()) if kind == "hermite" else {}
        prog.ops.append(Op(kind, out, src=v, shape_in=prog.shapes[v], shape_out=prog.shapes[v],
                           **consts))
        return out
    if isinstance(mod, K.GlobalAvgPool):
        out = prog.new_value((1, 1))
        prog.ops.append(Op("pool", out, src=v, shape_in=prog.shapes[v], shape_out=(1, 1)))
        return out
    if isinstance(mod, K.AvgPool2d):
        h, w = prog.shapes[v]
        ho, wo = avgpool_out_hw(mod, h, w)
        out = prog.new_value((ho, wo))
        prog.ops.append(Op("avgpool", out, src=v, shape_in=(h, w), shape_out=(ho, wo),
                           geom=PoolGeom(int(mod.kernel_size), int(mod.stride))))
        return out
    if isinstance(mod, K.Sequential):
        for m in mod.mods:
            v = _emit(prog, m, v)
        return v
    if isinstance(mod, (K.Sum, K.Mixture)):
        outs = [_emit(prog, m, v) for m in mod.mods]
        shp = {prog.shapes[o] for o in outs}
        if len(shp) != 1:
            raise RuntimeError(f"{type(mod).__name__} branches disagree on spatial size: {shp}")
        if isinstance(mod, K.Sum):
            if len(outs) == 1:
                return outs[0]          # 0 + kp == kp
            terms = [(None, o) for o in outs]
        else:
            props = mod.proportions()
            terms = [(props[i], o) for i, o in enumerate(outs)]
        out = prog.new_value(shp.pop())
        prog.ops.append(Op("add", out, terms=terms, shape_in=prog.shapes[out],
                           shape_out=prog.shapes[out]))
        return out
    if isinstance(mod, K.NNGPKernel):
        raise TypeError(f"no device lowering for {type(mod).__name__}")
    raise TypeError(f"not an NNGP kernel module: {type(mod).__name__}")


def compile_program(model, h: int, w: int) -> tuple:
    """Returns (Program, v0, v_final)."""
    prog = Program()
    v0 = prog.new_value((h, w))
    vf = _emit(prog, model, v0)
    return prog, v0, vf


# ------------------------------------------------------------------------------------
# fusion for the pair pipeline
# ------------------------------------------------------------------------------------
def _uses(ops, final):
    u = {}
    for op in ops:
        srcs = [op.src] if op.src is not None else []
        srcs += [t for _, t in op.terms]
        if op.addend is not None:
            srcs.append(op.addend)
        for s in srcs:
            u[s] = u.get(s, 0) + 1
    u[final] = u.get(final, 0) + 1
    return u


def fuse(prog: Program, v0: int, vf: int, enable: bool = True, pre_relu: bool = True,
         fold_moments: bool = True) -> list:
    """Return the fused op list for the pair pipeline (prog.ops is left untouched).
    ``pre_relu`` / ``fold_moments`` enable rules 3 / 4 (the whole-network kernel keeps
    standalone ReLU and moments ops: in LDS they cost no extra memory pass).  An erf, gelu,
    abrelu or sin op is never a conv's pre- or post-stage (rules 1 and 3 match ReLU only); rule 2 may
    give it an addend."""
    ops = [dataclasses.replace(o, terms=list(o.terms)) for o in prog.ops]
    if not enable:
        return ops
    producer = lambda ops_, v: next((i for i, o in enumerate(ops_) if o.dst == v), None)  # noqa

    # 1. conv -> relu  ==> conv(post=RELU)
    changed = True
    while changed:
        changed = False
        uses = _uses(ops, vf)
        for ri, r in enumerate(ops):
            if r.kind != "relu" or r.addend is not None:
                continue
            pi = producer(ops, r.src)
            if pi is None:
                continue
            c = ops[pi]
            if c.kind == "conv" and c.post == N.CGP_POST_NONE and c.addend is None \
                    and uses.get(r.src, 0) == 1:
                c.post, c.post_var, c.dst = N.CGP_POST_RELU, r.src, r.dst
                del ops[ri]
                changed = True
                break

    # 2. plain 2-term Sum folded into the producer of one term as its epilogue addend
    changed = True
    while changed:
        changed = False
        uses = _uses(ops, vf)
        for ai, a in enumerate(ops):
            if a.kind != "add" or len(a.terms) != 2 or any(c is not None for c, _ in a.terms):
                continue
            (_, t0), (_, t1) = a.terms
            for cand, other in ((t1, t0), (t0, t1)):
                pi = producer(ops, cand)
                if pi is None or ops[pi].kind not in ("conv",) + NONLIN_KINDS or \
                        ops[pi].addend is not None or uses.get(cand, 0) != 1:
                    continue
                oi = producer(ops, other)
                if oi is not None and oi > pi:
                    continue                    # the addend must exist before the producer
                if oi is not None and ops[oi].kind == "corrconv":
                    continue                    # a Sum with a CorrelatedConv2d runs as axpby
                if cand == other:
                    continue
                ops[pi].addend, ops[pi].dst = other, a.dst
                del ops[ai]
                changed = True
                break
            if changed:
                break

    # 3. relu -> conv  ==> conv(pre=RELU) when the relu output has no other consumer
    changed = pre_relu
    while changed:
        changed = False
        uses = _uses(ops, vf)
        for ci, c in enumerate(ops):
            if c.kind != "conv" or c.pre != N.CGP_PRE_NONE:
                continue
            ri = producer(ops, c.src)
            if ri is None:
                continue
            r = ops[ri]
            if r.kind == "relu" and r.addend is None and uses.get(c.src, 0) == 1:
                c.pre, c.pre_var, c.src = N.CGP_PRE_RELU, r.src, r.src
                c.shape_in = r.shape_in
                del ops[ri]
                changed = True
                break

    # 4. the input moments folded into a single consuming conv
    uses = _uses(ops, vf)
    if fold_moments and uses.get(v0, 0) == 1 and vf != v0:
        for c in ops:
            if c.kind == "conv" and c.src == v0 and c.pre == N.CGP_PRE_NONE:
                c.pre = N.CGP_PRE_MOMENTS
                break
    return ops


# the op kinds that read the per-image variances of their source
NONLIN_KINDS = ("relu", "erf", "gelu", "abrelu", "sin", "hermite")

# The layer-path entry point cgp_<name>_* of every nonlinearity: its argument class, that
# class's K' output field, whether the record takes the ReLU evaluation flags, the record's
# fields for the op's constants (an abrelu's (s, m, h), a sin's (A, B, C, D)), and what
# cgp_var_<kind>_* takes between `same` and its outputs.  The ReLU alone
# has an entry point of its own for the two-stream form; the others take theta or NULL.
NONLIN_CALLS = {
    "relu": (N.ReluArgs, "out", True, None, lambda op: ()),
    "relu_ntk": (N.ReluNtkArgs, "out_xy", True, None, None),
    "erf": (N.ErfArgs, "out_xy", False, None, lambda op: ()),
    "gelu": (N.GeluArgs, "out_xy", False, None, lambda op: ()),
    "abrelu": (N.ABReluArgs, "out_xy", True, lambda op: zip("smh", op.smh),
               lambda op: (op.smh[2],)),
    "sin": (N.SinArgs, "out_xy", False, lambda op: zip("ABCD", op.consts),
            lambda op: op.consts),
    # the record's tables and cgp_var_hermite_*'s node table live on a device: Plan fills them
    # in (_hermite_tables, _hermite_nodes)
    "hermite": (N.HermiteArgs, "out_xy", False, None, lambda op: op.rule),
}


def needed_variances(ops) -> set:
    need = set()
    for o in ops:
        if o.kind in NONLIN_KINDS:
            need.add(o.src)
        if o.pre == N.CGP_PRE_RELU:
            need.add(o.pre_var)
        if o.post == N.CGP_POST_RELU:
            need.add(o.post_var)
    return need


# ------------------------------------------------------------------------------------
# the neural tangent kernel: a second pair map Θ beside K
# ------------------------------------------------------------------------------------
@dataclasses.dataclass
class Step:
    """One launch of a lowered run: of the layer path's lists (layer_steps, ntk_steps: pair
    maps, Plan.run_layer_steps) or of a list on position-pair maps (pool_steps,
    pool_ntk_steps, Plan.run_cov_steps).  pool_steps names a buffer by the SSA value it holds;
    the other three by ("K", v) / ("T", v), the K and Θ maps of value v, with v = ("pre", d)
    in pool_ntk_steps for the conv output that a fused addend replaced in the forward program.
    ``free``: the buffers nothing reads after this launch (_schedule).

    The layer path's lists hold
    fn "conv":     dst = A(src)·weight + bias [+ addend]     cgp_conv_* (op.geom; ``bias``
                   replaces the geometry's: 0 on the Θ stream).  In layer_steps op is the FUSED
                   op, with its pre / post stages and their variances, and src is None where
                   the stage is the input moments (the conv reads the images)
    fn "tapconv":  dst = A_W(src) + bias [+ addend], the conv of a kernel buffer that is not
                   the box (op.geom: TapGeom; ``bias`` as for "conv")     cgp_tapconv_*
    fn "relu":     dst = relu(src) [+ addend], variances of value ``var``  cgp_relu_*
    fn "relu_ntk": dst, dst_theta = relu(src), theta·κ̇                   cgp_relu_ntk_*
    fn "erf":      dst = erf(src) [+ addend], variances of ``var``       cgp_erf_* (theta NULL)
    fn "erf_ntk":  dst, dst_theta = erf(src), theta·κ̇                    cgp_erf_*
    fn "gelu":     dst = gelu(src) [+ addend], variances of ``var``      cgp_gelu_* (theta NULL)
    fn "gelu_ntk": dst, dst_theta = gelu(src), theta·κ̇                   cgp_gelu_*
    fn "abrelu":   dst = abrelu(src; op.smh) [+ addend], variances of ``var``
                                                                         cgp_abrelu_* (theta NULL)
    fn "abrelu_ntk": dst, dst_theta = abrelu(src), theta·κ̇               cgp_abrelu_*
    fn "sin":      dst = sin(src; op.consts) [+ addend], variances of ``var``
                                                                         cgp_sin_* (theta NULL)
    fn "sin_ntk":  dst, dst_theta = sin(src), theta·κ̇                    cgp_sin_*
    fn "hermite":  dst = hermite(src; op.rule) [+ addend], variances of ``var``: the
                   coefficient tables of ``var`` (cgp_hermite_coef_*), then
                                                                         cgp_hermite_* (theta NULL)
    fn "hermite_ntk": dst, dst_theta = hermite(src), theta·κ̇: the tables of φ and φ', then
                                                                         cgp_hermite_*
    fn "axpby":    dst = Σ coef·buffer over ``terms`` (coef None: 1)     cgp_axpby_*

    Either list on position-pair maps may hold
    fn "moments": dst = mean_c x[c, p]·y[c, q]                          cgp_cov_moments_*
    fn "conv":    dst = A(src)·weight + bias [→ ReLU, variances of value ``var``]
                  [+ addend]; ``bias`` replaces the geometry's (0 on the Θ stream)
                                                                         cgp_cov_conv_*
    fn "nonlin":  dst = relu / erf (``post``) of src, variances of value ``var``
                  [+ addend]                                             cgp_cov_nonlin_*
    fn "gelu":    dst = gelu of src, variances of value ``var`` [+ addend]
                                                                         cgp_gelu_cov_*
    fn "abrelu":  dst = abrelu of src (op.smh), variances of value ``var`` [+ addend]
                                                                         cgp_abrelu_cov_*
    fn "sin":     dst = sin of src (op.consts), variances of value ``var`` [+ addend]
                                                                         cgp_sin_cov_*
    fn "hermite": dst = hermite of src (op.rule), variances of value ``var`` [+ addend]: the
                  coefficient tables of ``var`` (cgp_hermite_coef_*), then
                                                                         cgp_hermite_cov_*
    fn "pool":    dst = mean over (p, q) of src                          cgp_cov_pool_*
    fn "avgpool": dst = mean of src over the windows of p and of q (op.geom)
                                                                         cgp_covmap_avgpool_*
    fn "corrconv": dst = the correlated-weight conv of src (op.geom, ``bias``)
                                                                         cgp_corrconv_*
    fn "tapconv": dst = A_W(src) + bias [+ addend] (op.geom: TapGeom)    cgp_tapconv_cov_*
    fn "axpby":   dst = Σ coef·buffer over ``terms`` (coef None: 1)      cgp_axpby_*

    and the two-stream list also
    fn "conv_ntk":   dst, dst_theta = the two-stream conv of (src, theta), theta None for
                     Θ = 0, [→ nonlinearity ``post``] [+ addend, + addend_theta]
                                                                          cgp_covntk_conv_*
    fn "nonlin_ntk": dst, dst_theta = ``post`` of src [+ addend], theta·κ̇ [+ addend_theta]
                                                                          cgp_covntk_nonlin_*
    fn "abrelu_ntk": dst, dst_theta = abrelu of src [+ addend], theta·κ̇ [+ addend_theta]
                                                                          cgp_abrelu_cov_*
    fn "sin_ntk":    dst, dst_theta = sin of src [+ addend], theta·κ̇ [+ addend_theta]
                                                                          cgp_sin_cov_*
    fn "hermite_ntk": dst, dst_theta = hermite of src [+ addend], theta·κ̇ [+ addend_theta]: the
                     tables of φ and φ', then                             cgp_hermite_cov_*
    fn "accum":      dst = dst + src, in place                            cgp_axpby_*"""
    fn: str
    dst: object
    src: Optional[object] = None
    op: Optional[Op] = None
    post: int = N.CGP_COV_NONE
    var: Optional[int] = None
    addend: Optional[object] = None
    bias: Optional[float] = None
    theta: Optional[tuple] = None
    dst_theta: Optional[tuple] = None
    addend_theta: Optional[tuple] = None
    terms: list = dataclasses.field(default_factory=list)
    free: list = dataclasses.field(default_factory=list)

    def reads(self):
        r = [b for b in (self.src, self.addend, self.theta, self.addend_theta)
             if b is not None]
        if self.fn == "accum":
            r.append(self.dst)
        return r + [b for _, b in self.terms]

    def writes(self):
        return [b for b in (self.dst, self.dst_theta) if b is not None]


def _schedule(steps, elems, keep, key=None, given=()):
    """Sets every step's ``free`` -- the live buffers no later step reads, those of ``keep``
    never, sorted by ``key`` -- and returns (peak, largest): the elements, by ``elems(buffer)``,
    live at the fullest launch and of the largest buffer.  ``given``: the buffers that exist
    before the first launch."""
    last = {}
    for idx, st in enumerate(steps):
        for b in st.reads():
            last[b] = idx
    last.update((b, len(steps)) for b in keep)
    live = set(given)
    peak = largest = 0
    for idx, st in enumerate(steps):
        live.update(st.writes())
        peak = max(peak, sum(elems(b) for b in live))
        largest = max([largest] + [elems(b) for b in st.writes()])
        st.free = sorted((b for b in live if last.get(b, -1) <= idx), key=key)
        live.difference_update(st.free)
    return peak, largest


def _theta_sum(terms, theta, d):
    """The Sum / Mixture rule for Θ of value ``d`` = Σ coef·value over ``terms``, with
    theta[value] the buffer that holds a term's Θ (None: zero).  Zero terms are skipped and a
    single term of weight 1 passes its buffer on.  Returns (the buffer of Θ(d) or None, the
    terms of the cgp_axpby_* launch that writes it: none where no launch is needed)."""
    live = [(c, theta[t]) for c, t in terms if theta[t] is not None]
    if not live:
        return None, []
    if len(live) == 1 and live[0][0] is None:
        return live[0][1], []
    return ("T", d), live


def _layer_schedule(prog, steps, keep, given):
    """_schedule for a layer-path list: a buffer ("K", v) / ("T", v) is ho·wo elements per
    map."""
    _schedule(steps, lambda b: prog.shapes[b[1]][0] * prog.shapes[b[1]][1], keep, given=given)


def layer_steps(prog: Program, pair_ops, v0: int, vf: int):
    """The forward run of the layer path: the fused op list ``pair_ops`` (fuse) in step form,
    one step per op, in order.  Returns (steps, k, None) as ntk_steps does, k = ("K", vf).
    The input moments' maps ("K", v0) are given to the run unless a conv computes them as its
    pre-stage."""
    K = lambda v: None if v is None else ("K", v)                               # noqa: E731
    steps = []
    for op in pair_ops:
        if op.kind == "conv":
            src = None if op.pre == N.CGP_PRE_MOMENTS else K(op.src)
            steps.append(Step("conv", K(op.dst), src=src, op=op, bias=op.geom.bias,
                              addend=K(op.addend)))
        elif op.kind == "tapconv":
            steps.append(Step("tapconv", K(op.dst), src=K(op.src), op=op, bias=op.geom.bias,
                              addend=K(op.addend)))
        elif op.kind in NONLIN_KINDS:
            steps.append(Step(op.kind, K(op.dst), src=K(op.src), op=op, var=op.src,
                              addend=K(op.addend)))
        elif op.kind == "add":
            steps.append(Step("axpby", K(op.dst), op=op, terms=[(c, K(t)) for c, t in op.terms]))
        else:
            raise AssertionError(op.kind)
    fused = any(op.pre == N.CGP_PRE_MOMENTS for op in pair_ops)
    _layer_schedule(prog, steps, [K(vf)], [] if fused else [K(v0)])
    return steps, K(vf), None


def ntk_steps(prog: Program, v0: int, vf: int):
    """The launches that carry (K, Θ) through the UNFUSED program: returns (steps, k, theta)
    with ``k`` = ("K", vf) and ``theta`` the buffer holding Θ of vf, or None for Θ = 0.

    The recursion (the reference's conventions: ReLU without the √2, weight var_weight/k²
    per tap), with A the conv's constant-weight stencil without the bias:

        input moments   Θ = 0                         (inputs are not parameters)
        Conv2d          K' = A(K) + var_bias,  Θ' = A(Θ) + K'
        ReLU            K' = relu(K),          Θ' = Θ·κ̇,  κ̇ = (π - θ)/2π  (1/2 where the
                        reference overrides K': same and i = j, or same and diag)
        Erf             K' = erf(K),           Θ' = Θ·κ̇,  κ̇ = (4/π)/√D  
        Gelu            K' = gelu(K),          Θ' = Θ·κ̇,  κ̇ = E[φ'φ']   
        ABReLU          K' = abrelu(K),        Θ' = Θ·κ̇,  κ̇ = s·(π - θ)/2π + m  
        Sin             K' = sin(K),           Θ' = Θ·κ̇,  κ̇ = D·(e_d + C·e_s)   
        HermiteNonlin   K' = hermite(K),       Θ' = Θ·κ̇,  κ̇ = the series of φ'  
        Sum / Mixture   the same (weighted) sum on both streams

    A zero Θ is carried as None and costs nothing: the first conv's Θ' IS its K' (the same
    buffer), a ReLU / Erf / Gelu / ABReLU / Sin on a value with Θ = 0 is the plain cgp_relu_* /
    forward-only cgp_erf_* / cgp_gelu_* / cgp_abrelu_* / cgp_sin_*, sums skip zero terms
    (a sum whose only non-zero term has weight 1 passes that term's buffer on)."""
    steps = []
    theta = {v0: None}
    for op in prog.ops:
        d, th = op.dst, theta.get(op.src)
        if op.kind in ("conv", "tapconv"):
            # a tapconv is linear like the box: the same rule with its own stencil A_W
            steps.append(Step(op.kind, ("K", d), src=("K", op.src), op=op, bias=op.geom.bias))
            theta[d] = ("K", d)
            if th is not None:
                steps.append(Step(op.kind, ("T", d), src=th, op=op, bias=0.0, addend=("K", d)))
                theta[d] = ("T", d)
        elif op.kind in NONLIN_KINDS:
            theta[d] = None if th is None else ("T", d)
            steps.append(Step(op.kind if th is None else op.kind + "_ntk", ("K", d),
                              src=("K", op.src), op=op, var=op.src, theta=th,
                              dst_theta=theta[d]))
        elif op.kind == "add":
            steps.append(Step("axpby", ("K", d), op=op,
                              terms=[(c, ("K", t)) for c, t in op.terms]))
            theta[d], live = _theta_sum(op.terms, theta, d)
            if live:
                steps.append(Step("axpby", theta[d], op=op, terms=live))
        else:
            raise AssertionError(op.kind)
    final = [b for b in (("K", vf), theta[vf]) if b is not None]
    _layer_schedule(prog, steps, final, [("K", v0)])
    return steps, ("K", vf), theta[vf]


# ------------------------------------------------------------------------------------
# global average pooling: the program on position-pair maps
# ------------------------------------------------------------------------------------
POOL_RULE_NONLIN = ("a ReLU or Erf downstream of a GlobalAvgPool is not implemented: it would "
                    "need the pooled self-covariances of each image (DESIGN §8)")
POOL_RULE_ONE = ("every path from the input to the output must pass through exactly one "
                 "GlobalAvgPool in a model that contains one (DESIGN §8)")
POOL_RULE_CONV = ("a Conv2d downstream of a GlobalAvgPool must keep the value 1x1 "
                  "(e.g. Conv2d(1, var_weight=..., var_bias=...))")
POOL_RULE_NTK = ("ntk: the neural tangent kernel of a model with a GlobalAvgPool is not "
                 "implemented: Θ would have to be carried as position-pair maps (DESIGN §8)")
AVGPOOL_RULE_GLOBAL = ("an AvgPool2d downstream of a GlobalAvgPool is not implemented: the "
                       "value there is 1x1 per pair, with no window to average (DESIGN §8)")
AVGPOOL_RULE_NTK = ("ntk: the neural tangent kernel of a model with an AvgPool2d is not "
                    "implemented: Θ would have to be carried as position-pair maps (DESIGN §8)")
CORRCONV_RULE_GLOBAL = ("a CorrelatedConv2d downstream of a GlobalAvgPool is not implemented: "
                        "the value there is 1x1 per pair, with no taps to correlate (DESIGN §8)")
GELU_RULE_GLOBAL = ("a Gelu downstream of a GlobalAvgPool is not implemented: it would need "
                    "the pooled self-covariances of each image (DESIGN §8)")
ABRELU_RULE_GLOBAL = ("an ABReLU / LeakyReLU downstream of a GlobalAvgPool is not implemented: "
                      "it would need the pooled self-covariances of each image (DESIGN §8)")
SIN_RULE_GLOBAL = ("a Sin / Cos / Rbf downstream of a GlobalAvgPool is not implemented: it would "
                   "need the pooled self-covariances of each image (DESIGN §8)")
HERMITE_RULE_GLOBAL = ("a HermiteNonlin (Tanh, Sigmoid, Softplus, SiLU, GeluTanh) downstream of a "
                       "GlobalAvgPool is not implemented: it would need the pooled "
                       "self-covariances of each image (DESIGN §8)")
CORRCONV_RULE_NTK = ("ntk: the neural tangent kernel of a model with a CorrelatedConv2d is not "
                     "implemented: Θ would have to be carried as position-pair maps (DESIGN §8)")


@dataclasses.dataclass
class CovSteps:
    """A launch list on position-pair maps, pool_steps' or pool_ntk_steps' (there over the
    buffers of both streams): what Plan.run_cov_steps runs."""
    steps: list
    shapes: dict        # buffer -> (h, w) of its value
    maps: frozenset     # buffers that are position-pair maps: (h·w)² elements per pair
    scalars: frozenset  # buffers downstream of the pool: one element per pair
    final: object
    need_var: frozenset  # values whose per-image variance maps the nonlinearities read
    peak: int = 0       # elements per pair live at the fullest launch (_schedule)
    largest: int = 0    # elements per pair of the largest buffer (_schedule)
    # pool_steps only.  ``pooled``: every value of the unfused program at or after a pool.
    # AvgPool2d, CorrelatedConv2d: the values of the unfused program at or
    # downstream of one (either ends the closure of the per-image variances), the
    # values of need_var among them -- their variance maps are the p = q diagonals of the
    # images' self maps, extracted by a pass of steps[:self_last + 1] over the pairs (i, i)
    # (run_self_variances) -- and the index of the step that writes the last of those
    # (-1: no self pass)
    pooled: frozenset = frozenset()
    avgpooled: frozenset = frozenset()
    self_var: frozenset = frozenset()
    self_last: int = -1
    # pool_ntk_steps only: the buffer that holds Θ of the final value (``final`` itself after
    # a single conv, None for Θ = 0), the forward-only list of the same program (its self pass
    # gives the variances downstream of an AvgPool2d) and the ``fused`` it was lowered with
    final_theta: Optional[tuple] = None
    forward: Optional["CovSteps"] = None
    fused: bool = True

    def elems(self, b) -> int:
        h, w = self.shapes[b]
        return (h * w) ** 2 if b in self.maps else 1


# op kind -> the rule it breaks downstream of a GlobalAvgPool (its result is not pooled)
POOL_RULES = {"relu": POOL_RULE_NONLIN, "erf": POOL_RULE_NONLIN, "gelu": GELU_RULE_GLOBAL,
              "abrelu": ABRELU_RULE_GLOBAL, "sin": SIN_RULE_GLOBAL,
              "hermite": HERMITE_RULE_GLOBAL,
              "avgpool": AVGPOOL_RULE_GLOBAL, "corrconv": CORRCONV_RULE_GLOBAL}


def pool_steps(prog: Program, v0: int, vf: int, body: bool = False) -> CovSteps:
    """The launches of a program with a GlobalAvgPool, an AvgPool2d or a CorrelatedConv2d
    (which stands where an AvgPool2d may, and marks ``avgpooled`` like one), over the program
    fused with rules 1 and 2 (conv with a ReLU post-stage, a two-term Sum as an addend).
    Values upstream of the GlobalAvgPool are position-pair maps S[p, q]; downstream they are
    1x1 per pair, and only linear ops may follow (they read no variances).  ``body``: the
    program has no GlobalAvgPool and its final value is a map (position_covariance, and a
    model with an AvgPool2d that ends in a dense readout).

    A conv downstream of an AvgPool2d keeps its ReLU as a launch of its own: the ReLU's
    variances are the diagonal of the conv's output on the self pairs, which has to exist
    as a map to be read.

    Raises NotImplementedError naming the rule for a ReLU / Erf, a Gelu, an ABReLU, a Sin, an
    AvgPool2d or a CorrelatedConv2d after a GlobalAvgPool and for a path that does not pass exactly one
    GlobalAvgPool."""
    pooled = {v0: False}
    avgpooled = {v0: False}
    for op in prog.ops:
        if op.kind == "add":
            avgpooled[op.dst] = any(avgpooled[t] for _, t in op.terms)
        else:
            avgpooled[op.dst] = op.kind in ("avgpool", "corrconv") or avgpooled[op.src]
        if op.kind in POOL_RULES:
            if pooled[op.src]:
                raise NotImplementedError(POOL_RULES[op.kind])
            pooled[op.dst] = False
        elif op.kind == "pool":
            if body:
                raise ValueError("position_covariance: the model contains a GlobalAvgPool "
                                 "(it is the map the pool would read: pass the body)")
            if pooled[op.src]:
                raise NotImplementedError(POOL_RULE_ONE)
            pooled[op.dst] = True
        elif op.kind in ("conv", "tapconv"):
            if pooled[op.src] and tuple(op.shape_out) != (1, 1):
                raise NotImplementedError(POOL_RULE_CONV)
            pooled[op.dst] = pooled[op.src]
        elif op.kind == "add":
            sides = {pooled[t] for _, t in op.terms}
            if len(sides) != 1:
                raise NotImplementedError(POOL_RULE_ONE)
            pooled[op.dst] = sides.pop()
        else:
            raise AssertionError(op.kind)
    if not body and not pooled[vf]:
        raise NotImplementedError(POOL_RULE_ONE)

    steps = [Step("moments", v0)]
    for op in fuse(prog, v0, vf, True, pre_relu=False, fold_moments=False):
        if op.kind == "conv" and op.post == N.CGP_POST_RELU and avgpooled[op.post_var]:
            steps.append(Step("conv", op.post_var, src=op.src, op=op, bias=op.geom.bias))
            steps.append(Step("nonlin", op.dst, src=op.post_var, op=op, post=N.CGP_COV_RELU,
                                 var=op.post_var, addend=op.addend))
        elif op.kind == "conv":
            relu = op.post == N.CGP_POST_RELU
            steps.append(Step("conv", op.dst, src=op.src, op=op,
                                 post=N.CGP_COV_RELU if relu else N.CGP_COV_NONE,
                                 var=op.post_var if relu else None, addend=op.addend,
                                 bias=op.geom.bias))
        elif op.kind in ("relu", "erf"):
            steps.append(Step("nonlin", op.dst, src=op.src, op=op,
                                 post=N.CGP_COV_RELU if op.kind == "relu" else N.CGP_COV_ERF,
                                 var=op.src, addend=op.addend))
        elif op.kind in ("gelu", "abrelu", "sin", "hermite"):
            steps.append(Step(op.kind, op.dst, src=op.src, op=op, var=op.src,
                                 addend=op.addend))
        elif op.kind in ("pool", "avgpool"):
            steps.append(Step(op.kind, op.dst, src=op.src, op=op))
        elif op.kind == "corrconv":
            steps.append(Step("corrconv", op.dst, src=op.src, op=op, bias=op.geom.bias))
        elif op.kind == "tapconv":
            # an unfused conv: no post-nonlinearity (rule 1 matches "conv"), no addend
            steps.append(Step("tapconv", op.dst, src=op.src, op=op, bias=op.geom.bias))
        else:
            steps.append(Step("axpby", op.dst, op=op, terms=list(op.terms)))
    bufs = [st.dst for st in steps]
    ps = CovSteps(steps, {b: prog.shapes[b] for b in bufs},
                  frozenset(b for b in bufs if not pooled[b]),
                  frozenset(b for b in bufs if pooled[b]), vf,
                  frozenset(st.var for st in steps if st.var is not None),
                  pooled=frozenset(v for v, p in pooled.items() if p),
                  avgpooled=frozenset(v for v, a in avgpooled.items() if a))
    ps.self_var = frozenset(v for v in ps.need_var if avgpooled[v])
    ps.self_last = max((idx for idx, st in enumerate(steps) if st.dst in ps.self_var),
                       default=-1)
    ps.peak, ps.largest = _schedule(steps, ps.elems, [vf])
    return ps


# ------------------------------------------------------------------------------------
# the neural tangent kernel on position-pair maps
# ------------------------------------------------------------------------------------
# csrc/covntk.hip kMaxLds: bytes of LDS a cgp_covntk_conv_* workgroup may take
COV_NTK_MAX_LDS = 64 * 1024


def conv_ntk_fits(taps: int, w: int, streams: int, itemsize: int) -> bool:
    """cgp_covntk_conv_*'s own check: the ``taps`` w x w blocks of every staged stream and one
    row pair's index entries fit the LDS cap of a workgroup."""
    unit = streams * taps * w * w * itemsize + 8 * taps + 12
    return unit + 8 <= COV_NTK_MAX_LDS and taps <= 1024


def pool_ntk_steps(prog: Program, v0: int, vf: int, body: bool = False, fused: bool = True,
                   itemsize: int = 8) -> CovSteps:
    """The launches that carry (K, Θ) through a program on position-pair maps: the two-stream
    counterpart of pool_steps, over the same fused program and with the same rejections.

    The recursion, with Θ = 0 at the input moments and A a conv's stencil without the bias:

        Conv2d, CorrelatedConv2d   K' = A(K) + b,   Θ' = A(Θ) + K'   (correlated weights are a
                                   fixed linear map of i.i.d. parameters: the conv's rule, A_R)
        ReLU / Erf / Gelu          K' as forward,   Θ' = Θ·κ̇
        ABReLU, Sin, HermiteNonlin K' as forward,   Θ' = Θ·κ̇   (cgp_abrelu_cov_* / cgp_sin_cov_* /
                                   cgp_hermite_cov_* with theta: a launch of its own, never a
                                   conv's post-stage)
        AvgPool2d, GlobalAvgPool   the same linear op on both
        Sum / Mixture              the same (weighted) sum on both

    A zero Θ is carried as None and costs nothing, as in ntk_steps: the first conv's Θ' is its
    K' buffer, a nonlinearity on Θ = None is the forward-only launch, sums skip zero terms.

    ``fused``: a conv whose input has a Θ, or that carries a nonlinearity or an addend, is one
    cgp_covntk_conv_* launch when both streams' blocks fit its LDS cap at ``itemsize`` bytes
    per element; otherwise, and with fused=False, it is the launch-by-launch sequence
    (cgp_cov_conv_* on K, cgp_cov_conv_* on Θ with bias 0 and addend K', then
    cgp_covntk_nonlin_* or the addends), which gives the same bits.  A conv downstream of an
    AvgPool2d / CorrelatedConv2d keeps its nonlinearity as a launch of its own, as in
    pool_steps.  A corrconv on Θ is cgp_corrconv_* with bias 0, then cgp_axpby_* adding K'."""
    fwd = pool_steps(prog, v0, vf, body)
    K = lambda v: ("K", v)                                                      # noqa: E731
    steps = []
    shapes = {}
    scalar_vals = set(fwd.scalars)
    scalars = set()
    theta = {v0: None}

    def emit(st, shape, scalar):
        for b in st.writes():
            shapes[b] = tuple(shape)
            if scalar:
                scalars.add(b)
        steps.append(st)

    for st in fwd.steps:
        d, op = st.dst, st.op
        shape, sc = fwd.shapes[d], d in scalar_vals
        ts = theta.get(st.src) if st.src is not None else None
        ta = theta.get(st.addend) if st.addend is not None else None
        ka = K(st.addend) if st.addend is not None else None
        if st.fn == "moments":
            emit(Step("moments", K(d)), shape, sc)
        elif st.fn == "conv":
            g = op.geom
            plain = st.post == N.CGP_COV_NONE and st.addend is None
            if plain and ts is None:
                emit(Step("conv", K(d), src=K(st.src), op=op, bias=g.bias), shape, sc)
                theta[d] = K(d)
            elif fused and conv_ntk_fits(g.taps, fwd.shapes[st.src][1],
                                         1 if ts is None else 2, itemsize):
                emit(Step("conv_ntk", K(d), src=K(st.src), op=op, post=st.post,
                             var=st.var, addend=ka, bias=g.bias, theta=ts,
                             dst_theta=("T", d), addend_theta=ta), shape, sc)
                theta[d] = ("T", d)
            else:
                pre = d if plain else (st.var if st.post != N.CGP_COV_NONE else ("pre", d))
                emit(Step("conv", K(pre), src=K(st.src), op=op, bias=g.bias), shape, sc)
                tpre = K(pre)
                if ts is not None:
                    tpre = ("T", pre)
                    emit(Step("conv", tpre, src=ts, op=op, bias=0.0, addend=K(pre)),
                         shape, sc)
                if plain:
                    theta[d] = tpre
                elif st.post != N.CGP_COV_NONE:
                    emit(Step("nonlin_ntk", K(d), src=K(pre), op=op, post=st.post,
                                 var=st.var, addend=ka, theta=tpre, dst_theta=("T", d),
                                 addend_theta=ta), shape, sc)
                    theta[d] = ("T", d)
                else:
                    emit(Step("axpby", K(d), op=op, terms=[(None, K(pre)), (None, ka)]),
                         shape, sc)
                    if ta is None:
                        theta[d] = tpre
                    else:
                        emit(Step("axpby", ("T", d), op=op,
                                     terms=[(None, tpre), (None, ta)]), shape, sc)
                        theta[d] = ("T", d)
        elif st.fn in ("nonlin", "gelu"):
            if ts is None:
                emit(Step(st.fn, K(d), src=K(st.src), op=op, post=st.post, var=st.var,
                             addend=ka), shape, sc)
                theta[d] = ta
            else:
                emit(Step("nonlin_ntk", K(d), src=K(st.src), op=op,
                             post=N.CGP_COV_GELU if st.fn == "gelu" else st.post,
                             var=st.var, addend=ka, theta=ts, dst_theta=("T", d),
                             addend_theta=ta), shape, sc)
                theta[d] = ("T", d)
        elif st.fn in ("abrelu", "sin", "hermite"):
            # a launch of its own on either run: one entry point, with and without Θ
            if ts is None:
                emit(Step(st.fn, K(d), src=K(st.src), op=op, var=st.var, addend=ka),
                     shape, sc)
                theta[d] = ta
            else:
                emit(Step(st.fn + "_ntk", K(d), src=K(st.src), op=op, var=st.var, addend=ka,
                             theta=ts, dst_theta=("T", d), addend_theta=ta), shape, sc)
                theta[d] = ("T", d)
        elif st.fn in ("pool", "avgpool"):
            emit(Step(st.fn, K(d), src=K(st.src), op=op), shape, sc)
            theta[d] = None
            if ts is not None:
                emit(Step(st.fn, ("T", d), src=ts, op=op), shape, sc)
                theta[d] = ("T", d)
        elif st.fn == "tapconv":
            # the conv's rule launch by launch: Θ' = A_W(Θ) + K' is the same entry point on Θ
            # with bias 0 and addend K'
            emit(Step("tapconv", K(d), src=K(st.src), op=op, bias=op.geom.bias), shape, sc)
            theta[d] = K(d)
            if ts is not None:
                emit(Step("tapconv", ("T", d), src=ts, op=op, bias=0.0, addend=K(d)),
                     shape, sc)
                theta[d] = ("T", d)
        elif st.fn == "corrconv":
            emit(Step("corrconv", K(d), src=K(st.src), op=op, bias=op.geom.bias),
                 shape, sc)
            theta[d] = K(d)
            if ts is not None:
                emit(Step("corrconv", ("T", d), src=ts, op=op, bias=0.0), shape, sc)
                emit(Step("accum", ("T", d), src=K(d), op=op), shape, sc)
                theta[d] = ("T", d)
        elif st.fn == "axpby":
            emit(Step("axpby", K(d), op=op, terms=[(c, K(t)) for c, t in st.terms]),
                 shape, sc)
            theta[d], live = _theta_sum(st.terms, theta, d)
            if live:
                emit(Step("axpby", theta[d], op=op, terms=live), shape, sc)
        else:
            raise AssertionError(st.fn)

    ns = CovSteps(steps, shapes, frozenset(b for b in shapes if b not in scalars),
                  frozenset(scalars), K(vf), fwd.need_var, final_theta=theta[vf], forward=fwd,
                  fused=fused)
    ns.peak, ns.largest = _schedule(
        steps, ns.elems, [b for b in (ns.final, ns.final_theta) if b is not None], key=repr)
    return ns


# ------------------------------------------------------------------------------------
# execution
# ------------------------------------------------------------------------------------
def _adjacent(x, y) -> bool:
    """y's elements start where x's end (one allocation, x then y), both contiguous."""
    return (x.is_contiguous() and y.is_contiguous() and x.dtype == y.dtype
            and y.data_ptr() == x.data_ptr() + x.numel() * x.element_size())


def _axpby_terms(sfx, terms, out, n, stream):
    """out[:n] = Σ coef·tensor over ``terms`` (coef None: 1), one cgp_axpby_* launch per term:
    the first term overwrites, later terms accumulate."""
    for k, (coef, src) in enumerate(terms):
        c = 1.0 if coef is None else coef
        if k == 0:
            N.call(f"cgp_axpby_{sfx}", c, N.ptr(src), 0.0, None, N.ptr(out), n, stream)
        else:
            N.call(f"cgp_axpby_{sfx}", 1.0, N.ptr(out), c, N.ptr(src), N.ptr(out), n, stream)


# Plan._hermite_nodes' tables, per (device, quad_nodes)
_HERMITE_NODES = {}
# where the compressed Gauss–Hermite rule ends: h_n(z)·exp(−z²/2) is below exp(−z²/4) for every
# n, 1e-17 at |z| = 12.5
HERMITE_RANGE = 12.5


def hermite_rule(nq):
    """(z, w), float64 [nq] each: the nodes and weights of the rule E_z[f(z)] = Σ w_q·f(z_q)
    behind the Hermite coefficients.  numpy's hermegauss(nq), weights over
    √(2π), compressed by s = min(1, HERMITE_RANGE / max|z_q|): z = s·z_q, w = s·w_q·exp((1 −
    s²)·z_q²/2), the same integral after the substitution z → s·z.  The plain rule spends its
    outer nodes where every integrand is below rounding; pulled in to ±12.5 they sit closer
    together, which is what a φ with poles near the real axis (tanh: ±iπ/2) needs: at 96 nodes
    and v = 1 the coefficients of tanh go from 4.6e-10 to the rounding level.  s is 1 up to 46
    nodes."""
    z, w = np.polynomial.hermite_e.hermegauss(int(nq))
    s = min(1.0, HERMITE_RANGE / float(np.max(np.abs(z))))
    return s * z, s * w * np.exp((1 - s * s) * z * z / 2) / math.sqrt(2 * math.pi)


class DevPtr:
    """A device address inside ``base`` (kept alive by the handle, like a view would be):
    what the launch records need of a variance map, without building a tensor view."""
    __slots__ = ("base", "off")

    def __init__(self, base: torch.Tensor, off: int):
        self.base, self.off = base, off

    def data_ptr(self) -> int:
        return self.base.data_ptr() + self.off

class Plan:
    """A compiled model at one input geometry: the variance program and the fused pair
    program.  Cached per (H, W, fuse) on the model."""

    def __init__(self, model, h: int, w: int, enable_fusion: bool = True,
                 exact_relu: bool = False):
        self.flags = N.CGP_FLAG_EXACT_RELU if exact_relu else 0
        self.prog, self.v0, self.vf = compile_program(model, h, w)
        self.pair_ops = fuse(self.prog, self.v0, self.vf, enable_fusion)
        self.need_var = needed_variances(self.pair_ops)
        fh, fw = self.prog.shapes[self.vf]
        self.final_hw = (fh, fw)
        self.moments_fused = any(o.pre == N.CGP_PRE_MOMENTS for o in self.pair_ops)
        # a model with a GlobalAvgPool, an AvgPool2d or a CorrelatedConv2d runs on
        # position-pair maps (run_cov_steps); its rejections are raised here, when the program
        # is compiled.  Without a GlobalAvgPool the final value is a map (1x1 for forward)
        kinds = {o.kind for o in self.prog.ops}
        self.pool = pool_steps(self.prog, self.v0, self.vf, body="pool" not in kinds) \
            if kinds & {"pool", "avgpool", "corrconv"} else None

    # -- helpers -----------------------------------------------------------------------
    @staticmethod
    def _sfx(dtype):
        if dtype == torch.float64:
            return "f64"
        if dtype == torch.float32:
            return "f32"
        raise TypeError(f"unsupported dtype {dtype} (float32 or float64)")

    def _nonlin_launch(self, op, sfx, stream, src, out, var, n1, n2, same, diag, addend=None,
                       theta=None, out_theta=None):
        """Fills the argument record of a layer-path nonlinearity (NONLIN_CALLS) and launches
        it; with ``theta`` the two-stream form (Θ' = Θ·κ̇)."""
        name = "relu_ntk" if op.kind == "relu" and theta is not None else op.kind
        cls, out_field, has_flags, consts = NONLIN_CALLS[name][:4]
        vx, vy = var
        ho, wo = op.shape_out
        r = cls()
        r.xy = N.ptr(src)
        setattr(r, out_field, N.ptr(out))
        if addend is not None:
            r.addend = N.ptr(addend)
        if theta is not None:
            r.theta, r.out_theta = N.ptr(theta), N.ptr(out_theta)
        r.xx, r.yy = N.ptr(vx), N.ptr(vy)
        r.nmaps, r.n1, r.n2 = (n1 if diag else n1 * n2), n1, n2
        r.hw, r.same, r.diag = ho * wo, int(same), int(diag)
        for field, value in consts(op) if consts else ():
            setattr(r, field, value)
        if op.kind == "hermite":
            ws = self._hermite_tables(  # noqa: F841 (alive until the launch)
                r, op, sfx, stream, vx, vy, n1, n2, ho * wo, same, theta is not None, out)
        if has_flags:
            r.flags = self.flags
        N.check(getattr(N.load(), f"cgp_{name}_{sfx}")(r, stream), "cgp_" + name)

    @staticmethod
    def _hermite_nodes(dev, nq):
        """The device node table of cgp_hermite_coef_* / cgp_var_hermite_*: double [2][nq], the
        nodes and the weights of hermite_rule(nq), uploaded once per device and nq.  The copy is synchronous, as _corr_tables' is: the table is shared by every
        plan and stream, and none may see a copy in flight."""
        key = (str(dev), int(nq))
        tab = _HERMITE_NODES.get(key)
        if tab is None:
            tab = torch.from_numpy(np.stack(hermite_rule(nq))).to(dev).contiguous()
            torch.cuda.synchronize(dev)
            _HERMITE_NODES[key] = tab
        return tab

    def _hermite_tables(self, r, op, sfx, stream, vx, vy, n1, n2, hw, same, ntk, like):
        """The workspace of one hermite launch: the coefficient tables [order + 1][n·hw] of the
        variance maps vx ([n1, hw]) and vy ([n2, hw]; not with ``same``, where yy holds xx's
        values and the x tables serve both), and the tables of φ' with ``ntk``, written by
        cgp_hermite_coef_* on ``stream`` and set in the record ``r`` (cgp_hermite_args or
        cgp_hermite_cov_args).  (n1 + n2)·(order + 1)·hw values, n1·… with same, twice that
        with ntk.  Returns the workspace: the caller keeps it until the launch is enqueued."""
        phi, order, nq = op.rule
        nodes = self._hermite_nodes(like.device, nq)
        sides = [(vx, n1 * hw)] if same else [(vx, n1 * hw), (vy, n2 * hw)]
        ws = torch.empty(((2 if ntk else 1) * (order + 1) * sum(c for _, c in sides),),
                         dtype=like.dtype, device=like.device)
        item, at, tabs = ws.element_size(), ws.data_ptr(), []
        for v, count in sides:
            c = N.HermiteCoefArgs()
            c.var, c.nodes, c.count = v.data_ptr(), nodes.data_ptr(), count
            c.phi, c.order, c.nq = phi, order, nq
            c.a = at
            at += (order + 1) * count * item
            if ntk:
                c.da = at
                at += (order + 1) * count * item
            N.check(getattr(N.load(), f"cgp_hermite_coef_{sfx}")(c, stream), "cgp_hermite_coef")
            tabs.append((c.a, c.da, count))
        (r.ax, r.dax, r.stride_x), (r.ay, r.day, r.stride_y) = tabs[0], tabs[-1]
        r.order = order
        return ws

    @staticmethod
    def _conv_args(op, src, out, nmaps, n1, n2, same=0, diag=0, flags=0, bias=None, addend=None,
                   var=None, images=None):
        """The cgp_conv_* record of conv ``op`` from ``src`` (or, where its pre-stage is the
        moments, from ``images`` = (x, y)) to ``out``: geometry, shapes, the op's pre / post
        stages with their variance maps from ``var``, the addend and ``bias`` in place of the
        geometry's.  A new record is all zeros, so the stages and the addend are written only
        where the op has them."""
        g = op.geom
        a = N.ConvArgs()
        if op.pre == N.CGP_PRE_MOMENTS:
            x, y = images
            a.in_, a.in_y, a.channels, a.pre = x.data_ptr(), y.data_ptr(), x.shape[1], op.pre
        else:
            a.in_ = src.data_ptr()
            if op.pre == N.CGP_PRE_RELU:
                vx, vy = var[op.pre_var]
                a.pre_xx, a.pre_yy, a.pre = vx.data_ptr(), vy.data_ptr(), op.pre
        if op.post == N.CGP_POST_RELU:
            vx, vy = var[op.post_var]
            a.post_xx, a.post_yy, a.post = vx.data_ptr(), vy.data_ptr(), op.post
        a.out = out.data_ptr()
        if addend is not None:
            a.addend = addend.data_ptr()
        a.nmaps, a.n1, a.n2 = nmaps, n1, n2
        (a.h, a.w), (a.ho, a.wo) = op.shape_in, op.shape_out
        a.taps, a.offset, a.stride, a.dilation = g.taps, g.offset, g.stride, g.dilation
        a.same, a.diag, a.flags = same, diag, flags
        a.weight, a.bias = g.weight, g.bias if bias is None else bias
        return a

    def _tap_table(self, op, dev, dtype):
        """The k x k table of a tapconv op on ``dev``, rounded once to ``dtype``, uploaded once
        per plan, device and dtype.  The copy is synchronous, as _corr_tables' is: the table
        is shared by every stream that runs the plan, and none may see a copy in flight."""
        cache = self.__dict__.setdefault("_tap_tabs", {})
        key = (op.dst, str(dev), dtype)
        tab = cache.get(key)
        if tab is None:
            tab = torch.tensor(op.geom.table, dtype=torch.float64).to(dtype).to(dev).contiguous()
            torch.cuda.synchronize(dev)
            cache[key] = tab
        return tab

    def _tapconv_launch(self, op, sfx, stream, src, out, nmaps, bias, addend=None):
        """One cgp_tapconv_* launch of tapconv ``op`` over ``nmaps`` maps."""
        g = op.geom
        a = N.TapConvArgs()
        a.in_, a.out, a.nmaps = src.data_ptr(), out.data_ptr(), nmaps
        if addend is not None:
            a.addend = addend.data_ptr()
        a.table = self._tap_table(op, out.device, out.dtype).data_ptr()
        (a.h, a.w), (a.ho, a.wo) = op.shape_in, op.shape_out
        a.extent, a.offset, a.stride, a.dilation = g.extent, g.offset, g.stride, g.dilation
        a.bias = bias
        N.check(getattr(N.load(), f"cgp_tapconv_{sfx}")(a, stream), "cgp_tapconv")

    def _last_use(self, ops, extra_final):
        last = {}
        for idx, o in enumerate(ops):
            srcs = ([o.src] if o.src is not None else []) + [t for _, t in o.terms]
            if o.addend is not None:
                srcs.append(o.addend)
            for s in srcs:
                last[s] = idx
        last[extra_final] = len(ops)
        return last

    # -- variance pipeline --------------------------------------------------------------
    def run_variances(self, xx0, yy0, n1, n2, same, stream, need=None):
        """Per-image variance maps of every value a ReLU, Erf, Gelu, ABReLU or Sin reads (or of
        ``need``).
        xx0/yy0: [n, H, W]."""
        sfx = self._sfx(xx0.dtype)
        dev = xx0.device
        vals = {self.v0: (xx0, yy0)}
        need = self.need_var if need is None else need
        ops = self.prog.ops
        last = self._last_use(ops, self.vf)
        keep = {}
        if self.v0 in need:
            keep[self.v0] = vals[self.v0]
        pooled = self.pool.pooled | self.pool.avgpooled if self.pool is not None else ()
        for idx, op in enumerate(ops):
            if op.dst in pooled:
                # at or after a GlobalAvgPool: linear ops, no variances read; at or after an
                # AvgPool2d or a CorrelatedConv2d: the recursion is not closed,
                # run_self_variances has them
                continue
            ho, wo = op.shape_out
            if op.kind == "conv":
                xin, yin = vals[op.src]
                buf = torch.empty((n1 + n2, ho, wo), dtype=xx0.dtype, device=dev)
                # xx and yy may live in different allocations: launch per block, or once
                # over both when they are adjacent (every value after the first is)
                parts = ((xin, buf[:n1], n1), (yin, buf[n1:], n2))
                if _adjacent(xin, yin):
                    parts = ((xin, buf, n1 + n2),)
                for src, dst, n in parts:
                    a = self._conv_args(op, src, dst, n, n, 1)
                    N.check(getattr(N.load(), f"cgp_conv_{sfx}")(a, stream), "cgp_conv")
                out = (buf[:n1], buf[n1:])
            elif op.kind == "tapconv":
                # the same entry point over the [n1 + n2] variance maps (a pure map op)
                xin, yin = vals[op.src]
                buf = torch.empty((n1 + n2, ho, wo), dtype=xx0.dtype, device=dev)
                parts = ((xin, buf[:n1], n1), (yin, buf[n1:], n2))
                if _adjacent(xin, yin):
                    parts = ((xin, buf, n1 + n2),)
                for src, dst, n in parts:
                    self._tapconv_launch(op, sfx, stream, src, dst, n, op.geom.bias)
                out = (buf[:n1], buf[n1:])
            elif op.kind in NONLIN_KINDS:
                xin, yin = vals[op.src]
                buf = torch.empty((n1 + n2, ho, wo), dtype=xx0.dtype, device=dev)
                extra = NONLIN_CALLS[op.kind][4](op)
                if op.kind == "hermite":
                    extra += (N.ptr(self._hermite_nodes(dev, op.rule[2])),)
                N.call(f"cgp_var_{op.kind}_{sfx}", N.ptr(xin), N.ptr(yin), n1, n2, ho * wo,
                       int(same), *extra, N.ptr(buf[:n1]),
                       N.ptr(buf[n1:]), stream)
                out = (buf[:n1], buf[n1:])
            elif op.kind == "add":
                buf = torch.empty((n1 + n2, ho, wo), dtype=xx0.dtype, device=dev)
                outx, outy = buf[:n1], buf[n1:]
                whole = all(_adjacent(*vals[t]) for _, t in op.terms)
                for part, o, n in (((None, buf, n1 + n2),) if whole else
                                   ((0, outx, n1), (1, outy, n2))):
                    _axpby_terms(sfx, [(coef, vals[t][part or 0]) for coef, t in op.terms], o,
                                 n * ho * wo, stream)
                out = (outx, outy)
            else:
                raise AssertionError(op.kind)
            vals[op.dst] = out
            if op.dst in need:
                keep[op.dst] = out
            # free what no later op reads
            for v in [v for v in vals if last.get(v, -1) <= idx and v != op.dst]:
                del vals[v]
        return keep

    # -- the same program in one launch (cgp_var_chain_*) --------------------------------
    def _var_chain(self, need, quarter, dev):
        """cgp_var_op records of the variance program (cached per need/quarter/device):
        LDS slots by first fit over the values' live ranges, store offsets per image.
        None when the program has an op the chain kernel lacks (a Sum of > 4 terms, an
        Erf, a Gelu, an ABReLU, a Sin).  The records are uploaded once per plan, need set and device, and the
        copy is synchronous (on the uploading stream alone, not the device): the records are
        shared by every stream that runs the plan, and none may see a copy in flight."""
        key = (frozenset(need), frozenset(quarter), str(dev))
        cache = self.__dict__.setdefault("_var_chains", {})
        if key in cache:
            return cache[key]
        ops = self.prog.ops
        if any(op.kind not in ("conv", "relu", "add") for op in ops):
            cache[key] = None
            return None
        shapes = self.prog.shapes
        last = self._last_use(ops, self.vf)
        free = []                                  # (start, size) free LDS ranges
        top = [0]
        slot = {}

        def alloc(v):
            size = shapes[v][0] * shapes[v][1]
            size += size & 1                       # 16-byte aligned fp64 slots
            for k, (st, sz) in enumerate(free):
                if sz >= size:
                    free[k] = (st + size, sz - size)
                    slot[v] = st
                    return st
            slot[v] = top[0]
            top[0] += size
            return slot[v]

        def release(v):
            size = shapes[v][0] * shapes[v][1]
            free.append((slot.pop(v), size + (size & 1)))

        store, qstore, total, qtotal = {}, {}, 0, 0

        def stored(v):
            nonlocal total, qtotal
            if v not in need:
                return -1, -1
            hw = shapes[v][0] * shapes[v][1]
            store[v], total = total, total + hw
            if v in quarter:
                qstore[v], qtotal = qtotal, qtotal + hw
            return store[v], qstore.get(v, -1)

        recs = []
        h, w = shapes[self.v0]
        r = N.VarOp(kind=N.CGP_VAR_MOMENTS, dst=alloc(self.v0), h=h, w=w, ho=h, wo=w)
        r.src[:] = [-1, -1, -1, -1]
        r.store, r.qstore = stored(self.v0)
        recs.append(r)
        for idx, op in enumerate(ops):
            srcs = [op.src] if op.kind in ("conv", "relu") else [t for _, t in op.terms]
            # the chain kernel covers at most kVarE·kBlock = 1024 elements per pass, over
            # both the row pass (h·wo) and the output (ho·wo): a conv padded beyond "same"
            # grows its map past the input's, so the input size alone does not bound it
            (hi_, wi_), (ho_, wo_) = shapes[srcs[0]], op.shape_out
            if len(srcs) > 4 or max(hi_ * wo_, ho_ * wo_, hi_ * wi_) > 1024:
                cache[key] = None
                return None
            r = N.VarOp(dst=alloc(op.dst))
            r.src[:] = [slot[s] for s in srcs] + [-1] * (4 - len(srcs))
            (r.h, r.w), (r.ho, r.wo) = shapes[srcs[0]], op.shape_out
            if op.kind == "conv":
                g = op.geom
                r.kind = N.CGP_VAR_CONV
                r.taps, r.offset, r.stride, r.dilation = g.taps, g.offset, g.stride, g.dilation
                r.weight, r.bias = g.weight, g.bias
            elif op.kind == "relu":
                r.kind = N.CGP_VAR_HALF
            else:
                r.kind = N.CGP_VAR_SUM
                r.coef[:] = [1.0 if c is None else float(c) for c, _ in op.terms] + \
                    [0.0] * (4 - len(op.terms))
            r.store, r.qstore = stored(op.dst)
            recs.append(r)
            for s in set(srcs):
                if last.get(s, -1) <= idx and s in slot:
                    release(s)
            if last.get(op.dst, -1) <= idx and op.dst != self.vf:
                release(op.dst)
        # the convs' row-sum scratch after the slots: [h][wo] of the largest conv
        scratch = top[0]
        hs = max([r.h * r.wo for r in recs if r.kind == N.CGP_VAR_CONV] + [2])
        top[0] += hs + (hs & 1)
        arr = (N.VarOp * len(recs))(*recs)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        # a blocking copy: it returns once the uploading stream has run it
        chain = dict(ops=host.to(dev), nops=len(recs), lds=top[0],
                     scratch=scratch,
                     store=store, qstore=qstore, total=total, qtotal=qtotal)
        cache[key] = chain
        return chain

    def run_variances_fused(self, x, y, n1, n2, same, stream, need, quarter=(), views=True):
        """run_variances in one launch.  Returns (var, qvar): var[v] = (xx [n1,..],
        yy [n2,..]) for v in need (yy is xx when same), qvar[v] = xx scaled by
        cgp_net_xvar_scale() (1/16 from ABI 9; "quarter" is the round-2 name) for v in quarter
        (callers pass the values the library's map form wants scaled copies of --
        netplan.NetPlan.chain_quarter: none when cgp_net_var_form() is the rsqrt form);
        None when the chain kernel cannot run this program.  ``views=False`` gives
        DevPtr handles (data_ptr() only) instead of tensor views: a forward only needs the
        maps' addresses, and ~90 views cost ~0.1 ms of host time per ResNet tile."""
        need = set(need)
        quarter = set(quarter) & need
        chain = self._var_chain(need, quarter, x.device)
        # the chain kernel holds maps of up to 4·256 pixels per workgroup in 64 KB of LDS
        if chain is None or chain["lds"] * x.element_size() > 64 * 1024 or \
                x.shape[2] * x.shape[3] > 1024:
            return None
        m2 = 0 if same else n2
        n = n1 + m2
        out = torch.empty((n * chain["total"] + n1 * chain["qtotal"],), dtype=x.dtype,
                          device=x.device)
        a = N.VarArgs()
        a.x, a.y, a.out, a.ops = x.data_ptr(), y.data_ptr(), out.data_ptr(), \
            chain["ops"].data_ptr()
        a.n1, a.n2, a.store_total = n1, m2, chain["total"]
        a.nops, a.channels, a.h, a.w = chain["nops"], x.shape[1], x.shape[2], x.shape[3]
        a.lds_elems, a.scratch = chain["lds"], chain["scratch"]
        N.check(getattr(N.load(), f"cgp_var_chain_{self._sfx(x.dtype)}")(a, stream),
                "cgp_var_chain")
        shapes = self.prog.shapes
        var, qvar = {}, {}
        if not views:
            item = out.element_size()
            for v, off in chain["store"].items():
                ho, wo = shapes[v]
                px = DevPtr(out, n * off * item)
                var[v] = (px, px if same else DevPtr(out, (n * off + n1 * ho * wo) * item))
            for v, off in chain["qstore"].items():
                qvar[v] = DevPtr(out, (n * chain["total"] + n1 * off) * item)
            return var, qvar
        for v, off in chain["store"].items():
            ho, wo = shapes[v]
            blk = out[n * off:n * (off + ho * wo)].view(n, ho, wo)
            var[v] = (blk[:n1], blk[:n1] if same else blk[n1:])
        for v, off in chain["qstore"].items():
            ho, wo = shapes[v]
            base = n * chain["total"] + n1 * off
            qvar[v] = out[base:base + n1 * ho * wo].view(n1, ho, wo)
        return var, qvar

    # -- pair pipeline: the forward run and the NTK run (K and Θ) ---------------------------
    def ntk_need_var(self) -> set:
        """The values whose variance maps the NTK run reads: every ReLU's, Erf's, Gelu's,
        ABReLU's and Sin's source in the unfused program (run_variances(need=...))."""
        return {o.src for o in self.prog.ops if o.kind in NONLIN_KINDS}

    def layer_list(self, ntk: bool = False):
        """(steps, k, theta) of the forward run (layer_steps over pair_ops) or of the NTK run
        (ntk_steps over the unfused program), lowered and scheduled once per plan."""
        key = "_ntk_steps" if ntk else "_layer_steps"
        if key not in self.__dict__:
            self.__dict__[key] = ntk_steps(self.prog, self.v0, self.vf) if ntk else \
                layer_steps(self.prog, self.pair_ops, self.v0, self.vf)
        return self.__dict__[key]

    def run_layer_steps(self, steps, x, y, xy0, var, n1, n2, same, diag, stream):
        """Runs a layer-path list (layer_list) on the pair maps; returns (K, Θ) of the final
        value as [nmaps, fh, fw] tensors, Θ None for the forward list and where it is zero (a
        model without a Conv2d).  x, y: images [n, C, H, W] (read by a conv whose pre-stage is
        the moments); xy0: the input moments' pair maps [nmaps, H, W] (not modified; None when
        the moments are fused into the first conv); var: the variance maps of need_var, of
        ntk_need_var() for the NTK list.

        Every output is allocated at the step that writes it and dropped with the step's
        ``free``, after its last reader.  Peak live pair maps of the NTK run: 4 on a
        Conv2d/ReLU chain (K, Θ and K', Θ' of a cgp_relu_ntk_*, cgp_erf_* or cgp_gelu_* step;
        3 at a conv's Θ launch), plus 2 (K and Θ) for every Sum / Mixture branch result or skip
        value waiting for its sum -- 6 inside a residual block of the ResNets."""
        steps, kbuf, tbuf = steps
        sfx = self._sfx(x.dtype)
        conv = getattr(N.load(), f"cgp_conv_{sfx}")
        nmaps = n1 if diag else n1 * n2
        same, diag = int(same), int(diag)
        bufs = {} if xy0 is None else {("K", self.v0): xy0}
        dtype, dev = x.dtype, x.device
        for st in steps:
            op = st.op
            shape = (nmaps, *op.shape_out)
            out = bufs[st.dst] = torch.empty(shape, dtype=dtype, device=dev)
            if st.fn == "conv":
                a = self._conv_args(op, bufs.get(st.src), out, nmaps, n1, n2, same, diag,
                                    self.flags, st.bias, bufs.get(st.addend), var, (x, y))
                N.check(conv(a, stream), "cgp_conv")
            elif st.fn == "tapconv":
                self._tapconv_launch(op, sfx, stream, bufs[st.src], out, nmaps, st.bias,
                                     bufs.get(st.addend))
            elif st.fn == "axpby":
                _axpby_terms(sfx, [(c, bufs[b]) for c, b in st.terms], out, out.numel(), stream)
            else:
                tout = None
                if st.dst_theta is not None:
                    tout = bufs[st.dst_theta] = torch.empty(shape, dtype=dtype, device=dev)
                self._nonlin_launch(op, sfx, stream, bufs[st.src], out, var[st.var], n1, n2,
                                    same, diag, addend=bufs.get(st.addend),
                                    theta=bufs.get(st.theta), out_theta=tout)
            for b in st.free:
                del bufs[b]
        return bufs[kbuf], (None if tbuf is None else bufs[tbuf])

    # -- GlobalAvgPool: the program on position-pair maps ---------------------------------
    def body_steps(self) -> CovSteps:
        """pool_steps of a model without a pool (position_covariance): the final value is
        the position-pair map a GlobalAvgPool after the model would read."""
        if "_body_steps" not in self.__dict__:
            self._body_steps = pool_steps(self.prog, self.v0, self.vf, body=True)
        return self._body_steps

    def _corr_tables(self, op, dev, dtype):
        """The two tap correlation matrices of a corrconv op on ``dev`` in ``dtype``, uploaded
        once per plan, device and dtype.  The copy is synchronous: the tables are shared by
        every stream that runs the plan, and none may see a copy in flight."""
        cache = self.__dict__.setdefault("_corr_tabs", {})
        key = (op.dst, str(dev), dtype)
        tabs = cache.get(key)
        if tabs is None:
            tabs = tuple(torch.tensor(m, dtype=torch.float64).to(dtype).to(dev).contiguous()
                         for m in (op.geom.corr_rows, op.geom.corr_cols))
            torch.cuda.synchronize(dev)
            cache[key] = tabs
        return tabs

    def pool_ntk(self, body: bool, fused: bool, itemsize: int) -> CovSteps:
        """pool_ntk_steps of the plan's program, cached per (body, fused, itemsize)."""
        cache = self.__dict__.setdefault("_pool_ntk", {})
        key = (bool(body), bool(fused), int(itemsize))
        if key not in cache:
            cache[key] = pool_ntk_steps(self.prog, self.v0, self.vf, body=body, fused=fused,
                                        itemsize=itemsize)
        return cache[key]

    def run_self_variances(self, x, var, stream, ps=None, max_bytes=None, want=None):
        """The variance maps [n, h, w] of the values ``want`` (default ps.self_var: what the
        nonlinearities downstream of an AvgPool2d read) of the images x: the p = q diagonals
        of the values' position-pair maps on the self pairs (i, i), run with ``same`` so the
        nonlinearities' override applies there.  The launches are ps.steps up to the last one
        that writes a wanted value, chunked by run_cov_steps; a nonlinearity inside reads
        the diagonal just extracted from its own source.  var: value -> [n, h, w] maps of the
        values upstream of every AvgPool2d (one side of run_variances' pairs).  A wanted
        value must be a buffer of ps (the destination of a launch)."""
        ps = self.pool if ps is None else ps
        want = ps.self_var if want is None else frozenset(want)
        if not want <= {st.dst for st in ps.steps}:
            raise KeyError(f"run_self_variances: {sorted(want)} are not all launch outputs")
        n = x.shape[0]
        last = max(k for k, st in enumerate(ps.steps) if st.dst in want)
        written = {st.dst for st in ps.steps[:last + 1]}
        out = {v: torch.empty((n,) + tuple(ps.shapes[v]), dtype=x.dtype, device=x.device)
               for v in (want | ps.self_var) & written}
        both = {v: (m, m) for v, m in var.items()}
        both.update({v: (m, m) for v, m in out.items()})
        idx = torch.arange(n, device=x.device, dtype=torch.int32)
        self.run_cov_steps(ps, x, x, both, idx, idx, True, stream, max_bytes, last=last,
                           diag_out=out)
        return {v: out[v] for v in want}

    def run_cov_steps(self, cs, x, y, var, pair_i, pair_j, same, stream, max_bytes=None,
                      last=None, diag_out=None):
        """Runs the launch list ``cs`` (pool_steps or pool_ntk_steps) over the pairs
        (pair_i[m], pair_j[m]) -- device int32 arrays -- in chunks of pairs; returns (K, Θ) of
        the final value of every pair as [npairs, elements] tensors (one element per pair
        after a pool), Θ None for a forward list and where it is zero (a model without a conv).
        x, y: images [n, C, H, W]; var: the variance maps of cs.need_var (run_variances, and
        run_self_variances on the forward list for its self_var).  ``last``: run
        cs.steps[:last + 1] only and return nothing; ``diag_out``: value -> [n, h, w] tensor
        that takes the p = q diagonal of the value's map of pair m at image pair_i[m]
        (cgp_covmap_diag_*), right after the launch that writes it.

        A chunk takes cs.peak elements per pair at its fullest launch, both streams counted
        (every buffer is freed after its last reader); chunks are sized to stay under
        ``max_bytes`` (default: a quarter of the device's free memory).  Each kernel computes a
        pair from that pair's data alone in a fixed order, so the result does not depend on the
        chunking."""
        sfx = self._sfx(x.dtype)
        lib = N.load()
        dev = x.device
        item = x.element_size()
        npairs = pair_i.numel()
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(dev)[0] // 4
        per_pair = cs.peak * item
        chunk = int(max_bytes) // per_pair
        if chunk < 1:
            what, both = ("ntk_maps", ", K and Θ") if cs.forward is not None else \
                ("GlobalAvgPool", "")
            raise RuntimeError(
                f"{what}: one image pair needs {per_pair} bytes of position-pair maps "
                f"({cs.peak} live elements of {item} bytes at the fullest launch{both}; the "
                f"largest map holds {cs.largest}), more than the workspace of {int(max_bytes)} bytes "
                "(set_pool_workspace)")
        # pairs·elements of one launch stay below 2^40 (the entry points count blocks in int32)
        chunk = min(chunk, npairs, max(1, (1 << 40) // cs.largest))
        C = x.shape[1]
        steps = cs.steps if last is None else cs.steps[:last + 1]
        diag_out = diag_out or {}
        outs = {}                               # the final buffers are slices of the output
        if last is None:
            outs[cs.final] = torch.empty((npairs, cs.elems(cs.final)), dtype=x.dtype, device=dev)
            if cs.final_theta not in (None, cs.final):
                outs[cs.final_theta] = torch.empty_like(outs[cs.final])
        # device pointers are taken once per buffer, not once per use
        xp, yp, flags, same = N.ptr(x), N.ptr(y), self.flags, int(same)
        vptr = {v: (N.ptr(vx), N.ptr(vy)) for v, (vx, vy) in var.items()}

        def new(b):
            if b not in bufs:                          # fn "accum" writes in place
                bufs[b] = outs[b][a:a + n] if b in outs else \
                    torch.empty((n, cs.elems(b)), dtype=x.dtype, device=dev)
                ptr[b] = N.ptr(bufs[b])
            return ptr[b]

        def maps(r, st):
            """the fields every argument struct has: the maps in and out"""
            r.in_, r.out, r.npairs = ptr[st.src], ptr[st.dst], n
            r.h, r.w = cs.shapes[st.src]
            return r

        def stencil(r, st):
            """a conv's or corrconv's output size, taps, weight and the step's bias"""
            g = st.op.geom
            r.ho, r.wo = cs.shapes[st.dst]
            r.taps, r.offset, r.stride, r.dilation = g.taps, g.offset, g.stride, g.dilation
            r.weight, r.bias = g.weight, st.bias
            return r

        def pairwise(r, st):
            """the fields of the kernels that know the pair: its images' variances (only where
            a nonlinearity reads them), the addend and the second stream"""
            if st.var is not None:
                r.xx, r.yy = vptr[st.var]
            r.pair_i, r.pair_j, r.same, r.addend = pi, pj, same, ptr[st.addend]
            if st.dst_theta is not None:
                r.theta, r.out_theta = ptr[st.theta], new(st.dst_theta)
                r.addend_theta = ptr[st.addend_theta]
            return r

        for a in range(0, npairs, chunk):
            n = min(chunk, npairs - a)
            pi, pj = N.ptr(pair_i[a:a + n]), N.ptr(pair_j[a:a + n])
            bufs, ptr = {}, {None: None}        # the live tensors; every buffer's pointer
            for st in steps:
                h, w = cs.shapes[st.dst]
                dst = new(st.dst)
                ntk = st.dst_theta is not None
                if st.fn == "moments":
                    N.check(getattr(lib, f"cgp_cov_moments_{sfx}")(
                        xp, yp, pi, pj, n, C, h, w, dst, stream), "cgp_cov_moments")
                elif st.fn == "pool":
                    N.check(getattr(lib, f"cgp_cov_pool_{sfx}")(
                        ptr[st.src], n, cs.elems(st.src), dst, stream), "cgp_cov_pool")
                elif st.fn == "accum":
                    N.call(f"cgp_axpby_{sfx}", 1.0, dst, 1.0, ptr[st.src], dst,
                           n * cs.elems(st.dst), stream)
                elif st.fn == "axpby":
                    _axpby_terms(sfx, [(c, bufs[b]) for c, b in st.terms], bufs[st.dst],
                                 n * cs.elems(st.dst), stream)
                else:
                    if st.fn in ("conv", "conv_ntk"):
                        what = "cgp_covntk_conv" if ntk else "cgp_cov_conv"
                        r = N.CovConvNtkArgs() if ntk else N.CovConvArgs()
                        stencil(pairwise(maps(r, st), st), st)
                        r.post, r.flags = st.post, flags
                    elif st.fn in ("nonlin", "nonlin_ntk"):
                        what = "cgp_covntk_nonlin" if ntk else "cgp_cov_nonlin"
                        r = N.CovNonlinNtkArgs() if ntk else N.CovNonlinArgs()
                        pairwise(maps(r, st), st)
                        r.kind, r.flags = st.post, flags
                    elif st.fn == "gelu":
                        what = "cgp_gelu_cov"
                        r = pairwise(maps(N.GeluCovArgs(), st), st)
                    elif st.fn in ("abrelu", "abrelu_ntk"):
                        what = "cgp_abrelu_cov"
                        r = pairwise(maps(N.ABReluCovArgs(), st), st)
                        r.s, r.m, r.hh = st.op.smh
                        r.flags = flags
                    elif st.fn in ("sin", "sin_ntk"):
                        what = "cgp_sin_cov"
                        r = pairwise(maps(N.SinCovArgs(), st), st)
                        r.A, r.B, r.C, r.D = st.op.consts
                    elif st.fn in ("hermite", "hermite_ntk"):
                        what = "cgp_hermite_cov"
                        r = pairwise(maps(N.HermiteCovArgs(), st), st)
                        # the tables of every image of the variance maps, per launch: a map
                        # filled chunk by chunk (run_self_variances) changes between chunks
                        vx, vy = var[st.var]
                        ws = self._hermite_tables(  # noqa: F841 (alive until the launch)
                            r, st.op, sfx, stream, vx, vy, vx.shape[0], vy.shape[0],
                            r.h * r.w, same, ntk, x)
                    elif st.fn == "avgpool":
                        what = "cgp_covmap_avgpool"
                        r = maps(N.CovAvgPoolArgs(), st)
                        r.ho, r.wo, r.k, r.stride = h, w, st.op.geom.taps, st.op.geom.stride
                    elif st.fn == "corrconv":
                        what = "cgp_corrconv"
                        r = stencil(maps(N.CorrConvArgs(), st), st)
                        rr, rc = self._corr_tables(st.op, dev, x.dtype)
                        r.corr_rows, r.corr_cols = N.ptr(rr), N.ptr(rc)
                    elif st.fn == "tapconv":
                        what = "cgp_tapconv_cov"
                        r = maps(N.TapConvCovArgs(), st)
                        g = st.op.geom
                        r.ho, r.wo = h, w
                        r.extent, r.offset, r.stride, r.dilation = \
                            g.extent, g.offset, g.stride, g.dilation
                        r.bias, r.addend = st.bias, ptr[st.addend]
                        r.table = N.ptr(self._tap_table(st.op, dev, x.dtype))
                    else:
                        raise AssertionError(st.fn)
                    N.check(getattr(lib, f"{what}_{sfx}")(r, stream), what)
                if st.dst in diag_out:
                    N.check(getattr(lib, f"cgp_covmap_diag_{sfx}")(
                        dst, pi, n, h, w, N.ptr(diag_out[st.dst]), stream), "cgp_covmap_diag")
                for b in st.free:
                    del bufs[b]
        out_k = outs.get(cs.final)
        if last is None and cs.final_theta == cs.final:
            return out_k, out_k.clone()
        return out_k, outs.get(cs.final_theta)
