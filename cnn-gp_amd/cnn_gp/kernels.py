"""Drop-in NNGP kernel modules (reference: cnn_gp/kernels.py), evaluated on MI355X.

Same constructors, attributes and call surface as the reference —
``Sequential(*mods)(x, y=None, same=None, diag=False)`` — but ``forward`` runs a fused
device program (program.py) through libcnngp.so instead of torch ops.  Tensors are
storage only: no torch compute runs on the pair maps.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from .program import Plan

# the whole-network path computes the per-image variance maps with one cgp_var_chain launch
# (CGP_VAR_CHAIN=0: the layer-by-layer variance pipeline, one launch per op)
VAR_CHAIN = os.environ.get("CGP_VAR_CHAIN", "1") != "0"
# ntk_maps lowers a conv to the two-stream cgp_covntk_conv_* (DESIGN §3.7 has the measurement
# behind the default; set_ntk_maps_fusion overrides it per model)
NTK_MAPS_FUSED = True

__all__ = ("NNGPKernel", "Conv2d", "ReLU", "Erf", "Gelu", "ABReLU", "LeakyReLU",
           "Sin", "Cos", "Rbf",
           "HermiteNonlin", "Tanh", "Sigmoid", "Softplus", "SiLU", "GeluTanh", "gaussian_taps",
           "GlobalAvgPool", "AvgPool2d",
           "CorrelatedConv2d", "rbf_corr", "band_corr", "Sequential", "Mixture", "Sum",
           "resnet_block")


def _stream_handle(device):
    return torch.cuda.current_stream(device).cuda_stream


def _to_device(t: torch.Tensor, device) -> torch.Tensor:
    if t.device != device:
        t = t.to(device, non_blocking=True)
    return t.contiguous()


def _check_1x1(plan):
    """kernels.py:53-57: the kernel of a pair is the final value's one pixel."""
    if plan.final_hw != (1, 1):
        raise RuntimeError(f"the model's output is {plan.final_hw[0]}x{plan.final_hw[1]}"
                           " per pair, not 1x1: add a final Conv2d covering the map")


def _variances(plan, x, y, same, stream, need=None, what="cgp_moments_var"):
    """The per-image variances of the inputs (kernels.py:48-49), then the layer path's
    variance pipeline: the maps of plan.need_var, or of ``need``.  ``what`` names the first
    call in an error message (a run on position-pair maps adds the dtype)."""
    n1, c, h, w = x.shape
    n2 = y.shape[0]
    var0 = torch.empty((n1 + n2, h, w), dtype=x.dtype, device=x.device)
    N.check(getattr(N.load(), f"cgp_moments_var_{Plan._sfx(x.dtype)}")(
        N.ptr(x), N.ptr(y), n1, n2, c, h * w, N.ptr(var0[:n1]), N.ptr(var0[n1:]), stream),
        what)
    return plan.run_variances(var0[:n1], var0[n1:], n1, n2, same, stream, need=need)


def _moments_xy(x, y, diag, stream):
    """The input moments' pair maps (kernels.py:44-47): [N1·N2, H, W], or [N1, H, W] of the
    pairs (i, i) with diag."""
    n1, c, h, w = x.shape
    n2 = y.shape[0]
    xy0 = torch.empty((n1 if diag else n1 * n2, h, w), dtype=x.dtype, device=x.device)
    N.check(getattr(N.load(), f"cgp_moments_xy_{Plan._sfx(x.dtype)}")(
        N.ptr(x), N.ptr(y), n1, n2, c, h * w, int(diag), N.ptr(xy0), stream), "cgp_moments_xy")
    return xy0


def _pair_results(r, pi, pj, n1, n2, same, diag):
    """The [npairs] results of a run on position-pair maps as [n1] (diag), [n1, n2], or, from
    the pairs i <= j of a same tile, [n1, n1] mirrored: symmetric bit for bit."""
    if diag:
        return r.view(n1)
    if not same:
        return r.view(n1, n2)
    k = torch.empty((n1, n1), dtype=r.dtype, device=r.device)
    k[pj, pi] = r.view(-1)
    k[pi, pj] = r.view(-1)
    return k


def _pair_maps(r, pi, pj, lead, ho, wo, same, diag):
    """The [npairs, elements] maps of a run as ``lead`` + (p_row, p_col, q_row, q_col) from the
    internal layout [p_row][q_row][p_col][q_col]; on a same tile the pairs i > j are the
    mirror X_ji[q, p] = X_ij[p, q]."""
    r = r.view(-1, ho, ho, wo, wo).permute(0, 1, 3, 2, 4)
    if not same or diag:
        return r.reshape(lead + (ho, wo, ho, wo))
    s = torch.empty(lead + (ho, wo, ho, wo), dtype=r.dtype, device=r.device)
    s[pj, pi] = r.permute(0, 3, 4, 1, 2)
    s[pi, pj] = r
    return s


class _ImageVariances:
    """Variance maps of one image set for one Gram build (NNGPKernel.image_variances):
    var[v] = [N, h, w] maps of every value the whole-network kernel reads, and what the
    library's fp64 closed-form ReLU reads in their place (cgp_net_var_form): qvar[v], their
    x-side copies scaled by cgp_net_xvar_scale() = 1/16, or mvar[v], the 1/sqrt(v/8) maps
    that serve the set on either side of a tile; key = (H, W, dtype, plan flags)."""

    __slots__ = ("images", "var", "qvar", "mvar", "key")

    def __init__(self, images, var, qvar, key, mvar=None):
        self.images, self.var, self.qvar, self.key = images, var, qvar, key
        self.mvar = mvar or {}

    def __len__(self):
        return len(self.images)


# bumped by every change an NNGPKernel's structure key could see (attribute sets and
# deletes, add_module / register_buffer, .to() / .double() / .cuda() through _apply):
# _structure_key reuses its last walk while the generation is unchanged
_GENERATION = [0]


class NNGPKernel(nn.Module):
    """Base class; ``forward`` mirrors kernels.py:18-57."""

    def __setattr__(self, name, value):
        _GENERATION[0] += 1
        super().__setattr__(name, value)

    def __delattr__(self, name):
        _GENERATION[0] += 1
        super().__delattr__(name)

    def add_module(self, name, module):
        _GENERATION[0] += 1
        super().add_module(name, module)

    def register_buffer(self, name, tensor, persistent=True):
        _GENERATION[0] += 1
        super().register_buffer(name, tensor, persistent)

    def _apply(self, fn, *args, **kwargs):
        _GENERATION[0] += 1
        out = super()._apply(fn, *args, **kwargs)
        _GENERATION[0] += 1
        return out

    def _plan(self, h: int, w: int) -> Plan:
        cache = self.__dict__.setdefault("_cgp_plans", {})
        fusion = getattr(self, "_cgp_fusion", True)
        exact = getattr(self, "_cgp_exact_relu", False)
        key = (h, w, fusion, exact, self._structure_key())
        wver = self._weights_version()
        if self.__dict__.get("_cgp_wver") != wver:
            # a Conv2d weight buffer changed in place (load_state_dict, mul_, .data = …):
            # the reference reads self.kernel on every call (kernels.py:92-97), so every
            # plan built from the old weights goes
            cache.clear()
            self.__dict__["_cgp_wver"] = wver
        plan = cache.get(key)
        if plan is None:
            plan = Plan(self, h, w, enable_fusion=fusion, exact_relu=exact)
            cache[key] = plan
        return plan

    def _structure_key(self):
        """Changes whenever a hyper-parameter the program depends on changes.  Asked on
        every forward (the plan cache's key): ``modules()`` over the 114-module ResNets
        cost a quarter of a millisecond per call, as long as a B = 200 tile's kernels
        (bench.py ``dropin``).  So the last key is reused while no NNGPKernel has changed
        since (_GENERATION; a tree with a Mixture is walked every time, its logits can
        change in place), and the walk itself goes by hand (pre-order, attributes read
        from the instance dicts)."""
        memo = self.__dict__.get("_cgp_skey")
        if memo is not None and memo[0] == _GENERATION[0]:
            return memo[1]
        gen = _GENERATION[0]
        mixture = False
        key = []
        bufs = []
        stack = [self]
        while stack:
            m = stack.pop()
            d = m.__dict__
            if isinstance(m, Conv2d):
                # host-side attributes only: reading the (device) buffer would sync
                key.append(("c", d["kernel_size"], d["stride"], d["padding"], d["dilation"],
                            float(d["var_weight"]), float(d["var_bias"]),
                            d["_buffers"]["kernel"].dtype))
                bufs.append(d["_buffers"]["kernel"])
            elif isinstance(m, AvgPool2d):
                key.append(("a", d["kernel_size"], d["stride"]))
            elif isinstance(m, CorrelatedConv2d):
                # R lives on the host as tuples: nothing to sync, no in-place edits
                key.append(("r", d["kernel_size"], d["stride"], d["_padding_arg"], d["padding"],
                            d["dilation"], float(d["var_weight"]), float(d["var_bias"]),
                            d["lengthscale"], d["corr_rows"], d["corr_cols"]))
            elif isinstance(m, ABReLU):
                # the slopes are in the op records: a plan serves one (a, b)
                key.append(("ab", float(d["a"]), float(d["b"])))
            elif isinstance(m, Sin):
                # the constants are in the op records: a plan serves one (A, B, C, D)
                key.append(("sin", *m.constants()))
            elif isinstance(m, HermiteNonlin):
                # the rule is in the op records: a plan serves one (phi, order, quad_nodes)
                key.append(("hermite", *m.rule()))
            elif isinstance(m, Mixture):
                mixture = True
                key.append(("m", tuple(m.proportions())))
            else:
                key.append((type(m).__name__, len(d.get("mods", ()))))
            stack.extend(reversed(d["_modules"].values()))
        key = tuple(key)
        self.__dict__["_cgp_bufs"] = (gen, bufs)
        if not mixture:
            self.__dict__["_cgp_skey"] = (gen, key)     # not through __setattr__
        return key

    def _weights_version(self):
        """(version counter, address) of every Conv2d weight buffer in the tree, read on
        the host (no sync): in-place edits bump a tensor's version without touching
        __setattr__, so the structure key alone cannot see them."""
        memo = self.__dict__.get("_cgp_bufs")
        if memo is None or memo[0] != _GENERATION[0]:
            self.__dict__.pop("_cgp_skey", None)
            self._structure_key()
            memo = self.__dict__["_cgp_bufs"]
        return tuple((b._version, b.data_ptr()) for b in memo[1])

    def set_fusion(self, enabled: bool):
        """Enable/disable op fusion in the pair pipeline (for A/B tests; default on)."""
        for m in self.modules():
            m.__dict__["_cgp_fusion"] = bool(enabled)
        return self

    def set_fused_network(self, enabled: bool):
        """Run off-diagonal forwards on the whole-network kernel (csrc/netfuse.hip: one
        workgroup carries a pair's map through every layer in LDS; default) or on the
        layer-by-layer pipeline (one HBM pass per fused op).  Models the fused kernel
        has no instantiation for use the layer path either way."""
        for m in self.modules():
            m.__dict__["_cgp_netfuse"] = bool(enabled)
        return self

    def _net_plan(self, plan, itemsize):
        """The NetPlan of ``plan`` or None (unsupported program / disabled)."""
        if not getattr(self, "_cgp_netfuse", True):
            return None
        key = ("_net", itemsize)
        if key not in plan.__dict__:
            from .netplan import NetPlan, Unsupported
            try:
                plan.__dict__[key] = NetPlan(plan, itemsize)
            except Unsupported:
                plan.__dict__[key] = None
        return plan.__dict__[key]

    def set_exact_relu(self, enabled: bool):
        """Evaluate the ReLU map op by op exactly like the reference (correctly rounded
        1/sqrt, sqrt, acos, division) instead of the closed form (default; within 1e-14 of
        the exact map, see csrc/relu_poly.h).  For parity studies; ~2x slower.  An Erf and
        a Gelu have one evaluation mode and ignore it, and so do a Sin / Cos / Rbf and a
        HermiteNonlin; an ABReLU / LeakyReLU evaluates the
        ReLU map inside it in the chosen mode."""
        for m in self.modules():
            m.__dict__["_cgp_exact_relu"] = bool(enabled)
        return self

    def set_pool_workspace(self, max_bytes: Optional[int]):
        """Bytes of device memory the position-pair maps of a model with a GlobalAvgPool, an
        AvgPool2d or a CorrelatedConv2d (and position_covariance) may take at once; the pairs
        of a tile run in chunks sized to it, with bit-identical results.  None (default): a
        quarter of the device's free memory, as image_variances takes."""
        for m in self.modules():
            m.__dict__["_cgp_pool_ws"] = None if max_bytes is None else int(max_bytes)
        return self

    def _prologue(self, x, y, same, diag):
        """The argument rules of kernels.py:23-35, the dtype check and the empty-batch
        result shared by forward and ntk: (y, same, diag, empty) with ``empty`` the result
        tensor of an empty batch, else None."""
        if y is None:                                            # kernels.py:23-26
            assert same is None
            y = x
            same = True
        assert not diag or len(x) == len(y), (
            "diagonal kernels must operate with data of equal length")
        assert 4 == len(x.size())
        assert 4 == len(y.size())
        assert x.size(1) == y.size(1)
        assert x.size(2) == y.size(2)
        assert x.size(3) == y.size(3)
        same = bool(same)
        diag = bool(diag)
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"cnn_gp kernels compute in float32 or float64, got {x.dtype}")
        empty = None
        if len(x) == 0 or len(y) == 0:
            # the reference's torch ops return the empty [N1, N2] / [N1] result for an empty
            # batch (conv2d on a zero-size batch); there is nothing to evaluate
            empty = torch.empty((len(x),) if diag else (len(x), len(y)), dtype=x.dtype,
                                device=x.device)
        return y, same, diag, empty

    @staticmethod
    def _compute_device(x):
        if x.device.type == "cuda":
            return x.device
        if not torch.cuda.is_available():
            raise RuntimeError("cnn_gp on MI355X needs a HIP device: no GPU is visible "
                               "(there is no CPU path)")
        return torch.device("cuda", torch.cuda.current_device())

    def _on_compute_device(self, x, y, run):
        """run(x, y, stream) with the images on the compute device and that device current;
        the tensors it returns, moved back to where x lives."""
        out_device = x.device
        dev = self._compute_device(x)
        with torch.cuda.device(dev):
            xd = _to_device(x, dev)
            yd = xd if y is x else _to_device(y.to(x.dtype), dev)
            outs = run(xd, yd, _stream_handle(dev))
        return [o.to(out_device) for o in outs] if out_device != dev else outs

    def forward(self, x, y=None, same=None, diag=False):
        """[N1,C,H,W] × [N2,C,H,W] -> kernel [N1,N2] (or [N1] when diag)."""
        y, same, diag, empty = self._prologue(x, y, same, diag)
        if empty is not None:
            return empty
        return self._on_compute_device(
            x, y, lambda xd, yd, stream: [self._run(xd, yd, same, diag, stream)])[0]

    def ntk(self, x, y=None, same=None, diag=False, return_nngp=False):
        """The neural tangent kernel Θ of the model, [N1, N2] (or [N1] when diag); with
        ``return_nngp`` the pair (K, Θ), K the NNGP kernel ``forward`` gives.  Arguments,
        dtypes, devices, the empty-batch result and the "not 1x1" error are forward's.

        Θ is the infinite-width kernel of the network trained by gradient descent rather
        than at initialisation, in the reference's conventions (ReLU without the √2,
        weight var_weight/k² per tap).  It follows K through the module tree:

            inputs          Θ = 0                        (inputs are not parameters)
            Conv2d          K' = A(K) + var_bias,  Θ' = A(Θ) + K'   (A: the conv's stencil
                                                                      without the bias)
            ReLU            K' as forward,         Θ' = Θ·κ̇,  κ̇ = (π - θ)/2π with
                            θ = acos(clamp(c·rsqrt(v₁v₂ + f32_tiny), -1, 1)) of the
                            reference's ReLU (kernels.py:146-151); Θ' = Θ/2 exactly where
                            the reference overrides K' (same and i = j, or same and diag)
            Erf             K' = (2/π)·atan(2c/√D),  Θ' = Θ·κ̇,  κ̇ = (4/π)/√D with
                            D = 1 + 2(v₁ + v₂) + 4(v₁v₂ − c²), raised to 1 below 1;
                            κ̇ = (4/π)/√(1 + 4v) where K' is overridden  
            Gelu            K' as forward,         Θ' = Θ·κ̇,  κ̇ = E[φ'(u₁)φ'(u₂)] =
                            (1/Δ² + (1 − v₁v₂)/((1 + v₁)(1 + v₂)) + 1)·t/2π + 1/4 + atan(t)/2π,
                            t = c/Δ, Δ² = (1 + v₁)(1 + v₂) − c² raised to 1 below 1; the same
                            at c = v₁ = v₂ = v where K' is overridden  
            ABReLU(a, b)    K' as forward,         Θ' = Θ·κ̇,  κ̇ = (a − b)²·(π - θ)/2π + ab
                            with the ReLU's θ; Θ' = Θ·(a² + b²)/2 where K' is overridden
                            
            Sin(a, b, θ)    K' as forward,         Θ' = Θ·κ̇,  κ̇ = D·(e_d + C·e_s) with
                            e_d = exp(−B·(v₁ + v₂ − 2c)), e_s = exp(−B·(v₁ + v₂ + 2c)) and
                            (B, C, D) = (b²/2, cos 2θ, a²b²/2); κ̇ = D·(1 + C·exp(−4B·v)) where
                            K' is overridden; Cos is θ = π/2, Rbf(γ) is κ̇ = 2γ·K'  
            HermiteNonlin   K' as forward,         Θ' = Θ·κ̇,  κ̇ = Σ a'_n(v₁)·a'_n(v₂)·ρⁿ, the
                            series of φ' (Tanh, Sigmoid, Softplus, SiLU, GeluTanh)
            Sum / Mixture   the same (weighted) sum on both

        and the result is Θ of the final 1x1 value; a model without a Conv2d gives zeros
        (and K from forward itself).
        Equivalently Θ = Σ over all Conv2d outputs of ⟨∂K_final/∂K_xy^l, K_xy^l⟩ at fixed
        variances.  Always evaluated layer by layer (program.ntk_steps: the whole-network
        kernel carries one map); honours set_exact_relu.  A model with a GlobalAvgPool, an
        AvgPool2d or a CorrelatedConv2d raises NotImplementedError here: its Θ is carried on
        position-pair maps by ``ntk_maps`` (and ``position_ntk``), DESIGN §3.7."""
        y, same, diag, empty = self._prologue(x, y, same, diag)
        plan = self._plan(x.size(2), x.size(3))
        if plan.pool is not None:
            from .program import AVGPOOL_RULE_NTK, CORRCONV_RULE_NTK, POOL_RULE_NTK
            kinds = {o.kind for o in plan.prog.ops}
            raise NotImplementedError(CORRCONV_RULE_NTK if "corrconv" in kinds else
                                      AVGPOOL_RULE_NTK if "avgpool" in kinds else POOL_RULE_NTK)
        if empty is not None:
            return (empty, empty.clone()) if return_nngp else empty
        k, th = self._on_compute_device(
            x, y, lambda xd, yd, stream: self._run_ntk(xd, yd, same, diag, stream))
        return (k, th) if return_nngp else th

    def _run_ntk(self, x, y, same, diag, stream):
        n1, c, h, w = x.shape
        n2 = y.shape[0]
        plan = self._plan(h, w)
        _check_1x1(plan)
        if not any(o.kind in ("conv", "tapconv") for o in plan.prog.ops):
            # no Conv2d, no parameters: Θ = 0 and there is no second stream to carry, so K
            # is forward's own run, bit for bit whichever path forward takes (the
            # whole-network kernel's fp64 ReLU and cgp_relu_* differ by an ulp on some pixels)
            k = self._run(x, y, same, diag, stream)
            return k, torch.zeros_like(k)
        var = _variances(plan, x, y, same, stream, plan.ntk_need_var())
        k, th = plan.run_layer_steps(plan.layer_list(ntk=True), x, y,
                                     _moments_xy(x, y, diag, stream), var, n1, n2, same, diag,
                                     stream)
        if th is None:
            th = torch.zeros_like(k)
        elif th is k:
            th = k.clone()
        shape = (n1,) if diag else (n1, n2)
        return k.view(shape), th.view(shape)

    def _run(self, x, y, same, diag, stream):
        n1, c, h, w = x.shape
        n2 = y.shape[0]
        plan = self._plan(h, w)
        if plan.pool is not None:     # GlobalAvgPool, AvgPool2d, CorrelatedConv2d: DESIGN §3.3-5
            _check_1x1(plan)
            r, _, pi, pj = self._run_cov(plan, plan.pool, x, y, same, diag, stream)
            return _pair_results(r, pi, pj, n1, n2, same, diag)
        if diag and same and VAR_CHAIN and self._net_plan(plan, x.element_size()) is not None:
            # same and diag: the reference overrides every K' with the image's own variance
            # (kernels.py:134-165), so the result IS the variance chain's final value — the
            # launch that fills K[i, i] of a same tile.  Taken from it, the two agree bit for
            # bit in either precision (the layer pipeline below sums in another order: up to
            # 2 ulp apart in float32)
            fused = plan.run_variances_fused(x, x, n1, n1, True, stream, {plan.vf})
            if fused is not None:
                return fused[0][plan.vf][0].reshape(n1)
        net = None if diag else self._net_plan(plan, x.element_size())
        if net is not None and VAR_CHAIN:
            # the same launches from a recipe built once per tile shape and stream (record
            # upload, state buffers and argument structs done once; netplan.TileRecipe)
            rec = net.tile_recipe(plan, x, y, n1, n2, same, plan.flags, stream)
            if rec is not None:
                return rec.run(x, y, stream)
            # every variance map in one launch (cgp_var_chain_*), scaled (1/16) x-side copies
            # included (kernels.py:44-49 moments, then the program on each image)
            fused = plan.run_variances_fused(x, y, n1, n2, same, stream, net.need_var,
                                             net.chain_quarter(x.dtype, plan.flags),
                                             views=False)
            if fused is not None:
                var, qvar = fused
                return net.run(x, y, var, n1, n2, same, stream, plan.flags,
                               qvar=qvar or None)
        if net is not None:                                      # whole-network kernel
            var = _variances(plan, x, y, same, stream, net.need_var)
            return net.run(x, y, var, n1, n2, same, stream, plan.flags)
        var = _variances(plan, x, y, same, stream)
        xy0 = None if plan.moments_fused else _moments_xy(x, y, diag, stream)
        out, _ = plan.run_layer_steps(plan.layer_list(), x, y, xy0, var, n1, n2, same, diag,
                                      stream)
        _check_1x1(plan)
        return out.view(n1) if diag else out.view(n1, n2)

    # ---- position-pair maps: GlobalAvgPool, AvgPool2d, CorrelatedConv2d and their NTK ----
    def _run_cov(self, plan, cs, x, y, same, diag, stream):
        """Runs the launch list ``cs`` (program.pool_steps or pool_ntk_steps) on the pairs of a
        tile: all of them, the pairs i <= j of a same tile, or (i, i) for diag.  Returns
        (K, Θ, pair_i, pair_j): the final value of every pair [npairs, elements] -- Θ None for
        a forward list, zeros for a model without a conv -- and the pair lists as int64 index
        tensors."""
        pi, pj, var, ws = self._pool_pairs(plan, cs.forward or cs, x, y, same, diag, stream)
        k, th = plan.run_cov_steps(cs, x, y, var, pi.to(torch.int32), pj.to(torch.int32), same,
                                   stream, ws)
        if th is None and cs.forward is not None:
            th = torch.zeros_like(k)
        return k, th, pi, pj

    def _pool_pairs(self, plan, ps, x, y, same, diag, stream):
        """The pair lists of a tile (int64 index tensors), the variance maps ``ps`` reads
        and the workspace bound: what a run on position-pair maps starts from."""
        n1, n2, dev = x.shape[0], y.shape[0], x.device
        if diag:
            pi = pj = torch.arange(n1, device=dev)
        elif same:
            pi, pj = torch.triu_indices(n1, n1, device=dev)     # _pair_results mirrors them
        else:
            pi = torch.arange(n1, device=dev).repeat_interleave(n2)
            pj = torch.arange(n2, device=dev).repeat(n1)
        var = {}
        ws = getattr(self, "_cgp_pool_ws", None)
        if ps.need_var - ps.self_var:
            # the layer path's own pipeline
            var = _variances(plan, x, y, same, stream, set(ps.need_var - ps.self_var),
                             "cgp_moments_var_" + Plan._sfx(x.dtype))
        if ps.self_var:
            # downstream of an AvgPool2d the variances are the p = q diagonals of the images'
            # self position-pair maps: the same launches over the pairs (i, i)
            sx = plan.run_self_variances(x, {v: m[0] for v, m in var.items()}, stream, ps, ws)
            sy = sx if same else \
                plan.run_self_variances(y, {v: m[1] for v, m in var.items()}, stream, ps, ws)
            var = dict(var)
            var.update({v: (sx[v], sy[v]) for v in ps.self_var})
        return pi, pj, var, ws

    def set_ntk_maps_fusion(self, enabled: bool):
        """Lower the convs of ntk_maps / position_ntk to the two-stream cgp_covntk_conv_*
        (default) or to the launch-by-launch sequence; the results are the same bits."""
        for m in self.modules():
            m.__dict__["_cgp_ntk_maps_fused"] = bool(enabled)
        return self

    def _ntk_maps_steps(self, plan, body, x):
        """program.pool_ntk_steps of the plan as set_ntk_maps_fusion and x's dtype have it."""
        return plan.pool_ntk(body, getattr(self, "_cgp_ntk_maps_fused", NTK_MAPS_FUSED),
                             x.element_size())

    def ntk_maps(self, x, y=None, same=None, diag=False, return_nngp=False):
        """The neural tangent kernel Θ, [N1, N2] (or [N1] when diag), carried on position-pair
        maps; with ``return_nngp`` the pair (K, Θ).  Valid for every model forward runs on
        position-pair maps -- a GlobalAvgPool, AvgPool2d or CorrelatedConv2d anywhere the
        forward rules allow, with ReLU, Erf, Gelu, ABReLU, Sin / Cos / Rbf and HermiteNonlin -- and
        for a model
        with none of them,
        where it is a second, slower route to ``ntk``'s result.

        The recursion is ntk's, with the pooling layers the same linear op on both streams
        and a CorrelatedConv2d the conv's rule with its own stencil:

            Conv2d, CorrelatedConv2d   K' = A(K) + var_bias,  Θ' = A(Θ) + K'
            ReLU / Erf / Gelu / ABReLU K' as forward,         Θ' = Θ·κ̇   (ntk's κ̇ of
            / Sin / Cos / Rbf
                                       (S[p, q], xx_i[p], yy_j[q]); the override's value
                                       where same, i = j and p = q)
            AvgPool2d, GlobalAvgPool   the same average of K and of Θ
            Sum / Mixture              the same (weighted) sum on both

        Arguments, dtypes, devices, the empty-batch result, the "not 1x1" error and the
        same-tile handling (pairs i <= j, then mirrored: symmetric bit for bit) are
        forward's; for a model forward itself runs on position-pair maps K is forward's, bit
        for bit.  Honours set_exact_relu and set_pool_workspace (a chunk holds K and Θ)."""
        y, same, diag, empty = self._prologue(x, y, same, diag)
        plan = self._plan(x.size(2), x.size(3))
        body = not any(o.kind == "pool" for o in plan.prog.ops)
        plan.pool_ntk(body, True, 8)                  # the lowering's rejections come first
        if empty is not None:
            return (empty, empty.clone()) if return_nngp else empty
        self._compute_device(x)                       # forward's order: no device, then
        _check_1x1(plan)                              # a final value that is not 1x1

        def run(xd, yd, stream):
            k, th, pi, pj = self._run_cov(plan, self._ntk_maps_steps(plan, body, xd), xd, yd,
                                          same, diag, stream)
            return [_pair_results(r, pi, pj, len(x), len(y), same, diag) for r in (k, th)]

        with torch.no_grad():
            k, th = self._on_compute_device(x, y, run)
        return (k, th) if return_nngp else th

    def position_ntk(self, x, y=None, same=None, diag=False, return_nngp=False):
        """position_covariance's twin for Θ: Θ[i, j, p, q] of a model without a GlobalAvgPool,
        [N1, N2, H', W', H', W'] (diag: [N1, H', W', H', W']) in the order (p_row, p_col, q_row,
        q_col) -- what a GlobalAvgPool after this model averages in ntk_maps; on a same tile
        the pairs i > j are the mirror Θ_ji[q, p] = Θ_ij[p, q].  With ``return_nngp`` the pair
        (S, Θ), S position_covariance's map."""
        y, same, diag, empty = self._prologue(x, y, same, diag)
        plan = self._plan(x.size(2), x.size(3))
        ho, wo = plan.pool_ntk(True, True, 8).forward.shapes[plan.vf]
        lead = (len(x),) if diag else (len(x), len(y))
        if empty is not None:
            e = torch.empty(lead + (ho, wo, ho, wo), dtype=x.dtype, device=x.device)
            return (e, e.clone()) if return_nngp else e

        def run(xd, yd, stream):
            s, th, pi, pj = self._run_cov(plan, self._ntk_maps_steps(plan, True, xd), xd, yd,
                                          same, diag, stream)
            return [_pair_maps(r, pi, pj, lead, ho, wo, same, diag) for r in (s, th)]

        with torch.no_grad():
            s, th = self._on_compute_device(x, y, run)
        return (s, th) if return_nngp else th

    def position_covariance(self, x, y=None, same=None, diag=False):
        """The position-pair covariance map of the model's output: S[i, j, p, q], the
        covariance of pixel p of the output on x_i with pixel q of the output on y_j -- what
        a GlobalAvgPool after this model averages.  [N1, N2, H', W', H', W'] (diag:
        [N1, H', W', H', W']) in the order (p_row, p_col, q_row, q_col); its entries
        [i, j, p, p] are the pair maps the layer path carries.  The model itself has no
        GlobalAvgPool.  Arguments, dtypes and devices as forward; the maps of all pairs are
        held at once on top of the workspace of set_pool_workspace."""
        y, same, diag, empty = self._prologue(x, y, same, diag)
        plan = self._plan(x.size(2), x.size(3))
        ps = plan.body_steps()
        ho, wo = ps.shapes[ps.final]
        lead = (len(x),) if diag else (len(x), len(y))
        if empty is not None:
            return torch.empty(lead + (ho, wo, ho, wo), dtype=x.dtype, device=x.device)

        def run(xd, yd, stream):
            s, _, pi, pj = self._run_cov(plan, ps, xd, yd, same, diag, stream)
            return [_pair_maps(s, pi, pj, lead, ho, wo, same, diag)]

        return self._on_compute_device(x, y, run)[0]

    # ---- Gram builds: every image's variance maps once per build -------------------
    # The reference (and forward above) recomputes the per-image variance recursion
    # (kernels.py:44-49, then every layer on the same/diag path) for both image blocks of
    # every tile: a Gram build over B-row tiles of N images does it about 2N/B times per
    # image.  image_variances() runs the whole-network program's variance chain once over
    # an image set; tile_from_variances() evaluates one tile from slices of two such sets.
    # Nothing is kept between builds (the caller holds the maps for one build).

    def image_variances(self, x: torch.Tensor, max_bytes: Optional[int] = None):
        """The variance maps every whole-network tile of images ``x`` ([N, C, H, W], on the
        device) reads, computed in one launch: an object for tile_from_variances, or None
        when the model runs on the layer path (shapes netfuse lacks, CGP_VAR_CHAIN=0, maps
        the chain kernel cannot hold) or the maps would take more than ``max_bytes``
        (default: a quarter of the device's free memory) -- callers then fall back to
        forward() per tile."""
        if x.device.type != "cuda" or x.dtype not in (torch.float32, torch.float64) or \
                x.dim() != 4 or not VAR_CHAIN:
            return None
        n, _, h, w = x.shape
        plan = self._plan(h, w)
        net = self._net_plan(plan, x.element_size())
        if net is None:
            return None
        quarter = net.chain_quarter(x.dtype, plan.flags)
        chain = plan._var_chain(set(net.need_var), set(quarter) & set(net.need_var), x.device)
        if chain is None:
            return None
        # the rsqrt form's 1/sqrt(v/8) maps take the place of the scaled copies
        roots = net.root_elems(x.dtype, plan.flags)
        size = n * (chain["total"] + chain["qtotal"] + roots) * x.element_size()
        if max_bytes is None:
            max_bytes = torch.cuda.mem_get_info(x.device)[0] // 4
        if size > max_bytes:
            return None
        x = x.contiguous()
        mvar = {}
        with torch.cuda.device(x.device):
            stream = _stream_handle(x.device)
            fused = plan.run_variances_fused(x, x, n, n, True, stream, net.need_var, quarter)
            if fused is not None and roots:
                # one launch on the same stream, after the chain that writes the plain maps
                used = sorted(net.quarter_vars(x.dtype, plan.flags))
                mvar = {v: torch.empty_like(fused[0][v][0]) for v in used}
                k = len(used)
                N.call("cgp_rsqrt_batch_f64", k,
                       (ctypes.c_void_p * k)(*[fused[0][v][0].data_ptr() for v in used]),
                       (ctypes.c_void_p * k)(*[mvar[v].data_ptr() for v in used]),
                       (ctypes.c_int64 * k)(*[mvar[v].numel() for v in used]), stream)
        if fused is None:
            return None
        var, qvar = fused
        return _ImageVariances(x, {v: xx for v, (xx, _) in var.items()}, dict(qvar),
                               (h, w, x.dtype, plan.flags, self._weights_version()), mvar)

    def tile_from_variances(self, vx: "_ImageVariances", i0: int, i1: int,
                            vy: "_ImageVariances", j0: int, j1: int, same: bool,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K[i0:i1, j0:j1] of vx's images against vy's, equal to
        forward(vx.images[i0:i1], vy.images[j0:j1], same, False) (same: a diagonal tile,
        the same rows of one set).  ``out``: an [i1 - i0, j1 - j0] row-major view of the
        images' dtype to write into (e.g. a tile of the Gram matrix)."""
        if vx.key != vy.key:
            raise ValueError("tile_from_variances: the two image sets were prepared for "
                             "different shapes, dtypes or ReLU modes")
        if same and (vx is not vy or (i0, i1) != (j0, j1)):
            raise ValueError("a diagonal tile takes the same rows of one image set")
        # the kernel indexes the sliced maps by the tile's extents: they must be in range
        if not (0 <= i0 < i1 <= len(vx) and 0 <= j0 < j1 <= len(vy)):
            raise ValueError(f"tile rows [{i0}, {i1}) x cols [{j0}, {j1}) outside the image "
                             f"sets ({len(vx)}, {len(vy)})")
        h, w, dtype, flags, wver = vx.key
        plan = self._plan(h, w)
        if plan.flags != flags:
            raise ValueError("tile_from_variances: the model's ReLU mode changed since "
                             "image_variances")
        if self._weights_version() != wver:
            raise ValueError("tile_from_variances: a Conv2d weight buffer changed since "
                             "image_variances (bind the image sets again)")
        net = self._net_plan(plan, torch.empty((), dtype=dtype).element_size())
        x, y = vx.images[i0:i1], vy.images[j0:j1]
        var = {v: (m[i0:i1], vy.var[v][j0:j1]) for v, m in vx.var.items()}
        qvar = {v: q[i0:i1] for v, q in vx.qvar.items()}
        mvar = {v: (m[i0:i1], vy.mvar[v][j0:j1]) for v, m in vx.mvar.items()}
        with torch.cuda.device(x.device):
            return net.run(x, y, var, i1 - i0, j1 - j0, same, _stream_handle(x.device),
                           flags, out=out, qvar=qvar or None, mvar=mvar or None)

    def layers(self):
        return 0


def gaussian_taps(k, lengthscale):
    """The k x k table exp(-r²/(2ℓ²)) of relative tap variances, r the distance of a tap from
    the filter's centre ((k - 1)/2 on both axes), ℓ = ``lengthscale`` > 0 in taps: a Gaussian
    taper for ``Conv2d(..., tap_weights=...)``.  ℓ = inf is all ones, the reference's box."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"gaussian_taps: k must be a positive integer, got {k!r}")
    try:
        ls = float(lengthscale)
    except (TypeError, ValueError):
        ls = float("nan")
    if not ls > 0:
        raise ValueError(f"gaussian_taps: lengthscale must be positive, got {lengthscale!r}")
    c = np.arange(int(k), dtype=np.float64) - (int(k) - 1) / 2
    r2 = c[:, None] ** 2 + c[None, :] ** 2
    return torch.from_numpy(np.exp(-r2 / (2.0 * ls * ls)))


class Conv2d(NNGPKernel):
    """kernels.py:60-98 — constant k×k kernel of value var_weight/k², plus var_bias.

    As in the reference, ``kernel`` is an ordinary buffer read on every call: any finite
    buffer of its own shape is honoured, whatever wrote it (in-place ops, ``.data =``,
    ``load_state_dict``), as the prior variances of the conv's taps.
    ``tap_weights``: a k×k table (tensor, array or nested list) of finite non-negative
    relative variances W with a positive sum; the buffer is then var_weight·W/ΣW over the k×k
    taps (the zero first row and column of an even "same" kernel are kept).  None, and a
    table of ones, give the reference's box."""

    def __init__(self, kernel_size, stride=1, padding="same", dilation=1,
                 var_weight=1., var_bias=0., in_channel_multiplier=1,
                 out_channel_multiplier=1, tap_weights=None):
        super().__init__()
        self.kernel_size = kernel_size
        self.stride = stride
        self.dilation = dilation
        self.var_weight = var_weight
        self.var_bias = var_bias
        self.kernel_has_row_of_zeros = False
        self._padding_arg = padding
        if padding == "same":
            self.padding = dilation * (kernel_size // 2)
            self.kernel_has_row_of_zeros = kernel_size % 2 == 0
        else:
            self.padding = padding
        # the reference's kernel buffer: default dtype (float32), so model.double()
        # yields float32-rounded weights — kept for identical numerics and for
        # .cuda()/.double() semantics
        side = kernel_size + 1 if self.kernel_has_row_of_zeros else kernel_size
        kernel = torch.ones(1, 1, side, side)
        if self.kernel_has_row_of_zeros:
            kernel[:, :, 0, :] = 0.
            kernel[:, :, :, 0] = 0.
        if tap_weights is not None:
            # W/mean(W) in double over the k x k taps (ones for a table of ones, so the
            # product below has the box's bits), then the box's scale and dtype
            kernel = kernel.double()
            kernel[0, 0, side - kernel_size:, side - kernel_size:] = \
                self._relative_taps(tap_weights, kernel_size)
            kernel = (kernel * (self.var_weight / self.kernel_size ** 2)).to(
                torch.get_default_dtype())
            self.register_buffer("kernel", kernel)
        else:
            self.register_buffer("kernel",
                                 kernel * (self.var_weight / self.kernel_size ** 2))
        self.in_channel_multiplier = in_channel_multiplier
        self.out_channel_multiplier = out_channel_multiplier

    @staticmethod
    def _relative_taps(tap_weights, k):
        """``tap_weights`` as a k x k double tensor divided by its mean; ValueError naming
        what is wrong with it."""
        try:
            w = torch.as_tensor(np.asarray(tap_weights.detach().cpu() if
                                           isinstance(tap_weights, torch.Tensor)
                                           else tap_weights, dtype=np.float64))
        except (TypeError, ValueError) as e:
            raise ValueError(f"Conv2d: tap_weights is not a table of numbers ({e})") from None
        if tuple(w.shape) != (k, k):
            raise ValueError(f"Conv2d: tap_weights must be a {k}x{k} table for kernel_size="
                             f"{k}, got shape {tuple(w.shape)}")
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("Conv2d: tap_weights must be finite and non-negative, got "
                             f"{w.tolist()}")
        if not float(w.sum()) > 0:
            raise ValueError("Conv2d: tap_weights must have a positive sum")
        return w / w.mean()

    def _is_box(self):
        """The buffer is the constructor's constant box (program.conv_geometry's test)."""
        from .program import conv_geometry
        try:
            conv_geometry(self)
        except (NotImplementedError, RuntimeError):
            return False
        return True

    def layers(self):
        return 1

    def extra_repr(self):
        return (f"kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, dilation={self.dilation}, "
                f"var_weight={self.var_weight}, var_bias={self.var_bias}"
                + ("" if self._is_box() else ", taps=custom"))


class ReLU(NNGPKernel):
    """kernels.py:128-165 — the arc-cosine covariance map (device: relu_cov)."""
    f32_tiny = np.finfo(np.float32).tiny

    def layers(self):
        return 0


class Erf(NNGPKernel):
    """The erf nonlinearity (no reference counterpart; the paper's second closed form,
    Williams 1997): K' = (2/π)·asin(2c/√((1+2v₁)(1+2v₂))), evaluated in the atan form of
    DESIGN §3.2 (device: ErfMap).  Runs on the layer path; set_exact_relu has no effect
    on it."""

    def layers(self):
        return 0


class Gelu(NNGPKernel):
    """The GELU nonlinearity φ(x) = x·Φ(x), the exact one and not its tanh approximation (no
    reference counterpart; closed form of Tsuchida, Pearce et al. 2021).  With
    Δ² = (1 + v₁)(1 + v₂) − c² and t = c/Δ:
    K' = ((c² + v₁v₂·Δ²)/((1 + v₁)(1 + v₂)·Δ) + c·atan(t))/2π + c/4  (device:
    gelu_map).  Usable wherever Erf is: forward, ntk, position_covariance and the pooled
    path; a model with one runs on the layer path, and set_exact_relu has no effect on it.
    The map is not homogeneous (the scale of the inputs matters) and K' can be negative."""

    def layers(self):
        return 0


class ABReLU(NNGPKernel):
    """The two-slope ReLU φ(x) = a·min(x, 0) + b·max(x, 0) (no reference counterpart):
    LeakyReLU is (slope, 1), |x| is (−1, 1), a damped identity is (a, a), ReLU is (0, 1).  With
    R the ReLU map and k its κ̇, K' = (a − b)²·R + ab·c, κ̇ = (a − b)²·k + ab, and
    (a² + b²)/2 times the variance where the ReLU overrides (device: ABReluMap).
    Usable wherever Gelu is: forward, ntk, position_covariance, the pooled path and ntk_maps;
    a model with one runs on the layer path, and set_exact_relu applies to it as to ReLU.
    The slopes are plain floats: assigning ``a`` or ``b`` takes effect at the next call.  The
    map is homogeneous of degree 1 and K' can be negative."""

    def __init__(self, a, b):
        super().__init__()
        self.a = float(a)
        self.b = float(b)
        self._check()

    def _check(self):
        a, b = float(self.a), float(self.b)
        if not (math.isfinite(a) and math.isfinite(b)):
            raise ValueError(f"{type(self).__name__}: the slopes must be finite, got ({a}, {b})")
        if a == 0.0 and b == 0.0:
            raise ValueError(f"{type(self).__name__}: both slopes are zero (φ = 0)")
        return a, b

    def constants(self):
        """(s, m, h) = ((a − b)², a·b, (a² + b²)/2) in double: what the kernels take."""
        a, b = self._check()
        return (a - b) * (a - b), a * b, (a * a + b * b) / 2

    def layers(self):
        return 0

    def extra_repr(self):
        return f"a={self.a}, b={self.b}"


class LeakyReLU(ABReLU):
    """φ(x) = max(x, 0) + negative_slope·min(x, 0): ABReLU(negative_slope, 1), with torch's
    default slope."""

    def __init__(self, negative_slope=0.01):
        super().__init__(negative_slope, 1.0)

    @property
    def negative_slope(self):
        return self.a

    @negative_slope.setter
    def negative_slope(self, value):
        self.a = float(value)

    def extra_repr(self):
        return f"negative_slope={self.a}"


class Sin(NNGPKernel):
    """The sinusoid φ(x) = a·sin(b·x + phase) (no reference counterpart): the layer kernel of
    sine networks and of random Fourier features, a function of the distance d = v₁ + v₂ − 2c
    and of s = v₁ + v₂ + 2c,
    K' = A·(exp(−B·d) − C·exp(−B·s)),  κ̇ = D·(exp(−B·d) + C·exp(−B·s)),
    (A, B, C, D) = (a²/2, b²/2, cos(2·phase), a²b²/2), and A·(1 − C·exp(−4B·v)) where the ReLU
    overrides (device: SinMap).  Usable wherever ABReLU is: forward, ntk,
    position_covariance, the pooled path and ntk_maps; a model with one runs on the layer path,
    and set_exact_relu has no effect on it.  ``a``, ``b`` and ``phase`` are plain floats:
    assigning one takes effect at the next call.  |K'| <= a²; the map is not homogeneous."""

    def __init__(self, a=1.0, b=1.0, phase=0.0):
        super().__init__()
        self.a = float(a)
        self.b = float(b)
        self.phase = float(phase)
        self.constants()

    def constants(self):
        """(A, B, C, D) = (a²/2, b²/2, cos(2·phase), a²b²/2) in double: what the kernels take."""
        a, b, phase = float(self.a), float(self.b), float(self.phase)
        name = type(self).__name__
        if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(phase)):
            raise ValueError(f"{name}: a, b and phase must be finite, got ({a}, {b}, {phase})")
        if a == 0.0 or b == 0.0:
            raise ValueError(f"{name}: a and b must not be zero (φ is constant), got ({a}, {b})")
        consts = (a * a / 2, b * b / 2, math.cos(2 * phase), a * a * b * b / 2)
        if not all(math.isfinite(c) and c != 0.0 for c in (consts[0], consts[1], consts[3])):
            raise ValueError(f"{name}: a² or b² leaves the double range, got ({a}, {b})")
        return consts

    def layers(self):
        return 0

    def extra_repr(self):
        return f"a={self.a}, b={self.b}, phase={self.phase}"


class Cos(Sin):
    """φ(x) = a·cos(b·x): Sin(a, b, π/2), bit for bit (cos π is exactly −1)."""

    def __init__(self, a=1.0, b=1.0):
        super().__init__(a, b, math.pi / 2)

    def extra_repr(self):
        return f"a={self.a}, b={self.b}"


class Rbf(Sin):
    """The squared-exponential layer kernel K' = exp(−gamma·(v₁ + v₂ − 2c)), κ̇ = 2·gamma·K',
    variance 1: that of the random Fourier feature φ(x) = √2·sin(√(2·gamma)·x + π/4), with the
    constants set to (1, gamma, 0, 2·gamma) so that C is exactly 0 and the kernel evaluates one
    exponential.  K' lies in (0, 1].  ``gamma`` is a plain float: assigning it takes effect at
    the next call."""

    def __init__(self, gamma=1.0):
        NNGPKernel.__init__(self)
        self.gamma = float(gamma)
        self.constants()

    def constants(self):
        g = float(self.gamma)
        if not (math.isfinite(g) and g > 0.0 and math.isfinite(2 * g)):
            raise ValueError(f"Rbf: gamma must be positive and finite, got {g}")
        return 1.0, g, 0.0, 2 * g

    def extra_repr(self):
        return f"gamma={self.gamma}"


class HermiteNonlin(NNGPKernel):
    """Any smooth φ by its Hermite (Mehler) series (no reference counterpart):
    ``phi`` is one of "tanh", "sigmoid", "softplus", "silu", "gelu_tanh" (GELU's tanh
    approximation), and "erf" and "gelu" (the exact x·Φ(x)), which exist so that this path can
    be checked against Erf() and Gelu().  With ρ = c/√(v₁·v₂) and a_n(v) = E_z[φ(√v·z)·h_n(z)],
    h_n = He_n/√n!,
    K' = Σ_{n<=order} a_n(v₁)·a_n(v₂)·ρⁿ,  κ̇ = the same of φ',  v' = Σ a_n(v)²,
    the coefficients from a Gauss–Hermite rule of ``quad_nodes`` nodes, compressed to |z| <= 12.5
    (program.hermite_rule), per image pixel (device: hermite_coef_kernel, HermiteMap).  The truncated series is symmetric bit for bit and
    positive semi-definite by construction; its error is the dropped tail, largest at |ρ| = 1
    and growing with the variance for a saturating φ (2e-7 of E φ² for tanh at v = 1 and order
    32, 2e-4 at v = 4).  Usable wherever Sin is: forward, ntk, position_covariance, the pooled
    path and ntk_maps; a model with one runs on the layer path, and set_exact_relu has no effect
    on it.  ``phi``, ``order`` and ``quad_nodes`` are plain attributes: assigning one takes
    effect at the next call."""

    def __init__(self, phi, order=32, quad_nodes=96):
        super().__init__()
        self.phi = phi
        self.order = order
        self.quad_nodes = quad_nodes
        self.rule()

    def rule(self):
        """(function id, order, quad_nodes) as the kernels take them, validated."""
        name = type(self).__name__
        phi, order, nq = self.phi, self.order, self.quad_nodes
        if phi not in N.HERMITE_PHI:
            raise ValueError(f"{name}: phi must be one of {sorted(N.HERMITE_PHI)}, got {phi!r}")
        for what, val in (("order", order), ("quad_nodes", nq)):
            if isinstance(val, bool) or not isinstance(val, int):
                raise ValueError(f"{name}: {what} must be an int, got {val!r}")
        if not 1 <= order <= N.CGP_HERMITE_MAX_ORDER:
            raise ValueError(f"{name}: order must be in [1, {N.CGP_HERMITE_MAX_ORDER}], "
                             f"got {order}")
        if not order < nq <= N.CGP_HERMITE_MAX_NODES:
            raise ValueError(f"{name}: quad_nodes must be above order = {order} and at most "
                             f"{N.CGP_HERMITE_MAX_NODES}, got {nq}")
        return N.HERMITE_PHI[phi], order, nq

    def layers(self):
        return 0

    def extra_repr(self):
        return f"phi={self.phi!r}, order={self.order}, quad_nodes={self.quad_nodes}"


class Tanh(HermiteNonlin):
    """φ(x) = tanh x: HermiteNonlin("tanh")."""

    def __init__(self, order=32, quad_nodes=96):
        super().__init__("tanh", order, quad_nodes)

    def extra_repr(self):
        return f"order={self.order}, quad_nodes={self.quad_nodes}"


class Sigmoid(HermiteNonlin):
    """φ(x) = 1/(1 + exp(−x)): HermiteNonlin("sigmoid")."""

    def __init__(self, order=32, quad_nodes=96):
        super().__init__("sigmoid", order, quad_nodes)

    def extra_repr(self):
        return f"order={self.order}, quad_nodes={self.quad_nodes}"


class Softplus(HermiteNonlin):
    """φ(x) = log(1 + exp x): HermiteNonlin("softplus")."""

    def __init__(self, order=32, quad_nodes=96):
        super().__init__("softplus", order, quad_nodes)

    def extra_repr(self):
        return f"order={self.order}, quad_nodes={self.quad_nodes}"


class SiLU(HermiteNonlin):
    """φ(x) = x/(1 + exp(−x)), the swish: HermiteNonlin("silu")."""

    def __init__(self, order=32, quad_nodes=96):
        super().__init__("silu", order, quad_nodes)

    def extra_repr(self):
        return f"order={self.order}, quad_nodes={self.quad_nodes}"


class GeluTanh(HermiteNonlin):
    """φ(x) = x·(1 + tanh(√(2/π)·(x + 0.044715·x³)))/2, GELU's tanh approximation: HermiteNonlin("gelu_tanh")."""

    def __init__(self, order=32, quad_nodes=96):
        super().__init__("gelu_tanh", order, quad_nodes)

    def extra_repr(self):
        return f"order={self.order}, quad_nodes={self.quad_nodes}"


class GlobalAvgPool(NNGPKernel):
    """Global average pooling (no reference counterpart; the head of the CNN-GP and CNTK
    papers' best networks): the 1x1 value mean over p, q of S[p, q], the covariance of pixel p
    of x_i with pixel q of y_j.  Everything upstream of it runs on position-pair maps
    (DESIGN §3.3); only Conv2d layers that keep the value 1x1 and Sum / Mixture may follow."""

    def layers(self):
        return 0


class AvgPool2d(NNGPKernel):
    """Windowed average pooling (no reference counterpart; the 2x2 pools between the blocks
    of the Myrtle and LAP networks), torch.nn.AvgPool2d without padding: the output is
    floor((H - kernel_size)/stride) + 1 per side, ``stride`` defaulting to ``kernel_size``.
    On position-pair maps S'[p, q] is the mean of S over the window of p times the window of
    q; the model runs on them like one with a GlobalAvgPool, which may follow.
    Without one the final value must be 1x1, e.g. through a dense Conv2d(H', padding=0)."""

    def __init__(self, kernel_size, stride=None):
        super().__init__()
        self.kernel_size = kernel_size
        self.stride = kernel_size if stride is None else stride

    def layers(self):
        return 0

    def extra_repr(self):
        return f"kernel_size={self.kernel_size}, stride={self.stride}"


def rbf_corr(k, lengthscale):
    """The k x k float64 matrix exp(-(a - a')²/(2·lengthscale²)) of tap indices a, a': the
    RBF weight correlation of Garriga-Alonso & van der Wilk 2021 along one axis.
    lengthscale 0 gives the identity (independent taps, Conv2d), inf all ones (one shared
    weight, mean pooling)."""
    k, ls = int(k), float(lengthscale)
    if k < 1 or not ls >= 0:
        raise ValueError(f"rbf_corr(k={k}, lengthscale={lengthscale}): k must be at least 1 and "
                         "the lengthscale non-negative")
    d2 = (np.arange(k)[:, None] - np.arange(k)[None, :]).astype(np.float64) ** 2
    if ls == 0:
        return (d2 == 0).astype(np.float64)
    return np.exp(-d2 / (2 * ls * ls))


def band_corr(k, c):
    """The k x k float64 matrix 1(|a - a'| <= c): the local average pooling head of Li et al.
    2019 along one axis (zero padded).  Not positive semi-definite for 0 < c < k - 1."""
    k, c = int(k), int(c)
    if k < 1 or c < 0:
        raise ValueError(f"band_corr(k={k}, c={c}): k must be at least 1 and c non-negative")
    idx = np.arange(k)
    return (np.abs(idx[:, None] - idx[None, :]) <= c).astype(np.float64)


class CorrelatedConv2d(NNGPKernel):
    """A conv or readout whose weights are correlated across the taps of one filter (no
    reference counterpart; Garriga-Alonso & van der Wilk 2021).  With R[δ, δ'] the correlation
    of taps δ and δ',

        S'[p, q] = (var_weight/k²) · Σ_{δ, δ'} R[δ, δ'] · S[p·s + off + δ·d, q·s + off + δ'·d]
                   + var_bias

    on position-pair maps; R = I is Conv2d, R = ones at k = H the GlobalAvgPool
    head, a band at k = H local average pooling.  R is separable: R[(a, b), (a', b')] =
    R_rows[a, a']·R_cols[b, b'], given either as ``weight_corr=(R_rows, R_cols)``, two
    symmetric finite k x k array-likes, or as ``lengthscale``: both are rbf_corr(k,
    lengthscale).  Exactly one of the two is given.  Positive semi-definiteness is not
    checked (band_corr is not PSD); a non-separable R has no path here.  Geometry and padding
    rules are Conv2d's, an even "same" kernel keeps its tap offset, and R indexes the k real
    taps.  The model runs on position-pair maps like one with an AvgPool2d; the scale
    var_weight/k² is taken in double (there is no float32 kernel buffer)."""

    def __init__(self, kernel_size, stride=1, padding="same", dilation=1, var_weight=1.,
                 var_bias=0., weight_corr=None, lengthscale=None):
        super().__init__()
        k = int(kernel_size)
        if k < 1:
            raise ValueError(f"CorrelatedConv2d: kernel_size {kernel_size} must be at least 1")
        if (weight_corr is None) == (lengthscale is None):
            raise ValueError("CorrelatedConv2d: give exactly one of weight_corr=(R_rows, R_cols) "
                             "and lengthscale")
        if lengthscale is not None:
            rows = cols = rbf_corr(k, lengthscale)
            lengthscale = float(lengthscale)
        else:
            try:
                rows, cols = weight_corr
            except (TypeError, ValueError):
                raise ValueError("CorrelatedConv2d: weight_corr must be a pair (R_rows, R_cols) "
                                 "of k x k matrices") from None
        mats = []
        for name, r in (("R_rows", rows), ("R_cols", cols)):
            r = np.array(r, dtype=np.float64)
            if r.shape != (k, k):
                raise ValueError(f"CorrelatedConv2d: {name} has shape {r.shape}, not ({k}, {k})")
            if not np.all(np.isfinite(r)):
                raise ValueError(f"CorrelatedConv2d: {name} has entries that are not finite")
            if not np.array_equal(r, r.T):
                raise ValueError(f"CorrelatedConv2d: {name} is not symmetric")
            mats.append(tuple(tuple(float(v) for v in row) for row in r))
        self.kernel_size = k
        self.stride = stride
        self.dilation = dilation
        self.var_weight = var_weight
        self.var_bias = var_bias
        self.lengthscale = lengthscale
        self.corr_rows, self.corr_cols = mats        # immutable float64 tuples, on the host
        self.kernel_has_row_of_zeros = False
        self._padding_arg = padding
        if padding == "same":
            self.padding = dilation * (k // 2)
            self.kernel_has_row_of_zeros = k % 2 == 0
        else:
            self.padding = padding

    def layers(self):
        return 1

    def extra_repr(self):
        corr = f"lengthscale={self.lengthscale}" if self.lengthscale is not None else \
            "weight_corr=(R_rows, R_cols)"
        return (f"kernel_size={self.kernel_size}, stride={self.stride}, "
                f"padding={self.padding}, dilation={self.dilation}, "
                f"var_weight={self.var_weight}, var_bias={self.var_bias}, {corr}")


class Sequential(NNGPKernel):
    """kernels.py:178-200."""

    def __init__(self, *mods):
        super().__init__()
        self.mods = mods
        for idx, mod in enumerate(mods):
            self.add_module(str(idx), mod)

    def layers(self):
        return sum(mod.layers() for mod in self.mods)


class Mixture(NNGPKernel):
    """kernels.py:203-229 — softmax(logit)-weighted sum of branches."""

    def __init__(self, mods, logit_proportions=None):
        super().__init__()
        self.mods = mods
        for idx, mod in enumerate(mods):
            self.add_module(str(idx), mod)
        if logit_proportions is None:
            logit_proportions = torch.zeros(len(mods))
        self.logit = nn.Parameter(logit_proportions)

    def proportions(self):
        """softmax of the logits in their own dtype (kernels.py:221), as floats."""
        with torch.no_grad():
            lg = self.logit.detach().cpu()
            return [float(v) for v in torch.softmax(lg, dim=0)]

    def layers(self):
        return max(mod.layers() for mod in self.mods)


class Sum(NNGPKernel):
    """kernels.py:246-260 — elementwise sum of the branches' outputs."""

    def __init__(self, mods):
        super().__init__()
        self.mods = mods
        for idx, mod in enumerate(mods):
            self.add_module(str(idx), mod)

    def layers(self):
        return max(mod.layers() for mod in self.mods)


def resnet_block(stride=1, projection_shortcut=False, multiplier=1):
    """kernels.py:274-296."""
    if stride == 1 and not projection_shortcut:
        return Sum([
            Sequential(),
            Sequential(
                ReLU(),
                Conv2d(3, stride=stride, in_channel_multiplier=multiplier,
                       out_channel_multiplier=multiplier),
                ReLU(),
                Conv2d(3, in_channel_multiplier=multiplier, out_channel_multiplier=multiplier),
            )
        ])
    return Sequential(
        ReLU(),
        Sum([
            Conv2d(1, stride=stride, in_channel_multiplier=multiplier // stride,
                   out_channel_multiplier=multiplier),
            Sequential(
                Conv2d(3, stride=stride, in_channel_multiplier=multiplier // stride,
                       out_channel_multiplier=multiplier),
                ReLU(),
                Conv2d(3, in_channel_multiplier=multiplier, out_channel_multiplier=multiplier),
            )
        ]),
    )

