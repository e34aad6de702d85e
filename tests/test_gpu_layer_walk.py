"""GPU tests of the layer path where a workgroup walks many chunks.

Both conv kernels of csrc/cnngp.hip are persistent: min(chunks, resident workgroups)
workgroups each walk chunks blockIdx, blockIdx + grid, ...  What is delicate in them only
runs from a workgroup's second chunk on: conv_geo_kernel's two LDS-DMA input buffers, the
hand-counted s_waitcnt that covers them, the refill of the buffer stage 1 just consumed,
the re-fetch past the end and the ragged last chunk; conv_cov_kernel's register prefetch
across the barriers, its halo zeroed once, and its direct staging of chunks above 2048
elements.  A small launch has a chunk per workgroup and reaches none of it, so these tests
cap the grid (cgp_conv_args.max_groups) or launch enough maps to outnumber the real grid,
and assert from cgp_conv_plan_* that the walk they mean to test is the walk they get.

  a. every compiled geometry x type x fusion, 3 workgroups walking 6, 6 and 5 chunks
  b. the generic kernel on the shapes and fusions the compiled one declines
  c. the uncapped grid with 5 chunks and more per workgroup
  d. whole models on a 104 x 100 tile against 8-row strips of it
  e. the grid-stride elementwise kernels past grid_for's 8192-block cap

Tolerances are the project's own: a conv alone in float64 1e-13 relative
(test_conv_golden_cases), fusions with a ReLU 1e-12 (test_fused_geometries), float32
against the float64 oracle 2e-5, elementwise kernels 1e-14 / 1e-6.  A map's arithmetic does
not depend on which workgroup walks it or when, so every comparison between two walks of the
same maps is bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from oracle import nngp_oracle as O
from oracle import specs

import configs_util
import conv_walk_util as U
import erf_oracle as EO
import ntk_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
CONV_TOL = {"f64": 1e-13, "f32": 2e-5}      # no ReLU in the launch
RELU_TOL = {"f64": 1e-12, "f32": 2e-5}      # a fused ReLU
ELEM_TOL = {"f64": 1e-14, "f32": 1e-6}
RTOL64_FAST = 1e-8                          # test_gpu_parity.RTOL64["fast"], test_gpu_ntk
ERF_NET_TOL = 1e-10                         # test_gpu_erf.NET_TOL["f64"]
SENTINEL = -12345.0
FORMS = {"pairs": (0, 0), "diag": (0, 1), "same": (1, 0), "samediag": (1, 1)}


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dt)


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert np.all(np.isfinite(got)), "NaN or inf in the output: a map was not written"
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))


def f32r(a):
    """float64 values that float32 holds exactly"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ------------------------------------------------------------------------------------
# one launch
# ------------------------------------------------------------------------------------
def fire(dtn, geo, counts, mode, bufs, out, same=0, diag=0, channels=0, mpb=0, flags=0,
         max_groups=0):
    """cgp_conv_<dtn> on device tensors: bufs name -> tensor for what `mode` reads, out the
    tensor it writes (exactly nmaps maps of it)."""
    nmaps, n1, n2 = counts
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    ptrs["out"] = out.data_ptr()
    a = U.conv_args(geo, nmaps, n1, n2, mode, same=same, diag=diag, mpb=mpb, flags=flags,
                    max_groups=max_groups, channels=channels, ptrs=ptrs)
    N.check(getattr(N.load(), f"cgp_conv_{dtn}")(ctypes.byref(a), stream()), "cgp_conv")


def guarded_out(dtn, geo, nmaps):
    """[nmaps + 1] output maps: NaN where the launch must write, one sentinel map behind"""
    out = torch.full((nmaps + 1, geo["ho"], geo["wo"]), float("nan"), dtype=TORCH_DT[dtn],
                     device=DEV)
    out[nmaps] = SENTINEL
    return out


def with_nan_map(a, dt):
    """the input maps on the device with one NaN map behind them: a read past the last map
    that reached an output would show there"""
    a = np.asarray(a, np.float64)
    return dev(np.concatenate([a, np.full((1,) + a.shape[1:], np.nan)]), dt)


class Case:
    """Random images and everything derived from them for one (shape, conv, pair form): the
    float64 oracle's result of every fusion mode and the arrays each mode's launch reads.
    Images are float32-representable and in [0, 1); pair and variance maps fed to a launch
    as maps are rounded to float32 first, so both types read exactly what the oracle read."""

    def __init__(self, h, w, spec, form, counts, channels, seed, apart=False):
        self.geo, self.spec, self.form, self.counts = U.geometry(h, w, spec), spec, form, counts
        self.same, self.diag = FORMS[form]
        self.channels = channels
        nmaps, n1, n2 = counts
        rng = np.random.default_rng(seed)
        # apart: x in [0, 0.4), y in [0.6, 1), for one-channel images under a ReLU (below)
        lo, scale = (np.float32(0.6), np.float32(0.4)) if apart else (np.float32(0), np.float32(1))
        assert not (apart and self.same)
        self.X = (scale * rng.random((n1, channels, h, w), dtype=np.float32)).astype(np.float64)
        self.Y = self.X if self.same else \
            (lo + scale * rng.random((n2, channels, h, w), dtype=np.float32)).astype(np.float64)
        self.kp = O.moments(self.X, self.Y, bool(self.same), bool(self.diag))
        assert self.kp["xy"].shape[0] == nmaps
        self.kpm = O.make_kp(self.same, self.diag, f32r(self.kp["xy"]), f32r(self.kp["xx"]),
                             f32r(self.kp["yy"]))
        g = self.geo
        self.addend = rng.random((nmaps, g["ho"], g["wo"]), dtype=np.float32).astype(np.float64)

    @functools.lru_cache(maxsize=None)
    def mode(self, mode):
        """(reference output, host arrays the launch reads, whether a ReLU is fused)"""
        pre, post, add = U.MODES[mode]
        spec = self.spec
        bufs = {}
        if pre == N.CGP_PRE_MOMENTS:
            kp = self.kp
            bufs["in_"], bufs["in_y"] = self.X, self.Y
        elif pre == N.CGP_PRE_RELU:
            kp = O.relu(self.kpm)
            bufs["in_"] = self.kpm["xy"]
            bufs["pre_xx"], bufs["pre_yy"] = self.kpm["xx"], self.kpm["yy"]
        else:
            kp = self.kpm
            bufs["in_"] = self.kpm["xy"]
        c = O._conv_kp(kp, spec, "f32")
        ref = c["xy"]
        if post:
            ref = O.relu(c)["xy"]
            bufs["post_xx"], bufs["post_yy"] = c["xx"], c["yy"]
        if add:
            ref = ref + self.addend
            bufs["addend"] = self.addend
        return ref, bufs, bool(pre == N.CGP_PRE_RELU or post)

    def device_bufs(self, mode, dtn):
        dt = TORCH_DT[dtn]
        _, bufs, _ = self.mode(mode)
        maps_in = U.MODES[mode][0] != N.CGP_PRE_MOMENTS
        return {k: with_nan_map(v, dt) if k == "in_" and maps_in else dev(v, dt)
                for k, v in bufs.items()}


def check_walks(case, mode, dtn, expect_kernel, mpb=0, flags=0):
    """One fusion mode of one case under max_groups = CAP, 0 and 1: the plan's walk
    conditions, the capped result against the oracle, the guard map, and the three walks
    bit for bit.  Returns the capped run's error."""
    geo, counts = case.geo, case.counts
    nmaps = counts[0]
    kw = dict(same=case.same, diag=case.diag, channels=case.channels, mpb=mpb, flags=flags)
    p = U.plan(U.conv_args(geo, *counts, mode, max_groups=U.CAP, **kw), dtn)
    kernel, mpc, chunks, groups = p
    what = (case.form, mode, dtn, p)
    assert kernel == expect_kernel, what
    assert groups == U.CAP and chunks >= 17, what
    assert chunks % U.CAP == U.walk_remainder(mpc, case.form), what
    assert mpc == 1 or nmaps % mpc != 0, what
    assert mpc * (chunks - 1) < nmaps <= mpc * chunks, what
    free = U.plan(U.conv_args(geo, *counts, mode, max_groups=0, **kw), dtn)
    assert free[:3] == p[:3] and free[3] == chunks, (what, free)   # a chunk per workgroup
    ref, _, relu = case.mode(mode)
    bufs = case.device_bufs(mode, dtn)
    outs = {}
    for cap in (U.CAP, 0, 1):
        out = guarded_out(dtn, geo, nmaps)
        fire(dtn, geo, counts, mode, bufs, out[:nmaps], max_groups=cap, **kw)
        torch.cuda.synchronize()
        outs[cap] = out.cpu()
        assert torch.all(outs[cap][nmaps] == SENTINEL), (what, cap, "guard map written")
    err = rel_err(outs[U.CAP][:nmaps].numpy(), ref)
    assert err < (RELU_TOL if relu else CONV_TOL)[dtn], (what, err)
    for cap in (0, 1):
        assert torch.equal(bits(outs[cap]), bits(outs[U.CAP])), \
            (what, f"max_groups {cap} and {U.CAP} differ")
    return err


# ------------------------------------------------------------------------------------
# a. the compiled geometries
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("geom", U.GEOS, ids=lambda c: "-".join(map(str, c)))
def test_compiled_geometry_walk(geom, dtn):
    """Every fusion launch_geo_mode compiles, in each pair form, with 3 workgroups walking
    6, 6 and 5 chunks (prologue buffers, refilled buffers, the re-fetch past the end, the
    ragged tail) against the oracle and against the walks of 17+ and of 1 workgroup.

    Every mode runs on 3-channel images.  The modes that read images run on 1-channel
    images as well; there a pixel's moments are (x·y, x², y²), correlation exactly 1, and a
    1x1 conv leaves 1 - rho = (x - y)²/2v² + ..., where the oracle's acos(rho) loses half
    its digits and 1e-12 would measure the oracle.  So the 1-channel images
    under a ReLU are drawn apart (x < 0.4, y >= 0.6: 1 - rho > 3e-3), and a same tile or
    same diag list, whose two sides are one image set, runs its 1-channel images through the
    five 1x1 geometries without the ReLU (a wider window mixes pixels and needs neither)."""
    side, k, stride = geom
    spec = U.conv_spec(k, stride)
    mpc = U.plan(U.conv_args(U.geometry(side, side, spec), 1, 1, 1), dtn)[1]
    worst = {}
    for form in FORMS:
        counts = U.walk_counts(mpc, "diag" if form == "samediag" else form)
        same = FORMS[form][0]
        seed = side * 100 + k
        runs = [(Case(side, side, spec, form, counts, 3, seed), list(U.GEO_MODES)),
                (Case(side, side, spec, form, counts, 1, seed, apart=not same),
                 ["moments"] if same and k == 1 else ["moments", "moments_post"])]
        for case, modes in runs:
            for mode in modes:
                err = check_walks(case, mode, dtn, expect_kernel=1)
                worst[mode] = max(worst.get(mode, 0.0), err)
    print(f"geo walk {geom} {dtn} mpc={mpc}: "
          + " ".join(f"{m}={e:.1e}" for m, e in worst.items()))


# ------------------------------------------------------------------------------------
# b. the generic kernel
# ------------------------------------------------------------------------------------
EXACT, GENERIC = N.CGP_FLAG_EXACT_RELU, N.CGP_FLAG_GENERIC_CONV
# name -> (h, w, spec, maps_per_block, flags every launch carries)
GENERIC_SHAPES = {
    "12x12_k5": (12, 12, U.conv_spec(5), 0, 0),
    "9x9_k4_even": (9, 9, U.conv_spec(4), 0, 0),                 # offset = -pad + dilation
    "10x6_k3": (10, 6, U.conv_spec(3), 0, 0),                    # h != w
    "7x7_k3_dil2": (7, 7, U.conv_spec(3, dilation=2), 0, 0),
    "7x7_k7_pad0": (7, 7, U.conv_spec(7, padding=0), 0, 0),      # 1x1 output
    "14to7_s2_forced": (14, 14, U.conv_spec(3, stride=2), 0, GENERIC),
    "12x12_k3_mpb20": (12, 12, U.conv_spec(3), 20, 0),           # 2880-element chunks
    "48x48_k3": (48, 48, U.conv_spec(3), 1, 0),                  # one map above 2048 pixels
    "11x11_k6": (11, 11, U.conv_spec(6), 0, 0),                  # TAPS == 0: runtime tap loop
}
# (mode, extra flags): the fusions of launch_geo_mode's switch the generic kernel also runs,
# the two it alone runs, and the op-by-op ReLU
GENERIC_MODES = [("none", 0), ("post_add", 0), ("prerelu", 0), ("prerelu_post_add", 0),
                 ("prerelu_post", EXACT), ("prerelu", EXACT), ("moments_post", 0),
                 ("moments", EXACT)]


@pytest.mark.parametrize("dtn", ["f64", "f32"])
@pytest.mark.parametrize("name", list(GENERIC_SHAPES))
def test_generic_kernel_walk(name, dtn):
    """conv_cov_kernel with 3 workgroups walking 6, 6 and 5 chunks: the register prefetch
    across the barriers, the halo that is zeroed once and must stay zero under every later
    chunk's interior writes, the direct staging loop of chunks above 2048 elements, the
    ragged last chunk."""
    h, w, spec, mpb, flags = GENERIC_SHAPES[name]
    geo = U.geometry(h, w, spec)
    mpc = U.plan(U.conv_args(geo, 1, 1, 1, mpb=mpb, flags=flags), dtn)[1]
    if name == "12x12_k3_mpb20":
        assert mpc == 20 and mpc * h * w > 2048
    if name == "48x48_k3":
        assert mpc == 1 and h * w > 2048
    if name == "7x7_k7_pad0":
        assert (geo["ho"], geo["wo"]) == (1, 1)
    if name == "9x9_k4_even":
        assert geo["offset"] == -2 + 1
    worst = {}
    for form in FORMS:
        counts = U.walk_counts(mpc, "diag" if form == "samediag" else form)
        case = Case(h, w, spec, form, counts, 3, seed=h * 100 + w)
        for mode, extra in GENERIC_MODES:
            err = check_walks(case, mode, dtn, expect_kernel=0, mpb=mpb, flags=flags | extra)
            key = mode + ("_exact" if extra else "")
            worst[key] = max(worst.get(key, 0.0), err)
    print(f"generic walk {name} {dtn} mpc={mpc}: "
          + " ".join(f"{m}={e:.1e}" for m, e in worst.items()))


# ------------------------------------------------------------------------------------
# c. the real grid
# ------------------------------------------------------------------------------------
REAL_GRID = {
    "geo_28_k3_f64": (28, U.conv_spec(3), "f64", 0, 1),
    "geo_7_k3_f32": (7, U.conv_spec(3), "f32", 0, 1),
    "generic_12_k5_f64": (12, U.conv_spec(5), "f64", 0, 0),
}


@pytest.mark.parametrize("name", list(REAL_GRID))
def test_real_grid_walk(name):
    """max_groups = 0, a diag list of maps_per_chunk·(5·groups + 1) + 1 maps: every resident
    workgroup walks 5 or 6 chunks and the last chunk holds one map.  POST + ADD.  Bit for bit
    against the same maps launched in slices of one chunk per workgroup; 64 sampled maps
    against the oracle."""
    side, spec, dtn, flags, kernel = REAL_GRID[name]
    dt = TORCH_DT[dtn]
    geo = U.geometry(side, side, spec)
    mode = "post_add"
    big = 1 << 22
    _, mpc, _, groups = U.plan(U.conv_args(geo, big, big, big, mode, diag=1, flags=flags), dtn)
    nmaps = mpc * (5 * groups + 1) + 1
    counts = (nmaps, nmaps, nmaps)
    p = U.plan(U.conv_args(geo, *counts, mode, diag=1, flags=flags), dtn)
    assert p == [kernel, mpc, 5 * groups + 2, groups], p
    assert p[2] >= 5 * p[3] and nmaps - mpc * (p[2] - 1) == 1     # one map in the last chunk

    gen = torch.Generator(device=DEV).manual_seed(side)

    def rand(*shape, lo=0.0):
        return (lo + torch.rand(shape, dtype=torch.float32, device=DEV, generator=gen)).to(dt)

    # inputs in [0, 1): the conv output is at most var_weight + var_bias = 2.5, and variances
    # in [3, 4) keep every correlation inside (0.1, 0.84)
    assert spec["var_weight"] + spec["var_bias"] <= 2.5
    hw = (side, side)
    bufs = {"in_": torch.cat([rand(nmaps, *hw), torch.full((1, *hw), float("nan"), dtype=dt,
                                                           device=DEV)]),
            "addend": rand(nmaps, *hw), "post_xx": rand(nmaps, *hw, lo=3.0),
            "post_yy": rand(nmaps, *hw, lo=3.0)}
    out = guarded_out(dtn, geo, nmaps)
    fire(dtn, geo, counts, mode, bufs, out[:nmaps], diag=1, flags=flags)
    sliced = guarded_out(dtn, geo, nmaps)
    step = groups * mpc
    for m0 in range(0, nmaps, step):
        m1 = min(m0 + step, nmaps)
        part = (m1 - m0,) * 3
        q = U.plan(U.conv_args(geo, *part, mode, diag=1, flags=flags), dtn)
        assert q[2] == q[3] and q[:2] == p[:2], q          # one chunk per workgroup
        fire(dtn, geo, part, mode, {k: v[m0:m1] for k, v in bufs.items()}, sliced[m0:m1],
             diag=1, flags=flags)
    torch.cuda.synchronize()
    assert torch.all(out[nmaps] == SENTINEL) and torch.all(sliced[nmaps] == SENTINEL)
    assert bool(torch.isfinite(out[:nmaps]).all())
    assert torch.equal(bits(out), bits(sliced))

    rng = np.random.default_rng(1)
    pick = np.unique(np.concatenate([rng.integers(0, nmaps, 61), [0, nmaps - 2, nmaps - 1]]))
    idx = torch.as_tensor(pick, device=DEV)
    host = {k: v[idx].cpu().numpy().astype(np.float64) for k, v in bufs.items()}
    c = O.make_kp(False, True, O.conv_maps(host["in_"], spec), host["post_xx"], host["post_yy"])
    ref = O.relu(c)["xy"] + host["addend"]
    err = rel_err(out[idx].cpu().numpy(), ref)
    print(f"real grid {name}: {nmaps} maps, mpc={mpc}, {p[2]} chunks on {groups} workgroups, "
          f"{len(pick)} sampled maps err={err:.1e}")
    assert err < RELU_TOL[dtn]


# ------------------------------------------------------------------------------------
# d. through a model
# ------------------------------------------------------------------------------------
TILE = (104, 100)


@functools.lru_cache(maxsize=None)
def tile_images():
    rng = np.random.default_rng(2024)
    X = rng.random((TILE[0], 1, 28, 28), dtype=np.float32).astype(np.float64)
    Z = rng.random((TILE[1], 1, 28, 28), dtype=np.float32).astype(np.float64)
    ii = rng.integers(0, TILE[0], 16)
    jj = rng.integers(0, TILE[1], 16)
    ii[0], jj[0], ii[1], jj[1] = 0, 0, TILE[0] - 1, TILE[1] - 1
    return X, Z, ii, jj


def erf_net():
    """the 3-conv erf network of test_gpu_erf.py (convnet_bias) at 28x28"""
    C, E = cnn_gp.Conv2d, cnn_gp.Erf
    return cnn_gp.Sequential(C(3, var_bias=0.2), E(), C(3, var_weight=1.5, var_bias=0.1), E(),
                             C(3), E(), C(28, padding=0, var_bias=0.1))


def first_conv_plan(model, ntk):
    """cgp_conv_plan_f64 of the model's first 28x28 conv launch on the whole tile: the fused
    op of the forward program, or the bare conv the NTK run launches in its place"""
    plan = model._plan(28, 28)
    op = next(o for o in plan.pair_ops if o.kind == "conv")
    assert tuple(op.shape_in) == (28, 28)
    g = op.geom
    geo = dict(h=28, w=28, ho=op.shape_out[0], wo=op.shape_out[1], taps=g.taps,
               offset=g.offset, stride=g.stride, dilation=g.dilation, weight=g.weight,
               bias=g.bias)
    mode = "none" if ntk else \
        next(m for m, v in U.MODES.items()
             if v == (op.pre, op.post, int(op.addend is not None)))
    n1, n2 = TILE
    return U.plan(U.conv_args(geo, n1 * n2, n1, n2, mode, channels=1, flags=plan.flags), "f64")


def assert_tile_walks(model, ntk):
    kernel, mpc, chunks, groups = first_conv_plan(model, ntk)
    assert kernel == 1 and chunks >= 5 * groups, (kernel, mpc, chunks, groups)
    return chunks, groups


def strips(fn, X, Z):
    """fn(X[a:a + 8], Z) for every 8-row strip, stacked: [(104, 100), ...]"""
    parts = [fn(X[a:a + 8], Z) for a in range(0, X.shape[0], 8)]
    return [torch.cat([p[k] for p in parts]) for k in range(len(parts[0]))]


def sampled(t, ii, jj):
    return t[torch.as_tensor(ii, device=DEV), torch.as_tensor(jj, device=DEV)].cpu().numpy()


def test_model_tile_nngp():
    """mnist_as_tf's layer path on a 104 x 100 tile: bit-equal to its 8-row strips, 16
    entries against the oracle"""
    Xh, Zh, ii, jj = tile_images()
    model = configs_util.model("mnist_as_tf").double().to(DEV).set_fused_network(False)
    chunks, groups = assert_tile_walks(model, ntk=False)
    X, Z = dev(Xh, torch.float64), dev(Zh, torch.float64)
    with torch.no_grad():
        k = model(X, Z, False, False)
        (ks,) = strips(lambda x, z: (model(x, z, False, False),), X, Z)
    assert tuple(k.shape) == TILE and torch.equal(bits(k), bits(ks))
    ref = O.kernel(specs.mnist_as_tf(), Xh[ii], Zh[jj], False, True)
    err = rel_err(sampled(k, ii, jj), ref)
    print(f"model tile nngp: first conv {chunks} chunks on {groups} workgroups, err={err:.1e}")
    assert err < RTOL64_FAST


def test_model_tile_ntk():
    """K and Θ of model.ntk on the same tile"""
    Xh, Zh, ii, jj = tile_images()
    model = configs_util.model("mnist_as_tf").double().to(DEV).set_fused_network(False)
    chunks, groups = assert_tile_walks(model, ntk=True)
    X, Z = dev(Xh, torch.float64), dev(Zh, torch.float64)
    with torch.no_grad():
        k, th = model.ntk(X, Z, False, False, return_nngp=True)
        ks, ths = strips(lambda x, z: model.ntk(x, z, False, False, return_nngp=True), X, Z)
    assert tuple(k.shape) == tuple(th.shape) == TILE
    assert torch.equal(bits(k), bits(ks)) and torch.equal(bits(th), bits(ths))
    rk, rth = ntk_oracle.ntk(specs.mnist_as_tf(), Xh[ii], Zh[jj], False, True)
    errs = rel_err(sampled(k, ii, jj), rk), rel_err(sampled(th, ii, jj), rth)
    print(f"model tile ntk: first conv {chunks} chunks on {groups} workgroups, "
          f"K err={errs[0]:.1e} T err={errs[1]:.1e}")
    assert max(errs) < RTOL64_FAST


def test_model_tile_erf():
    """a 3-conv erf network (layer path only; its 28-tap head runs the generic kernel's
    runtime tap loop): forward and ntk on the same tile"""
    Xh, Zh, ii, jj = tile_images()
    model = erf_net().double().to(DEV)
    chunks, groups = assert_tile_walks(model, ntk=False)
    assert_tile_walks(model, ntk=True)
    X, Z = dev(Xh, torch.float64), dev(Zh, torch.float64)
    with torch.no_grad():
        fwd = model(X, Z, False, False)
        k, th = model.ntk(X, Z, False, False, return_nngp=True)
        (fs,) = strips(lambda x, z: (model(x, z, False, False),), X, Z)
        ks, ths = strips(lambda x, z: model.ntk(x, z, False, False, return_nngp=True), X, Z)
    assert tuple(fwd.shape) == TILE
    assert torch.equal(bits(fwd), bits(fs))
    assert torch.equal(bits(k), bits(ks)) and torch.equal(bits(th), bits(ths))
    cpu = erf_net().double()
    rk, rth = EO.ntk_autograd(cpu, Xh[ii], Zh[jj], diag=True)
    errs = (rel_err(sampled(fwd, ii, jj), rk), rel_err(sampled(k, ii, jj), rk),
            rel_err(sampled(th, ii, jj), rth))
    print(f"model tile erf: first conv {chunks} chunks on {groups} workgroups, "
          f"forward err={errs[0]:.1e} K err={errs[1]:.1e} T err={errs[2]:.1e}")
    assert max(errs) < ERF_NET_TOL


# ------------------------------------------------------------------------------------
# e. grid-stride elementwise kernels past grid_for's cap
# ------------------------------------------------------------------------------------
NELEM = 2 * 8192 * 256 + 77       # two full grid strides of 8192 blocks x 256 threads, + 77


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_axpby_past_the_grid_cap(dtn):
    dt = TORCH_DT[dtn]
    rng = np.random.default_rng(3)
    a = rng.random(NELEM, dtype=np.float32).astype(np.float64) + 0.5
    b = rng.random(NELEM, dtype=np.float32).astype(np.float64) + 0.5
    alpha, beta = 1.5, 0.75
    da, db = dev(a, dt), dev(b, dt)

    def run(x, y, out, be):
        guard = torch.full((NELEM + 64,), SENTINEL, dtype=dt, device=DEV)
        if out is None:
            out = guard[:NELEM]
            out.fill_(float("nan"))
        N.call(f"cgp_axpby_{dtn}", alpha, N.ptr(x), be, N.ptr(y), N.ptr(out), NELEM, stream())
        torch.cuda.synchronize()
        assert torch.all(guard[NELEM:] == SENTINEL)
        return out.cpu().numpy()

    errs = {"ab": rel_err(run(da, db, None, beta), alpha * a + beta * b),
            "b_null": rel_err(run(da, None, None, beta), alpha * a)}
    x = da.clone()
    errs["in_place"] = rel_err(run(x, db, x, beta), alpha * a + beta * b)
    x = da.clone()
    errs["in_place_b_null"] = rel_err(run(x, None, x, beta), alpha * a)
    print(f"axpby {dtn} n={NELEM}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < ELEM_TOL[dtn], errs


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_moments_past_the_grid_cap(dtn):
    """cgp_moments_xy_* (diag and not) and cgp_moments_var_* writing more than NELEM
    elements, against numpy"""
    dt = TORCH_DT[dtn]
    rng = np.random.default_rng(4)
    hw, c = 77, 3
    errs = {}

    def images(n):
        return rng.random((n, c, hw), dtype=np.float32).astype(np.float64)

    def guarded(n):
        buf = torch.full((n + 64,), SENTINEL, dtype=dt, device=DEV)
        buf[:n] = float("nan")
        return buf

    for diag, n1, n2 in [(0, 241, 227), (1, 54473, 54473)]:
        x, y = images(n1), images(n2)
        nout = (n1 if diag else n1 * n2) * hw
        assert nout > NELEM
        buf = guarded(nout)
        dx, dy = dev(x, dt), dev(y, dt)
        N.call(f"cgp_moments_xy_{dtn}", N.ptr(dx), N.ptr(dy), n1, n2, c, hw, diag, N.ptr(buf),
               stream())
        torch.cuda.synchronize()
        assert torch.all(buf[nout:] == SENTINEL)
        ref = (x * y).sum(1) / c if diag else (x[:, None] * y[None]).sum(2) / c
        errs["xy_diag" if diag else "xy"] = rel_err(buf[:nout].cpu().numpy(), ref.reshape(-1))
    n1, n2 = 30011, 24473
    assert (n1 + n2) * hw > NELEM
    x, y = images(n1), images(n2)
    bx, by = guarded(n1 * hw), guarded(n2 * hw)
    dx, dy = dev(x, dt), dev(y, dt)
    N.call(f"cgp_moments_var_{dtn}", N.ptr(dx), N.ptr(dy), n1, n2, c, hw, N.ptr(bx), N.ptr(by),
           stream())
    torch.cuda.synchronize()
    assert torch.all(bx[n1 * hw:] == SENTINEL) and torch.all(by[n2 * hw:] == SENTINEL)
    errs["xx"] = rel_err(bx[:n1 * hw].cpu().numpy(), ((x * x).sum(1) / c).reshape(-1))
    errs["yy"] = rel_err(by[:n2 * hw].cpu().numpy(), ((y * y).sum(1) / c).reshape(-1))
    print(f"moments {dtn}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < ELEM_TOL[dtn], errs
