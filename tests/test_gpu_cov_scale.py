"""GPU tests of the position-pair kernels at the size they run by default: launches of more
than 2^31 and 2^32 elements (DESIGN §3.3-3.7, §5 "Position-pair maps at their production
size").

Plan.run_cov_steps sizes a chunk of pairs from the free device memory, so one launch of a
28x28 network carries thousands of pairs of 614 656 elements; every other test of this path
launches about 10^6.  Here every cgp_cov_* / cgp_covmap_* / cgp_corrconv_* / cgp_gelu_cov_* /
cgp_covntk_* entry point and cgp_axpby_* run on the pair list of an 84x84 tile of 28x28 images:

    float32   7 056 pairs, 4 337 012 736 elements (17.35 GB): past 2^32
    float64   3 528 pairs (the same bytes), 2 168 506 368 elements: past 2^31

and cgp_cov_nonlin_* once more on 4 225 pairs of 33x31 maps (h != w, (h·w)² odd).  Every test
asserts its element counts against 1 << 31 and 1 << 32 from its shapes.

Checks of every case (``check``): the outputs are NaN-filled before the launch and finite after
it; the whole buffer equals, bit for bit and on the device, the same entry point run on
consecutive pieces of 1 001 pairs (below 2^31 elements; a piece boundary falls inside a
2048-element chunk of the whole launch: DESIGN §3.3, "the chunking changes no bit"); and the
pairs around both boundaries, the first self pair behind each and the last pair are compared
with the float64 numpy oracles of the small tests, which start from that pair's inputs copied
to the host.  The input maps are produced on the device by cgp_cov_moments_* (itself the first
case), so an in-place case regenerates a piece's inputs instead of keeping a second copy.

The float64 list is the second half of the square, pairs (42, 0) .. (83, 83): a list of 3 528
pairs has no pair 3 570, and the first half has no self pair behind 2^31; in this half the last
pair, 3 527, is the self pair (83, 83).

Then forward and ntk_maps of pooled networks with the whole tile as one chunk against the same
call in chunks of a few hundred pairs, bit for bit, and against the oracles.

Tolerances are the project's own (tests/test_gpu_pool.py): the op alone 1e-12 in float64 and
2e-5 in float32, end to end 1e-10 and 2e-5, errors as max|got - ref| / max|ref|.

No test holds more than three buffers of 17.35 GB plus the pieces' scratch; a test that finds
less free memory than it needs plus 10 % skips with both figures."""
import numpy as np
import pytest
import torch

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import program as P

import avgpool_oracle as AO
import corrconv_oracle as CO
import gelu_oracle as GO
import pool_ntk_oracle as NO
import pool_oracle as PO

pytestmark = pytest.mark.gpu

DEV = "cuda"
OP_TOL = {"f64": 1e-12, "f32": 2e-5}
NET_TOL = {"f64": 1e-10, "f32": 2e-5}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}
NP_DT = {"f64": np.float64, "f32": np.float32}
B31, B32 = 1 << 31, 1 << 32
PIECE = 1001           # pairs of one piece: odd, so its end is no multiple of 2048 elements
DTYPES = ["f64", "f32"]

m = cnn_gp
C, R, S, G, A, CC = m.Conv2d, m.ReLU, m.Sequential, m.GlobalAvgPool, m.AvgPool2d, \
    m.CorrelatedConv2d
KINDS = {"relu": N.CGP_COV_RELU, "erf": N.CGP_COV_ERF, "gelu": N.CGP_COV_GELU}


def stream():
    return torch.cuda.current_stream().cuda_stream


def max_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module", autouse=True)
def release_memory():
    torch.cuda.reset_peak_memory_stats()
    yield
    print(f"\npeak device memory of this file: {torch.cuda.max_memory_allocated()} bytes in "
          f"tensors, {torch.cuda.max_memory_reserved()} reserved")
    WORLDS.clear()
    torch.cuda.empty_cache()


def require(nbytes):
    """skips unless the device has ``nbytes`` plus 10 % free (the card is shared)"""
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < nbytes * 1.1:
        pytest.skip(f"needs {nbytes} bytes of device memory plus 10 %, {free} are free")


def finite(t):
    """torch.isfinite(t).all() of a [pairs, elements] tensor, a piece of pairs at a time: on the
    whole of a 17 GB tensor its temporaries are another 26 GB"""
    step = max(1, (1 << 29) // t.shape[1])
    return all(bool(torch.isfinite(t[a:a + step]).all()) for a in range(0, t.shape[0], step))


def sample_pairs(i, j, elems):
    """pair 0, the pairs before, at and after the elements 2^31 and 2^32 of a list of maps of
    ``elems`` elements, the first self pair (i == j) behind each, and the last pair"""
    n = len(i)
    out = {0, n - 1}
    for bound in (B31, B32):
        at = bound // elems                            # the pair that holds element `bound`
        if at + 1 < n:
            assert at * elems < bound < (at + 1) * elems
            out |= {at - 1, at, at + 1}
            out.add(next(k for k in range(at + 2, n) if i[k] == j[k]))
    return sorted(out)


class World:
    """the images, their variance maps and the pair list of one (h, w, dtype): ``nimg`` +
    ``nimg`` small random float32-representable images of 4 channels (test_gpu_pool.op_inputs
    has why four) and the pairs [first:] of the full square of x with itself, run with ``same``"""

    def __init__(self, h, w, nimg, dtn, first=0):
        self.h, self.w, self.dtn, self.dt = h, w, dtn, TORCH_DT[dtn]
        self.elems = (h * w) ** 2
        rng = np.random.default_rng(1000 * h + w)
        draw = lambda: rng.random((nimg, 4, h, w), dtype=np.float32).astype(np.float64)  # noqa
        self.x, self.y = draw(), draw()
        i, j = PO.pair_lists(nimg, nimg, False, False)
        self.i, self.j = i[first:], j[first:]
        self.n = len(self.i)
        self.samples = sample_pairs(self.i, self.j, self.elems)
        self.vx = self.rnd(PO.variances(self.x))
        self.xd, self.yd, self.vxd = self.dev(self.x), self.dev(self.y), self.dev(self.vx)
        self.pi = torch.as_tensor(self.i).to(DEV, torch.int32)
        self.pj = torch.as_tensor(self.j).to(DEV, torch.int32)
        self.item = self.xd.element_size()

    def rnd(self, a):
        return np.asarray(a).astype(NP_DT[self.dtn]).astype(np.float64)

    def dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a)).to(DEV, self.dt)

    def crosses(self):
        """asserts from the shapes that one map per pair passes 2^32 elements in float32 and
        2^31 in float64"""
        assert self.n * self.elems > (B32 if self.dtn == "f32" else B31), (self.n, self.elems)

    def gen(self, name, pi, pj, n, out):
        """fills out[:n] with a map per pair, on the device: "k" the moments of (x_i, x_j), what
        the nonlinearities read with ``same``; "t" those of (y_i, x_j) and "a" of (y_i, y_j),
        for Θ and the addends"""
        a, b = {"k": (self.xd, self.xd), "t": (self.yd, self.xd), "a": (self.yd, self.yd)}[name]
        N.call(f"cgp_cov_moments_{self.dtn}", N.ptr(a), N.ptr(b), N.ptr(pi), N.ptr(pj), n, 4,
               self.h, self.w, N.ptr(out), stream())

    def call(self, name, args):
        N.check(getattr(N.load(), f"{name}_{self.dtn}")(args, stream()), name)

    def maps(self, a):
        """[pairs, (h·w)²] in the library's layout -> the oracles' [pairs, h, w, h, w]"""
        return PO.from_device_layout(a, self.h, self.w)


WORLDS = {}


def world(dtn, h=28, w=28, nimg=84):
    """28x28: the 84x84 square, 7 056 pairs, in float32; its second half, 3 528 pairs, in
    float64 (the same bytes)"""
    key = (dtn, h, w, nimg)
    if key not in WORLDS:
        WORLDS[key] = World(h, w, nimg, dtn, first=nimg * nimg // 2 if dtn == "f64" else 0)
    return WORLDS[key]


def test_the_sizes():
    """the boundaries, worked out on paper, and the pairs every case samples"""
    assert 614656 * 3493 < B31 < 614656 * 3494 and 614656 * 6987 < B32 < 614656 * 6988
    assert 1046529 * 4104 < B32 < 1046529 * 4105
    w32, w64 = world("f32"), world("f64")
    assert (w32.n, w32.n * w32.elems) == (7056, 4337012736)
    assert (w64.n, w64.n * w64.elems) == (3528, 2168506368)
    assert w32.n * w32.elems * 4 == w64.n * w64.elems * 8
    assert w32.samples == [0, 3492, 3493, 3494, 3570, 6986, 6987, 6988, 7055]
    assert w64.samples == [0, 3492, 3493, 3494, 3527]
    for w, selfs in ((w32, (3570, 7055)), (w64, (3527,))):
        assert all(w.i[k] == w.j[k] for k in selfs)
    wo = world("f32", 33, 31, 65)
    assert wo.n * wo.elems > B32 and wo.samples[-1] == wo.n - 1 == 4224
    assert {2051, 2052, 2053, 4103, 4104, 4105} < set(wo.samples)


def flat(ref):
    """the oracles' [pairs, h, w, h, w] -> [pairs, elements] in the library's layout"""
    return PO.to_device_layout(ref).reshape(len(ref), -1)


def check(w, roles, launch, outs, oracle, what, tol=None):
    """One case.  roles: name -> (elements per pair, generator of World.gen, or None for an
    output that starts NaN-filled); launch(bufs, pair_i, pair_j, npairs) runs the entry point
    on tensors [npairs, elements]; outs: the roles it writes; oracle(ins, i, j) -> the
    expected [pairs, elements] array of every role of outs for the pairs of images (i[k], j[k]),
    from the float64 host copies ``ins`` of those pairs' generated inputs."""
    tol = OP_TOL[w.dtn] if tol is None else tol
    piece = min(PIECE, w.n)
    # every role whole and as a piece
    require(sum(e for e, _ in roles.values()) * (w.n + piece) * w.item)

    def fill(bufs, pi, pj, n):
        for name, (_, g) in roles.items():
            if g is None:
                bufs[name].fill_(float("nan"))
            else:
                w.gen(g, pi, pj, n, bufs[name])

    def alloc(n):
        return {k: torch.empty((n, e), dtype=w.dt, device=DEV) for k, (e, _) in roles.items()}

    whole = alloc(w.n)
    fill(whole, w.pi, w.pj, w.n)
    launch(whole, w.pi, w.pj, w.n)
    torch.cuda.synchronize()
    for o in outs:
        assert finite(whole[o]), f"{what}: {o} has unwritten elements"
    # the whole buffer against the same entry point on pieces
    scratch = alloc(piece)
    for a in range(0, w.n, piece):
        n = min(piece, w.n - a)
        assert n * max(e for e, _ in roles.values()) < B31
        part = {k: v[:n] for k, v in scratch.items()}
        fill(part, w.pi[a:a + n], w.pj[a:a + n], n)
        launch(part, w.pi[a:a + n], w.pj[a:a + n], n)
        for o in outs:
            assert torch.equal(part[o], whole[o][a:a + n]), f"{what}: {o} of pairs {a}..{a + n}"
    del scratch, part
    # the oracle on the sampled pairs, all in one call
    idx = torch.as_tensor(w.samples, device=DEV)
    pi, pj = w.pi[idx].contiguous(), w.pj[idx].contiguous()
    some = alloc(len(idx))
    fill(some, pi, pj, len(idx))
    ins = {r: some[r].cpu().numpy().astype(np.float64) for r, (_, g) in roles.items()
           if g is not None}
    ref = oracle(ins, [int(w.i[k]) for k in w.samples], [int(w.j[k]) for k in w.samples])
    worst = 0.0
    for o in outs:
        got = whole[o][idx].cpu().numpy()
        assert got.shape == ref[o].shape
        for row, k in enumerate(w.samples):
            err = max_err(got[row], ref[o][row])
            assert err < tol, f"{what}: {o} of pair {k} ({w.i[k]}, {w.j[k]}) is off by {err:.2e}"
            worst = max(worst, err)
    print(f"{what} {w.dtn} {w.h}x{w.w}: {w.n} pairs, {w.n * w.elems} elements, pairs "
          f"{w.samples} worst {worst:.2e}")
    del whole, some


# ------------------------------------------------------------------------------------
# 1. each entry point alone
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", DTYPES)
def test_cov_moments(dtn):
    w = world(dtn)
    w.crosses()

    def launch(b, pi, pj, n):
        N.call(f"cgp_cov_moments_{dtn}", N.ptr(w.xd), N.ptr(w.yd), N.ptr(pi), N.ptr(pj), n, 4,
               w.h, w.w, N.ptr(b["o"]), stream())

    def oracle(ins, i, j):
        return {"o": flat(PO.moments(w.x, w.y, i, j))}

    check(w, {"o": (w.elems, None)}, launch, ["o"], oracle, "cov_moments")


def nonlin_case(w, kind, flags, addend, what):
    """cgp_cov_nonlin_* in place, with ``same`` on x = y, optionally with an addend"""
    ref_map = PO.relu_map if kind == N.CGP_COV_RELU else PO.erf_map

    def launch(b, pi, pj, n):
        a = N.CovNonlinArgs()
        a.in_ = a.out = N.ptr(b["s"])
        a.addend = N.ptr(b.get("a"))
        a.xx = a.yy = N.ptr(w.vxd)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pj), n
        a.h, a.w, a.kind, a.same, a.flags = w.h, w.w, kind, 1, flags
        w.call("cgp_cov_nonlin", a)

    def oracle(ins, i, j):
        ref = ref_map(w.maps(ins["s"]), w.vx, w.vx, i, j, True)
        return {"s": flat(ref + w.maps(ins["a"]) if addend else ref)}

    roles = {"s": (w.elems, "k")}
    if addend:
        roles["a"] = (w.elems, "a")
    check(w, roles, launch, ["s"], oracle, what)


NONLIN_CASES = {"relu": (N.CGP_COV_RELU, 0, False),
                "relu_exact": (N.CGP_COV_RELU, N.CGP_FLAG_EXACT_RELU, False),
                "erf": (N.CGP_COV_ERF, 0, False),
                "relu_addend": (N.CGP_COV_RELU, 0, True)}


@pytest.mark.parametrize("dtn", DTYPES)
@pytest.mark.parametrize("case", list(NONLIN_CASES))
def test_cov_nonlin(case, dtn):
    w = world(dtn)
    w.crosses()
    nonlin_case(w, *NONLIN_CASES[case], f"cov_nonlin {case}")


def test_cov_nonlin_33x31():
    """h != w and (h·w)² = 1 046 529 odd: 4 225 pairs, past 2^32 elements from pair 4 104"""
    w = world("f32", 33, 31, 65)
    w.crosses()
    nonlin_case(w, N.CGP_COV_RELU, 0, False, "cov_nonlin relu")


@pytest.mark.parametrize("dtn", DTYPES)
def test_gelu_cov(dtn):
    w = world(dtn)
    w.crosses()

    def launch(b, pi, pj, n):
        a = N.GeluCovArgs()
        a.in_ = a.out = N.ptr(b["s"])
        a.xx = a.yy = N.ptr(w.vxd)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pj), n
        a.h, a.w, a.same = w.h, w.w, 1
        w.call("cgp_gelu_cov", a)

    def oracle(ins, i, j):
        return {"s": flat(GO.gelu_map(w.maps(ins["s"]), w.vx, w.vx, i, j, True))}

    check(w, {"s": (w.elems, "k")}, launch, ["s"], oracle, "gelu_cov")


@pytest.mark.parametrize("dtn", DTYPES)
@pytest.mark.parametrize("kind, theta_is_in", [("relu", False), ("erf", False), ("gelu", True)])
def test_covntk_nonlin(kind, theta_is_in, dtn):
    """both streams in place; for the GELU theta == in (Θ = K, as behind a first conv), K in
    place and Θ' into a buffer of its own"""
    w = world(dtn)
    w.crosses()

    def launch(b, pi, pj, n):
        a = N.CovNonlinNtkArgs()
        a.in_ = a.out = N.ptr(b["s"])
        a.theta = N.ptr(b["s" if theta_is_in else "t"])
        a.out_theta = N.ptr(b["t"])
        a.xx = a.yy = N.ptr(w.vxd)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pj), n
        a.h, a.w, a.kind, a.same = w.h, w.w, KINDS[kind], 1
        w.call("cgp_covntk_nonlin", a)

    def oracle(ins, i, j):
        s = w.maps(ins["s"])
        th = s if theta_is_in else w.maps(ins["t"])
        k, t = NO.nonlin_ntk(kind, s, th, w.vx, w.vx, i, j, True)
        return {"s": flat(k), "t": flat(t)}

    roles = {"s": (w.elems, "k"), "t": (w.elems, None if theta_is_in else "t")}
    check(w, roles, launch, ["s", "t"], oracle, f"covntk_nonlin {kind}")


@pytest.mark.parametrize("dtn", DTYPES)
def test_axpby_accum(dtn):
    """the executor's ``accum`` form: dst = 1·dst + 1·src, in place"""
    w = world(dtn)
    w.crosses()

    def launch(b, pi, pj, n):
        N.call(f"cgp_axpby_{dtn}", 1.0, N.ptr(b["d"]), 1.0, N.ptr(b["s"]), N.ptr(b["d"]),
               n * w.elems, stream())

    def oracle(ins, i, j):
        npdt = NP_DT[dtn]                                  # one rounding: exact in the type
        return {"d": (ins["d"].astype(npdt) + ins["s"].astype(npdt)).astype(np.float64)}

    check(w, {"d": (w.elems, "k"), "s": (w.elems, "a")}, launch, ["d"], oracle, "axpby accum",
          tol=1e-300)


@pytest.mark.parametrize("dtn", DTYPES)
def test_cov_pool(dtn):
    w = world(dtn)
    w.crosses()

    def launch(b, pi, pj, n):
        N.call(f"cgp_cov_pool_{dtn}", N.ptr(b["s"]), n, w.elems, N.ptr(b["o"]), stream())

    def oracle(ins, i, j):
        return {"o": ins["s"].mean(axis=1, keepdims=True)}

    check(w, {"s": (w.elems, "k"), "o": (1, None)}, launch, ["o"], oracle, "cov_pool")


@pytest.mark.parametrize("dtn", DTYPES)
def test_covmap_diag(dtn):
    """the p = q diagonal of pair m's map, written at image index m (pair_i is the index of
    the row it writes: one row per pair here, so that no two pairs share one)"""
    w = world(dtn)
    w.crosses()

    def launch(b, pi, pj, n):
        rows = torch.arange(n, device=DEV, dtype=torch.int32)
        N.call(f"cgp_covmap_diag_{dtn}", N.ptr(b["s"]), N.ptr(rows), n, w.h, w.w, N.ptr(b["o"]),
               stream())

    def oracle(ins, i, j):
        return {"o": AO.diag(w.maps(ins["s"])).reshape(len(i), -1)}

    check(w, {"s": (w.elems, "k"), "o": (w.h * w.w, None)}, launch, ["o"], oracle, "covmap_diag",
          tol=1e-300)                                      # a gather: exact


@pytest.mark.parametrize("dtn", DTYPES)
def test_covmap_avgpool(dtn):
    w = world(dtn)
    w.crosses()
    ho, wo = w.h // 2, w.w // 2

    def launch(b, pi, pj, n):
        a = N.CovAvgPoolArgs()
        a.in_, a.out, a.npairs = N.ptr(b["s"]), N.ptr(b["o"]), n
        a.h, a.w, a.ho, a.wo, a.k, a.stride = w.h, w.w, ho, wo, 2, 2
        w.call("cgp_covmap_avgpool", a)

    def oracle(ins, i, j):
        return {"o": flat(AO.avgpool_map(w.maps(ins["s"]), 2, 2))}

    check(w, {"s": (w.elems, "k"), "o": ((ho * wo) ** 2, None)}, launch, ["o"], oracle,
          "covmap_avgpool")


def stencil(a, g, w, ho, wo):
    a.h, a.w, a.ho, a.wo = w.h, w.w, ho, wo
    a.taps, a.offset, a.stride, a.dilation = g.taps, g.offset, g.stride, g.dilation
    a.weight, a.bias = g.weight, g.bias


@pytest.mark.parametrize("dtn", DTYPES)
def test_cov_conv(dtn):
    """3x3 same with the ReLU post-stage and the addend written over (out == addend): the
    input and the output cross"""
    w = world(dtn)
    w.crosses()
    mod = C(3, var_weight=1.3, var_bias=0.1)
    g = P.conv_geometry(mod)
    ox = w.rnd(PO.conv_var(w.vx, mod))
    oxd = w.dev(ox)

    def launch(b, pi, pj, n):
        a = N.CovConvArgs()
        a.in_, a.out, a.addend = N.ptr(b["s"]), N.ptr(b["o"]), N.ptr(b["o"])
        a.xx = a.yy = N.ptr(oxd)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pj), n
        stencil(a, g, w, w.h, w.w)
        a.post, a.same = N.CGP_COV_RELU, 1
        w.call("cgp_cov_conv", a)

    def oracle(ins, i, j):
        ref = PO.relu_map(PO.conv_map(w.maps(ins["s"]), mod), ox, ox, i, j, True)
        return {"o": flat(ref + w.maps(ins["o"]))}

    check(w, {"s": (w.elems, "k"), "o": (w.elems, "a")}, launch, ["o"], oracle, "cov_conv")


@pytest.mark.parametrize("dtn", DTYPES)
@pytest.mark.parametrize("case", ["band3", "readout28"])
def test_corrconv(case, dtn):
    """a 3x3 same conv with a band table (in and out cross), and a 28-tap readout: the
    1024-thread instantiation with 16-byte loads, one output per pair"""
    w = world(dtn)
    w.crosses()
    if case == "band3":
        mod = CC(3, var_weight=1.5, var_bias=0.1, weight_corr=(m.band_corr(3, 1),) * 2)
    else:
        mod = CC(28, padding=0, var_weight=1.5, var_bias=0.1,
                 weight_corr=(m.band_corr(28, 1),) * 2)
    g = P.corrconv_geometry(mod)
    ho, wo = P.conv_out_hw(mod, w.h, w.w)
    assert (ho, wo) == ((w.h, w.w) if case == "band3" else (1, 1))
    rr, rc = w.dev(np.array(g.corr_rows)), w.dev(np.array(g.corr_cols))

    def launch(b, pi, pj, n):
        a = N.CorrConvArgs()
        a.in_, a.out, a.npairs = N.ptr(b["s"]), N.ptr(b["o"]), n
        a.corr_rows, a.corr_cols = N.ptr(rr), N.ptr(rc)
        stencil(a, g, w, ho, wo)
        assert b["s"].data_ptr() % 16 == 0                 # the 16-byte loads of the readout
        w.call("cgp_corrconv", a)

    def oracle(ins, i, j):
        return {"o": flat(CO.corrconv_map(w.maps(ins["s"]), mod))}

    check(w, {"s": (w.elems, "k"), "o": ((ho * wo) ** 2, None)}, launch, ["o"], oracle,
          f"corrconv {case}")


def conv_ntk_case(w, mod, post, what):
    g = P.conv_geometry(mod)
    ho, wo = P.conv_out_hw(mod, w.h, w.w)
    ox = w.rnd(PO.conv_var(w.vx, mod))
    oxd = w.dev(ox)

    def launch(b, pi, pj, n):
        a = N.CovConvNtkArgs()
        a.in_, a.theta, a.out, a.out_theta = (N.ptr(b[k]) for k in ("s", "t", "o", "ot"))
        a.xx = a.yy = N.ptr(oxd)
        a.pair_i, a.pair_j, a.npairs = N.ptr(pi), N.ptr(pj), n
        stencil(a, g, w, ho, wo)
        a.post, a.same = post, 1
        w.call("cgp_covntk_conv", a)

    def oracle(ins, i, j):
        k, t = NO.conv_ntk(w.maps(ins["s"]), w.maps(ins["t"]), mod)
        if post == N.CGP_COV_RELU:
            k, t = NO.nonlin_ntk("relu", k, t, ox, ox, i, j, True)
        return {"o": flat(k), "ot": flat(t)}

    oe = (ho * wo) ** 2
    check(w, {"s": (w.elems, "k"), "t": (w.elems, "t"), "o": (oe, None), "ot": (oe, None)},
          launch, ["o", "ot"], oracle, what)


@pytest.mark.parametrize("dtn", DTYPES)
def test_covntk_conv_stride2(dtn):
    """stride-2 3x3 with Θ and the ReLU post-stage: both inputs cross, the outputs are 16x
    smaller"""
    w = world(dtn)
    w.crosses()
    conv_ntk_case(w, C(3, stride=2, var_bias=0.1), N.CGP_COV_RELU, "covntk_conv stride 2")


def test_covntk_conv_same_four_buffers():
    """3x3 same on the float64 case's 3 528 pairs in float32: K, Θ, K' and Θ' all cross 2^31"""
    w64 = world("f64")
    key = ("f32", 28, 28, "half")
    if key not in WORLDS:
        WORLDS[key] = World(28, 28, 84, "f32", first=3528)
    w = WORLDS[key]
    assert w.n == w64.n == 3528 and w.samples == w64.samples
    assert w.n * w.elems > B31
    conv_ntk_case(w, C(3, var_weight=1.3, var_bias=0.1), N.CGP_COV_NONE, "covntk_conv same")


# ------------------------------------------------------------------------------------
# 2. end to end: the whole tile as one chunk against chunks of a few hundred pairs
# ------------------------------------------------------------------------------------
def gap_net():
    """the README's pooled head: two full-size convs with ReLU, the pool, a dense readout"""
    return S(C(3, var_bias=0.1), R(), C(3), R(), G(), C(1, var_weight=2.0, var_bias=0.3))


def tile_images(n, dtn):
    rng = np.random.default_rng(28 + n)
    draw = lambda: rng.random((n, 4, 28, 28), dtype=np.float32).astype(np.float64)   # noqa
    return draw(), draw()


def tile_samples(n):
    """twelve entries of an n x n tile, its corners among them"""
    rng = np.random.default_rng(n)
    inner = [(int(a), int(b)) for a, b in rng.integers(1, n - 1, size=(8, 2))]
    return [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1)] + inner


def one_chunk_against_chunks(model, cs, run, n, dtn, bound):
    """run() with the workspace at cs.peak of the whole n x n tile (one chunk, whose largest
    launch holds more than ``bound`` elements) and at 2 GB; returns the one-chunk results
    after requiring the two bit for bit equal"""
    item = 4 if dtn == "f32" else 8
    ws = cs.peak * item * n * n
    require(ws)
    assert ws // (cs.peak * item) == n * n                  # run_cov_steps' chunk: every pair
    assert n * n * cs.largest > bound
    assert (2 << 30) // (cs.peak * item) < 1024             # the chunks of the second call
    seen = []
    real = N.check

    def check_(rc, what):
        seen.append(what)
        return real(rc, what)
    N.check = check_
    try:
        with torch.no_grad():
            whole = run(model.set_pool_workspace(ws))
            one = seen.count("cgp_cov_moments")
            parts = run(model.set_pool_workspace(2 << 30))
    finally:
        N.check = real
        model.set_pool_workspace(None)
    # one launch of the moments for the tile (and one per self pass of x and of y, a few
    # pairs each); the second call takes a launch per chunk of its pairs
    chunks = -(-n * n // ((2 << 30) // (cs.peak * item)))
    self_passes = 2 if (cs.forward or cs).self_var else 0
    assert one == 1 + self_passes and chunks > 3
    assert seen.count("cgp_cov_moments") - one == chunks + self_passes
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    return whole


def forward_case(n, dtn, bound):
    X, Z = tile_images(n, dtn)
    model = gap_net().to(DEV, TORCH_DT[dtn])
    Xd, Zd = (torch.as_tensor(a).to(DEV, TORCH_DT[dtn]) for a in (X, Z))
    cs = model._plan(28, 28).pool
    k, = one_chunk_against_chunks(model, cs, lambda mod: [mod(Xd, Zd, False)], n, dtn, bound)
    assert tuple(k.shape) == (n, n) and finite(k)
    kh = k.cpu().numpy()
    worst = 0.0
    for i, j in tile_samples(n):
        ref = PO.kernel(model, X[i:i + 1], Z[j:j + 1], False, False)
        worst = max(worst, abs(kh[i, j] - ref[0, 0]) / abs(ref[0, 0]))
    print(f"forward {dtn} {n}x{n}: largest launch {n * n * cs.largest} elements, peak "
          f"{cs.peak * n * n * k.element_size()} bytes, worst {worst:.2e}")
    assert worst < NET_TOL[dtn]


def test_forward_pooled_f32():
    forward_case(84, "f32", B32)


def test_forward_pooled_f64():
    forward_case(60, "f64", B31)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "launch_by_launch"])
def test_ntk_maps(fused):
    """K and Θ of a 60x60 tile in float32, one chunk: both streams past 2^31 per launch"""
    n, dtn = 60, "f32"
    X, Z = tile_images(n, dtn)
    model = gap_net().to(DEV, torch.float32).set_ntk_maps_fusion(fused)
    Xd, Zd = (torch.as_tensor(a).to(DEV, torch.float32) for a in (X, Z))
    cs = model._ntk_maps_steps(model._plan(28, 28), False, Xd)
    assert cs.fused == fused and cs.peak * 4 * n * n < 60e9
    k, th = one_chunk_against_chunks(
        model, cs, lambda mod: mod.ntk_maps(Xd, Zd, False, return_nngp=True), n, dtn, B31)
    assert finite(k) and finite(th)
    kh, th = k.cpu().numpy(), th.cpu().numpy()
    worst = 0.0
    for i, j in tile_samples(n):
        rk, rt = NO.ntk(model, X[i:i + 1], Z[j:j + 1], False, False)
        worst = max(worst, abs(kh[i, j] - rk[0, 0]) / abs(rk[0, 0]),
                    abs(th[i, j] - rt[0, 0]) / abs(rt[0, 0]))
    print(f"ntk_maps f32 {n}x{n} fused={fused}: peak {cs.peak * 4 * n * n} bytes, worst "
          f"{worst:.2e}")
    assert worst < NET_TOL[dtn]


def test_myrtle_f32():
    """conv/ReLU, AvgPool2d(2), conv/ReLU, GlobalAvgPool: cgp_covmap_avgpool_* and the self
    pass through the executor at size"""
    n, dtn = 84, "f32"
    X, Z = tile_images(n, dtn)
    model = S(C(3, var_bias=0.1), R(), A(2), C(3), R(), G()).to(DEV, torch.float32)
    Xd, Zd = (torch.as_tensor(a).to(DEV, torch.float32) for a in (X, Z))
    cs = model._plan(28, 28).pool
    assert any(st.fn == "avgpool" for st in cs.steps) and cs.self_var
    k, = one_chunk_against_chunks(model, cs, lambda mod: [mod(Xd, Zd, False)], n, dtn, B32)
    kh = k.cpu().numpy()
    worst = 0.0
    for i, j in tile_samples(n)[:6]:
        ref = AO.kernel(model, X[i:i + 1], Z[j:j + 1], False, False)
        worst = max(worst, abs(kh[i, j] - ref[0, 0]) / abs(ref[0, 0]))
    print(f"myrtle f32 {n}x{n}: peak {cs.peak * 4 * n * n} bytes, worst {worst:.2e}")
    assert worst < NET_TOL[dtn]
