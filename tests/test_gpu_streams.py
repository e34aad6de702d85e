"""Stream ordering: calls made while the work that produces their inputs is still pending.

Every other GPU test quiesces the device before the call it checks.  Here a calibrated delay
(tests/stream_util.py) holds a stream, the producer work (a copy into the buffer the call
reads, an in-place weight edit, a cached upload) is queued behind it, a control read on
fresh non-blocking streams proves the buffer still holds its old contents, and only then the
call under test is made.  Every result is compared bit for bit with the same call made
quiesced on a fresh instance of the same model; the end-to-end family (D) also pins each
quiesced result to its float64 oracle at NET_TOL of tests/test_gpu_erf.py.

A  save_K's helper streams against pending work on the caller's stream
B  shared cached uploads (Plan._var_chain, Plan._corr_tables) are resident on return
C  save_K(overlap=4) as a fresh model's very first call: four streams make first use at once
D  every path on a side stream behind pending producer work, on a fresh model and on one
   that has run on another stream only
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
from torch.utils.data import Subset, TensorDataset

import cnn_gp
from cnn_gp import _native as N
from cnn_gp import gram
from cnn_gp.kernel_save_tools import save_K
from oracle import nngp_oracle as O
from oracle import specs

import avgpool_oracle as AO
import configs_util
import gelu_oracle as GO
import ntk_oracle
import test_gpu_avgpool as TA
import test_gpu_gelu as TG
from stream_util import Control, delay, delay_seconds
from test_gpu_erf import NET_TOL, TORCH_DT, MemH5, dev, max_err, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda"


def test_the_delay_is_calibrated():
    """about 0.1-0.3 s, never more than 0.5 s (the machine is shared)"""
    assert 0.1 <= delay_seconds() <= 0.3


def rand_images(n, seed, c=1, side=28):
    """float32-representable images as float64 arrays: one oracle serves both precisions"""
    rng = np.random.default_rng(seed)
    return rng.random((n, c, side, side), dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------
# A. save_K against pending work on the caller's stream
# ------------------------------------------------------------------------------------
def build(model, X, X2=None, diag=False, overlap=1, batch_size=16):
    """save_K with save_kernel.py's kern into the in-memory stand-in; the float32 dataset"""
    def kern(x, x2, same, diag):
        with torch.no_grad():
            return model(x.cuda(), x2.cuda(), same, diag).detach().cpu().numpy()

    f = MemH5()
    save_K(f, kern, "K", X, X2, diag, batch_size, print_interval=1e9, overlap=overlap)
    return f.d["K"]


def device_dataset(images):
    """images and labels on the images' device"""
    return TensorDataset(images, torch.zeros(len(images), device=images.device))


@functools.lru_cache(maxsize=None)
def final_images():
    X = dev(rand_images(40, 1), torch.float32)
    Z = dev(rand_images(24, 2), torch.float32)
    torch.cuda.synchronize()
    return X, Z


SHUFFLED = [int(k) for k in np.random.default_rng(3).permutation(40)]


def as_given(ds, subset):
    return Subset(ds, SHUFFLED) if subset else ds


@functools.lru_cache(maxsize=None)
def quiesced_build(x2, diag, subset):
    """overlap=1 on the final images with a fresh model and the device quiet on both sides"""
    X, Z = final_images()
    model = configs_util.model("mnist_as_tf").cuda()
    torch.cuda.synchronize()
    want = build(model, as_given(device_dataset(X), subset),
                 device_dataset(Z) if x2 else None, diag, overlap=1)
    torch.cuda.synchronize()
    assert np.isfinite(want[0] if x2 or diag else want[0][np.triu_indices(40)]).all()
    return want


A_CASES = {
    "overlap4": dict(),
    "overlap2": dict(overlap=2),
    "kxz": dict(x2=True),
    "diag": dict(diag=True),
    "subset": dict(subset=True),
}


def racing_build(x2=False, diag=False, subset=False, overlap=4, producer_stream=True):
    Xf, Zf = final_images()
    want = quiesced_build(x2, diag, subset)
    model = configs_util.model("mnist_as_tf").cuda()
    Xd, Zd = torch.zeros_like(Xf), torch.zeros_like(Zf)
    ctl = Control(Xd)                                        # synchronises
    P = torch.cuda.Stream() if producer_stream else torch.cuda.current_stream()
    with torch.cuda.stream(P):
        delay()
        Xd.copy_(Xf)
        Zd.copy_(Zf)
        ctl.check()
        got = build(model, as_given(device_dataset(Xd), subset),
                    device_dataset(Zd) if x2 else None, diag, overlap=overlap)
    torch.cuda.synchronize()
    stale = int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want)))))
    print(f"save_K behind pending work: {stale} of {got.size} entries differ")
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("case", list(A_CASES))
def test_save_K_waits_for_the_callers_pending_writes(case):
    """A device-resident dataset is written on the caller's stream behind a delay, the control
    sees it still zero, and save_K is called at once: every tile equals the serial build on
    the final images.  Variants: overlap 2, a Kxz build, the diagonal, and a Subset with
    shuffled indices (each batch is gathered on the caller's stream during the iteration;
    the gather's index upload waits for that stream on the host, so this variant's window
    is the gather kernel alone)."""
    racing_build(**A_CASES[case])


def test_save_K_waits_for_the_default_stream():
    """The same with the producer on the default stream.  The helper streams and the control's
    stream are non-blocking, so the null stream orders neither: the control does see zeros
    here, and this is a race test like the others, not only an ordered-result check."""
    racing_build(producer_stream=False)


def first_conv(model):
    return next((n, mod) for n, mod in model.named_modules() if isinstance(mod, cnn_gp.Conv2d))


def edit_weights(model, how, new=None):
    """the edit forms of test_in_place_weight_edit_reaches_the_next_forward; ``data`` rebinds
    the buffer to ``new``, prepared (zero) beforehand so that the control has old contents"""
    name, conv = first_conv(model)
    if how == "mul_":
        conv.kernel.mul_(2.0)
    elif how == "load_state_dict":
        sd = model.state_dict()
        sd[f"{name}.kernel"] = sd[f"{name}.kernel"] * 2
        model.load_state_dict(sd)
    else:
        new = torch.zeros_like(conv.kernel) if new is None else new
        new.copy_(conv.kernel * 2)
        conv.kernel.data = new


@functools.lru_cache(maxsize=None)
def quiesced_edited_build():
    X, _ = final_images()
    model = configs_util.model("mnist_as_tf").cuda()
    with torch.no_grad():
        edit_weights(model, "mul_")
    torch.cuda.synchronize()
    want = build(model, device_dataset(X.cpu()), overlap=1)
    torch.cuda.synchronize()
    iu = np.triu_indices(40)
    assert np.isfinite(want[0][iu]).all()
    assert not np.array_equal(want[0][iu], quiesced_build(False, False, False)[0][iu])
    return want


@pytest.mark.parametrize("how", ["mul_", "load_state_dict", "data"])
def test_save_K_waits_for_a_pending_weight_edit(how):
    """a Conv2d weight buffer edited in place on the caller's stream behind a delay, right
    before save_K: the dataset is the edited model's.  The images are on the host here, so
    the tiles are ordered by save_K's entry event alone."""
    Xh = final_images()[0].cpu()
    want = quiesced_edited_build()
    model = configs_util.model("mnist_as_tf").cuda()
    conv = first_conv(model)[1]
    new = torch.zeros_like(conv.kernel)
    ctl = Control(new if how == "data" else conv.kernel)
    P = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(P):
        delay()
        edit_weights(model, how, new)
        ctl.check()
        got = build(model, device_dataset(Xh), overlap=4)
    torch.cuda.synchronize()
    print(f"save_K behind a weight edit ({how}): "
          f"{int(np.sum(got[0][np.triu_indices(40)] != want[0][np.triu_indices(40)]))} of 820 "
          "entries differ")
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------
# B. shared cached uploads are resident when their getter returns
# ------------------------------------------------------------------------------------
def poison(nbytes):
    """allocate, fill with 0xA5 and free a block on the current stream: the next allocation
    of that size on this stream is likely to land on these bytes"""
    blk = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    del blk


def window_marker():
    """a flag set on the current stream, behind the delay already queued there: its control
    proves the stream was still held when the getter was called"""
    flag = torch.zeros(8, dtype=torch.int32, device=DEV)
    ctl = Control(flag)
    return flag, ctl


def chain_args(plan):
    need = set(range(plan.prog.n_values))          # as test_var_chain_matches_layer_pipeline
    return need, set(list(need)[::3])


def test_var_chain_records_are_resident_on_return():
    """Plan._var_chain's op records are shared by every stream that runs the plan: read on a
    second stream the moment the getter returns, with the uploading stream held by a delay,
    they are the bytes a full synchronise shows, and those are the host records.  No kernel
    reads the records here."""
    model = configs_util.model("mnist_as_tf").cuda()
    plan = model._plan(28, 28)
    need, quarter = chain_args(plan)
    nbytes = ctypes.sizeof(N.VarOp) * (len(plan.prog.ops) + 1)
    flag, ctl = window_marker()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(A):
        poison(nbytes)
        delay()
        flag.fill_(1)
        ctl.check()
        chain = plan._var_chain(need, quarter, torch.device(DEV, torch.cuda.current_device()))
    assert chain is not None and chain["ops"].numel() == nbytes
    with torch.cuda.stream(B):
        got = chain["ops"].cpu()
    torch.cuda.synchronize()
    want = chain["ops"].cpu()
    plan2 = configs_util.model("mnist_as_tf").cuda()._plan(28, 28)
    torch.cuda.synchronize()
    host = plan2._var_chain(need, quarter, torch.device(DEV, torch.cuda.current_device()))
    torch.cuda.synchronize()
    print(f"var chain records: {int((got != want).sum())} of {nbytes} bytes in flight on return")
    assert torch.equal(want, host["ops"].cpu())
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtn", ["f64", "f32"])
def test_corr_tables_are_resident_on_return(dtn):
    """the same for Plan._corr_tables, whose copy has been synchronous from the start"""
    dt = TORCH_DT[dtn]
    model = TG.pooled_nets()["corr_readout"].to(DEV, dt)
    plan = model._plan(8, 8)
    op = next(st.op for st in plan.pool.steps if st.fn == "corrconv")
    rows, cols = (torch.tensor(m, dtype=torch.float64).to(dt)
                  for m in (op.geom.corr_rows, op.geom.corr_cols))
    flag, ctl = window_marker()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(A):
        poison(rows.numel() * rows.element_size())
        poison(rows.numel() * rows.element_size())
        delay()
        flag.fill_(1)
        ctl.check()
        tabs = plan._corr_tables(op, torch.device(DEV, torch.cuda.current_device()), dt)
    with torch.cuda.stream(B):
        got = [t.cpu() for t in tabs]
    torch.cuda.synchronize()
    assert torch.equal(got[0], rows) and torch.equal(got[1], cols)
    assert torch.equal(tabs[0].cpu(), rows) and torch.equal(tabs[1].cpu(), cols)


# ------------------------------------------------------------------------------------
# C. first use by several streams at once
# ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtn", ["f32", "f64"])
@pytest.mark.parametrize("cfg", ["mnist_paper_convnet_gp", "mnist_as_tf"])
def test_first_use_by_four_streams_at_once(cfg, dtn):
    """save_K(overlap=4, batch_size=8) is a fresh model's very first call: 40 images make 15
    tiles, and the first four make first use of the plan, its variance chain and their tile
    recipes concurrently.  Equal to the serial build of another fresh instance."""
    dt = TORCH_DT[dtn]
    X = torch.from_numpy(rand_images(40, 6)).to(dt)
    ds = TensorDataset(X, torch.zeros(len(X)))
    serial = build(configs_util.model(cfg).to(DEV, dt), ds, overlap=1, batch_size=8)
    torch.cuda.synchronize()
    got = build(configs_util.model(cfg).to(DEV, dt), ds, overlap=4, batch_size=8)
    assert np.isfinite(serial[0][np.triu_indices(40)]).all()
    np.testing.assert_array_equal(got, serial)


# ------------------------------------------------------------------------------------
# D. every path: first use on a side stream behind pending producer work
# ------------------------------------------------------------------------------------
class Case:
    """make(dt) -> a fresh model on the device; images() -> (X, Z) float64 arrays;
    call(model, X, Z) -> tuple of device tensors; oracle(X, Z) -> tuple of float64 arrays;
    err: the metric the path's own tests use against that oracle (max_err skips the entries
    the oracle leaves NaN: a Gram's lower triangle)"""

    def __init__(self, name, dtn, make, images, call, oracle, err=rel_err, okey=None):
        self.name, self.dtn, self.make, self.images = name, dtn, make, images
        self.call, self.oracle, self.err = call, oracle, err
        self.okey = okey or name             # cases of one okey share the oracle's result


def xx(m, X, Z):
    return (m(X),)


def xz(m, X, Z):
    return (m(X, Z, False, False),)


def ntk_xz(m, X, Z):
    return m.ntk(X, Z, False, False, return_nngp=True)


def gram_xx(m, X, Z):
    return (gram.gram_matrix(m, X, batch_size=4),)


def cases():
    out = []
    mnist = lambda: (rand_images(6, 7), rand_images(3, 8))                       # noqa: E731
    for cfg in ("mnist_paper_convnet_gp", "mnist_as_tf"):
        spec = getattr(specs, cfg)()
        for mode, call in (("xx", xx), ("xz", xz)):
            oracle = (lambda X, Z, spec=spec: (O.kernel(spec, X),)) if mode == "xx" else \
                (lambda X, Z, spec=spec: (O.kernel(spec, X, Z, False, False),))
            for dtn in ("f64", "f32"):
                out.append(Case(f"fused-{cfg}-{mode}-{dtn}", dtn,
                                lambda dt, cfg=cfg: configs_util.model(cfg).to(DEV, dt),
                                mnist, call, oracle, okey=f"{cfg}-{mode}"))
            if cfg == "mnist_as_tf":
                out.append(Case(f"layer-{cfg}-{mode}-f64", "f64",
                                lambda dt: configs_util.model("mnist_as_tf").to(DEV, dt)
                                .set_fused_network(False), mnist, call, oracle,
                                okey=f"{cfg}-{mode}"))
    out.append(Case("layer-mnist_as_tf-ntk-f64", "f64",
                    lambda dt: configs_util.model("mnist_as_tf").to(DEV, dt),
                    lambda: (rand_images(4, 9), rand_images(3, 10)), ntk_xz,
                    lambda X, Z: ntk_oracle.ntk(specs.mnist_as_tf(), X, Z, False, False)))
    mixed = lambda dt: TG.nets(8)["mixed"][0].to(DEV, dt)                        # noqa: E731
    mixed_ref = lambda: TG.nets(8)["mixed"][0].double()                          # noqa: E731
    out.append(Case("mixed-forward-f64", "f64", mixed, lambda: TG.images(8, 1), xz,
                    lambda X, Z: (GO.kernel(mixed_ref(), X, Z, False, False),)))
    out.append(Case("mixed-ntk-f64", "f64", mixed, lambda: TG.images(8, 1), ntk_xz,
                    lambda X, Z: GO.ntk_stepwise(mixed_ref(), X, Z, False, False)))
    out.append(Case("pairs-myrtle-f64", "f64",
                    lambda dt: TA.pooled_nets()["myrtle"][0].to(DEV, dt),
                    lambda: TA.images(8, 6), xz,
                    lambda X, Z: (AO.kernel(TA.pooled_nets()["myrtle"][0].double(), X, Z, False,
                                            False),), max_err))
    corr_ref = lambda X, Z: (GO.pooled_kernel(TG.pooled_nets()["corr_readout"].double(), X, Z,  # noqa
                                              False, False),)

    def corr(dt, one_pair=False):
        m = TG.pooled_nets()["corr_readout"].to(DEV, dt)
        if one_pair:      # one pair per chunk: the allocator recycles buffers inside the call
            per_pair = m._plan(8, 8).pool.peak * torch.empty((), dtype=dt).element_size()
            m.set_pool_workspace(per_pair + per_pair // 2)
        return m
    out.append(Case("pairs-corr_readout-f64", "f64", corr, TG.pool_images, xz, corr_ref, max_err))
    out.append(Case("pairs-corr_readout-one_pair_chunks-f64", "f64",
                    lambda dt: corr(dt, True), TG.pool_images, xz, corr_ref, max_err))
    gspec = specs.mnist_paper_convnet_gp()
    out.append(Case("gram-mnist_paper_convnet_gp-f64", "f64",
                    lambda dt: configs_util.model("mnist_paper_convnet_gp").to(DEV, dt),
                    lambda: (rand_images(10, 11), rand_images(3, 12)), gram_xx,
                    lambda X, Z: (np.where(np.triu(np.ones((10, 10), bool)),
                                           O.kernel(gspec, X), np.nan),), max_err))
    return out


D_CASES = cases()
_QUIESCED, _ORACLE = {}, {}


def quiesced(case):
    """the call on a fresh model with the device quiet on both sides, once per case, pinned to
    the case's float64 oracle at NET_TOL"""
    if case.name not in _QUIESCED:
        dt = TORCH_DT[case.dtn]
        X, Z = case.images()
        m = case.make(dt)
        Xd, Zd = dev(X, dt), dev(Z, dt)
        torch.cuda.synchronize()
        with torch.no_grad():
            want = [t.cpu().numpy() for t in case.call(m, Xd, Zd)]
        torch.cuda.synchronize()
        if case.okey not in _ORACLE:
            _ORACLE[case.okey] = case.oracle(X, Z)
        errs = [case.err(w, ref) for w, ref in zip(want, _ORACLE[case.okey])]
        print(f"{case.name}: quiesced vs oracle " + " ".join(f"{e:.1e}" for e in errs))
        assert max(errs) < NET_TOL[case.dtn], (case.name, errs)
        _QUIESCED[case.name] = want
    return _QUIESCED[case.name]


@pytest.mark.parametrize("first", ["fresh", "other_stream"])
@pytest.mark.parametrize("case", D_CASES, ids=lambda c: c.name)
def test_first_use_on_a_side_stream(case, first):
    """Everything under one non-default stream with no synchronise in between: the delay, the
    copies of the final images into zero-filled buffers, the control read showing zeros, the
    call, the copy back.  Bit-equal to the quiesced call: a launch or copy of the path that
    strayed onto another stream would read the zeros, or a buffer not yet written.

    ``fresh``: the model's very first call.  Building its plan reads the weights back and
    the shared uploads of B block, so part of such a call runs after the stream has drained.
    ``other_stream``: the model has run once, on the default stream and on other images; on
    the side stream this is still the first use (tile recipes are per stream), and nothing
    in it waits on the host, so every launch of it falls inside the window."""
    dt = TORCH_DT[case.dtn]
    want = quiesced(case)
    X, Z = case.images()
    Xf, Zf = dev(X, dt), dev(Z, dt)
    m = case.make(dt)
    if first == "other_stream":
        with torch.no_grad():
            case.call(m, torch.rand_like(Xf), torch.rand_like(Zf))
    Xd, Zd = torch.zeros_like(Xf), torch.zeros_like(Zf)
    ctl = Control(Xd)                                        # synchronises
    S = torch.cuda.Stream()
    with torch.no_grad(), torch.cuda.stream(S):
        delay()
        Xd.copy_(Xf)
        Zd.copy_(Zf)
        ctl.check()
        got = [t.cpu().numpy() for t in case.call(m, Xd, Zd)]
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
