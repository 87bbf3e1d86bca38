"""CAF covariance-filter GAR on the GPU: the one-workgroup filter on the Gram (k_caf_select) against the fp64
oracle on the exact distances, the non-finite policy, batched launches, max_passes, the n > 128 host route,
arc-caf and the engine (HIP graph, layer-wise device path, sharded).

Inputs and preconditions: tests/_caf_common.py. Every case with colluders (f >= 1) first asserts the three
preconditions on the oracle, so the pass count, the pass kept and the set of exact-zero weights are compared
exactly; the weights and the λ of every pass are compared within WEIGHT_RTOL / LAM_RTOL."""
import math

import pytest
import torch
import torch.nn.functional as F

from _caf_common import assert_preconditions, attacked, case
from garfield_amd.models import build_model
from garfield_amd.ops import gar
from garfield_amd.ops import reference as ref
from garfield_amd.ops.selection import distances_from_gram
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-3}   # the combine tests' tolerance
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 16 / 17: the wave-per-row wrap; 64 / 65: the second lane column; 128: the LDS maximum
SIZES = [1, 2, 3, 4, 5, 8, 16, 17, 33, 64, 65, 127, 128]
HALF_SIZES = [5, 8, 17, 65, 128]   # also with f = (n - 1) // 2: the most passes
DIMS = [64, 2000]
CASES = [(n, (n - 1) // 4) for n in SIZES] + [(n, (n - 1) // 2) for n in HALF_SIZES]
# The kernel's weights (relative to the largest weight) and the λ of every pass (relative) against the fp64
# oracle on the exact distances: the kernel iterates in fp64, so what is left is the fp32 Gram's rounding of
# D. Measured on an MI355X over CASES x DIMS x DTYPES and n = 130 (profiles/r19/caf/test_error.log): the
# maximum weight error is 1.035e-5 (n = 128, f = 63, d = 64, bf16: 16 passes, each update 1 - τ_i / τ_max
# cancels), the maximum λ error 5.726e-6 (n = 33, f = 8, d = 2000, fp16). On the kernel's own Gram, the
# distances rebuilt as the kernel builds them, the oracle's fp32 weights equal the kernel's bit for bit in
# every case: the errors above are the fp32 Gram's rounding of D alone. The bound is 20 x the maximum, the
# margin for Gram-derived quantities; it may never exceed 1e-4 (which caps both here): needing more means a bug.
WEIGHT_ERR_MEASURED = 1.035e-5
LAM_ERR_MEASURED = 5.726e-6
WEIGHT_RTOL = min(20 * WEIGHT_ERR_MEASURED, 1e-4)
LAM_RTOL = min(20 * LAM_ERR_MEASURED, 1e-4)


def close(a, b, dtype):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() <= TOL[dtype] * max(b.abs().max().item(), 1.0)


def select(native, G, f, iters=16, max_passes=0):
    """(weights, lams, Gram) of k_caf_select on the Gram of G."""
    rows = gar.prepare(G)
    n = rows.n
    g = gar._gram_into(native, rows, gar.workspace(rows))
    w = torch.full((n,), -1.0, device=G.device)
    lams = torch.full((n,), -1.0, device=G.device)
    native.gpu_caf_select(g, n, f, iters, max_passes, w, lams)
    return w, lams, g


def errors(w, lams, w_ref, lams_ref):
    """(max |w - w_ref| / max w_ref, max relative λ error) after the exact comparisons: the pass count, the
    pass kept (the first of smallest λ) and the set of exact-zero weights."""
    w, lams = w.double().cpu(), lams.double().cpu()
    w_ref, lams_ref = w_ref.double(), lams_ref.double()
    fin = torch.isfinite(lams_ref)
    assert torch.equal(torch.isfinite(lams), fin) and bool((lams[~fin] == math.inf).all())
    if fin.any():
        assert int(torch.argmin(lams[fin])) == int(torch.argmin(lams_ref[fin]))
    assert torch.equal(w == 0, w_ref == 0)
    assert float(w.min()) >= 0.0 and abs(float(w.sum()) - 1.0) <= 1e-5
    werr = float((w - w_ref).abs().max() / w_ref.max())
    lerr = float(((lams[fin] - lams_ref[fin]).abs() / lams_ref[fin]).max()) if fin.any() else 0.0
    return werr, lerr


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n,f", CASES)
def test_kernel_matches_oracle(cuda, native, n, f, d, dtype):
    X, trace, w_ref, lams_ref, out_ref = case(n, d, dtype, f)
    G = X.to(cuda)
    w, lams, g = select(native, G, f)
    out = gar.caf(G, f)
    wp = gar.caf_weights(G, f).clone()
    torch.cuda.synchronize()
    assert int(torch.isfinite(lams).sum()) == len(trace["lams"])
    if trace["best"] is not None:
        assert int(torch.argmin(lams)) == trace["best"]
    werr, lerr = errors(w, lams, w_ref, lams_ref)
    # rounding noise alone: the oracle on the kernel's own Gram, the distances rebuilt as the kernel builds them
    Dk = distances_from_gram(g.view(native.gram_padded(n), -1)[:n, :n].cpu())
    wk, lk = ref.caf_weights(Dk, f)
    own = float((w.double().cpu() - wk.double()).abs().max() / wk.double().max())
    print(f"caf n={n} f={f} d={d} {dtype}: passes {len(trace['lams'])} kept {trace['best']} "
          f"weight error / largest weight {werr:.3e}, relative lambda error {lerr:.3e}, on its own Gram {own:.3e}")
    assert w.dtype == torch.float32 and out.dtype == dtype and out.shape == (d,)
    assert torch.equal(wp, w)
    assert werr <= WEIGHT_RTOL and lerr <= LAM_RTOL
    # fp64 on both sides of the same fp32 distances: what is left is the cast of the weights to fp32
    assert torch.equal(torch.isfinite(lk), torch.isfinite(lams.cpu())) and own <= 2.0 ** -22
    assert close(out, out_ref, dtype)
    # list input: same kernels on a row table
    assert close(gar.caf([G[i].clone() for i in range(n)], f), out_ref, dtype)
    if f == 0:   # no pass: the plain average, bit for bit
        assert torch.equal(w.cpu(), torch.full((n,), 1.0 / n, dtype=torch.float64).float())
        assert torch.equal(out, gar.average(G))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_host_route(cuda, native, d, dtype):
    """n = 130 > 128: the pairwise distances on the device, the filter in C++ on the host."""
    X, trace, w_ref, lams_ref, out_ref = case(130, d, dtype, 32)
    G = X.to(cuda)
    w = gar.caf_weights(G, 32)
    out = gar.caf(G, 32)
    assert w.is_cuda and w.dtype == torch.float32
    assert torch.equal(w.cpu() == 0, w_ref == 0)
    werr = float((w.cpu().double() - w_ref.double()).abs().max() / w_ref.double().max())
    print(f"caf n=130 f=32 d={d} {dtype} (host route): passes {len(trace['lams'])} weight error / largest weight {werr:.3e}")
    assert werr <= WEIGHT_RTOL
    assert close(out, out_ref, dtype)


def test_max_passes(cuda, native):
    X, trace, w_ref, lams_ref, _ = case(33, 2000, torch.float32, 16)
    assert len(trace["lams"]) >= 4
    G = X.to(cuda)
    D = ref.pairwise_sqdist(X)
    for mp in (1, 3):
        wr, lr = ref.caf_weights(D, 16, max_passes=mp)
        w, lams, _ = select(native, G, 16, max_passes=mp)
        werr, lerr = errors(w, lams, wr, lr)
        assert int(torch.isfinite(lams).sum()) == mp and werr <= WEIGHT_RTOL and lerr <= LAM_RTOL
        assert torch.equal(gar.caf_weights(G, 16, max_passes=mp), w)
    w1, _, _ = select(native, G, 16, max_passes=1)   # one pass: the weights it started from
    assert torch.equal(w1.cpu(), torch.full((33,), 1.0 / 33, dtype=torch.float64).float())
    w, lams, _ = select(native, G, 16, max_passes=33)   # the cap n is no cap
    w0, lams0, _ = select(native, G, 16)
    assert torch.equal(w, w0) and torch.equal(lams, lams0)
    # fewer power rounds are another filter
    wr, lr = ref.caf_weights(D, 16, iters=4)
    w, lams, _ = select(native, G, 16, iters=4)
    assert int(torch.isfinite(lams).sum()) == int(torch.isfinite(lr).sum())
    assert float((w.cpu().double() - wr.double()).abs().max() / wr.double().max()) <= WEIGHT_RTOL


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(cuda, native, dtype):
    X = attacked(9, 1, 500, dtype).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    D = ref.pairwise_sqdist(X)
    G = X.to(cuda)
    for f in (1, 2, 3):   # f = 1: the budget n - 2f = 7 is used up by the two non-finite rows, no pass runs
        trace = ref.caf_trace(D, f)
        if f > 1:   # f = 1: Σc = 7 = n - 2f, both exact integers (a sum of ones): nothing hangs on rounding
            assert_preconditions(trace, 9, f)
        assert (len(trace["lams"]) == 0) == (f == 1)
        w_ref, lams_ref = ref.caf_weights(D, f)
        w, lams, _ = select(native, G, f)
        out = gar.caf(G, f)
        torch.cuda.synchronize()
        werr, lerr = errors(w, lams, w_ref, lams_ref)
        assert float(w[4]) == 0.0 and float(w[6]) == 0.0 and werr <= WEIGHT_RTOL and lerr <= LAM_RTOL
        if f == 1:
            assert torch.equal(w.cpu()[keep], torch.full((7,), 1.0 / 7, dtype=torch.float64).float())
        assert torch.isfinite(out).all()
        assert close(out, ref.combine(X[keep], w_ref.double()[keep]), dtype)


def test_identical_rows_and_all_non_finite(cuda, native):
    X = torch.randn(1, 300, generator=torch.Generator().manual_seed(3)).repeat(7, 1)
    w, lams, _ = select(native, X.to(cuda), 2)
    w_ref, lams_ref = ref.caf_weights(ref.pairwise_sqdist(X), 2)
    assert torch.equal(w.cpu(), w_ref) and torch.equal(lams.cpu(), lams_ref)
    assert torch.equal(w.cpu(), torch.full((7,), 1.0 / 7, dtype=torch.float64).float())
    assert lams.tolist() == [0.0] + [math.inf] * 6   # one pass, λ = 0
    X = torch.full((3, 128), math.nan)
    w, lams, _ = select(native, X.to(cuda), 1)
    assert torch.equal(w.cpu(), torch.full((3,), 1.0 / 3, dtype=torch.float64).float()) and lams.tolist() == [math.inf] * 3


def test_batched_launch_equals_single_launches(cuda, native):
    n, L, f = 9, 3, 2
    np_ = native.gram_padded(n)
    grams = []
    for k in range(L):
        rows = gar.prepare(attacked(n, 2, 900 + 13 * k, seed=k).to(cuda))
        grams.append(gar._gram_into(native, rows, gar.workspace(rows)).clone())
    batch = torch.cat(grams)
    assert batch.numel() == L * np_ * np_
    wb = torch.full((L + 1, n), -1.0, device=cuda)   # one row more than the batch: the tail stays untouched
    lb = torch.full((L + 1, n), -1.0, device=cuda)
    native.gpu_caf_select(batch, n, f, 16, 0, wb, lb, L)
    assert bool((wb[L] == -1.0).all()) and bool((lb[L] == -1.0).all())
    for k in range(L):
        w1 = torch.full((n,), -1.0, device=cuda)
        l1 = torch.full((n,), -1.0, device=cuda)
        native.gpu_caf_select(grams[k], n, f, 16, 0, w1, l1)
        assert torch.equal(w1, wb[k]) and torch.equal(l1, lb[k])
        assert float(w1.min()) == 0.0 and abs(float(w1.sum()) - 1.0) <= 1e-5 and math.isfinite(float(l1[0]))
    assert not torch.equal(lb[0], lb[1])
    # the same launch again: the same bits
    wb2, lb2 = torch.empty_like(wb), torch.empty_like(lb)
    native.gpu_caf_select(batch, n, f, 16, 0, wb2, lb2, L)
    assert torch.equal(wb2[:L], wb[:L]) and torch.equal(lb2[:L], lb[:L])
    with pytest.raises(RuntimeError):
        native.gpu_caf_select(batch, n, f, 16, 0, wb[:2], lb, L)       # weights too small for the batch
    with pytest.raises(RuntimeError):
        native.gpu_caf_select(batch, 129, f, 16, 0, wb, lb, 1)         # beyond the LDS matrix
    with pytest.raises(RuntimeError):
        native.gpu_caf_select(batch, n, 5, 16, 0, wb, lb, L)           # n < 2f + 1
    with pytest.raises(RuntimeError):
        native.gpu_caf_select(batch, n, f, 0, 0, wb, lb, L)            # iters < 1


@pytest.mark.parametrize("n,d", [(9, 500), (33, 2000), (130, 300)])
def test_arc_caf(cuda, n, d):
    f = (n - 1) // 4
    X = attacked(n, f, d)
    X[n - 1] *= 4.0   # a row ARC clips
    w_ref = ref.arc_weights(X, f, "caf")
    G = X.to(cuda)
    w = gar.arc_weights(G, f, "caf")
    out = gar.aggregate("arc-caf", G, f=f)
    assert torch.equal(w.cpu() == 0, w_ref == 0)
    assert float((w.cpu().double() - w_ref).abs().max() / w_ref.max()) <= WEIGHT_RTOL
    assert close(out, ref.arc(X, f, "caf"), torch.float32)


def _run(cuda, steps=3, pre=None, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar="caf", f=1, workers_per_rank=5, byzantine={4: "reverse"}, lr=0.05, pre_aggregation=pre, **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


# Models of two paths whose Grams sum the coordinates in another order: the filter's weights differ within
# WEIGHT_RTOL (their zeros exactly), the combine runs on another split of the coordinates; after one step
# of lr 0.05 the parameters agree to rtol 1e-5 and the absolute floor of the other engine tests.
MODEL_ATOL = 1e-7


def assert_same_filter(w1, w0, p1, p0):
    w1, w0 = w1.double().reshape(-1, 5), w0.double().reshape(-1, 5)
    assert w1.shape == w0.shape and torch.equal(w1 == 0, w0 == 0)
    err = float(((w1 - w0).abs().max(1).values / w0.max(1).values).max())
    print("weights: max difference / largest weight", err, "models: max abs difference", float((p1 - p0).abs().max()))
    assert err <= WEIGHT_RTOL
    torch.testing.assert_close(p1, p0, rtol=1e-5, atol=MODEL_ATOL)


@pytest.mark.parametrize("pre", [None, "arc"])
def test_engine_graph_equals_eager(cuda, pre):
    eager = _run(cuda, pre=pre, cuda_graph=False)
    graph = _run(cuda, pre=pre, cuda_graph=True)
    w = eager.last_weights.cpu()
    assert float(w.min()) >= 0.0 and float(w[4]) < 0.02 and float(w.sum()) <= 1.0 + 1e-5   # the reversed row is filtered
    expect = gar.caf_weights(eager.G, 1, pre=pre)
    assert torch.equal(w, expect.cpu())
    assert torch.equal(eager.last_weights, graph.last_weights)
    assert torch.equal(eager.flat_model(), graph.flat_model())


def _segment_preconditions(eng, layerwise):
    """The preconditions on the engine's rows: on every parameter segment (layer-wise) or on the whole rows."""
    G = eng.G[:, : eng.d].float().cpu()
    for off, numel in sorted(zip(eng.flat.offsets, eng.flat.numels)) if layerwise else [(0, eng.d)]:
        assert_preconditions(ref.caf_trace(ref.pairwise_sqdist(G[:, off:off + numel]), 1), 5, 1)


def test_engine_layerwise_device_vs_segment_loop(cuda, monkeypatch):
    import garfield_amd.parallel.engine as E

    outs = []
    for dev_path in (False, True):
        monkeypatch.setattr(E, "LW_DEVICE", dev_path)
        eng = _run(cuda, steps=1, layerwise=True, cuda_graph=False)
        assert (getattr(eng, "_lw", None) is not None) == dev_path
        outs.append((eng.flat_model().clone(), eng.last_weights.clone()))
    _segment_preconditions(eng, True)
    (p0, w0), (p1, w1) = outs
    assert w0.shape == w1.shape and w0.shape[0] >= 2 and w0.shape[1] == 5
    assert_same_filter(w1, w0, p1, p0)


@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_sharded_one_rank_vs_unsharded(cuda, layerwise):
    """The per-bucket partial Grams sum in another order than the whole-row Gram: the same filter."""
    outs = []
    for shard in (True, False):
        eng = _run(cuda, steps=1, shard_gar=shard, layerwise=layerwise, cuda_graph=False)
        assert (eng._shard is not None) == shard
        outs.append((eng.flat_model().clone(), eng.last_weights.clone().float()))
    _segment_preconditions(eng, layerwise)   # the unsharded engine's rows
    (p1, w1), (p0, w0) = outs
    assert_same_filter(w1, w0, p1, p0)
