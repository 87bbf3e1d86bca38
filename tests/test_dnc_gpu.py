"""DnC spectral-filtering GAR on the GPU: the one-workgroup power iteration on the Gram (k_dnc_select)
against the fp64 oracle on the exact distances, the non-finite policy, batched launches, the n > 128
path and the engine (HIP graph, layer-wise device path, sharded).

Inputs: attacked(n, f, d, dtype): rows N(0, I), the last f = (n - 1) // 4 rows shifted by one common
3 N(0, I); the oracle sees the rows after the cast to dtype. Every case with colluders (f >= 1) first
asserts the two preconditions on the oracle: lambda_2 <= 0.5 lambda_1 of K and a relative gap >= 1e-4
between the last kept and the first dropped score. At n <= 4, f = 0: nothing is removed, so there is no
selection to protect, and a cloud of N(0, I) rows without colluders has no spectral gap to assert; the
kernel and the oracle still run the same 16 rounds from the same start and are compared in full."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from garfield_amd.models import build_model
from garfield_amd.ops import gar
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-3}   # the combine tests' tolerance
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 16 / 17: the wave-per-row wrap; 64 / 65: the second lane column; 128: the LDS maximum
SIZES = [1, 2, 3, 4, 8, 16, 17, 33, 64, 65, 127, 128]
DIMS = [64, 2000]
# Scores on the valid rows against the fp64 oracle, relative to the largest score. Measured on an
# MI355X over SIZES x DIMS x DTYPES and n = 130 (profiles/r13/dnc/test_scores_error.log): the maximum
# is 1.678e-6 (n = 4, d = 2000, fp32: f = 0 there, no spectral gap, so the unconverged iterate is more
# sensitive to the fp32 Gram's rounding of D; with colluders, f >= 1, the maximum is 4.32e-7, of the order
# of the 2.4e-7 an fp32 emulation of the Gram predicts; the kernel iterates in fp64). The bound is 20 x the
# maximum, the margin for Gram-derived quantities; it may never exceed 1e-4: needing more means a bug.
SCORE_ERR_MEASURED = 1.678e-6
SCORE_RTOL = min(20 * SCORE_ERR_MEASURED, 1e-4)


def attacked(n, f, d, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(1000 * n + d + seed)
    X = torch.randn(n, d, generator=g)
    if f:
        X[n - f:] += 3.0 * torch.randn(d, generator=g)
    return X.to(dtype)


def assert_preconditions(D, m, iters=16):
    """On the oracle, for an all-finite D: the spectral gap of K = -1/2 J D J and the selection gap."""
    n = D.shape[0]
    Dz = D.clone().double()
    Dz.fill_diagonal_(0.0)
    J = torch.eye(n, dtype=torch.float64) - 1.0 / n
    ev = torch.linalg.eigvalsh(-0.5 * J @ Dz @ J)
    assert float(ev[-2]) <= 0.5 * float(ev[-1]), (float(ev[-2]), float(ev[-1]))
    if m < n:
        s = sorted(ref.dnc_scores(D, iters).tolist())
        assert s[m] - s[m - 1] >= 1e-4 * s[m], (s[m - 1], s[m])


@functools.lru_cache(maxsize=None)
def case(n, d, dtype):
    """(rows on the CPU, f, oracle weights, oracle scores, oracle output): computed once, shared, never modified."""
    f = (n - 1) // 4
    X = attacked(n, f, d, dtype)
    D = ref.pairwise_sqdist(X)
    if f:
        assert_preconditions(D, n - f)
    w, s = ref.dnc_weights(D, n - f)
    return X, f, w, s, ref.combine(X, w.double())


def score_err(s, s_ref):
    s, s_ref = s.double().cpu(), s_ref.double().cpu()
    fin = torch.isfinite(s_ref)
    assert torch.equal(torch.isfinite(s), fin)
    err, top = float((s[fin] - s_ref[fin]).abs().max()), float(s_ref[fin].max())
    return err / top if top > 0.0 else err   # all-zero scores (one row, identical rows): absolute


def close(a, b, dtype):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() <= TOL[dtype] * max(b.abs().max().item(), 1.0)


def select(native, G, m, iters=16):
    """(weights, scores) of k_dnc_select on the Gram of G."""
    rows = gar.prepare(G)
    n = rows.n
    g = gar._gram_into(native, rows, gar.workspace(rows))
    w = torch.full((n,), -1.0, device=G.device)
    s = torch.full((n,), -1.0, device=G.device)
    native.gpu_dnc_select(g, n, m, iters, w, s)
    return w, s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_oracle(cuda, native, n, d, dtype):
    X, f, w_ref, s_ref, out_ref = case(n, d, dtype)
    G = X.to(cuda)
    w, s = select(native, G, n - f)
    out = gar.dnc(G, f)
    wp = gar.dnc_weights(G, f).clone()
    torch.cuda.synchronize()
    err = score_err(s, s_ref)
    print(f"dnc scores n={n} d={d} {dtype}: max error / largest score {err:.3e}")
    assert w.dtype == torch.float32 and out.dtype == dtype and out.shape == (d,)
    assert torch.equal(w.cpu(), w_ref) and torch.equal(wp.cpu(), w_ref)
    assert err <= SCORE_RTOL
    assert close(out, out_ref, dtype)
    # list input: same kernels on a row table
    assert close(gar.dnc([G[i].clone() for i in range(n)], f), out_ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_large_path(cuda, native, d, dtype):
    """n = 130 > 128: the large Gram kernel + the vectorised rounds on the device."""
    X, f, w_ref, s_ref, out_ref = case(130, d, dtype)
    G = X.to(cuda)
    w, s = gar.dnc_weights_from_gram(gar.large_gram(G), 130 - f, 16, with_scores=True)
    out = gar.dnc(G, f)
    err = score_err(s, s_ref)
    print(f"dnc scores n=130 d={d} {dtype} (large path): max error / largest score {err:.3e}")
    assert w.is_cuda and w.dtype == torch.float32
    assert torch.equal(w.cpu(), w_ref) and torch.equal(gar.dnc_weights(G, f).cpu(), w_ref)
    assert err <= SCORE_RTOL
    assert close(out, out_ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(cuda, native, dtype):
    X = attacked(9, 1, 500, dtype).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    assert_preconditions(ref.pairwise_sqdist(X[keep]), 6)
    D = ref.pairwise_sqdist(X)
    G = X.to(cuda)
    for f, sel in ((2, keep), (3, keep[:-1])):   # f = 2: the budget is used up by the two non-finite rows
        w_ref, s_ref = ref.dnc_weights(D, 9 - f)
        assert sorted(torch.nonzero(w_ref).reshape(-1).tolist()) == sel
        w, s = select(native, G, 9 - f)
        out = gar.dnc(G, f)
        torch.cuda.synchronize()
        assert torch.equal(w.cpu(), w_ref) and float(w[4]) == 0.0 and float(w[6]) == 0.0
        assert math.isinf(float(s[4])) and math.isinf(float(s[6])) and float(s[4]) > 0 and float(s[6]) > 0
        assert score_err(s, s_ref) <= SCORE_RTOL
        assert torch.isfinite(out).all()
        assert close(out, ref.combine(X[sel], torch.full((len(sel),), 1.0 / len(sel), dtype=torch.float64)), dtype)


def test_identical_rows_and_all_non_finite(cuda, native):
    X = torch.randn(1, 300, generator=torch.Generator().manual_seed(3)).repeat(7, 1)
    w, s = select(native, X.to(cuda), 5)
    w_ref, s_ref = ref.dnc_weights(ref.pairwise_sqdist(X), 5)
    assert torch.equal(s.cpu(), torch.zeros(7)) and torch.equal(w.cpu(), w_ref)
    X = torch.full((3, 128), math.nan)
    w, s = select(native, X.to(cuda), 2)
    assert torch.equal(w.cpu(), torch.full((3,), 1.0 / 3, dtype=torch.float64).float()) and s.tolist() == [0.0] * 3


def test_batched_launch_equals_single_launches(cuda, native):
    n, L, m = 9, 3, 7
    np_ = native.gram_padded(n)
    grams = []
    for k in range(L):
        rows = gar.prepare(attacked(n, 2, 900 + 13 * k, seed=k).to(cuda))
        grams.append(gar._gram_into(native, rows, gar.workspace(rows)).clone())
    batch = torch.cat(grams)
    assert batch.numel() == L * np_ * np_
    wb = torch.full((L, n), -1.0, device=cuda)
    sb = torch.full((L, n), -1.0, device=cuda)
    native.gpu_dnc_select(batch, n, m, 16, wb, sb, L)
    for k in range(L):
        w1 = torch.full((n,), -1.0, device=cuda)
        s1 = torch.full((n,), -1.0, device=cuda)
        native.gpu_dnc_select(grams[k], n, m, 16, w1, s1)
        assert torch.equal(w1, wb[k]) and torch.equal(s1, sb[k])
        assert int((w1 > 0).sum()) == m and float(w1.min()) == 0.0 and float(s1.min()) >= 0.0
    assert not torch.equal(sb[0], sb[1])
    # the same launch again: the same bits
    wb2, sb2 = torch.empty_like(wb), torch.empty_like(sb)
    native.gpu_dnc_select(batch, n, m, 16, wb2, sb2, L)
    assert torch.equal(wb2, wb) and torch.equal(sb2, sb)
    with pytest.raises(RuntimeError):
        native.gpu_dnc_select(batch, n, m, 16, wb[:2], sb, L)       # weights too small for the batch
    with pytest.raises(RuntimeError):
        native.gpu_dnc_select(batch, 129, m, 16, wb, sb, 1)         # beyond the LDS matrix
    with pytest.raises(RuntimeError):
        native.gpu_dnc_select(batch, n, n + 1, 16, wb, sb, L)       # m > n


def _run(cuda, steps=3, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar="dnc", f=1, workers_per_rank=5, byzantine={4: "reverse"}, lr=0.05, **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


# Models of two paths that select the same rows with the same weights (0 or 1 / kv, exactly): what is left
# is the combine's own arithmetic on another split of the coordinates, rtol 1e-5 and the absolute floor of
# the other engine tests for parameters near zero.
MODEL_ATOL = 1e-7


def assert_models_close(p1, p0):
    print("models: max abs difference", float((p1 - p0).abs().max()))
    torch.testing.assert_close(p1, p0, rtol=1e-5, atol=MODEL_ATOL)


def test_engine_graph_equals_eager(cuda):
    eager = _run(cuda, cuda_graph=False)
    graph = _run(cuda, cuda_graph=True)
    w = eager.last_weights.cpu()
    assert sorted(w.tolist()) == [0.0, 0.25, 0.25, 0.25, 0.25]
    assert torch.equal(w, gar.dnc_weights(eager.G, 1).cpu())
    assert torch.equal(eager.last_weights, graph.last_weights)
    assert torch.equal(eager.flat_model(), graph.flat_model())


def test_engine_layerwise_device_vs_segment_loop(cuda, monkeypatch):
    import garfield_amd.parallel.engine as E

    outs = []
    for dev_path in (False, True):
        monkeypatch.setattr(E, "LW_DEVICE", dev_path)
        eng = _run(cuda, layerwise=True, cuda_graph=False)
        assert (getattr(eng, "_lw", None) is not None) == dev_path
        outs.append((eng.flat_model().clone(), eng.last_weights.clone()))
    (p0, w0), (p1, w1) = outs
    assert w0.shape == w1.shape and w0.shape[0] >= 2 and w0.shape[1] == 5
    assert ((w1 > 0).sum(1) == 4).all() and torch.equal(w1, w0)
    assert_models_close(p1, p0)


@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_sharded_one_rank_vs_unsharded(cuda, layerwise):
    """The per-bucket partial Grams sum in another order than the whole-row Gram: the same selection."""
    outs = []
    for shard in (False, True):
        eng = _run(cuda, shard_gar=shard, layerwise=layerwise, cuda_graph=False)
        assert (eng._shard is not None) == shard
        outs.append((eng.flat_model().clone(), eng.last_weights.clone().float()))
    (p0, w0), (p1, w1) = outs
    assert w0.shape == w1.shape and torch.equal(w1, w0)
    assert_models_close(p1, p0)
