"""Geometric-median GAR on the GPU: the one-workgroup smoothed-Weiszfeld kernel on the Gram
(k_geomed_select) against the fp64 oracle, the non-finite policy, the smoothing floor, batched
launches, the n > 128 path and the engine (HIP graph, layer-wise device path, sharded)."""
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

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 16 / 17: the wave-per-row wrap; 64 / 65: the second lane column; 128: the LDS maximum
SHAPES = [(1, 64), (2, 100), (3, 100), (7, 1000), (16, 4096), (17, 5003), (64, 777), (65, 300), (128, 2000)]
# Per-weight relative bound against the fp64 oracle. Measured on an MI355X over SHAPES x DTYPES: the
# maximum is 9.14e-7 (n = 128, d = 2000, fp32; the fp32 Gram's rounding of D, the kernel itself
# iterates in fp64). The bound is 20 x that; it may never exceed 1e-4: needing more means a bug.
WEIGHT_RTOL = 20 * 9.14e-7


def separated(n, d, dtype, seed=0):
    """Rows with clearly distinct pairwise distances (distinct per-row noise scales), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(d, generator=g)
    scales = torch.linspace(0.5, 3.0, n)[torch.randperm(n, generator=g)]
    X = base + scales[:, None] * torch.randn(n, d, generator=g)
    return X.to(dtype)


@functools.lru_cache(maxsize=None)
def case(n, d, dtype):
    """(rows on the CPU, oracle weights, oracle output): computed once, shared, never modified."""
    X = separated(n, d, dtype)
    w = ref.geomed_weights(ref.pairwise_sqdist(X))
    return X, w, ref.combine(X, w)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs() / b.abs()).max().item()


def close(a, b, dtype):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() <= TOL[dtype] * max(b.abs().max().item(), 1.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_weights_and_output_match_oracle(cuda, native, n, d, dtype):
    X, w_ref, out_ref = case(n, d, dtype)
    G = X.to(cuda)
    w = gar.geomed_weights(G).clone()
    out = gar.geomed(G)
    torch.cuda.synchronize()
    assert w.dtype == torch.float32 and w.shape == (n,) and out.dtype == dtype and out.shape == (d,)
    err = relerr(w, w_ref)
    print(f"geomed weights n={n} d={d} {dtype}: max relative error {err:.3e}")
    assert abs(float(w.double().sum()) - 1.0) < 1e-6
    assert err <= WEIGHT_RTOL
    assert close(out, out_ref, dtype)
    # list input: same kernels on a row table
    out_l = gar.geomed([G[i].clone() for i in range(n)])
    assert close(out_l, out_ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(cuda, native, dtype):
    X = separated(9, 500, dtype).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    wk = ref.geomed_weights(ref.pairwise_sqdist(X[keep]))
    G = X.to(cuda)
    w = gar.geomed_weights(G).clone()
    out = gar.geomed(G)
    torch.cuda.synchronize()
    assert float(w[4]) == 0.0 and float(w[6]) == 0.0
    assert relerr(w[keep], wk) <= WEIGHT_RTOL
    assert torch.isfinite(out).all()
    assert close(out, ref.combine(X[keep], wk), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_smoothing_floor(cuda, native, dtype):
    """Three identical rows: the iterate sits on them, r falls under nu there and rounding noise in
    D decides b, so no per-weight comparison: finite weights summing to 1, the output on row 0."""
    g = torch.Generator().manual_seed(5)
    row = torch.randn(512, generator=g)
    X = torch.stack([row, row, row, torch.randn(512, generator=g), torch.randn(512, generator=g)]).to(dtype)
    G = X.to(cuda)
    w = gar.geomed_weights(G).clone()
    out = gar.geomed(G)
    torch.cuda.synchronize()
    assert torch.isfinite(w).all() and abs(float(w.double().sum()) - 1.0) < 1e-6
    assert close(out, X[0], dtype)


def test_batched_launch_equals_single_launches(cuda, native):
    n, L = 7, 3
    np_ = native.gram_padded(n)
    grams = []
    for s in range(L):
        rows = gar.prepare(separated(n, 900 + 13 * s, torch.float32, seed=s).to(cuda))
        grams.append(gar._gram_into(native, rows, gar.workspace(rows)).clone())
    batch = torch.cat(grams)
    assert batch.numel() == L * np_ * np_
    wb = torch.full((L, n), -1.0, device=cuda)
    db = torch.full((L, n), -1.0, device=cuda)
    native.gpu_geomed_select(batch, n, 32, 1e-6, wb, db, L)
    for s in range(L):
        w1 = torch.full((n,), -1.0, device=cuda)
        d1 = torch.full((n,), -1.0, device=cuda)
        native.gpu_geomed_select(grams[s], n, 32, 1e-6, w1, d1)
        assert torch.equal(w1, wb[s]) and torch.equal(d1, db[s])
        assert float(w1.min()) > 0.0 and float(d1.min()) > 0.0
    assert not torch.equal(wb[0], wb[1])
    with pytest.raises(RuntimeError):
        native.gpu_geomed_select(batch, n, 32, 1e-6, wb[:2], db, L)       # weights too small for the batch
    with pytest.raises(RuntimeError):
        native.gpu_geomed_select(batch, 129, 32, 1e-6, wb, db, 1)         # beyond the LDS matrix


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_path(cuda, native, dtype):
    """n = 130 > 128: large Gram kernel + the vectorised iteration on the device."""
    X, w_ref, out_ref = case(130, 300, dtype)
    G = X.to(cuda)
    w = gar.geomed_weights(G)
    out = gar.geomed(G)
    assert w.is_cuda and w.dtype == torch.float32
    err = relerr(w, w_ref)
    print(f"geomed weights n=130 d=300 {dtype} (large path): max relative error {err:.3e}")
    assert abs(float(w.double().sum()) - 1.0) < 1e-6
    assert err <= WEIGHT_RTOL
    assert close(out, out_ref, dtype)


def _run(cuda, steps=3, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar="geomed", f=1, workers_per_rank=5, byzantine={4: "reverse"}, lr=0.05, **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


# Models of two paths that compute the same weights up to the summation order of the Gram: rtol 1e-5
# and, for parameters near zero, the absolute floor the CPU test uses. Two such paths' weights differ
# by fp32 ulps (1e-7 relative), which moves an fp32 parameter by about lr * 1e-7 * |gradient| < 1e-8.
MODEL_ATOL = 1e-7


def assert_models_close(p1, p0):
    print("models: max abs difference", float((p1 - p0).abs().max()))
    torch.testing.assert_close(p1, p0, rtol=1e-5, atol=MODEL_ATOL)


def test_engine_graph_equals_eager(cuda):
    eager = _run(cuda, cuda_graph=False)
    graph = _run(cuda, cuda_graph=True)
    w = eager.last_weights.cpu()
    assert abs(float(w.double().sum()) - 1.0) < 1e-6 and int(w.argmin()) == 4
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
    assert ((w1.double().sum(1) - 1.0).abs() < 1e-5).all()
    print("layer-wise device vs loop: weights", relerr(w1, w0))
    assert relerr(w1, w0) <= WEIGHT_RTOL
    assert_models_close(p1, p0)


@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_sharded_one_rank_vs_unsharded(cuda, layerwise):
    """The per-bucket partial Grams sum in another order than the whole-row Gram: not bitwise."""
    outs = []
    for shard in (False, True):
        eng = _run(cuda, shard_gar=shard, layerwise=layerwise, cuda_graph=False)
        assert (eng._shard is not None) == shard
        outs.append((eng.flat_model().clone(), eng.last_weights.clone().float()))
    (p0, w0), (p1, w1) = outs
    assert w0.shape == w1.shape
    print("sharded vs unsharded: weights", relerr(w1, w0))
    assert relerr(w1, w0) <= WEIGHT_RTOL
    assert_models_close(p1, p0)
