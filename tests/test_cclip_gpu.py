"""Centered-clipping GAR on the GPU: the one-workgroup clipping kernel on the Gram (k_cclip_select)
against the fp64 oracle on the exact distances (fixed and data-derived radius; mean, Krum and centre
starts), the exact consequences of the semantics, the non-finite policy, batched launches, the
n > 128 path, centered clipping after nearest-neighbour mixing and the engine (HIP graph, layer-wise
device path)."""
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
# 16 / 17: the wave-per-row wrap; 64 / 65: the second lane column; 127 + a centre: the full LDS table
# with a basis-only row; 128: the LDS maximum (129 rows with a centre: the vectorised path); 130: the
# vectorised path
NS = [1, 2, 3, 16, 17, 64, 65, 127, 128, 130]
DS = [64, 2000]
GAP = 1e-4
# Seeds (found on the CPU, on the oracle alone) at which the Krum start's selection is well separated:
# see case(). Seed 0 unless listed.
SEEDS = {(127, 64, torch.float32): 1, (127, 64, torch.bfloat16): 1, (127, 64, torch.float16): 1}
# Per-weight relative bound against the fp64 oracle on the exact distances: 20 x the maximum measured on
# an MI355X over NS x DS x DTYPES, both radii and every start (the fp32 Gram's rounding of D; the kernel
# itself iterates in fp64). It may never exceed 1e-4: needing more means a bug. The measured maximum is
# 3.112e-6 (n = 17, d = 2000, fp32, centre start, data-derived radius), on the centre row: its weight is
# the product of the rounds' 1 - Λ/|V|, a difference of nearly equal numbers (2e-6 to 7e-5 here). Without
# the centre row the maximum is 4.56e-7. Log: profiles/r10/cclip/test_weights_error.log.
WEIGHT_MEASURED = 3.112e-6
WEIGHT_RTOL = 20 * WEIGHT_MEASURED
assert WEIGHT_RTOL <= 1e-4
# Centered clipping after the mix against the oracle chain: measured maximum 1.178e-7 (n = 3, d = 100, f = 1).
NNM_MEASURED = 1.178e-7
NNM_RTOL = 20 * NNM_MEASURED
assert NNM_RTOL <= 1e-4


def separated(n, d, dtype, seed=0):
    """Rows with clearly distinct pairwise distances (distinct per-row noise scales), on the CPU."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(d, generator=g)
    scales = torch.linspace(0.5, 3.0, n)[torch.randperm(n, generator=g)]
    X = base + scales[:, None] * torch.randn(n, d, generator=g)
    return X.to(dtype)


def latent(n, d, dtype, seed=0):
    """A latent geometry (4 factors + small noise), on the CPU: neighbour sets differ from row to row."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, 4, generator=g)
    P = torch.randn(4, d, generator=g)
    X = torch.randn(d, generator=g) + Z @ P + 0.05 * torch.randn(n, d, generator=g)
    return X.to(dtype)


def f_of(n):
    return max((n - 3) // 4, 0)


def krum_ok(n, f):
    """Whether the Krum start is tested against the oracle: Krum's own requirement n >= 2f + 3, and more
    than one neighbour in a score. At n = 3 (f = 0, one neighbour, one row selected) the two mutually
    nearest rows have the same score for every input, so no input separates the selection: n = 1, 2 and 3
    run the mean and centre starts."""
    return n >= 2 * f + 3 and n - f - 2 >= 2


def tau_of(d):
    """A fixed radius between the nearest and the farthest rows' distances to their mean."""
    return math.sqrt(d)


def krum_gap(D, f):
    """Relative gap of the Krum scores on either side of the selection of m = n - f - 2 rows."""
    n = D.shape[0]
    sc = ref.krum_scores(D, f)
    o = ref._order(sc)
    lo, hi = o[n - f - 3], o[n - f - 2]
    return (sc[hi] - sc[lo]) / sc[hi]


@functools.lru_cache(maxsize=None)
def case(n, d, dtype):
    """(rows and a centre on the CPU, {(start, tau): (oracle weights, oracle output)}): computed once,
    shared, never modified. Asserts the precondition of the Krum start ON THE ORACLE: the Krum scores on
    either side of the selection differ by >= GAP relative, so a selection flipped by the fp32 Gram
    cannot pass as a tolerance problem."""
    X = separated(n, d, dtype, SEEDS.get((n, d, dtype), 0))
    c = (0.5 * separated(1, d, torch.float32, 77)[0]).to(dtype)
    f = f_of(n)
    D = ref.pairwise_sqdist(X)
    Xc = torch.cat([X, c[None]])
    Dc = ref.pairwise_sqdist(Xc)
    starts = {"mean": (X, D, None), "center": (Xc, Dc, [0.0] * n + [1.0])}
    if krum_ok(n, f):
        assert krum_gap(D, f) >= GAP, (n, d, dtype)
        starts["krum"] = (X, D, ref.krum_weights(D, f))
    out = {}
    for start, (rows, dist, a0) in starts.items():
        for tau in (tau_of(d), None):
            w = ref.cclip_weights(dist, n, a0, tau, f, 3)
            out[(start, tau)] = (w, ref.combine(rows, w))
    return X, c, out


def relerr(a, b):
    """Maximum relative error; where the reference is exactly zero the value must be too."""
    a, b = a.double().cpu(), b.double().cpu()
    zero = b == 0
    assert (a[zero] == 0).all()
    return ((a - b).abs()[~zero] / b.abs()[~zero]).max().item() if (~zero).any() else 0.0


def close(a, b, dtype):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() <= TOL[dtype] * max(b.abs().max().item(), 1.0)


def own_gram(native, G):
    """The kernel's own Gram of G (pitch gram_padded(n)), cloned out of the workspace."""
    rows = gar.prepare(G)
    return gar._gram_into(native, rows, gar.workspace(rows)).clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_weights_and_output_match_oracle(cuda, native, n, d, dtype):
    X, c, oracle = case(n, d, dtype)
    G, cg = X.to(cuda), c.to(cuda)
    f = f_of(n)
    rows = [G[i].clone() for i in range(n)]
    for (start, tau), (w_ref, out_ref) in oracle.items():
        kw = {"center": cg} if start == "center" else {"start": start}
        w = gar.cclip_weights(G, f, tau, 3, **kw).clone()
        out = gar.cclip(G, f, tau, 3, **kw)
        torch.cuda.synchronize()
        nr = n + (start == "center")
        assert w.is_cuda and w.dtype == torch.float32 and w.shape == (nr,) and out.dtype == dtype and out.shape == (d,)
        err = relerr(w, w_ref)
        print(f"cclip weights n={n} d={d} {dtype} start={start} tau={tau}: max relative error {err:.3e}")
        assert abs(float(w.double().sum()) - 1.0) < 1e-6
        assert err <= WEIGHT_RTOL
        assert close(out, out_ref, dtype)
        # list input: the same kernels on a row table
        assert torch.equal(gar.cclip_weights(rows, f, tau, 3, **kw), w)
        # a start given as a weight tensor
        if start == "krum":
            assert torch.equal(gar.cclip_weights(G, f, tau, 3, start=gar.krum_weights(G, f).clone()), w)


@pytest.mark.parametrize("n", [3, 17, 65, 127, 128])
def test_one_round_with_a_huge_radius_is_exactly_uniform(cuda, native, n):
    X, c, _ = case(n, 64, torch.float32)
    G = X.to(cuda)
    uniform = torch.full((n,), 1.0 / n, dtype=torch.float64).float().to(cuda)
    one_hot = torch.zeros(n, device=cuda)
    one_hot[n // 2] = 1.0
    starts = ["mean", one_hot, torch.rand(n, generator=torch.Generator().manual_seed(n)).to(cuda)]
    starts.append("krum")   # any start gives the uniform weights, a tied Krum selection too
    for start in starts:
        assert torch.equal(gar.cclip_weights(G, f_of(n), 1e30, 1, start), uniform)
    w = gar.cclip_weights(G, f_of(n), 1e30, 1, center=c.to(cuda))
    assert torch.equal(w[:n], uniform) and float(w[n]) == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(cuda, native, dtype):
    X = separated(9, 500, dtype).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    G = X.to(cuda)
    for tau in (tau_of(500), None):
        wk = ref.cclip_weights(ref.pairwise_sqdist(X[keep]), 7, None, tau, 2, 3)
        w = gar.cclip_weights(G, 2, tau).clone()
        out = gar.cclip(G, 2, tau)
        torch.cuda.synchronize()
        assert float(w[4]) == 0.0 and float(w[6]) == 0.0
        assert relerr(w[keep], wk) <= WEIGHT_RTOL
        assert torch.isfinite(out).all()
        assert close(out, ref.combine(X[keep], wk), dtype)
        # a start that lies entirely on an invalid row falls back to uniform on the valid rows
        on_bad = torch.zeros(9, device=cuda)
        on_bad[4] = 1.0
        assert torch.equal(gar.cclip_weights(G, 2, tau, start=on_bad), w)
    # every row non-finite: uniform
    Y = separated(5, 64, dtype).clone()
    Y[:, 0] = math.nan
    assert torch.equal(gar.cclip_weights(Y.to(cuda), 1), torch.full((5,), 0.2, device=cuda))


def test_batched_launch_equals_single_launches(cuda, native):
    n, f, L = 17, 3, 3
    np_ = native.gram_padded(n)
    grams = [own_gram(native, separated(n, 900 + 13 * s, torch.float32, seed=s).to(cuda)) for s in range(L)]
    batch = torch.cat(grams)
    assert batch.numel() == L * np_ * np_
    for tau, start in ((0.0, "krum"), (30.0, "krum"), (0.0, None), (30.0, None)):
        wb = torch.full((L, n), -1.0, device=cuda)
        db = torch.full((L, n), -1.0, device=cuda)
        if start == "krum":   # the batched Krum selection writes every problem's start in place
            native.gpu_krum_select(batch, n, f, n - f - 2, wb, torch.empty((L, n), dtype=torch.int32, device=cuda),
                                   torch.empty((L, n), device=cuda), L)
        native.gpu_cclip_select(batch, n, n, wb if start else None, tau, f, 3, wb, db, L)
        for s in range(L):
            w1 = torch.full((n,), -1.0, device=cuda)
            d1 = torch.full((n,), -1.0, device=cuda)
            if start == "krum":
                native.gpu_krum_select(grams[s], n, f, n - f - 2, w1, torch.empty(n, dtype=torch.int32, device=cuda),
                                       torch.empty(n, device=cuda))
            native.gpu_cclip_select(grams[s], n, n, w1 if start else None, tau, f, 3, w1, d1)
            assert torch.equal(w1, wb[s]) and torch.equal(d1, db[s])
            assert float(w1.min()) > 0.0 and float(d1.min()) > 0.0
        assert not torch.equal(wb[0], wb[1])
    with pytest.raises(RuntimeError):
        native.gpu_cclip_select(batch, n, n, None, 0.0, f, 3, wb[:2], db, L)      # weights too small for the batch
    with pytest.raises(RuntimeError):
        native.gpu_cclip_select(batch, 129, 129, None, 0.0, f, 3, wb, db, 1)      # beyond the LDS matrix
    with pytest.raises(RuntimeError):
        native.gpu_cclip_select(batch, n, n + 1, None, 0.0, f, 3, wb, db, 1)      # nw <= n
    with pytest.raises(RuntimeError):
        native.gpu_cclip_select(batch, n, n, None, 0.0, f, 0, wb, db, 1)          # iters >= 1


@pytest.mark.parametrize("n", [17, 128, 130])
def test_two_runs_are_bit_identical(cuda, native, n):
    X, c, _ = case(n, 2000, torch.bfloat16)
    G = X.to(cuda)
    for kw in ({"start": "krum"}, {"center": c.to(cuda)}, {"start": "mean", "tau": 40.0}):
        a = gar.cclip_weights(G, f_of(n), **kw).clone()
        oa = gar.cclip(G, f_of(n), **kw)
        b = gar.cclip_weights(G, f_of(n), **kw).clone()
        ob = gar.cclip(G, f_of(n), **kw)
        assert torch.equal(a, b) and torch.equal(oa, ob)


NNM_SHAPES = [(3, 100, 1), (17, 5003, 4), (128, 2000, 31)]
# the seeds at which the oracle's neighbour sets and Krum selection after the mix are well separated
NNM_SEEDS = {(17, 5003, 4, torch.float32): 1, (17, 5003, 4, torch.bfloat16): 1, (17, 5003, 4, torch.float16): 1,
             (128, 2000, 31, torch.float32): 2, (128, 2000, 31, torch.bfloat16): 5, (128, 2000, 31, torch.float16): 2}


@functools.lru_cache(maxsize=None)
def nnm_case(n, d, f, dtype):
    """(rows, {(start, tau): oracle row weights}) of the chain nnm_distances -> cclip_weights ->
    nnm_row_weights. Asserts ON THE ORACLE that every row's c-th and (c + 1)-th nearest distances differ
    by >= GAP relative, and so do the Krum scores of the mixed rows on either side of the selection."""
    X = latent(n, d, dtype, NNM_SEEDS.get((n, d, f, dtype), 0))
    D = ref.pairwise_sqdist(X)
    c = n - f
    for i in range(n):
        o = sorted(float(D[i, j]) for j in range(n) if j != i)
        inner = o[c - 2] if c >= 2 else 0.0
        assert (o[c - 1] - inner) / o[c - 1] >= GAP, (n, d, f, dtype, i)
    sets, Dm = ref.nnm_distances(D, f)
    starts = {"mean": None}
    if krum_ok(n, f):
        assert krum_gap(Dm, f) >= GAP, (n, d, f, dtype)
        starts["krum"] = ref.krum_weights(Dm, f)
    tau = 0.5 * math.sqrt(float(Dm[torch.isfinite(Dm)].median()))
    out = {}
    for start, a0 in starts.items():
        for t in (tau, None):
            out[(start, t)] = ref.nnm_row_weights(sets, ref.cclip_weights(Dm, n, a0, t, f, 3))
    return X, out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", NNM_SHAPES)
def test_nnm_cclip_matches_oracle_chain(cuda, native, n, d, f, dtype):
    X, oracle = nnm_case(n, d, f, dtype)
    G = X.to(cuda)
    for (start, tau), w_ref in oracle.items():
        w = gar.nnm_weights(G, f, "cclip", tau=tau, start=start).clone()
        out = gar.nnm(G, f, "cclip", tau=tau, start=start)
        torch.cuda.synchronize()
        err = relerr(w, w_ref)
        print(f"nnm-cclip weights n={n} d={d} f={f} {dtype} start={start} tau={tau}: max relative error {err:.3e}")
        assert w.shape == (n,) and abs(float(w.double().sum()) - 1.0) < 1e-6
        assert err <= NNM_RTOL
        assert close(out, ref.combine(X, w_ref.double()), dtype)
    with pytest.raises(ValueError):
        gar.cclip_weights(G, f, center=G[0], pre="nnm")


def _run(cuda, steps=3, gar_kwargs=None, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar="cclip", f=1, workers_per_rank=5, byzantine={4: "reverse"}, lr=0.05,
                       gar_kwargs=gar_kwargs or {}, **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("gkw", [{}, {"start": "krum"}, {"tau": 0.05, "iters": 2}])
def test_engine_graph_equals_eager(cuda, gkw):
    eager = _run(cuda, gar_kwargs=gkw, cuda_graph=False)
    graph = _run(cuda, gar_kwargs=gkw, cuda_graph=True)
    w = eager.last_weights.cpu()
    assert abs(float(w.double().sum()) - 1.0) < 1e-6 and float(w.min()) >= 0.0
    assert torch.equal(eager.last_weights, graph.last_weights)
    assert torch.equal(eager.flat_model(), graph.flat_model())
    assert torch.equal(eager.last_weights, gar.cclip_weights(eager.G, 1, gkw.get("tau"), gkw.get("iters", 3),
                                                             gkw.get("start", "mean")))


def test_engine_nnm_graph_equals_eager(cuda):
    eager = _run(cuda, gar_kwargs={"start": "krum"}, cuda_graph=False, pre_aggregation="nnm")
    graph = _run(cuda, gar_kwargs={"start": "krum"}, cuda_graph=True, pre_aggregation="nnm")
    assert torch.equal(eager.last_weights, graph.last_weights)
    assert torch.equal(eager.flat_model(), graph.flat_model())
    assert torch.equal(eager.last_weights, gar.nnm_weights(eager.G, 1, "cclip", start="krum"))


# Models of two paths that compute the same weights up to the summation order of the Gram: the
# tolerance the geometric median's test of equivalent paths uses.
def assert_models_close(p1, p0):
    print("models: max abs difference", float((p1 - p0).abs().max()))
    torch.testing.assert_close(p1, p0, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("gkw", [{}, {"start": "krum"}])
def test_engine_layerwise_device_vs_segment_loop(cuda, monkeypatch, gkw):
    import garfield_amd.parallel.engine as E

    outs = []
    for dev_path in (False, True):
        monkeypatch.setattr(E, "LW_DEVICE", dev_path)
        eng = _run(cuda, gar_kwargs=gkw, layerwise=True, cuda_graph=False)
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
        eng = _run(cuda, gar_kwargs={"start": "krum"}, shard_gar=shard, layerwise=layerwise, cuda_graph=False)
        assert (eng._shard is not None) == shard
        outs.append((eng.flat_model().clone(), eng.last_weights.clone().float()))
    (p0, w0), (p1, w1) = outs
    assert w0.shape == w1.shape
    print("sharded vs unsharded: weights", relerr(w1, w0))
    assert relerr(w1, w0) <= WEIGHT_RTOL
    assert_models_close(p1, p0)
