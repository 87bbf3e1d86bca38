"""DnC spectral-filtering GAR (power iteration on the doubly centred pairwise distances) on the CPU: the
fp64 oracle on D against the SVD scores on the vectors, the C++ weights and scores against the oracle,
the exact consequences of the semantics (docs/GAR_SEMANTICS.md "Spectral filtering"), the registry, the
engine (flat / layer-wise) and the sharded exchange on gloo.

Inputs: attacked(n, f, d, dtype, seed): rows N(0, I), the last f rows shifted by one common 3 N(0, I);
the oracle sees the rows after the cast to dtype. Every case that compares a selection or scores first
asserts the two preconditions on the oracle (a spectral gap lambda_2 <= 0.5 lambda_1 of K and a relative
gap >= 1e-4 between the last kept and the first dropped score): f >= 1 everywhere here, since without
colluders a cloud of N(0, I) rows has no dominant direction."""
import functools
import math
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from garfield_amd import aggregators
from garfield_amd.models import build_model
from garfield_amd.ops import gar
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

SIZES = (3, 4, 5, 8, 16, 17, 33, 64, 65, 127, 128)
DIMS = (64, 2000)


def attacked(n, f, d, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(1000 * n + d + seed)
    X = torch.randn(n, d, generator=g)
    if f:
        X[n - f:] += 3.0 * torch.randn(d, generator=g)
    return X.to(dtype)


def kept(n, ids):
    """The fp32 weight vector with 1 / |ids| on ``ids``."""
    w = torch.zeros(n, dtype=torch.float64)
    w[list(ids)] = 1.0 / len(ids)
    return w.float()


def f_of(n):
    return max(1, (n - 1) // 4)


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
def case(n, d):
    """(X, D, fp64 scores, w, fp32 scores) of attacked(n, f_of(n), d): computed once, shared, never modified."""
    f = f_of(n)
    X = attacked(n, f, d)
    D = ref.pairwise_sqdist(X)
    assert_preconditions(D, n - f)
    w, s = ref.dnc_weights(D, n - f)
    return X, D, ref.dnc_scores(D), w, s


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_oracle_on_distances_equals_svd_on_vectors(n, d):
    X, D, s64, _, _ = case(n, d)
    sv = ref.dnc_svd_scores(X)
    err = float((s64 - sv).abs().max() / sv.max())
    print(f"n={n} d={d} identity error {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_cpu_matches_oracle(native, n, d):
    X, D, _, w, s = case(n, d)
    f = f_of(n)
    wc, sc = native.cpu_dnc_weights(D, n - f, 16)
    assert wc.dtype == torch.float32 and sc.dtype == torch.float32
    assert torch.equal(wc, w)
    assert float((sc.double() - s.double()).abs().max() / s.double().max()) <= 1e-6
    # the public entry (C++ pairwise distances) selects the same rows
    assert torch.equal(gar.dnc_weights(X, f), w)
    # the f shifted rows get weight 0, the rest 1 / (n - f), exactly
    expect = torch.zeros(n, dtype=torch.float64)
    expect[: n - f] = 1.0 / (n - f)
    assert torch.equal(w, expect.float())


def test_large_path_matches_oracle():
    """n > 128: the vectorised rounds on the Gram, rank masks in place of a host-side kv."""
    n, f = 130, 32
    X = attacked(n, f, 300)
    D = ref.pairwise_sqdist(X)
    assert_preconditions(D, n - f)
    w, s = ref.dnc_weights(D, n - f)
    assert torch.equal(gar.dnc_weights(X, f), w)
    wg, sg = gar.dnc_weights_from_gram(X.double() @ X.double().T, n - f, 16, with_scores=True)
    assert torch.equal(wg, w)
    assert float((sg.double() - s.double()).abs().max() / s.double().max()) <= 1e-6
    # no valid row (a single gradient): uniform, zero scores
    w1, s1 = gar.dnc_weights_from_gram(torch.full((1, 1), 2.0), 1, 16, with_scores=True)
    assert w1.tolist() == [1.0] and s1.tolist() == [0.0]
    # non-finite rows: weight exactly 0, score +inf, charged to the budget
    g = X[:9].double() @ X[:9].double().T
    g[2, :] = math.nan
    g[:, 2] = math.nan
    w9, s9 = gar.dnc_weights_from_gram(g, 7, 16, with_scores=True)
    D9 = ref.pairwise_sqdist(X[:9])
    D9[2, :] = math.inf
    D9[:, 2] = math.inf
    wr, sr = ref.dnc_weights(D9, 7)
    assert torch.equal(w9, wr) and float(w9[2]) == 0.0 and math.isinf(float(s9[2]))
    assert int((w9 > 0).sum()) == 7


def test_identical_rows():
    X = torch.randn(1, 50, generator=torch.Generator().manual_seed(3)).repeat(7, 1)
    D = ref.pairwise_sqdist(X)
    w, s = ref.dnc_weights(D, 5)
    assert torch.equal(s, torch.zeros(7)) and torch.equal(w, kept(7, range(5)))
    assert torch.equal(gar.dnc_weights(X, 2), w)


def test_symmetric_clusters(native):
    """Two clusters at +a and -a: equal scores, ties broken by index."""
    X = torch.zeros(8, 4)
    X[0::2, 0] = 1.0
    X[1::2, 0] = -1.0
    D = ref.pairwise_sqdist(X)
    for fn in (lambda: ref.dnc_weights(D, 5), lambda: native.cpu_dnc_weights(D, 5, 16)):
        w, s = fn()
        assert torch.equal(s, torch.full((8,), float(s[0]))) and float(s[0]) == 1.0
        assert torch.equal(w, kept(8, range(5)))


def test_one_and_two_rows(native):
    for n in (1, 2):
        X = attacked(n, 0, 40)
        D = ref.pairwise_sqdist(X)
        for w, s in (ref.dnc_weights(D, n), native.cpu_dnc_weights(D, n, 16)):
            assert torch.equal(w, kept(n, range(n)))
            if n == 1:
                assert s.tolist() == [0.0]
            else:   # each row projects half the distance on the line through both
                assert abs(float(s[0]) - float(D[0, 1]) / 4) <= 1e-6 * float(D[0, 1]) and float(s[0]) == float(s[1])
        assert torch.equal(gar.dnc_weights(X, 0), kept(n, range(n)))
    X = attacked(2, 0, 40)
    assert gar.dnc_weights(X, 0, m=1).tolist() == [1.0, 0.0]   # equal scores: the lower index
    assert torch.equal(gar.dnc(attacked(1, 0, 40), 0), attacked(1, 0, 40)[0])


def test_non_finite_rows(native):
    X = attacked(9, 1, 500)
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    D = ref.pairwise_sqdist(X)
    assert_preconditions(ref.pairwise_sqdist(X[keep]), 6)
    for f, sel in ((2, keep), (3, keep[:-1])):   # f = 2: the budget is used up by the two non-finite rows
        m = 9 - f
        w, s = ref.dnc_weights(D, m)
        assert torch.equal(w, kept(9, sel))
        assert math.isinf(float(s[4])) and math.isinf(float(s[6])) and torch.isfinite(s[keep]).all()
        # the valid rows are scored as if the non-finite rows were absent
        sk = ref.dnc_weights(ref.pairwise_sqdist(X[keep]), len(sel))[1]
        assert float((s[keep].double() - sk.double()).abs().max() / sk.double().max()) <= 1e-6
        wc, sc = native.cpu_dnc_weights(D, m, 16)
        assert torch.equal(wc, w) and torch.equal(torch.isinf(sc), torch.isinf(s))
        assert torch.equal(gar.dnc_weights(X, f), w)
        out = gar.dnc(X, f)
        assert torch.isfinite(out).all()
        ex = ref.combine(X[sel], torch.full((len(sel),), 1.0 / len(sel), dtype=torch.float64))
        assert (out.double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())
    # every pair non-finite: uniform 1/n, zero scores
    Dinf = torch.full((3, 3), math.inf, dtype=torch.float64)
    for w, s in (ref.dnc_weights(Dinf, 2), native.cpu_dnc_weights(Dinf, 2, 16)):
        assert torch.equal(w, torch.full((3,), 1.0 / 3, dtype=torch.float64).float()) and s.tolist() == [0.0] * 3


def test_m_equals_n_keeps_all_valid():
    X = attacked(9, 2, 200)
    assert torch.equal(gar.dnc_weights(X, 0, m=9), torch.full((9,), 1.0 / 9, dtype=torch.float64).float())
    X[5, 0] = math.nan
    w = gar.dnc_weights(X, 0, m=9)
    assert float(w[5]) == 0.0 and torch.equal(w[[0, 1, 2, 3, 4, 6, 7, 8]], torch.full((8,), 0.125))


def test_check_messages():
    for name in ("dnc", "native-dnc"):
        rule = aggregators.gars[name]
        assert callable(rule.check) and callable(rule.checked) and callable(rule.influence)
        assert rule.upper_bound is None
    check = aggregators.gars["dnc"].check
    G = attacked(9, 2, 50)
    assert "f = 5" in check(gradients=G, f=5) and "f = -1" in check(gradients=G, f=-1)
    assert check(gradients=G, f=4) is None and check(gradients=G, f=0) is None
    assert "m = 0" in check(gradients=G, f=2, m=0) and "m = 10" in check(gradients=G, f=2, m=10)
    assert check(gradients=G, f=2, m=9) is None and check(gradients=G, f=2, m=1) is None
    for bad in (0, -1, 1.5, True, None):
        assert "iters" in check(gradients=G, f=2, iters=bad)
    assert check(gradients=G, f=2, iters=1) is None
    for call in (lambda: gar.dnc_weights(G, 5), lambda: gar.dnc_weights(G, 2, m=10), lambda: gar.dnc(G, 2, iters=0),
                 lambda: gar.dnc(G, 2, iters=2.0)):
        with pytest.raises(ValueError):
            call()


def test_determinism(native):
    X, D, _, w, s = case(33, 2000)
    w2, s2 = ref.dnc_weights(D, 33 - f_of(33))
    assert torch.equal(w, w2) and torch.equal(s, s2)
    a, b = native.cpu_dnc_weights(D, 25, 16), native.cpu_dnc_weights(D.clone(), 25, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(gar.dnc(X, 8), gar.dnc(X.clone(), 8))


def test_calling_contract_and_influence(native):
    X = attacked(9, 2, 700)
    assert_preconditions(ref.pairwise_sqdist(X), 7)
    rule = aggregators.gars["dnc"]
    a = rule(gradients=X, f=2)
    assert torch.equal(a, rule(gradients=[X[i].clone() for i in range(9)], f=2))
    assert a.dtype == torch.float32 and a.shape == (700,)
    assert torch.equal(rule(gradients=X, f=2, unknown_option=3), a) and torch.equal(a, gar.aggregate("dnc", X, f=2))
    ex = ref.dnc(X, 2)
    assert (a.double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())
    Xb = X.bfloat16()
    ob = rule(gradients=Xb, f=2)
    eb = ref.dnc(Xb, 2)
    assert ob.dtype == torch.bfloat16 and (ob.double() - eb).abs().max().item() <= 2e-2 * max(1.0, eb.abs().max().item())
    rows = list(X)
    assert rule.influence(rows[:7], rows[7:], f=2) == 0.0
    assert abs(rule.influence(rows[:7], rows[7:], f=0, m=9) - 2.0 / 9) < 1e-6
    # fewer rounds are another rule instance, not a silent default
    inst = aggregators.instantiate("dnc", 9, 2, [])
    assert torch.equal(inst.aggregate(X), a) and torch.equal(inst.aggregate(rows), a)
    assert torch.equal(aggregators.instantiate("dnc", 9, 2, ["m:5", "iters:3"]).aggregate(X),
                       rule(gradients=X, f=2, m=5, iters=3))


def test_listings():
    from garfield_amd.aggregators import classreg
    from garfield_amd.apps import gar_bench
    from garfield_amd.grpcnet import aggregator
    from garfield_amd.parallel import engine, sharded

    assert "dnc" in gar.RULES and "dnc" in gar_bench.RULES and gar_bench.default_f("dnc", 8) == 2
    assert classreg.DnCGAR.rule_name == "dnc" and aggregator._RULES["DnC"] == "dnc"
    assert "dnc" in engine.WEIGHTED_RULES and "dnc" in engine.LAYERWISE_RULES
    assert "dnc" in sharded.DISTANCE_RULES and "dnc" in sharded.LAYERWISE_RULES and "dnc" in sharded.SUPPORTED
    assert sharded.layerwise_device_ok("dnc", 128, 2) and not sharded.layerwise_device_ok("dnc", 129, 2)
    assert "dnc" not in gar.NNM_RULES
    mk = lambda **kw: RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                         EngineConfig(gar="dnc", workers_per_rank=8, **kw))
    with pytest.raises(ValueError, match="pre_aggregation='nnm' is not yet supported"):
        mk(f=2, pre_aggregation="nnm")
    with pytest.raises(ValueError):   # the engine runs the registry's check: n >= 2f + 1
        mk(f=4)
    with pytest.raises(ValueError, match="iters"):
        mk(f=2, gar_kwargs={"iters": 0})


@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_cpu(layerwise):
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="dnc", f=2, workers_per_rank=8, byzantine={7: "reverse"},
                                          layerwise=layerwise))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    before = eng.flat_model().clone()
    for _ in range(2):
        eng.step(b)
        w = eng.last_weights
        assert w is not None
        w = w.reshape(-1, 8)
        segs = sorted(zip(eng.flat.offsets, eng.flat.numels))
        assert w.shape[0] == (len(segs) if layerwise else 1)
        assert ((w == 0) | (w == torch.tensor(1.0 / 6, dtype=torch.float64).float())).all() and ((w > 0).sum(1) == 6).all()
        if layerwise:   # every segment's weights are the rule on that segment's slice of the rows
            for (off, numel), ws in zip(segs, w):
                assert torch.equal(ws, gar.dnc_weights(eng.G[:, off:off + numel].float(), 2))
        else:
            assert torch.equal(w[0], gar.dnc_weights(eng.G.float(), 2))
    assert torch.isfinite(eng.flat_model()).all() and not torch.equal(eng.flat_model(), before)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, outdir, shard):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from garfield_amd.parallel.comm import init_distributed, shutdown

    ctx = init_distributed(backend="gloo", device="cpu")
    out = {}
    for layerwise in (False, True):
        torch.manual_seed(0)
        eng = RobustDataParallel(build_model("mlp"), F.nll_loss, ctx,
                                 EngineConfig(gar="dnc", f=1, workers_per_rank=3, byzantine={5: "reverse"},
                                              shard_gar=shard, lr=0.05, layerwise=layerwise))
        assert (eng._shard is not None) == shard
        b = synthetic_batches(3, 8, (1, 28, 28), 10, "cpu", seed=rank)
        for _ in range(2):
            eng.step(b)
        out[layerwise] = {"flat": eng.flat_model().clone(), "sum": eng.replica_checksum(),
                          "w": eng.last_weights.clone().float()}
    torch.save(out, os.path.join(outdir, f"{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_two_rank_sharded_equals_redundant():
    """2 gloo ranks x 3 workers: the selection runs on the summed distances, the weights are 0 or 1 / kv,
    so sharded and redundant agree bit for bit, flat and layer-wise, on every rank."""
    world = 2
    with tempfile.TemporaryDirectory() as d:
        for shard in (False, True):
            mp.spawn(_rank_worker, args=(world, free_port(), d, shard), nprocs=world, join=True)
        res = {(s, r): torch.load(os.path.join(d, f"{s}r{r}.pt"), weights_only=True)
               for s in (0, 1) for r in range(world)}
        for layerwise in (False, True):
            for s in (0, 1):
                assert res[(s, 1)][layerwise]["sum"] == res[(s, 0)][layerwise]["sum"], (layerwise, s)
                assert torch.equal(res[(s, 1)][layerwise]["flat"], res[(s, 0)][layerwise]["flat"]), (layerwise, s)
            red, sh = res[(0, 0)][layerwise], res[(1, 0)][layerwise]
            assert sh["w"].numel() >= 6 and torch.equal(sh["w"].reshape(-1), red["w"].reshape(-1)), layerwise
            assert int((sh["w"].reshape(-1, 6) > 0).sum(1).min()) == 5
            assert torch.equal(sh["flat"], red["flat"]), layerwise
