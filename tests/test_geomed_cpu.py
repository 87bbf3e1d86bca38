"""Geometric-median GAR (smoothed Weiszfeld iterated on the pairwise distances) on the CPU: the
registry contract, the fp64 oracle against a direct Weiszfeld on the vectors, the C++ weights, the
non-finite policy, robustness, the engine (flat / layer-wise) and the sharded exchange on gloo."""
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


def separated(n, d, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(d, generator=g)
    scales = torch.linspace(0.5, 3.0, n)[torch.randperm(n, generator=g)]
    return (base + scales[:, None] * torch.randn(n, d, generator=g)).to(dtype)


def weiszfeld(X, iters=32, nu=1e-6):
    """Smoothed Weiszfeld on the vectors themselves (fp64): the weights of the iterate."""
    X = X.double()
    n = X.shape[0]
    a = torch.full((n,), 1.0 / n, dtype=torch.float64)
    for _ in range(iters):
        z = a @ X
        b = 1.0 / (X - z).norm(dim=1).clamp(min=nu)
        a = b / b.sum()
    return a


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs() / b.abs()).max().item()


def test_registry_contract():
    for name in ("geomed", "native-geomed"):
        assert name in aggregators.gars
        rule = aggregators.gars[name]
        assert callable(rule.check) and callable(rule.checked) and callable(rule.influence)
        assert rule.upper_bound is None
    check = aggregators.gars["geomed"].check
    G = separated(9, 50)
    assert check(gradients=G, f=5) is not None
    assert check(gradients=G, f=4) is None
    assert check(gradients=G, f=2, iters=0) is not None
    assert check(gradients=G, f=2, nu=0) is not None
    assert check(gradients=G, f=2, nu=0.0) is not None
    assert check(gradients=G, f=-1) is not None
    assert check(gradients=G, f=2, iters=4, nu=1e-3) is None


@pytest.mark.parametrize("n,d", [(3, 100), (7, 2000), (33, 500)])
def test_oracle_equals_direct_weiszfeld(n, d):
    X = separated(n, d)
    w = ref.geomed_weights(ref.pairwise_sqdist(X))
    direct = weiszfeld(X)
    assert abs(float(w.sum()) - 1.0) < 1e-12
    assert relerr(w, direct) < 1e-9


@pytest.mark.parametrize("n,d", [(3, 100), (7, 2000), (33, 500)])
def test_cpu_weights_match_oracle(native, n, d):
    X = separated(n, d)
    D = ref.pairwise_sqdist(X)
    w = native.cpu_geomed_weights(D, 32, 1e-6)
    assert w.dtype == torch.float32
    assert relerr(w, ref.geomed_weights(D)) < 1e-6   # fp32 rounding of the output
    assert relerr(gar.geomed_weights(X), ref.geomed_weights(D)) < 1e-6


def test_calling_contract(native):
    X = separated(9, 700)
    rule = aggregators.gars["geomed"]
    a = rule(gradients=X, f=2)
    b = rule(gradients=[X[i].clone() for i in range(9)], f=2)
    assert torch.equal(a, b)
    assert a.dtype == torch.float32 and a.shape == (700,)
    assert torch.equal(rule(gradients=X, f=2, unknown_option=3, m=5), a)
    rows = [X[i].clone() for i in range(9)]
    out = rule(gradients=rows, f=2)
    assert all(out.data_ptr() != r.data_ptr() for r in rows) and out.data_ptr() != X.data_ptr()
    one = [X[0].clone()]
    o1 = rule(gradients=one, f=0)
    assert o1.data_ptr() != one[0].data_ptr() and torch.equal(o1, one[0])
    Xb = X.bfloat16()
    ob = rule(gradients=Xb, f=2)
    assert ob.dtype == torch.bfloat16
    expect = ref.geomed(Xb)
    assert (ob.double() - expect).abs().max().item() <= 2e-2 * max(1.0, expect.abs().max().item())
    # the aggregate against the oracle (fp32 combine)
    assert (a.double() - ref.geomed(X)).abs().max().item() <= 1e-5 * max(1.0, ref.geomed(X).abs().max().item())


def test_non_finite_rows(native):
    X = separated(9, 500)
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    w = gar.geomed_weights(X)
    assert float(w[4]) == 0.0 and float(w[6]) == 0.0
    keep = [0, 1, 2, 3, 5, 7, 8]
    wk = ref.geomed_weights(ref.pairwise_sqdist(X[keep]))
    assert relerr(w[keep], wk) < 1e-6
    assert torch.equal(ref.geomed_weights(ref.pairwise_sqdist(X))[[4, 6]], torch.zeros(2, dtype=torch.float64))
    assert relerr(ref.geomed_weights(ref.pairwise_sqdist(X))[keep], wk) < 1e-12
    out = gar.geomed(X)
    assert torch.isfinite(out).all()
    expect = ref.combine(X[keep], wk)
    assert (out.double() - expect).abs().max().item() <= 1e-5 * max(1.0, expect.abs().max().item())
    # the C++ selection on a distance matrix directly: a row of +inf gets 0, a lone row 1
    D = ref.pairwise_sqdist(separated(11, 300))
    D[3, :] = math.inf
    D[:, 3] = math.inf
    wc = native.cpu_geomed_weights(D, 32, 1e-6)
    assert float(wc[3]) == 0.0 and abs(float(wc.double().sum()) - 1.0) < 1e-6
    assert relerr(wc[[i for i in range(11) if i != 3]], ref.geomed_weights(D)[[i for i in range(11) if i != 3]]) < 1e-6
    assert native.cpu_geomed_weights(torch.full((1, 1), math.inf, dtype=torch.float64), 32, 1e-6).tolist() == [1.0]
    assert gar.geomed_weights(separated(1, 40)).tolist() == [1.0]
    assert gar.geomed_weights(separated(2, 40)).tolist() == [0.5, 0.5]
    assert ref.geomed_weights(ref.pairwise_sqdist(separated(1, 40))).tolist() == [1.0]
    assert ref.geomed_weights(ref.pairwise_sqdist(separated(2, 40))).tolist() == [0.5, 0.5]


def test_large_path_matches_oracle():
    """n > 128: the vectorised form on the Gram."""
    X = separated(130, 300)
    w = gar.geomed_weights(X)
    assert w.dtype == torch.float32 and abs(float(w.double().sum()) - 1.0) < 1e-6
    assert relerr(w, ref.geomed_weights(ref.pairwise_sqdist(X))) < 1e-4
    # no valid row (a single gradient): uniform
    assert gar.geomed_weights_from_gram(torch.full((1, 1), 2.0)).tolist() == [1.0]
    # a non-finite row gets weight exactly 0 here too
    g = X[:5].double() @ X[:5].double().T
    g[2, :] = math.nan
    g[:, 2] = math.nan
    w5 = gar.geomed_weights_from_gram(g)
    assert float(w5[2]) == 0.0 and abs(float(w5.double().sum()) - 1.0) < 1e-6


def test_robustness():
    X = separated(10, 2000)
    honest_mean = X[:8].double().mean(0)
    X[8] = -50.0 * X[8]
    X[9] = X[9] + 1000.0
    w = gar.geomed_weights(X).double()
    print("byzantine weights", float(w[8]), float(w[9]), "honest min", float(w[:8].min()))
    assert float(w[8]) < float(w[:8].min()) and float(w[9]) < float(w[:8].min())
    infl = aggregators.gars["geomed"].influence(list(X[:8]), list(X[8:]), f=2)
    assert abs(infl - float(w[8] + w[9])) < 1e-6 and infl < 0.01
    out = gar.geomed(X).double()
    avg = X.double().mean(0)
    assert (out - honest_mean).norm() * 10 <= (avg - honest_mean).norm()


@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_cpu(layerwise):
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="geomed", f=2, workers_per_rank=8, byzantine={7: "reverse"},
                                          layerwise=layerwise))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    for _ in range(2):
        eng.step(b)
        w = eng.last_weights
        assert w is not None
        w = w.double().reshape(-1, 8)
        assert w.shape[0] == (len(list(eng.flat.offsets)) if layerwise else 1)
        assert ((w.sum(1) - 1.0).abs() < 1e-5).all()
        assert (w[:, 7:8] < w[:, :7]).all(), w
    assert torch.isfinite(eng.flat_model()).all()


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
                                 EngineConfig(gar="geomed", f=2, workers_per_rank=2, byzantine={3: "reverse"},
                                              shard_gar=shard, lr=0.05, layerwise=layerwise))
        assert (eng._shard is not None) == shard
        b = synthetic_batches(2, 8, (1, 28, 28), 10, "cpu", seed=rank)
        for _ in range(2):
            eng.step(b)
        out[layerwise] = {"flat": eng.flat_model().clone(), "sum": eng.replica_checksum(),
                          "w": eng.last_weights.clone().float()}
    torch.save(out, os.path.join(outdir, f"{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_four_rank_sharded_vs_redundant():
    """4 gloo ranks x 2 workers. Sharded replicas are bitwise identical (every rank iterates on the
    same summed distances). Sharded vs redundant is not bitwise: the weights are continuous and the
    partial distances are summed in another order (a few ulps of D; the iteration is well
    conditioned away from nu), so 1e-5 relative leaves more than 100x margin."""
    world = 4
    with tempfile.TemporaryDirectory() as d:
        for shard in (False, True):
            mp.spawn(_rank_worker, args=(world, free_port(), d, shard), nprocs=world, join=True)
        res = {(s, r): torch.load(os.path.join(d, f"{s}r{r}.pt"), weights_only=True)
               for s in (0, 1) for r in range(world)}
        for layerwise in (False, True):
            for s in (0, 1):
                for r in range(1, world):
                    assert res[(s, r)][layerwise]["sum"] == res[(s, 0)][layerwise]["sum"], (layerwise, s, r)
                    assert torch.equal(res[(s, r)][layerwise]["flat"], res[(s, 0)][layerwise]["flat"]), (layerwise, s, r)
            red, sh = res[(0, 0)][layerwise], res[(1, 0)][layerwise]
            assert sh["w"].shape == red["w"].shape and sh["w"].numel() >= 8
            print("layerwise", layerwise, "weights rel", relerr(sh["w"], red["w"]))
            assert relerr(sh["w"], red["w"]) < 1e-5
            torch.testing.assert_close(sh["flat"], red["flat"], rtol=1e-5, atol=1e-7)


def test_routing_limits():
    from garfield_amd.parallel import engine, sharded

    assert sharded.layerwise_device_ok("geomed", 128, 2) and not sharded.layerwise_device_ok("geomed", 129, 2)
    assert "geomed" in sharded.SUPPORTED and "geomed" in sharded.DISTANCE_RULES
    assert "geomed" in sharded.LAYERWISE_RULES and "geomed" in engine.LAYERWISE_RULES
    assert "geomed" in engine.WEIGHTED_RULES
    with pytest.raises(ValueError):   # the engine runs the registry's check
        RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                           EngineConfig(gar="geomed", f=2, workers_per_rank=4))


def test_class_registry():
    X = separated(9, 300)
    inst = aggregators.instantiate("geomed", 9, 2, [])
    out = inst.aggregate(X)
    assert torch.equal(out, aggregators.gars["geomed"](gradients=X, f=2))
    assert torch.equal(inst.aggregate([X[i] for i in range(9)]), out)
    fewer = aggregators.instantiate("geomed", 9, 2, ["iters:3"]).aggregate(X)
    assert torch.equal(fewer, aggregators.gars["geomed"](gradients=X, f=2, iters=3))
    assert not torch.equal(fewer, out)
