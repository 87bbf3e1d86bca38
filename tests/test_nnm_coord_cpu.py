"""Nearest-neighbour mixing in front of a coordinate-wise rule (nnm-trimmed-mean, nnm-median) on the CPU:
the oracle against explicitly mixed rows, f = 0 and c = 1, the C++ path against the oracle and its
independence of the column split, the registry, the argument errors, the engine and the sharded exchange
on gloo (docs/GAR_SEMANTICS.md "Nearest-neighbour mixing before a coordinate-wise rule")."""
import functools
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

RULES = ("trimmed-mean", "median")
CASES = [(3, 100, 1), (8, 1000, 2), (16, 4096, 3), (17, 5003, 4), (33, 517, 8), (64, 777, 15), (65, 300, 16),
         (128, 2000, 31), (128, 2000, 1), (130, 300, 20)]
SEEDS = {(17, 5003, 4): 1, (128, 2000, 31): 2, (130, 300, 20): 1}   # fp32 inputs
GAP = 1e-4


def latent(n, d, dtype, seed=0):
    """A latent geometry (4 factors + small noise), on the CPU: neighbour sets differ from row to row."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, 4, generator=g)
    P = torch.randn(4, d, generator=g)
    X = torch.randn(d, generator=g) + Z @ P + 0.05 * torch.randn(n, d, generator=g)
    return X.to(dtype)


def assert_gaps(D, f, tag):
    """The precondition of every end-to-end comparison, on the oracle: for each row the c-th and (c + 1)-th
    nearest distances (the row itself first) differ by >= GAP relative."""
    n = D.shape[0]
    c = n - f
    if f == 0:
        return
    for i in range(n):
        o = sorted(float(D[i, j]) for j in range(n) if j != i)
        inner = o[c - 2] if c >= 2 else 0.0
        assert (o[c - 1] - inner) / o[c - 1] >= GAP, (tag, i)


@functools.lru_cache(maxsize=None)
def case(n, d, f):
    """(fp32 rows, their squared distances, the oracle's sets and outputs per rule): computed once, shared,
    never modified."""
    X = latent(n, d, torch.float32, SEEDS.get((n, d, f), 0))
    D = ref.pairwise_sqdist(X)
    assert_gaps(D, f, (n, d, f))
    return X, D, ref.nnm_sets(D, f), {r: ref.nnm_coord(X, f, r) for r in RULES}


@pytest.mark.parametrize("n,d,f", [(3, 100, 1), (8, 1000, 2), (17, 503, 4), (65, 300, 16)])
def test_oracle_is_the_rule_on_explicitly_mixed_rows(n, d, f):
    X, D, sets, out = case(n, d, f)
    W = torch.zeros((n, n), dtype=torch.float64)
    for i, s in enumerate(sets):
        assert len(s) == n - f and i in s
        W[i, s] = 1.0
    Y = ref.nnm_mixed_rows(X, sets)
    assert Y.dtype == torch.float64 and Y.shape == (n, d)
    # the same members: the matrix product sums in another order, so within fp64 rounding
    assert (Y - (W @ X.double()) / (n - f)).abs().max().item() <= 1e-12 * X.abs().max().item()
    assert torch.equal(out["trimmed-mean"], ref.trimmed_mean(Y, f))
    assert torch.equal(out["median"], ref.median(Y))


@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_f0_is_the_mean(native, n):
    X = latent(n, 200, torch.float32, 3)
    mean = X.double().sum(0) / n
    for rule in RULES:
        o = ref.nnm_coord(X, 0, rule)
        assert (o - mean).abs().max().item() <= 1e-14 * X.abs().max().item()
        g = gar.nnm_coord(X, 0, rule)
        assert g.dtype == torch.float32 and (g.double() - mean).abs().max().item() <= 1e-6 * X.abs().max().item()


@pytest.mark.parametrize("n", [1, 2, 8, 65])
def test_c1_median_is_the_median_exactly(native, n):
    X = latent(n, 300, torch.float32, 4)
    assert torch.equal(ref.nnm_coord(X, n - 1, "median"), ref.median(X))
    assert torch.equal(gar.nnm_coord(X, n - 1, "median"), gar.median(X))
    assert torch.equal(gar.nnm_coord(X.double(), n - 1, "median"), gar.median(X.double()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,d,f", CASES)
def test_cpp_matches_oracle(native, n, d, f, dtype):
    X, D, sets, out = case(n, d, f)
    A = X.abs().max(0).values.double()
    for rule in RULES:
        g = gar.nnm_coord(X.to(dtype), f, rule)
        assert g.dtype == dtype and g.shape == (d,)
        err = ((g.double() - out[rule]).abs() / A).max().item()
        print(f"cpu nnm-{rule} n={n} d={d} f={f} {dtype}: max error / A = {err:.3e}")
        assert err <= 1e-6    # the sums are fp64: only the fp32 output rounds
        if dtype == torch.float64 and n <= gar.MAX_ROWS:   # the oracle's sums in the oracle's order
            assert torch.equal(g, out[rule])
    if n <= gar.MAX_ROWS:
        masks = native.cpu_nnm_mix(D, f)[1]
        assert torch.equal(masks, gar.masks_from_sets(sets))
        rows = [X[i].clone() for i in range(n)]
        assert torch.equal(native.cpu_mixed_coordwise(rows, masks, n - f, "median", f),
                           native.cpu_mixed_coordwise(X, masks, n - f, "median", f))


@pytest.mark.parametrize("n,d,f", [(8, 1000, 2), (17, 5003, 4), (65, 300, 16)])
def test_cpp_is_independent_of_the_column_split(native, n, d, f):
    X, D, sets, _ = case(n, d, f)
    masks = gar.masks_from_sets(sets)
    h = d // 2 + 1
    for dtype in (torch.float32, torch.float64):
        Xd = X.to(dtype)
        for rule in RULES:
            whole = native.cpu_mixed_coordwise(Xd, masks, n - f, rule, f)
            halves = torch.cat([native.cpu_mixed_coordwise(Xd[:, :h].contiguous(), masks, n - f, rule, f),
                                native.cpu_mixed_coordwise(Xd[:, h:].contiguous(), masks, n - f, rule, f)])
            assert torch.equal(whole, halves)
            assert torch.equal(whole, gar.nnm_coord_from_distances(native, Xd, D, f, rule))


def test_non_finite_rows(native):
    """f non-finite rows: exactly their mixed values are non-finite, and both rules leave them out."""
    X = latent(9, 500, torch.float32, 5).clone()
    X[4] = float("nan")
    X[6] = float("inf")
    D = ref.pairwise_sqdist(X)
    sets = ref.nnm_sets(D, 2)
    keep = [0, 1, 2, 3, 5, 7, 8]
    assert all(sets[i] == keep for i in keep)
    Y = ref.nnm_mixed_rows(X, sets)
    assert torch.isfinite(Y[keep]).all() and not torch.isfinite(Y[[4, 6]]).any()
    for rule in RULES:
        o = ref.nnm_coord(X, 2, rule)
        g = gar.nnm_coord(X, 2, rule)
        assert torch.isfinite(o).all() and torch.isfinite(g).all()
        assert (g.double() - o).abs().max().item() <= 1e-6 * X[keep].abs().max().item()


def test_registry():
    for base in RULES:
        for name in ("nnm-" + base, "native-nnm-" + base):
            assert name in aggregators.gars
            rule = aggregators.gars[name]
            assert callable(rule.check) and callable(rule.checked)
            assert rule.upper_bound is None and rule.influence is None
    X = latent(9, 300, torch.float32, 6)
    rows = [X[i].clone() for i in range(9)]
    for base in RULES:
        rule = aggregators.gars["nnm-" + base]
        out = rule(gradients=X, f=2)
        assert out.shape == (300,) and torch.equal(out, rule(gradients=rows, f=2))
        assert torch.equal(out, gar.nnm_coord(X, 2, base)) and torch.equal(out, gar.aggregate("nnm-" + base, X, f=2))
        assert torch.equal(out, rule(gradients=X, f=2, m=3, iters=5))   # other rules' arguments are ignored
        expect = ref.nnm_coord(X, 2, base)
        assert (out.double() - expect).abs().max().item() <= 1e-6 * X.abs().max().item()
    tm, med = (aggregators.gars["nnm-" + b].check for b in RULES)
    assert tm(gradients=X, f=4) is None and "Byzantine" in tm(gradients=X, f=5)      # 2f + 1 <= n
    assert "Byzantine" in tm(gradients=X, f=2.0)
    assert med(gradients=X, f=0) is None and med(gradients=X, f=8) is None and med(gradients=X) is None
    assert "mix out" in med(gradients=X, f=9) and "mix out" in med(gradients=X, f=-1)
    assert "mix out" in med(gradients=X, f=2.0)
    assert "at least one gradient" in med(gradients=[], f=0)   # the plain rule's own check comes first
    with pytest.raises(Exception, match="cannot be used"):
        aggregators.gars["nnm-trimmed-mean"].checked(gradients=X, f=5)
    with pytest.raises(Exception, match="cannot be used"):
        aggregators.gars["nnm-median"].checked(gradients=X, f=9)


def test_argument_errors():
    X = latent(9, 300, torch.float32, 6)
    assert gar.NNM_COORD_RULES == RULES and gar.NNM_RULES == ("krum", "geomed", "cclip", "average")
    for bad in (lambda: gar.nnm_coord(X, 9, "median"), lambda: gar.nnm_coord(X, -1, "median"),
                lambda: gar.nnm_coord(X, 5, "trimmed-mean"), lambda: gar.nnm_coord(X, 2, "krum"),
                lambda: gar.nnm_coord(X, 2, "averaged-median"), lambda: gar.nnm_coord(X, 2.0, "median"),
                lambda: gar.nnm_weights(X, 2, "median"), lambda: gar.nnm_weights(X, 2, "trimmed-mean"),
                lambda: ref.nnm_coord(X, 5, "trimmed-mean"), lambda: ref.nnm_coord(X, 2, "krum")):
        with pytest.raises(ValueError):
            bad()
    assert gar.nnm_coord(X, 4, "trimmed-mean").shape == (300,) and gar.nnm_coord(X, 8, "median").shape == (300,)
    # 16-bit rows on the CPU: computed in fp32, returned in the input dtype
    assert gar.nnm_coord(X.bfloat16(), 2, "median").dtype == torch.bfloat16


def test_gar_bench_defaults():
    from garfield_amd.apps import gar_bench

    for name in ("nnm-trimmed-mean", "nnm-median"):
        assert name in gar_bench.RULES and name in gar.RULES
        for n in (8, 32, 128):
            assert gar_bench.default_f(name, n) == gar_bench.default_f("trimmed-mean", n) is not None
    assert gar_bench.default_f("median", 8) is None


def test_engine_cpu():
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="trimmed-mean", f=1, workers_per_rank=5, byzantine={4: "reverse"},
                                          lr=0.05, momentum=0.0, weight_decay=0.0, pre_aggregation="nnm"))
    b = synthetic_batches(5, 16, (1, 28, 28), 10, "cpu")
    before = eng.flat_model().clone()
    eng.step(b)
    assert eng.last_weights is None
    # plain SGD: the parameters moved by exactly -lr * the aggregate of the rows of this step
    g = gar.nnm_coord(eng.G.float(), 1, "trimmed-mean").float()
    assert g.abs().max().item() > 0 and torch.equal(eng.flat_model(), before.add(g, alpha=-0.05))
    plain = gar.trimmed_mean(eng.G.float(), 1).float()
    assert not torch.equal(g, plain)   # the mixing is not a no-op
    for _ in range(2):
        eng.step(b)
    assert torch.isfinite(eng.flat_model()).all()


def test_engine_update_from_rows_cpu():
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="trimmed-mean", f=1, workers_per_rank=6, lr=0.05, momentum=0.0,
                                          weight_decay=0.0, pre_aggregation="nnm"))
    rows = [r.clone() for r in latent(6, eng.d, torch.float32, 8)]
    before = eng.flat_model().clone()
    eng._update_from_rows(rows)
    assert torch.equal(eng.flat_model(), before.add(gar.nnm_coord(torch.stack(rows), 1, "trimmed-mean"), alpha=-0.05))


def test_engine_still_rejects():
    def make(**kw):
        return RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                  EngineConfig(f=2, workers_per_rank=9, pre_aggregation="nnm", **kw))

    assert make(gar="trimmed-mean").cfg.pre_aggregation == "nnm"
    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="median")
    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="bulyan")
    with pytest.raises(ValueError, match="layerwise"):
        make(gar="trimmed-mean", layerwise=True)
    with pytest.raises(ValueError, match="Byzantine"):   # the registry's check of nnm-trimmed-mean: n >= 2f + 1
        RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                           EngineConfig(gar="trimmed-mean", f=5, workers_per_rank=9, pre_aggregation="nnm"))


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
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, ctx,
                             EngineConfig(gar="trimmed-mean", f=1, workers_per_rank=3, byzantine={3: "reverse"},
                                          shard_gar=shard, lr=0.05, pre_aggregation="nnm"))
    assert (eng._shard is not None) == shard
    b = synthetic_batches(3, 8, (1, 28, 28), 10, "cpu", seed=rank)
    for _ in range(3):
        eng.step(b)
    assert eng.last_weights is None
    torch.save({"flat": eng.flat_model().clone(), "sum": eng.replica_checksum()},
               os.path.join(outdir, f"{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_two_rank_sharded_equals_redundant_bitwise():
    """2 gloo ranks x 3 workers, 3 steps: the sets come from the distances summed over ranks (the same on
    every rank), and a coordinate's result does not depend on the shard that holds it: the sharded and
    the redundant parameters are bit-equal."""
    world = 2
    with tempfile.TemporaryDirectory() as d:
        for shard in (False, True):
            mp.spawn(_rank_worker, args=(world, free_port(), d, shard), nprocs=world, join=True)
        res = {(s, r): torch.load(os.path.join(d, f"{s}r{r}.pt"), weights_only=True)
               for s in (0, 1) for r in range(world)}
        for s in (0, 1):
            assert res[(s, 1)]["sum"] == res[(s, 0)]["sum"], s
            assert torch.equal(res[(s, 1)]["flat"], res[(s, 0)]["flat"]), s
        assert torch.isfinite(res[(0, 0)]["flat"]).all()
        assert torch.equal(res[(1, 0)]["flat"], res[(0, 0)]["flat"])
