"""Nearest-neighbour mixing (NNM) on the CPU: the fp64 oracle's distance identity against explicitly
mixed rows, the edge cases (f = 0, c = 1), the C++ mix / un-mix against the oracle, ties, the
non-finite policy, the registry, the engine and the sharded exchange on gloo."""
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

RULES = ("krum", "geomed", "average")


def latent(n, d, seed=0, dtype=torch.float32):
    """A latent geometry (4 factors + small noise): neighbour sets differ from row to row."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, 4, generator=g)
    P = torch.randn(4, d, generator=g)
    X = torch.randn(d, generator=g) + Z @ P + 0.05 * torch.randn(n, d, generator=g)
    return X.to(dtype)


def relerr(a, b):
    """Maximum relative error; where the reference is exactly zero the value must be too."""
    a, b = a.double().cpu(), b.double().cpu()
    zero = b == 0
    assert (a[zero] == 0).all()
    return ((a - b).abs()[~zero] / b.abs()[~zero]).max().item() if (~zero).any() else 0.0


def mixing_matrix(sets, n):
    W = torch.zeros((n, n), dtype=torch.float64)
    for i, s in enumerate(sets):
        W[i, s] = 1.0 / len(s)
    return W


def off_diagonal(n):
    return ~torch.eye(n, dtype=torch.bool)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,d,f", [(3, 100, 1), (8, 1000, 2), (17, 5003, 4), (64, 777, 15), (128, 500, 31),
                                   (128, 500, 1)])
def test_oracle_identity(n, d, f, dtype):
    """D' from D alone against the distances of explicitly mixed fp64 rows."""
    X = latent(n, d, 1, dtype)
    sets, Dm = ref.nnm_distances(ref.pairwise_sqdist(X), f)
    assert all(len(s) == n - f and i in s and s == sorted(s) for i, s in enumerate(sets))
    Y = mixing_matrix(sets, n) @ X.double()
    E = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    off = off_diagonal(n)
    same = torch.tensor([[sets[i] == sets[j] for j in range(n)] for i in range(n)])
    assert torch.equal(Dm, Dm.T)
    assert (Dm[same & off] == 0).all()        # equal sets: exactly zero
    m = off & ~same
    err = ((Dm - E).abs()[m] / E[m]).max().item() if m.any() else 0.0
    print(f"identity n={n} f={f} {dtype}: {int((same & off).sum()) // 2} duplicate pairs, max relative error {err:.2e}")
    assert err <= 1e-9


@pytest.mark.parametrize("n", [1, 2, 5, 33])
def test_edge_cases(native, n):
    X = latent(n, 200, 3)
    D = ref.pairwise_sqdist(X)
    # f = 0: every set is everything, D' is zero and w exactly uniform
    sets, Dm = ref.nnm_distances(D, 0)
    assert all(s == list(range(n)) for s in sets) and (Dm[off_diagonal(n)] == 0).all()
    for rule in RULES:
        if rule == "krum" and n < 3:
            continue
        assert torch.equal(ref.nnm_weights(D, 0, rule), torch.full((n,), 1.0 / n).float())
        assert torch.equal(gar.nnm_weights(X, 0, rule), torch.full((n,), 1.0 / n).float())
    # c = 1: every set is the row alone and D' is D bit for bit
    sets, Dm = ref.nnm_distances(D, n - 1)
    assert sets == [[i] for i in range(n)] and torch.equal(Dm, D)
    Dc, masks = native.cpu_nnm_mix(D, n - 1)
    assert torch.equal(Dc, D) and torch.equal(masks, gar.masks_from_sets(sets))


@pytest.mark.parametrize("n,d,f", [(3, 100, 1), (8, 1000, 2), (17, 5003, 4), (64, 777, 15), (65, 300, 16),
                                   (128, 500, 31), (128, 500, 1)])
def test_cpp_matches_oracle(native, n, d, f):
    X = latent(n, d, 2)
    D = ref.pairwise_sqdist(X)
    sets, Dm = ref.nnm_distances(D, f)
    Dc, masks = native.cpu_nnm_mix(D, f)
    assert masks.dtype == torch.int64 and masks.shape == (n, 2) and Dc.dtype == torch.float64
    assert torch.equal(masks, gar.masks_from_sets(sets))
    off = off_diagonal(n) & (Dm > 0)
    assert torch.equal(Dc == 0, Dm == 0) and torch.isinf(torch.diagonal(Dc)).all()
    assert ((Dc - Dm).abs()[off] / Dm[off]).max().item() <= 1e-12
    for rule in RULES:
        if rule == "krum" and n - f - 2 < 1:
            continue
        w = gar.nnm_weights(X, f, rule)
        assert w.dtype == torch.float32 and w.shape == (n,)
        assert relerr(w, ref.nnm_weights(D, f, rule)) <= 1e-6   # fp32 rounding of a and w
    a = torch.rand(n).float()
    a[0] = 0.0
    assert torch.equal(native.cpu_nnm_unmix(a, masks, n - f), ref.nnm_row_weights(sets, a))


def test_duplicate_gradients(native):
    """Two identical rows: exact distance ties, broken by index, as the oracle breaks them."""
    X = latent(9, 400, 4)
    X[5] = X[2]
    D = ref.pairwise_sqdist(X)
    assert float(D[2, 5]) == 0.0
    for f in (1, 3, 6):
        sets, Dm = ref.nnm_distances(D, f)
        assert 5 in sets[2] and 2 in sets[5]
        Dc, masks = native.cpu_nnm_mix(D, f)
        assert torch.equal(masks, gar.masks_from_sets(sets)) and torch.equal(Dc, Dm)
        for rule in RULES:
            if rule == "krum" and 9 < 2 * f + 3:
                continue
            assert relerr(gar.nnm_weights(X, f, rule), ref.nnm_weights(D, f, rule)) <= 1e-6
    # all distances tied (an equilateral set): the sets are the first indices
    T = torch.ones((6, 6), dtype=torch.float64)
    T.fill_diagonal_(math.inf)
    assert ref.nnm_sets(T, 3) == [[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5]]
    assert torch.equal(native.cpu_nnm_mix(T, 3)[1], gar.masks_from_sets(ref.nnm_sets(T, 3)))


@pytest.mark.parametrize("rule", RULES)
def test_non_finite_rows(native, rule):
    """f non-finite rows: exactly zero weight on them and a finite output."""
    X = latent(9, 500, 5)
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    D = ref.pairwise_sqdist(X)
    sets, Dm = ref.nnm_distances(D, 2)
    assert torch.isinf(Dm[4]).all() and torch.isinf(Dm[6]).all()      # tainted rows
    keep = [0, 1, 2, 3, 5, 7, 8]
    assert all(4 not in sets[i] and 6 not in sets[i] for i in keep)
    w_ref = ref.nnm_weights(D, 2, rule)
    w = gar.nnm_weights(X, 2, rule)
    if rule == "average":   # a = 1/n on the tainted rows too: their sets hold themselves
        assert float(w[4]) > 0 and float(w_ref[4]) > 0
        return
    assert float(w[4]) == 0.0 and float(w[6]) == 0.0 and float(w_ref[4]) == 0.0 and float(w_ref[6]) == 0.0
    assert relerr(w[keep], w_ref[keep]) <= 1e-6 and abs(float(w.double().sum()) - 1.0) < 1e-6
    out = gar.nnm(X, 2, rule)
    assert torch.isfinite(out).all()
    expect = ref.combine(X[keep], w_ref[keep].double())
    assert (out.double() - expect).abs().max().item() <= 1e-5 * max(1.0, expect.abs().max().item())


def test_large_path_matches_oracle():
    """n > 128: vectorised on the Gram."""
    X = latent(130, 300, 1)
    D = ref.pairwise_sqdist(X)
    H, S = gar.nnm_mix(X, 20)
    sets, Dm = ref.nnm_distances(D, 20)
    assert torch.equal(S, mixing_matrix(sets, 130) > 0)
    assert torch.equal(H, H.T) and (torch.diagonal(H) == 0).all()
    same = torch.tensor([[sets[i] == sets[j] for j in range(130)] for i in range(130)])
    assert (H[same] == 0).all()
    for rule in RULES:
        w = gar.nnm_weights(X, 20, rule)
        assert w.dtype == torch.float32 and relerr(w, ref.nnm_weights(D, 20, rule)) <= 1e-4
    X[7, 0] = math.nan
    w = gar.nnm_weights(X, 20, "krum")
    assert float(w[7]) == 0.0 and abs(float(w.double().sum()) - 1.0) < 1e-6


def test_registry():
    for base in RULES:
        for name in ("nnm-" + base, "native-nnm-" + base):
            assert name in aggregators.gars
            rule = aggregators.gars[name]
            assert callable(rule.check) and callable(rule.checked) and callable(rule.influence)
            assert rule.upper_bound is None
    X = latent(9, 300, 6)
    rows = [X[i].clone() for i in range(9)]
    D = ref.pairwise_sqdist(X)
    for base, kw in (("krum", {"m": 3}), ("geomed", {"iters": 5}), ("average", {})):
        rule = aggregators.gars["nnm-" + base]
        out = rule(gradients=X, f=2, **kw)
        assert torch.equal(out, rule(gradients=rows, f=2, **kw)) and out.shape == (300,)
        expect = ref.combine(X, ref.nnm_weights(D, 2, base, **kw).double())
        assert (out.double() - expect).abs().max().item() <= 1e-5 * max(1.0, expect.abs().max().item())
        assert torch.equal(gar.aggregate("nnm-" + base, X, f=2, **kw), out)
    # the rule's own check plus 0 <= f < n
    krum, geomed, avg = (aggregators.gars["nnm-" + b].check for b in RULES)
    assert krum(gradients=X, f=3) is None and "Byzantine" in krum(gradients=X, f=4)     # 2f + 3 <= n
    assert "selected" in krum(gradients=X, f=2, m=6)
    assert geomed(gradients=X, f=4) is None and "Byzantine" in geomed(gradients=X, f=5)
    assert "iterations" in geomed(gradients=X, f=2, iters=0)
    assert avg(gradients=X, f=0) is None and avg(gradients=X, f=8) is None
    assert "mix out" in avg(gradients=X, f=9) and "mix out" in avg(gradients=X, f=-1)
    assert "mix out" in avg(gradients=X, f=2.0)
    with pytest.raises(Exception, match="cannot be used"):
        aggregators.gars["nnm-average"].checked(gradients=X, f=9)
    # influence: the total w on the attack rows
    Xa = X.clone()
    Xa[7] = -30.0 * Xa[7]
    Xa[8] = Xa[8] + 500.0
    for base in RULES:
        infl = aggregators.gars["nnm-" + base].influence(list(Xa[:7]), list(Xa[7:]), f=2)
        w = gar.nnm_weights(Xa, 2, base).double()
        assert abs(infl - float(w[7:].sum())) < 1e-6
        # no honest row's set holds an attack row: only the attackers' own mixed rows carry them, with
        # weight a_i / c per membership: 1 / (n c) under the average, less under the geometric median,
        # none under Krum
        sets = ref.nnm_sets(ref.pairwise_sqdist(Xa), 2)
        assert all(7 not in s and 8 not in s for s in sets[:7])
        members = sum((7 in s) + (8 in s) for s in sets)
        if base == "krum":
            assert infl == 0.0
        elif base == "geomed":
            assert 0.0 < infl < members / 63
        else:
            assert abs(infl - members / 63) < 1e-6
    # the class registry and the gRPC names
    inst = aggregators.instantiate("nnm-krum", 9, 2, [])
    assert torch.equal(inst.aggregate(X), aggregators.gars["nnm-krum"](gradients=X, f=2))
    inst = aggregators.instantiate("nnm-geomed", 9, 2, ["iters:3"])
    assert torch.equal(inst.aggregate(X), aggregators.gars["nnm-geomed"](gradients=X, f=2, iters=3))
    assert torch.equal(aggregators.instantiate("nnm-average", 9, 2, []).aggregate(X),
                       aggregators.gars["nnm-average"](gradients=X, f=2))
    from garfield_amd.grpcnet.aggregator import Aggregator_tf

    for name, base in (("NNM-Krum", "krum"), ("NNM-GeoMed", "geomed"), ("NNM-Average", "average")):
        out = Aggregator_tf(name, 9, 2).aggregate([r.numpy() for r in rows])
        assert torch.equal(torch.from_numpy(out), aggregators.gars["nnm-" + base](gradients=rows, f=2))


def test_pre_argument_and_errors():
    X = latent(9, 300, 6)
    assert torch.equal(gar.krum_weights(X, 2, pre="nnm"), gar.nnm_weights(X, 2, "krum"))
    assert torch.equal(gar.krum_weights(X, 2, 3, pre="nnm"), gar.nnm_weights(X, 2, "krum", m=3))
    assert torch.equal(gar.geomed_weights(X, 8, 1e-6, pre="nnm", f=2), gar.nnm_weights(X, 2, "geomed", iters=8))
    assert not torch.equal(gar.krum_weights(X, 2), gar.krum_weights(X, 2, pre="nnm"))
    for bad in (lambda: gar.nnm_weights(X, 9, "average"), lambda: gar.nnm_weights(X, -1, "average"),
                lambda: gar.nnm_weights(X, 2, "median"), lambda: gar.krum_weights(X, 2, pre="bucketing"),
                lambda: gar.nnm_weights(X, 7, "krum"), lambda: gar.nnm_mix(X, 9)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("rule", RULES)
def test_engine_cpu(rule):
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar=rule, f=2, workers_per_rank=8, byzantine={7: "reverse"},
                                          pre_aggregation="nnm"))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    for _ in range(2):
        eng.step(b)
        w = eng.last_weights
        assert w is not None and w.shape == (8,)
        kw = {"iters": 32, "nu": 1e-6} if rule == "geomed" else {}
        assert torch.equal(w, gar.nnm_weights(eng.G.float(), 2, rule, **kw))
        assert abs(float(w.double().sum()) - 1.0) < 1e-6
        assert float(w[7]) < 1 / 8 if rule != "average" else float(w[7]) <= 1 / 8 + 1e-7
    assert torch.isfinite(eng.flat_model()).all()


def test_engine_update_from_rows_cpu():
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="krum", f=1, workers_per_rank=6, pre_aggregation="nnm"))
    rows = [r.clone() for r in latent(6, eng.d, 8)]
    before = eng.flat_model().clone()
    eng._update_from_rows(rows)
    assert torch.equal(eng.last_weights, gar.nnm_weights(torch.stack(rows), 1, "krum"))
    assert not torch.equal(before, eng.flat_model())


def test_engine_rejects_unsupported():
    def make(**kw):
        return RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                  EngineConfig(f=2, workers_per_rank=9, pre_aggregation="nnm", **kw))

    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="median")
    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="bulyan")
    with pytest.raises(ValueError, match="layerwise"):
        make(gar="krum", layerwise=True)
    with pytest.raises(ValueError, match="unknown pre_aggregation"):
        RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                           EngineConfig(gar="krum", f=2, workers_per_rank=9, pre_aggregation="bucketing"))
    with pytest.raises(ValueError, match="selected gradients"):   # the registry's check of nnm-krum
        make(gar="krum", m=7)
    assert make(gar="krum").cfg.pre_aggregation == "nnm"
    assert EngineConfig().pre_aggregation is None


def test_apps_flag():
    import argparse

    from garfield_amd.apps.common import add_common, gar_name

    a = add_common(argparse.ArgumentParser()).parse_args(["--gar", "krum", "--pre_aggregation", "nnm"])
    assert gar_name(a) == "nnm-krum" and gar_name(a) in aggregators.gars
    a = add_common(argparse.ArgumentParser()).parse_args(["--gar", "krum"])
    assert a.pre_aggregation is None and gar_name(a) == "krum"


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
    for rule in RULES:
        torch.manual_seed(0)
        eng = RobustDataParallel(build_model("mlp"), F.nll_loss, ctx,
                                 EngineConfig(gar=rule, f=1, workers_per_rank=3, byzantine={3: "reverse"},
                                              shard_gar=shard, lr=0.05, pre_aggregation="nnm"))
        assert (eng._shard is not None) == shard
        b = synthetic_batches(3, 8, (1, 28, 28), 10, "cpu", seed=rank)
        for _ in range(2):
            eng.step(b)
        out[rule] = {"flat": eng.flat_model().clone(), "sum": eng.replica_checksum(),
                     "w": eng.last_weights.clone().float()}
    torch.save(out, os.path.join(outdir, f"{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_two_rank_sharded_vs_unsharded():
    """2 gloo ranks x 3 workers: the mix runs on the distances summed over ranks, so every rank gets
    the same w (replicas bitwise identical). Krum's and the average's folded weights are rationals
    k / (m c) and k / (n c) of the same sets: sharded and unsharded weights are bitwise equal. The
    geometric median's are continuous in distances summed in another order: 1e-5 relative, as the
    geomed rehearsal."""
    world = 2
    with tempfile.TemporaryDirectory() as d:
        for shard in (False, True):
            mp.spawn(_rank_worker, args=(world, free_port(), d, shard), nprocs=world, join=True)
        res = {(s, r): torch.load(os.path.join(d, f"{s}r{r}.pt"), weights_only=True)
               for s in (0, 1) for r in range(world)}
        for rule in RULES:
            for s in (0, 1):
                assert res[(s, 1)][rule]["sum"] == res[(s, 0)][rule]["sum"], (rule, s)
                assert torch.equal(res[(s, 1)][rule]["flat"], res[(s, 0)][rule]["flat"]), (rule, s)
                assert torch.equal(res[(s, 1)][rule]["w"], res[(s, 0)][rule]["w"]), (rule, s)
            red, sh = res[(0, 0)][rule], res[(1, 0)][rule]
            assert sh["w"].shape == red["w"].shape == (6,)
            if rule == "geomed":
                assert relerr(sh["w"], red["w"]) < 1e-5
            else:
                assert torch.equal(sh["w"], red["w"]), (rule, sh["w"], red["w"])
            torch.testing.assert_close(sh["flat"], red["flat"], rtol=1e-5, atol=1e-7)
