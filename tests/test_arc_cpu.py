"""Adaptive robust clipping (ARC) on the CPU: the oracle's clip count and tie rules on hand-made norms, the
f = 0 identities, gar.arc_* against the oracle on the vectors, the registry, the error cases, the engine,
the apps flag and the sharded exchange on gloo."""
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
from garfield_amd.ops import gar, selection
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

WEIGHTED = ("krum", "geomed", "cclip", "dnc", "average")
MIXED = ("krum", "geomed", "cclip", "average")
COORD = ("trimmed-mean", "median")
# gar.arc_weights against the oracle on the vectors, per weight: the CPU path is fp64 up to the fp32 casts of the
# scales and of the weights (2^-24 each) and the C++ rules' own fp32 outputs
W_RTOL = 1e-6


def latent(n, d, seed=0, dtype=torch.float32):
    """A latent geometry (4 factors + small noise): the rows differ in norm and in their neighbour sets."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, 4, generator=g)
    P = torch.randn(4, d, generator=g)
    X = torch.randn(d, generator=g) + Z @ P + 0.05 * torch.randn(n, d, generator=g)
    return X.to(dtype)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    zero = b == 0
    assert (a[zero] == 0).all()
    return ((a - b).abs()[~zero] / b.abs()[~zero]).max().item() if (~zero).any() else 0.0


def f32(v):
    return float(torch.tensor(v, dtype=torch.float64).float())


def test_clip_count():
    for n in range(1, 40):
        assert ref.arc_count(n, 0) == 0
        for f in range(n):
            k = ref.arc_count(n, f)
            assert k == (2 * f * (n - f)) // n == selection.arc_count(n, f) and 0 <= k < n
            assert (k == 0) == (f == 0)
    assert ref.arc_count(8, 2) == 3 and ref.arc_count(128, 63) == 63 and ref.arc_count(9, 3) == 4
    for bad in ((4, 4), (4, -1), (0, 0)):
        with pytest.raises(ValueError):
            ref.arc_count(*bad)


def both(s, f):
    """The oracle's scales, after checking that the vectorised form gives the same bits."""
    s = torch.tensor(s, dtype=torch.float32)
    c = ref.arc_scales(s, f)
    assert c.dtype == torch.float32 and torch.equal(c, selection.arc_scales_from_sqnorms(s, f))
    assert torch.equal(c, selection.arc_scales_from_sqnorms(s.double(), f))
    return c.tolist()


def test_scales_on_hand_made_norms():
    # n = 4, f = 1: k = 1; the largest is clipped to the second largest
    assert both([1.0, 16.0, 4.0, 2.0], 1) == [1.0, 0.5, 1.0, 1.0]
    # n = 5, f = 2: k = 2; C² = the third largest
    assert both([9.0, 1.0, 36.0, 4.0, 0.25], 2) == [f32(math.sqrt(4 / 9)), 1.0, f32(math.sqrt(4 / 36)), 1.0, 1.0]
    # equal norms: nothing is above the threshold
    assert both([3.0] * 6, 2) == [1.0] * 6
    # ties with C²: rows 1 and 3 hold positions 1 and 2 of (s descending, index ascending), k = 2 -> C² = 5;
    # row 1 ties with it and stays: fewer than k rows are clipped
    assert both([7.0, 5.0, 1.0, 5.0, 2.0], 2) == [f32(math.sqrt(5 / 7)), 1.0, 1.0, 1.0, 1.0]
    # zero rows are never clipped, and a zero threshold clips to zero without a division by zero
    assert both([0.0, 0.0, 4.0, 0.0], 1) == [1.0, 1.0, 0.0, 1.0]
    assert both([0.0] * 5, 2) == [1.0] * 5
    inf, nan = math.inf, math.nan
    # more than k non-finite rows: C² is non-finite and nothing is clipped
    assert both([nan, 9.0, inf, 4.0, -inf, 2.0, 3.0], 2) == [1.0] * 7


def test_scales_non_finite_positions():
    """n = 7, f = 3: k = 3. Two non-finite rows hold positions 0 and 1, the largest finite row position 2 and
    the second largest is C²."""
    s = [math.nan, 9.0, 1.0, 4.0, math.inf, 2.0, 3.0]
    assert ref.arc_count(7, 3) == 3
    assert both(s, 3) == [1.0, f32(math.sqrt(4 / 9)), 1.0, 1.0, 1.0, 1.0, 1.0]
    # f = 2: k = 2, C² = 9 (position 2): no finite row is above it
    assert both(s, 2) == [1.0] * 7
    assert ref.arc_clip_rows(ref.arc_scales(torch.tensor(s), 3)) == [1]


def test_gram_and_distances_of_the_clipped_rows():
    X = latent(9, 300, 2).double()
    c = ref.arc_scales((X * X).sum(1), 3)
    Y = c.double()[:, None] * X
    assert torch.equal(ref.arc_clip(X, 3), Y)
    G = (X @ X.T).float()
    G2 = ref.arc_gram(G, c)
    assert torch.equal(G2, G2.T)
    one = c == 1
    assert torch.equal(G2[one][:, one], G[one][:, one])
    assert torch.equal(G2, selection.arc_gram(G, c))
    torch.testing.assert_close(G2.double(), Y @ Y.T, rtol=1e-6, atol=0)
    D = ref.pairwise_sqdist(X)
    Dc = selection.arc_distances(D, (X * X).sum(1), c)
    off = ~torch.eye(9, dtype=torch.bool)
    torch.testing.assert_close(Dc[off], ref.pairwise_sqdist(Y)[off], rtol=1e-9, atol=0)
    assert torch.equal(Dc[one][:, one], D[one][:, one]) and torch.isinf(torch.diagonal(Dc)).all()


def test_f0_is_the_path_without_arc_bitwise():
    X = latent(9, 400, 1)
    before = X.clone()
    assert torch.equal(gar.arc_scales(X, 0), torch.ones(9))
    for rule in WEIGHTED:
        plain = {"krum": lambda: gar.krum_weights(X, 0), "geomed": lambda: gar.geomed_weights(X),
                 "cclip": lambda: gar.cclip_weights(X, 0), "dnc": lambda: gar.dnc_weights(X, 0),
                 "average": lambda: torch.full((9,), 1.0 / 9)}[rule]()
        assert torch.equal(gar.arc_weights(X, 0, rule), plain), rule
    for rule in MIXED:
        assert torch.equal(gar.arc_weights(X, 0, rule, nnm=True), gar.nnm_weights(X, 0, rule)), rule
    assert torch.equal(gar.arc(X, 0, "krum"), gar.krum(X, 0))
    assert torch.equal(gar.arc_coord(X, 0, "median"), gar.median(X))
    assert torch.equal(gar.arc_coord(X, 0, "trimmed-mean"), gar.trimmed_mean(X, 0))
    assert torch.equal(gar.arc_coord(X, 0, "median", nnm=True), gar.nnm_coord(X, 0, "median"))
    assert torch.equal(X, before)


@pytest.mark.parametrize("n,d,f", [(3, 100, 1), (8, 1000, 2), (9, 1000, 3), (17, 503, 4), (64, 300, 15), (130, 200, 20)])
def test_functions_match_oracle(n, d, f):
    X = latent(n, d, 0)
    before = X.clone()
    s = (X.double() ** 2).sum(1)
    c = gar.arc_scales(X, f)
    assert torch.equal(c, ref.arc_scales(s, f)) and int((c != 1).sum()) <= ref.arc_count(n, f)
    rows = [r.clone() for r in X]
    for nnm, rules in ((False, WEIGHTED), (True, MIXED)):
        for rule in rules:
            if rule == "krum" and n < 2 * f + 3 or rule == "dnc" and n < 2 * f + 1:
                continue
            w = gar.arc_weights(X, f, rule, nnm=nnm)
            w_ref = ref.arc_weights(X, f, rule, nnm)
            assert w.dtype == torch.float32 and w.shape == (n,)
            assert relerr(w, w_ref) <= W_RTOL, (rule, nnm, relerr(w, w_ref))
            assert float(w.double().sum()) <= 1.0 + 1e-6
            out = gar.arc(X, f, rule, nnm=nnm)
            torch.testing.assert_close(out.double(), ref.combine(X, w_ref), rtol=1e-5, atol=1e-5)
            assert torch.equal(gar.arc_weights(rows, f, rule, nnm=nnm), w)
    for rule in COORD:
        for nnm in (False, True):
            out = gar.arc_coord(X, f, rule, nnm)
            assert out.dtype == X.dtype and out.shape == (d,)
            torch.testing.assert_close(out.double(), ref.arc_coord(X, f, rule, nnm), rtol=1e-5, atol=1e-5)
    assert torch.equal(X, before) and all(torch.equal(a, b) for a, b in zip(rows, before))


def test_oracle_without_the_extension(monkeypatch):
    """The pure-Python host backend (no C++ functions): the same weights within the C++ rules' fp32 outputs."""
    X = latent(9, 300, 4)
    sel = selection.resolve("krum", 9, 2, None, "arc+nnm")
    D, s = ref.pairwise_sqdist(X), (X.double() ** 2).sum(1)
    w = sel.on_host(None, D, s)
    assert relerr(w, ref.arc_weights(X, 2, "krum", True)) <= W_RTOL
    assert torch.equal(w, gar.arc_weights(X, 2, "krum", nnm=True))
    with pytest.raises(ValueError, match="squared norms"):
        sel.on_host(None, D)


def test_large_norms_are_tamed():
    """Two rows scaled by 1e3 drag the plain average away; arc-average clips them to an honest norm."""
    X = latent(8, 500, 3)
    honest = X[:6].double().mean(0)
    X[6:] *= 1e3
    out = gar.arc(X, 2, "average")
    torch.testing.assert_close(out.double(), ref.arc(X, 2, "average"), rtol=1e-5, atol=1e-5)
    assert float((out.double() - honest).norm()) < float(honest.norm())
    assert float((gar.average(X).double() - honest).norm()) > 100 * float(honest.norm())
    c = gar.arc_scales(X, 2)
    assert float(c[6]) < 2e-3 and float(c[7]) < 2e-3


def test_non_finite_rows():
    X = latent(9, 500, 5)
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    c = gar.arc_scales(X, 2)
    assert float(c[4]) == 1.0 and float(c[6]) == 1.0      # they take the k = 3 top slots' first two, unclipped
    assert int((c != 1).sum()) == 1
    keep = [0, 1, 2, 3, 5, 7, 8]
    for rule in ("krum", "geomed"):
        w = gar.arc_weights(X, 2, rule)
        w_ref = ref.arc_weights(X, 2, rule)
        assert float(w[4]) == 0.0 and float(w[6]) == 0.0 and float(w_ref[4]) == 0.0 and float(w_ref[6]) == 0.0
        assert relerr(w, w_ref) <= W_RTOL
        out = gar.arc(X, 2, rule)
        assert torch.isfinite(out).all()
        torch.testing.assert_close(out.double(), ref.combine(X[keep], w_ref[keep]), rtol=1e-5, atol=1e-5)


def test_registry():
    X = latent(9, 300, 4)
    rows = [r.clone() for r in X]
    names = (["arc-" + r for r in WEIGHTED + COORD] + ["arc-nnm-" + r for r in MIXED + COORD])
    assert len(names) == 13
    for name in names:
        for nm in (name, "native-" + name):
            assert nm in aggregators.gars, nm
        assert name in gar.RULES
        rule = aggregators.gars[name]
        assert rule.upper_bound is None
        nnm = name.startswith("arc-nnm-")
        base = name[len("arc-nnm-" if nnm else "arc-"):]
        out = rule(gradients=rows, f=2)
        assert out.shape == (300,) and not any(out.data_ptr() == r.data_ptr() for r in rows)
        assert torch.equal(out, gar.aggregate(name, rows, f=2))
        if base in COORD:
            assert rule.influence is None
            assert torch.equal(out, gar.arc_coord(X, 2, base, nnm))
        else:
            assert torch.equal(out, gar.arc(X, 2, base, nnm))
            infl = rule.influence(rows[:7], rows[7:], f=2)
            w = gar.arc_weights(X, 2, base, nnm)
            assert abs(infl - float(w.double()[7:].sum())) < 1e-12 and 0.0 <= infl <= 1.0
        assert rule.check(gradients=rows, f=9) is not None and rule.check(gradients=rows, f=-1) is not None
        assert rule.check(gradients=rows, f=True) is not None
        assert rule.check(gradients=rows, f=2) is None
    assert aggregators.gars["arc-krum"].check(gradients=rows, f=4) is not None          # Krum's own n >= 2f + 3
    assert aggregators.gars["arc-trimmed-mean"].check(gradients=rows, f=5) is not None  # the trimmed mean's 2f < n
    assert aggregators.gars["arc-cclip"].check(gradients=rows, f=2, start=torch.ones(9)) is not None
    for absent in ("arc-bulyan", "arc-brute", "arc-aksel", "arc-nnm-dnc", "bucketing-krum"):
        assert absent not in aggregators.gars and absent not in gar.RULES
    from garfield_amd.apps import gar_bench

    for name in names:
        assert name in gar_bench.RULES
    assert gar_bench.default_f("arc-krum", 8) == gar_bench.default_f("krum", 8) == 2
    assert gar_bench.default_f("arc-nnm-median", 8) == gar_bench.default_f("trimmed-mean", 8)
    assert gar_bench.default_f("arc-average", 8) == gar_bench.default_f("nnm-average", 8)


def test_pre_argument_and_errors():
    X = latent(9, 300, 6)
    assert torch.equal(gar.krum_weights(X, 2, pre="arc"), gar.arc_weights(X, 2, "krum"))
    assert torch.equal(gar.krum_weights(X, 2, 3, pre="arc+nnm"), gar.arc_weights(X, 2, "krum", nnm=True, m=3))
    assert torch.equal(gar.geomed_weights(X, 8, 1e-6, pre="arc", f=2), gar.arc_weights(X, 2, "geomed", iters=8))
    assert torch.equal(gar.cclip_weights(X, 2, pre="arc"), gar.arc_weights(X, 2, "cclip"))
    assert torch.equal(gar.dnc_weights(X, 2, pre="arc"), gar.arc_weights(X, 2, "dnc"))
    assert not torch.equal(gar.krum_weights(X, 2), gar.krum_weights(X, 2, pre="arc"))
    assert not torch.equal(gar.krum_weights(X, 2, pre="nnm"), gar.krum_weights(X, 2, pre="arc+nnm"))
    for bad in (lambda: gar.arc_weights(X, 9, "average"), lambda: gar.arc_weights(X, -1, "average"),
                lambda: gar.arc_weights(X, 2, "median"), lambda: gar.arc_weights(X, 2, "bulyan"),
                lambda: gar.arc_weights(X, 2, "brute"), lambda: gar.arc_weights(X, 2, "aksel"),
                lambda: gar.arc_weights(X, 2, "dnc", nnm=True), lambda: gar.krum_weights(X, 2, pre="bucketing"),
                lambda: gar.krum_weights(X, 2, pre="nnm+arc"), lambda: gar.arc_weights(X, 4, "krum"),
                lambda: gar.arc_weights(X, 2, "cclip", start=torch.ones(9)),
                lambda: gar.cclip_weights(X, 2, center=torch.zeros(300), pre="arc"),
                lambda: gar.arc_scales(X, 9), lambda: gar.arc_scales(X, True), lambda: gar.arc_coord(X, 2, "krum"),
                lambda: gar.arc_coord(X, 2, "averaged-median"), lambda: gar.arc_coord(X, 5, "trimmed-mean"),
                lambda: gar.arc_coord(X, 9, "median")):
        with pytest.raises(ValueError):
            bad()


ENGINE_RULES = (("arc", "krum"), ("arc", "geomed"), ("arc", "cclip"), ("arc", "dnc"), ("arc", "average"),
                ("arc+nnm", "krum"), ("arc+nnm", "geomed"), ("arc+nnm", "average"))


@pytest.mark.parametrize("pre,rule", ENGINE_RULES)
def test_engine_cpu(pre, rule):
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar=rule, f=2, workers_per_rank=8, byzantine={7: "reverse"},
                                          pre_aggregation=pre))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    for _ in range(2):
        eng.step(b)
        w = eng.last_weights
        assert w is not None and w.shape == (8,)
        assert torch.equal(w, gar.arc_weights(eng.G.float(), 2, rule, nnm=pre == "arc+nnm"))
        assert float(w.double().sum()) <= 1.0 + 1e-6
    assert torch.isfinite(eng.flat_model()).all()


@pytest.mark.parametrize("pre,rule", [("arc", "trimmed-mean"), ("arc", "median"), ("arc+nnm", "trimmed-mean")])
def test_engine_cpu_coordinate_wise(pre, rule):
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar=rule, f=2, workers_per_rank=8, byzantine={7: "reverse"}, lr=0.05,
                                          momentum=0.0, weight_decay=0.0, pre_aggregation=pre))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    before = eng.flat_model().clone()
    eng.step(b)
    assert eng.last_weights is None
    g = gar.arc_coord(eng.G.float(), 2, rule, pre == "arc+nnm")
    torch.testing.assert_close(eng.flat_model(), before - 0.05 * g[: eng.d], rtol=1e-6, atol=1e-7)


def test_engine_update_from_rows_cpu():
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="krum", f=1, workers_per_rank=6, pre_aggregation="arc"))
    rows = [r.clone() for r in latent(6, eng.d, 8)]
    before = eng.flat_model().clone()
    eng._update_from_rows(rows)
    assert torch.equal(eng.last_weights, gar.arc_weights(torch.stack(rows), 1, "krum"))
    assert not torch.equal(before, eng.flat_model())


def test_engine_rejects_unsupported():
    def make(pre, **kw):
        return RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                  EngineConfig(f=2, workers_per_rank=9, pre_aggregation=pre, **kw))

    for pre in ("arc", "arc+nnm"):
        for rule in ("bulyan", "brute", "aksel", "averaged-median"):
            with pytest.raises(ValueError, match="not yet supported"):
                make(pre, gar=rule)
        with pytest.raises(ValueError, match="not yet supported with layerwise"):
            make(pre, gar="krum", layerwise=True)
        assert make(pre, gar="krum").cfg.pre_aggregation == pre
    with pytest.raises(ValueError, match="not yet supported"):
        make("arc+nnm", gar="dnc")
    with pytest.raises(ValueError, match="not yet supported"):
        make("arc+nnm", gar="median")
    with pytest.raises(ValueError, match="unknown pre_aggregation"):
        make("nnm+arc", gar="krum")
    with pytest.raises(ValueError, match="selected gradients"):   # the registry's check of arc-krum
        make("arc", gar="krum", m=7)
    assert make("arc", gar="median")._rule_name() == "arc-median"
    assert make("arc+nnm", gar="trimmed-mean")._rule_name() == "arc-nnm-trimmed-mean"


def test_apps_flag():
    import argparse

    from garfield_amd.apps.common import add_common, gar_name

    for pre, name in (("arc", "arc-krum"), ("arc+nnm", "arc-nnm-krum"), ("nnm", "nnm-krum")):
        a = add_common(argparse.ArgumentParser()).parse_args(["--gar", "krum", "--pre_aggregation", pre])
        assert gar_name(a) == name and name in aggregators.gars
    with pytest.raises(SystemExit):
        add_common(argparse.ArgumentParser()).parse_args(["--gar", "krum", "--pre_aggregation", "bucketing"])
    from garfield_amd.apps import garfield_cc

    src = open(garfield_cc.__file__).read()
    assert 'choices=["nnm", "arc", "arc+nnm"]' in src


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


SHARDED = (("arc", "krum"), ("arc", "average"), ("arc", "geomed"), ("arc+nnm", "krum"), ("arc", "trimmed-mean"))


def _rank_worker(rank, world, port, outdir, shard):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from garfield_amd.parallel.comm import init_distributed, shutdown

    ctx = init_distributed(backend="gloo", device="cpu")
    out = {}
    for pre, rule in SHARDED:
        torch.manual_seed(0)
        eng = RobustDataParallel(build_model("mlp"), F.nll_loss, ctx,
                                 EngineConfig(gar=rule, f=1, workers_per_rank=3, byzantine={3: "reverse"},
                                              shard_gar=shard, lr=0.05, pre_aggregation=pre))
        assert (eng._shard is not None) == shard
        b = synthetic_batches(3, 8, (1, 28, 28), 10, "cpu", seed=rank)
        for _ in range(2):
            eng.step(b)
        w = eng.last_weights
        out[pre + rule] = {"flat": eng.flat_model().clone(), "sum": eng.replica_checksum(),
                           "w": None if w is None else w.clone().float()}
    torch.save(out, os.path.join(outdir, f"{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_two_rank_sharded_vs_unsharded():
    """2 gloo ranks x 3 workers: the scales come from the squared norms summed over ranks beside the distances,
    so every rank gets the same scales and the same w (replicas bitwise identical). Krum's and the average's
    weights are c_j times a rational: sharded and unsharded are bitwise equal unless a norm's fp64 sum, taken in
    another order, crosses an fp32 rounding boundary of c. The geometric median's are continuous in
    distances summed in another order: 1e-5 relative, as the NNM rehearsal."""
    world = 2
    with tempfile.TemporaryDirectory() as d:
        for shard in (False, True):
            mp.spawn(_rank_worker, args=(world, free_port(), d, shard), nprocs=world, join=True)
        res = {(s, r): torch.load(os.path.join(d, f"{s}r{r}.pt"), weights_only=True)
               for s in (0, 1) for r in range(world)}
        for pre, rule in SHARDED:
            key = pre + rule
            for s in (0, 1):
                assert res[(s, 1)][key]["sum"] == res[(s, 0)][key]["sum"], (key, s)
                assert torch.equal(res[(s, 1)][key]["flat"], res[(s, 0)][key]["flat"]), (key, s)
                if res[(s, 0)][key]["w"] is not None:
                    assert torch.equal(res[(s, 1)][key]["w"], res[(s, 0)][key]["w"]), (key, s)
            red, sh = res[(0, 0)][key], res[(1, 0)][key]
            if rule == "trimmed-mean":
                assert sh["w"] is None and red["w"] is None
            else:
                assert sh["w"].shape == red["w"].shape == (6,)
                assert float(sh["w"].double().sum()) <= 1.0 + 1e-6
                if rule == "geomed":
                    assert relerr(sh["w"], red["w"]) < 1e-5
                else:
                    assert torch.equal(sh["w"], red["w"]), (key, sh["w"], red["w"])
            torch.testing.assert_close(sh["flat"], red["flat"], rtol=1e-5, atol=1e-7)


def test_sharded_f0_is_the_plain_step():
    """ARC with f = 0 in front of a coordinate-wise rule clips nothing: the sharded step takes the path
    without it (no distances, no all-reduce) and gives the same bits."""
    outs = []
    for pre, f in ((None, 0), ("arc", 0), ("arc", 1)):
        torch.manual_seed(0)
        eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                 EngineConfig(gar="median", f=f, workers_per_rank=5, shard_gar=True, lr=0.05,
                                              pre_aggregation=pre))
        assert eng._shard is not None and eng._shard._pre_aggregates(eng.cfg) == (pre is not None and f > 0)
        for it in range(2):
            eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, "cpu", seed=11 + it))
        outs.append(eng.flat_model().clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
