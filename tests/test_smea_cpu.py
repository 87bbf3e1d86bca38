"""SMEA on the CPU: the fp64 oracle against itself, against the DnC loop and against the dense covariance, the
C++ search against the oracle, the rule's behaviour (f = 0, non-finite rows, ties), the colluders Brute cannot
see, the registry contract, the argument checks and the engine. Inputs: tests/_smea_common.py."""
import math
from itertools import combinations

import pytest
import torch
import torch.nn.functional as F

from _smea_common import COLLUDERS_SEED, COLLUDERS_Z, MARGIN, best_of, colluders, members_of, plain, rank_of, rows
from garfield_amd import aggregators
from garfield_amd.models import build_model
from garfield_amd.ops import gar, selection
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

SMALL = [(5, 2), (8, 2), (9, 4)]


def uniform(n):
    return torch.full((n,), 1.0 / n, dtype=torch.float64).float()


def by_mask(n, k):
    return sorted(combinations(range(n), k), key=lambda c: sum(1 << i for i in c))


@pytest.mark.parametrize("n,f", SMALL + [(6, 5), (7, 0), (64, 1)])
def test_subsets_are_in_mask_order(n, f):
    subs = ref.smea_subsets(n, n - f)
    assert subs.tolist() == [list(c) for c in by_mask(n, n - f)]
    for r in (0, len(subs) // 2, len(subs) - 1):
        assert rank_of(subs[r].tolist()) == r


@pytest.mark.parametrize("n,f", SMALL)
def test_oracle_vectorised_equals_scalar(n, f):
    D = ref.pairwise_sqdist(plain(n, 40, torch.float64))
    lams = ref.smea_lambdas(D, f)
    subs = by_mask(n, n - f)
    assert lams.shape == (len(subs),) and lams.dtype == torch.float64
    for r, c in enumerate(subs):
        a = ref.smea_lambda(D, c)
        assert abs(a - float(lams[r])) <= 1e-12 * a, (r, a, float(lams[r]))
    assert torch.equal(ref.smea_lambdas(D, f, chunk=7), lams)   # the chunking is not visible


@pytest.mark.parametrize("n,f", SMALL)
def test_oracle_is_the_dnc_loop_on_the_block(n, f):
    g = torch.Generator().manual_seed(n)   # a planted top direction: the rounds converge
    X = torch.randn(n, 40, generator=g, dtype=torch.float64)
    X += 4.0 * torch.randn(n, 1, generator=g, dtype=torch.float64) * torch.randn(1, 40, generator=g, dtype=torch.float64)
    D = ref.pairwise_sqdist(X)
    for c in by_mask(n, n - f)[:: max(1, math.comb(n, f) // 5)]:
        k = len(c)
        sub = D[list(c)][:, list(c)]
        dist = [[0.0 if a == b else float(sub[a, b]) for b in range(k)] for a in range(k)]
        assert ref.smea_lambda(D, c) == ref._dnc_power(dist, list(range(k)), 16)[0] / k   # the same loop, bit for bit
        # dnc_scores on the block: Σ_i (K u)_i² / λ = λ once the rounds have converged
        lam = float(ref.dnc_scores(sub, 300).sum()) / k
        assert abs(lam - ref.smea_lambda(D, c, 300)) <= 1e-9 * lam


@pytest.mark.parametrize("n,f", SMALL)
def test_gram_identity(n, f):
    """λ from the distances alone is the top eigenvalue of the members' d x d covariance."""
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, 40, generator=g, dtype=torch.float64)
    X += 4.0 * torch.randn(n, 1, generator=g, dtype=torch.float64) * torch.randn(1, 40, generator=g, dtype=torch.float64)
    D = ref.pairwise_sqdist(X)
    for c in by_mask(n, n - f)[:: max(1, math.comb(n, f) // 5)]:
        a, b = ref.smea_lambda(D, c, 200), ref.smea_dense_lambda(X, c)
        assert abs(a - b) <= 1e-9 * b, (c, a, b)
    assert ref.smea_lambda(D, [3]) == 0.0 and ref.smea_dense_lambda(X, [3]) == 0.0


@pytest.mark.parametrize("kind", ["plain", "planted"])
@pytest.mark.parametrize("n,f", SMALL + [(16, 4), (20, 3)])
def test_cpp_matches_oracle(native, n, f, kind):
    X = rows(kind, n, f, 64)
    D = ref.pairwise_sqdist(X)
    lams = ref.smea_lambdas(D, f)
    key, rank, margin = best_of(lams)
    w, lam = native.cpu_smea_weights(D, f, 16)
    assert w.dtype == torch.float32 and lam.shape == (1,)
    assert rank_of(members_of(w)) == rank and torch.equal(w, ref.smea_weights(D, f)[0])
    # the C++ sums in index order, as the scalar oracle: the same fp32 λ
    assert float(lam) == float(torch.tensor(ref.smea_lambda(D, members_of(w))).float()) == float(key[rank])
    if kind == "planted":
        assert margin > MARGIN and members_of(w) == list(range(n - f))
    assert torch.equal(gar.smea_weights(X, f), w)
    ex = ref.smea(X, f)
    assert (gar.smea(X, f).double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())


def test_f_zero_is_the_uniform_combine():
    X = plain(7, 300)
    w = gar.smea_weights(X, 0)
    assert torch.equal(w, uniform(7)) and torch.equal(ref.smea_weights(ref.pairwise_sqdist(X), 0)[0], uniform(7))
    assert torch.equal(gar.smea(X, 0), gar.combine(gar.prepare(X), uniform(7)))
    assert (gar.smea(X, 0) - gar.average(X)).abs().max().item() <= 1e-6   # the CPU's average is torch's mean


def test_non_finite_rows_are_never_selected(native):
    X = plain(9, 120).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    D = ref.pairwise_sqdist(X)
    for f in (2, 3):
        for w in (ref.smea_weights(D, f)[0], native.cpu_smea_weights(D, f, 16)[0], gar.smea_weights(X, f)):
            assert float(w[4]) == 0.0 and float(w[6]) == 0.0 and len(members_of(w)) == 9 - f
        assert torch.isfinite(gar.smea(X, f)).all()
    # more non-finite rows than f: every subset holds one, scores +inf, and rank 0 wins
    w, lam = native.cpu_smea_weights(D, 1, 16)
    wr, lr = ref.smea_weights(D, 1)
    assert members_of(w) == list(range(8)) and torch.equal(w, wr) and math.isinf(float(lam)) and math.isinf(float(lr))
    assert ref.smea_lambda(D, [0, 1, 4]) == math.inf


def test_ties_go_to_the_lowest_rank(native):
    X = plain(6, 50).clone()
    X[5] = X[1]   # two subsets of 5 with the same members up to the duplicate
    D = ref.pairwise_sqdist(X)
    lams = ref.smea_lambdas(D, 1)
    key, rank, _ = best_of(lams)
    twins = [r for r in range(6) if float(key[r]) == float(key[rank])]
    w, _ = native.cpu_smea_weights(D, 1, 16)
    assert rank_of(members_of(w)) == rank == min(twins) and torch.equal(w, ref.smea_weights(D, 1)[0])
    Y = plain(1, 50).repeat(5, 1)   # identical rows: λ = 0 everywhere, rank 0
    w, lam = native.cpu_smea_weights(ref.pairwise_sqdist(Y), 2, 16)
    assert members_of(w) == [0, 1, 2] and float(lam) == 0.0
    w, lam = native.cpu_smea_weights(ref.pairwise_sqdist(X), 5, 16)   # k = 1: λ = 0, row 0
    assert members_of(w) == [0] and float(w[0]) == 1.0 and float(lam) == 0.0


def test_colluders_brute_cannot_see():
    """n = 12, f = 3, d = 200; the three colluders identical at the honest mean + z along one coordinate
    (z and the seed: tests/_smea_common.py). Brute keeps colluders, SMEA keeps none."""
    assert (COLLUDERS_Z, COLLUDERS_SEED) == (17.0, 9)
    X = colluders()
    D = ref.pairwise_sqdist(X)
    honest = list(range(9))
    wb = ref.brute_weights(D, 3)
    assert int((wb[9:] > 0).sum()) >= 1
    lams = ref.smea_lambdas(D, 3)
    key, rank, margin = best_of(lams)
    ws, lam = ref.smea_weights(D, 3)
    assert members_of(ws) == honest and rank == rank_of(honest) and margin > MARGIN
    # on the vectors themselves: the honest rows' covariance has a smaller top eigenvalue than Brute's choice
    assert ref.smea_dense_lambda(X, honest) < ref.smea_dense_lambda(X, members_of(wb))
    assert abs(ref.smea_lambda(D, honest, 200) - ref.smea_dense_lambda(X, honest)) <= 1e-9 * float(lam)
    Xf = X.float()
    assert int((gar.brute_weights(Xf, 3)[9:] > 0).sum()) >= 1 and members_of(gar.smea_weights(Xf, 3)) == honest
    inf = aggregators.gars["smea"].influence
    assert inf(list(Xf[:9]), list(Xf[9:]), f=3) == 0.0 and aggregators.gars["brute"].influence(list(Xf[:9]), list(Xf[9:]), f=3) > 0.0


def test_registry_contract():
    from garfield_amd.aggregators import classreg

    X = rows("planted", 9, 2, 300)
    rule = aggregators.gars["smea"]
    assert "native-smea" in aggregators.gars and rule.upper_bound is None and callable(rule.influence)
    grads = [X[i].clone() for i in range(9)]
    keep = [g.clone() for g in grads]
    out = rule(gradients=grads, f=2)
    assert all(torch.equal(a, b) for a, b in zip(grads, keep))   # the inputs are left alone
    assert all(out.data_ptr() != g.data_ptr() for g in grads)    # and the result aliases none of them
    ex = ref.smea(X, 2)
    assert (out.double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())
    assert torch.equal(aggregators.gars["native-smea"](gradients=grads, f=2), out)
    check = rule.check
    assert check(gradients=grads, f=2) is None and check(gradients=grads, f=0) is None and check(gradients=grads, f=8) is None
    for bad in (-1, 9, 1.5, True, None):
        assert "Invalid number of Byzantine" in check(gradients=grads, f=bad)
    for bad in (0, -1, 1.5, True, None):
        assert "iters" in check(gradients=grads, f=2, iters=bad)
    assert "subsets" in check(gradients=[torch.zeros(3)] * 40, f=20)
    assert check(gradients=[], f=0) is not None
    with pytest.raises(Exception):
        rule.checked(gradients=grads, f=9)
    inst = aggregators.instantiate("smea", 9, 2, [])
    assert isinstance(inst, classreg.SMEAGAR) and classreg.SMEAGAR.rule_name == "smea"
    assert torch.equal(inst.aggregate(X), out) and torch.equal(inst.aggregate(grads), out)
    assert torch.equal(aggregators.instantiate("smea", 9, 2, ["iters:3"]).aggregate(X),
                       rule(gradients=X, f=2, iters=3))
    Xb = X.bfloat16()
    ob, eb = rule(gradients=Xb, f=2), ref.smea(Xb, 2)
    assert ob.dtype == torch.bfloat16 and (ob.double() - eb).abs().max().item() <= 2e-2 * max(1.0, eb.abs().max().item())


def test_resolve_and_listings():
    from garfield_amd.apps import gar_bench
    from garfield_amd.grpcnet import aggregator
    from garfield_amd.parallel import engine, sharded

    s = selection.resolve("smea", 9, 2)
    assert (s.rule, s.n, s.f, s.iters, s.pre) == ("smea", 9, 2, 16, None) and s.device_rows == 64
    assert not s.has_gram_form(True) and not s.has_gram_form(False)
    assert selection.resolve("smea", 9, 0).f == 0 and selection.resolve("smea", 9, 8).f == 8
    assert selection.resolve("smea", 9, 2, gar_kwargs={"iters": 4}).iters == 4
    for bad in (0, -3, 2.0, True, None, "16"):
        with pytest.raises(ValueError, match="smea: expected an int iters"):
            selection.resolve("smea", 9, 2, gar_kwargs={"iters": bad})
    for n, f in ((9, 9), (9, -1), (4, 7), (9, True), (9, 1.0)):
        with pytest.raises(ValueError, match="smea: expected 0 <= f < n"):
            selection.resolve("smea", n, f)
    # the subset cap: C(32, 8) = 10 518 300 is the largest case admitted at n = 32, C(32, 9) is refused
    assert selection.SMEA_MAX_SUBSETS <= 2 ** 24 and selection.SMEA_MAX_SUBSETS & (selection.SMEA_MAX_SUBSETS - 1) == 0
    for n, f in ((40, 20), (64, 8), (128, 5)):
        assert math.comb(n, f) > selection.SMEA_MAX_SUBSETS
        with pytest.raises(ValueError, match="subsets exceeds"):
            selection.resolve("smea", n, f)
    if math.comb(32, 8) <= selection.SMEA_MAX_SUBSETS:
        assert selection.resolve("smea", 32, 8).f == 8
    assert selection.resolve("smea", 100, 1).device_rows == 64   # above 64 rows: the host route, under the same cap
    for pre in ("nnm", "arc", "arc+nnm"):
        with pytest.raises(ValueError, match="unsupported rule 'smea'"):
            selection.resolve("smea", 9, 2, pre=pre)
        with pytest.raises(ValueError, match="unsupported rule 'smea'"):
            gar.smea_weights(plain(9, 20), 2, pre=pre)
    G = plain(9, 50)
    for call in (lambda: gar.smea_weights(G, 9), lambda: gar.smea(G, 2, iters=0), lambda: gar.smea(G, -1)):
        with pytest.raises(ValueError):
            call()
    assert "smea" in gar.RULES and "smea" not in gar.ARC_RULES and "smea" not in gar.NNM_RULES
    assert not any(r.endswith("-smea") for r in gar.RULES) and not any(r.endswith("-smea") for r in aggregators.gars
                                                                       if r != "native-smea")
    assert "smea" in gar_bench.RULES and gar_bench.default_f("smea", 8) == gar_bench.default_f("brute", 8) == 2
    assert aggregator._RULES["SMEA"] == "smea"
    assert "smea" in engine.WEIGHTED_RULES and "smea" in engine.LAYERWISE_RULES
    assert "smea" in sharded.DISTANCE_RULES and "smea" in sharded.SUPPORTED
    assert sharded.layerwise_device_ok("smea", 64, 2) and not sharded.layerwise_device_ok("smea", 65, 2)
    mk = lambda **kw: RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                         EngineConfig(gar="smea", workers_per_rank=8, **kw))
    for pre in ("nnm", "arc", "arc+nnm"):
        with pytest.raises(ValueError, match=f"pre_aggregation='{pre}' is not yet supported".replace("+", r"\+")):
            mk(f=2, pre_aggregation=pre)
    with pytest.raises(ValueError):   # the engine runs the registry's check: f < n
        mk(f=8)
    with pytest.raises(ValueError, match="iters"):
        mk(f=2, gar_kwargs={"iters": 0})


def test_host_route_above_64_rows():
    """n = 65, f = 1: the mask no longer fits one word, the oracle enumerates the 65 subsets."""
    X = rows("planted", 65, 1, 64)
    w = gar.smea_weights(X, 1)
    assert members_of(w) == list(range(64)) and torch.equal(w, ref.smea_weights(ref.pairwise_sqdist(X), 1)[0])


@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_cpu(layerwise):
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="smea", f=2, workers_per_rank=8, byzantine={7: "reverse"},
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
        if layerwise:   # every segment's weights are the rule on that segment's slice of the rows
            for (off, numel), ws in zip(segs, w):
                assert torch.equal(ws, gar.smea_weights(eng.G[:, off:off + numel].float(), 2))
        else:
            assert torch.equal(w[0], gar.smea_weights(eng.G.float(), 2))
            assert float(w[0, 7]) == 0.0 and len(members_of(w[0])) == 6   # the reversed gradient is left out
    assert torch.isfinite(eng.flat_model()).all() and not torch.equal(eng.flat_model(), before)
