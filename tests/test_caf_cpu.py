"""CAF covariance-filter GAR on the CPU: the fp64 oracle on D against the d x d weighted covariance on the
vectors, the C++ filter against the oracle, the exact consequences of the semantics (docs/GAR_SEMANTICS.md
"Covariance filter"), the registry, the class interface, arc-caf and the engine.

Inputs and preconditions: tests/_caf_common.py. Every case that compares a decision of the filter (pass
count, pass kept, exact zeros) first asserts the three preconditions on the oracle's trace."""
import math

import pytest
import torch
import torch.nn.functional as F

from _caf_common import SEEDS, assert_preconditions, attacked, case
from garfield_amd import aggregators
from garfield_amd.models import build_model
from garfield_amd.ops import gar, selection
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

SIZES = (3, 4, 5, 8, 16, 17, 33, 64, 65, 127, 128, 130)
DIMS = (64, 2000)


def uniform(n, ids=None):
    """The fp32 weight vector with 1 / |ids| on ``ids`` (default: all rows)."""
    ids = list(range(n) if ids is None else ids)
    w = torch.zeros(n, dtype=torch.float64)
    w[ids] = 1.0 / len(ids)
    return w.float()


@pytest.mark.parametrize("n", [5, 9])
def test_oracle_on_distances_equals_covariance_on_vectors(n):
    """The first pass (uniform a) and a later pass (the fractional a the filter reaches after one update):
    λ and τ from the n x n iteration equal those of the d x d weighted covariance."""
    f = (n - 1) // 2
    X = attacked(n, f, 40).double()
    D, valid = ref._caf_distances(ref.pairwise_sqdist(X))
    a = torch.full((n,), 1.0 / n, dtype=torch.float64)
    for later in (False, True):
        lam, tau = ref.caf_pass(D, valid, a, 400)
        lam_d, tau_d = ref.caf_dense_pass(X, a)
        err = float((tau - tau_d).abs().max() / tau_d.max())
        print(f"n={n} later={later}: lambda {lam:.12g} / {lam_d:.12g}, tau error {err:.3e}")
        assert abs(lam - lam_d) <= 1e-9 * lam_d and err <= 1e-9
        c = a * (1.0 - tau / tau.max())
        a = c / c.sum()
        assert 0 < int((a > 0).sum()) < n and len(set(a.tolist())) > 2   # fractional, one exact zero


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("n", SIZES)
def test_cpp_matches_oracle(native, n, d):
    for f in sorted({(n - 1) // 4, (n - 1) // 2}):
        X, trace, w, lams, _ = case(n, d, torch.float32, f)
        D = ref.pairwise_sqdist(X)
        wc, lc = native.cpu_caf_weights(D, f, 16, 0)
        assert wc.dtype == torch.float32 and lc.dtype == torch.float32
        fin = torch.isfinite(lams)
        assert torch.equal(torch.isfinite(lc), fin) and int(fin.sum()) == len(trace["lams"])   # the pass count
        assert torch.equal(wc == 0, w == 0)
        assert float((wc.double() - w.double()).abs().max()) <= 1e-12 * float(w.max())
        if fin.any():
            assert float(((lc[fin].double() - lams[fin].double()).abs() / lams[fin].double()).max()) <= 1e-12
        # the public entry (C++ distances up to 128 rows) runs the same filter
        wp = gar.caf_weights(X, f)
        assert torch.equal(wp == 0, w == 0) and float((wp.double() - w.double()).abs().max()) <= 1e-6 * float(w.max())
        wo, lo = ref.caf_weights(D, f)
        assert torch.equal(wo, w) and torch.equal(lo, lams)


@pytest.mark.parametrize("n,d,f", [(16, 64, 3), (33, 2000, 8), (64, 64, 15), (128, 2000, 63)])
def test_colluders_are_filtered(n, d, f):
    X, trace, w, lams, _ = case(n, d, torch.float32, f)
    w = w.double()
    assert float(w.min()) >= 0.0 and abs(float(w.sum()) - 1.0) <= 1e-6
    assert float(w[n - f:].sum()) < 0.02 and int((w == 0).sum()) >= 1
    # every pass zeroes at least one more row; the kept pass is the first of smallest λ
    assert 1 <= len(trace["lams"]) <= n and int((w == 0).sum()) >= trace["best"]
    assert trace["lams"][trace["best"]] == min(trace["lams"])


def test_f_zero_is_the_average(native):
    for n in (1, 2, 9):
        X = attacked(n, 0, 200)
        D = ref.pairwise_sqdist(X)
        for w, lams in (ref.caf_weights(D, 0), native.cpu_caf_weights(D, 0, 16, 0)):
            assert torch.equal(w, uniform(n)) and lams.tolist() == [math.inf] * n
        assert torch.equal(gar.caf_weights(X, 0), uniform(n))
        # the CPU average is torch's mean, not the combine with the weights 1/n: the same up to fp32 rounding
        # (on the GPU both are the combine kernel: bit for bit, tests/test_caf_gpu.py)
        assert torch.equal(gar.caf(X, 0), gar.combine(X, uniform(n)))
        torch.testing.assert_close(gar.caf(X, 0), gar.average(X), rtol=1e-6, atol=1e-6)


def test_max_passes(native):
    X, trace, w, lams, _ = case(33, 2000, torch.float32, 16)
    D = ref.pairwise_sqdist(X)
    assert len(trace["lams"]) >= 4
    for fn in (lambda mp: ref.caf_weights(D, 16, max_passes=mp), lambda mp: native.cpu_caf_weights(D, 16, 16, mp)):
        w1, l1 = fn(1)   # one pass: the weights it started from
        assert torch.equal(w1, uniform(33)) and int(torch.isfinite(l1).sum()) == 1 and float(l1[0]) == float(lams[0])
        w3, l3 = fn(3)
        assert torch.equal(l3[:3], lams[:3]) and int(torch.isfinite(l3).sum()) == 3
        wn, ln = fn(33)
        assert torch.equal(wn, w) and torch.equal(ln, lams)
    assert torch.equal(native.cpu_caf_weights(D, 16, 16, 0)[0], native.cpu_caf_weights(D, 16, 16, 1000)[0])
    assert torch.equal(gar.caf_weights(X, 16, max_passes=1), uniform(33))


def test_identical_rows(native):
    X = torch.randn(1, 50, generator=torch.Generator().manual_seed(3)).repeat(7, 1)
    D = ref.pairwise_sqdist(X)
    for w, lams in (ref.caf_weights(D, 2), native.cpu_caf_weights(D, 2, 16, 0)):
        assert torch.equal(w, uniform(7)) and lams.tolist() == [0.0] + [math.inf] * 6   # one pass, λ = 0
    assert torch.equal(gar.caf_weights(X, 2), uniform(7))


def test_non_finite_rows(native):
    X = attacked(9, 1, 500)
    X[4, 17] = math.nan
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    D = ref.pairwise_sqdist(X)
    Dk = ref.pairwise_sqdist(X[keep])
    # f = 1: 8 valid rows against n - 2f = 7, one pass runs; with a second non-finite row the budget is used up
    for f in (1, 2, 3):
        trace = ref.caf_trace(D, f)
        assert_preconditions(trace, 9, f)
        w, lams = ref.caf_weights(D, f)
        assert float(w[4]) == 0.0 and len(trace["lams"]) >= 1 and abs(float(w.double().sum()) - 1.0) <= 1e-6
        # the first pass sees the valid rows as if the NaN row were absent
        assert abs(trace["lams"][0] - ref.caf_trace(Dk, 1)["lams"][0]) <= 1e-12 * trace["lams"][0]
        wc, lc = native.cpu_caf_weights(D, f, 16, 0)
        assert torch.equal(wc == 0, w == 0) and float((wc.double() - w.double()).abs().max()) <= 1e-12
        assert torch.equal(torch.isfinite(lc), torch.isfinite(lams))
        out = gar.caf(X, f)
        assert torch.isfinite(out).all()
        ex = ref.combine(X[keep], w.double()[keep])
        assert (out.double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())
    X[6, 3] = math.inf
    D = ref.pairwise_sqdist(X)
    for w, lams in (ref.caf_weights(D, 1), native.cpu_caf_weights(D, 1, 16, 0)):   # 7 valid rows, n - 2f = 7: no pass
        assert torch.equal(w, uniform(9, [0, 1, 2, 3, 5, 7, 8])) and lams.tolist() == [math.inf] * 9
    # every pair non-finite: uniform 1/n
    Dinf = torch.full((3, 3), math.inf, dtype=torch.float64)
    for w, lams in (ref.caf_weights(Dinf, 1), native.cpu_caf_weights(Dinf, 1, 16, 0)):
        assert torch.equal(w, uniform(3)) and lams.tolist() == [math.inf] * 3


def test_determinism(native):
    X, trace, w, lams, _ = case(33, 2000, torch.float32, 8)
    D = ref.pairwise_sqdist(X)
    a, b = native.cpu_caf_weights(D, 8, 16, 0), native.cpu_caf_weights(D.clone(), 8, 16, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(gar.caf(X, 8), gar.caf(X.clone(), 8))


@pytest.mark.parametrize("name", ["caf", "native-caf", "arc-caf"])
def test_registry_contract(name):
    X = attacked(9, 2, 700)
    rule = aggregators.gars[name]
    assert callable(rule.check) and callable(rule.checked) and callable(rule.influence) and rule.upper_bound is None
    a = rule(gradients=X, f=2)
    rows = [X[i].clone() for i in range(9)]
    assert torch.equal(a, rule(gradients=rows, f=2))
    assert a.dtype == torch.float32 and a.shape == (700,)
    assert all(a.data_ptr() != r.data_ptr() for r in rows) and a.data_ptr() != X.data_ptr()   # no aliasing
    assert torch.equal(rule(gradients=X, f=2, unknown_option=3), a)
    assert torch.equal(a, gar.aggregate(name.replace("native-", ""), X, f=2))
    arc = name.startswith("arc-")
    ex = ref.arc(X, 2, "caf") if arc else ref.caf(X, 2)
    assert (a.double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())
    w = gar.arc_weights(X, 2, "caf") if arc else gar.caf_weights(X, 2)
    assert abs(rule.influence(rows[:7], rows[7:], f=2) - float(w.double()[7:].sum())) <= 1e-12
    assert rule.influence(rows[:7], rows[7:], f=2) < 0.02
    assert abs(rule.influence(rows[:7], rows[7:], f=0) - 2.0 / 9) < 1e-6
    check = rule.check
    assert "f = 5" in check(gradients=X, f=5) and "f = -1" in check(gradients=X, f=-1)   # n < 2f + 1, f < 0
    assert check(gradients=X, f=4) is None and check(gradients=X, f=0) is None
    for bad in (0, -1, 1.5, True, None):
        assert "iters" in check(gradients=X, f=2, iters=bad)
    for bad in (0, -1, 1.5, True):
        assert "max_passes" in check(gradients=X, f=2, max_passes=bad)
    assert check(gradients=X, f=2, iters=1, max_passes=1) is None and check(gradients=X, f=2, max_passes=None) is None
    Xb = X.bfloat16()
    ob = rule(gradients=Xb, f=2)
    eb = ref.arc(Xb, 2, "caf") if arc else ref.caf(Xb, 2)
    assert ob.dtype == torch.bfloat16 and (ob.double() - eb).abs().max().item() <= 2e-2 * max(1.0, eb.abs().max().item())


def test_class_interface():
    from garfield_amd.aggregators import classreg

    X = attacked(9, 2, 700)
    a = aggregators.gars["caf"](gradients=X, f=2)
    inst = aggregators.instantiate("caf", 9, 2, [])
    assert isinstance(inst, classreg.CAFGAR) and classreg.CAFGAR.rule_name == "caf"
    assert torch.equal(inst.aggregate(X), a) and torch.equal(inst.aggregate(list(X)), a)
    assert torch.equal(aggregators.instantiate("caf", 9, 2, ["iters:3", "max_passes:2"]).aggregate(X),
                       aggregators.gars["caf"](gradients=X, f=2, iters=3, max_passes=2))
    assert not torch.equal(aggregators.instantiate("caf", 9, 2, ["max_passes:1"]).aggregate(X), a)


@pytest.mark.parametrize("n,d", [(9, 500), (33, 2000), (130, 300)])
def test_arc_caf_matches_oracle(n, d):
    f = (n - 1) // 4
    X = attacked(n, f, d)
    X[n - 1] *= 4.0   # a row ARC clips
    w_ref = ref.arc_weights(X, f, "caf")
    c = ref.arc_scales((X.double() * X.double()).sum(1), f)
    assert float(c[n - 1]) < 1.0
    w = gar.arc_weights(X, f, "caf")
    assert torch.equal(w == 0, w_ref == 0) and float(w.double().sum()) < 1.0
    assert float((w.double() - w_ref).abs().max() / w_ref.max()) <= 1e-6
    ex = ref.arc(X, f, "caf")
    assert (gar.aggregate("arc-caf", X, f=f).double() - ex).abs().max().item() <= 1e-5 * max(1.0, ex.abs().max().item())
    # f = 0: no clipping, no pass: the plain average
    assert torch.equal(gar.arc_weights(X, 0, "caf"), uniform(n))


def test_resolve_and_listings():
    from garfield_amd.apps import gar_bench
    from garfield_amd.grpcnet import aggregator
    from garfield_amd.parallel import engine, sharded

    s = selection.resolve("caf", 9, 2)
    assert (s.rule, s.iters, s.max_passes, s.pre) == ("caf", 16, 0, None) and s.device_rows == 128
    assert not s.has_gram_form(True) and not s.has_gram_form(False)
    assert selection.resolve("caf", 9, 2, gar_kwargs={"iters": 4, "max_passes": 3}).max_passes == 3
    assert selection.resolve("caf", 9, 2, gar_kwargs={"max_passes": 50}).max_passes == 9
    assert selection.resolve("caf", 9, 2, pre="arc").clips == selection.arc_count(9, 2)
    for bad in ({"iters": 0}, {"iters": 2.0}, {"iters": True}, {"max_passes": 0}, {"max_passes": 1.5},
                {"max_passes": True}):
        with pytest.raises(ValueError, match="caf"):
            selection.resolve("caf", 9, 2, gar_kwargs=bad)
    for n, f in ((9, 5), (9, -1), (4, 2)):
        with pytest.raises(ValueError, match="n >= 2f"):
            selection.resolve("caf", n, f)
    for pre in ("nnm", "arc+nnm"):
        with pytest.raises(ValueError, match="unsupported rule 'caf'"):
            selection.resolve("caf", 9, 2, pre=pre)
    G = attacked(9, 2, 50)
    for call in (lambda: gar.caf_weights(G, 5), lambda: gar.caf(G, 2, iters=0), lambda: gar.caf(G, 2, max_passes=0)):
        with pytest.raises(ValueError):
            call()
    assert "caf" in gar.RULES and "arc-caf" in gar.RULES and "caf" in gar.ARC_RULES and "caf" not in gar.NNM_RULES
    assert "caf" in gar_bench.RULES and "arc-caf" in gar_bench.RULES and gar_bench.default_f("caf", 8) == 2
    assert gar_bench.default_f("arc-caf", 8) == 2 and aggregator._RULES["CAF"] == "caf"
    assert "caf" in engine.WEIGHTED_RULES and "caf" in engine.LAYERWISE_RULES
    assert "caf" in sharded.DISTANCE_RULES and "caf" in sharded.LAYERWISE_RULES and "caf" in sharded.SUPPORTED
    assert sharded.layerwise_device_ok("caf", 128, 2) and not sharded.layerwise_device_ok("caf", 129, 2)
    mk = lambda **kw: RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                                         EngineConfig(gar="caf", workers_per_rank=8, **kw))
    for pre in ("nnm", "arc+nnm"):
        with pytest.raises(ValueError, match=f"pre_aggregation='{pre}' is not yet supported".replace("+", r"\+")):
            mk(f=2, pre_aggregation=pre)
    with pytest.raises(ValueError):   # the engine runs the registry's check: n >= 2f + 1
        mk(f=4)
    with pytest.raises(ValueError, match="iters"):
        mk(f=2, gar_kwargs={"iters": 0})
    with pytest.raises(ValueError, match="max_passes"):
        mk(f=2, gar_kwargs={"max_passes": 0})


@pytest.mark.parametrize("pre", [None, "arc"])
@pytest.mark.parametrize("layerwise", [False, True])
def test_engine_cpu(layerwise, pre):
    if layerwise and pre:
        with pytest.raises(ValueError, match="layerwise"):
            RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                               EngineConfig(gar="caf", f=2, workers_per_rank=8, layerwise=True, pre_aggregation=pre))
        return
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="caf", f=2, workers_per_rank=8, byzantine={7: "reverse"},
                                          layerwise=layerwise, pre_aggregation=pre))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    before = eng.flat_model().clone()
    for _ in range(2):
        eng.step(b)
        w = eng.last_weights
        assert w is not None
        w = w.reshape(-1, 8)
        segs = sorted(zip(eng.flat.offsets, eng.flat.numels))
        assert w.shape[0] == (len(segs) if layerwise else 1)
        assert float(w.min()) >= 0.0 and float(w.double().sum(1).max()) <= 1.0 + 1e-6
        if layerwise:   # every segment's weights are the rule on that segment's slice of the rows
            for (off, numel), ws in zip(segs, w):
                assert torch.equal(ws, gar.caf_weights(eng.G[:, off:off + numel].float(), 2))
        else:
            assert torch.equal(w[0], gar.caf_weights(eng.G.float(), 2, pre=pre))
            assert float(w[0, 7]) < 0.02   # the reversed gradient is filtered
    assert torch.isfinite(eng.flat_model()).all() and not torch.equal(eng.flat_model(), before)


def test_seed_table():
    """The cases of SEEDS do need another seed: with seed 0 some dtype misses a precondition there."""
    for (n, d, f) in SEEDS:
        missed = 0
        for dtype in (torch.float32, torch.float16):
            try:
                assert_preconditions(ref.caf_trace(ref.pairwise_sqdist(attacked(n, f, d, dtype, 0)), f), n, f)
            except AssertionError:
                missed += 1
        assert missed >= 1, (n, d, f)
