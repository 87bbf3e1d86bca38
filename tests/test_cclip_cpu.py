"""Centered-clipping GAR (clipping rounds iterated on the pairwise distances) on the CPU: the fp64
oracle against centered clipping iterated on the vectors themselves, the C++ weights, the exact
consequences of the semantics, robustness, the registry contract and the engine."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from garfield_amd import aggregators
from garfield_amd.models import build_model
from garfield_amd.ops import gar
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

D_ID = 256
TAU = 8.0   # rows at about 16 from their mean: a radius that clips every row from the mean start
NS = [2, 3, 8, 33, 128]
STARTS = ["mean", "krum", "center"]


def separated(n, d, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(d, generator=g)
    scales = torch.linspace(0.5, 3.0, n)[torch.randperm(n, generator=g)]
    return (base + scales[:, None] * torch.randn(n, d, generator=g)).to(dtype)


def f_of(n):
    return min(max((n - 3) // 2, 0), 3)


def krum_ok(n, f):
    return n >= 2 * f + 3


# every n with every start; Krum's own requirement n >= 2f + 3 leaves no Krum start at n = 2
CASES = [(n, s) for n in NS for s in STARTS if s != "krum" or krum_ok(n, f_of(n))]


def explicit_cc(X, v, tau, f, iters=3):
    """Centered clipping iterated on the vectors themselves (fp64): the centre after ``iters`` rounds."""
    X = X.double()
    n = X.shape[0]
    v = v.double().clone()
    for _ in range(iters):
        diff = X - v
        r = diff.norm(dim=1)
        t = sorted(r.tolist())[max(n - f, 1) - 1] if tau is None else tau
        lam = torch.where(r <= t, torch.ones_like(r), t / r)
        v = v + (lam[:, None] * diff).sum(0) / n
    return v


@functools.lru_cache(maxsize=None)
def problem(n):
    """(rows, a centre vector, fp64 distances of the rows, of the rows + the centre): shared, never modified."""
    X = separated(n, D_ID)
    c = separated(1, D_ID, seed=99)[0] * 0.5
    return X, c, ref.pairwise_sqdist(X), ref.pairwise_sqdist(torch.cat([X, c[None]]))


def start_of(n, start):
    """(all rows, nw, oracle a0, the start vector) of a named start."""
    X, c, D, Dc = problem(n)
    f = f_of(n)
    if start == "center":
        return torch.cat([X, c[None]]), n, [0.0] * n + [1.0], c.double(), Dc
    if start == "krum":
        a0 = ref.krum_weights(D, f)
        return X, n, a0, ref.combine(X, a0), D
    return X, n, None, X.double().mean(0), D


# The identity is exact; only fp64 rounding separates the two routes. The maximum measured over the
# cases below is 6.52e-16 (n = 128); the bound 1e-9 is the one the geometric median's identity test has.
IDENTITY_RTOL = 1e-9


@pytest.mark.parametrize("tau", [TAU, None])
@pytest.mark.parametrize("n,start", CASES)
def test_oracle_equals_explicit_clipping_on_the_vectors(n, start, tau):
    f = f_of(n)
    Xall, nw, a0, v0, D = start_of(n, start)
    w = ref.cclip_weights(D, nw, a0, tau, f, 3)
    assert abs(float(w.sum()) - 1.0) < 1e-12
    out = ref.combine(Xall, w)
    direct = explicit_cc(Xall[:nw], v0, tau, f)
    err = float((out - direct).norm() / direct.norm())
    print(f"cclip identity n={n} start={start} tau={tau}: relative error of the aggregate {err:.3e}")
    assert err < IDENTITY_RTOL
    # the functional oracle takes the same route
    X, c, _, _ = problem(n)
    kw = {"center": c} if start == "center" else {"start": start}
    assert torch.equal(ref.cclip(X, f, tau, 3, **kw), out)


@pytest.mark.parametrize("tau", [TAU, None])
@pytest.mark.parametrize("n,start", CASES)
def test_cpu_weights_match_oracle(native, n, start, tau):
    f = f_of(n)
    Xall, nw, a0, _, D = start_of(n, start)
    w_ref = ref.cclip_weights(D, nw, a0, tau, f, 3)
    a0t = None if a0 is None else torch.as_tensor(a0, dtype=torch.float64)
    w = native.cpu_cclip_weights(D, nw, a0t, 0.0 if tau is None else tau, f, 3)
    assert w.dtype == torch.float32 and w.shape == (Xall.shape[0],)
    assert (w.double() - w_ref).abs().max().item() < 1e-6   # fp32 rounding of the output
    X, c, _, _ = problem(n)
    kw = {"center": c} if start == "center" else {"start": start}
    wf = gar.cclip_weights(X, f, tau, 3, **kw)
    assert (wf.double() - w_ref).abs().max().item() < 1e-6
    out = gar.cclip(X, f, tau, 3, **kw)
    expect = ref.combine(Xall, w_ref)
    assert out.dtype == torch.float32 and out.shape == (D_ID,)
    assert (out.double() - expect).abs().max().item() <= 1e-5 * max(1.0, expect.abs().max().item())


def test_vectorised_path_matches_oracle():
    """More than MAX_ROWS rows (centre included): cclip_weights_from_gram, same semantics."""
    X = separated(130, 300)
    c = separated(1, 300, seed=3)[0]
    D = ref.pairwise_sqdist(X)
    for tau, start in ((None, "mean"), (TAU, "mean"), (None, "krum"), (TAU, "krum")):
        a0 = ref.krum_weights(D, 3) if start == "krum" else None
        w_ref = ref.cclip_weights(D, 130, a0, tau, 3, 3)
        w = gar.cclip_weights(X, 3, tau, 3, start)
        assert w.shape == (130,) and (w.double() - w_ref).abs().max().item() < 1e-6
    w = gar.cclip_weights(X[:128], 3, None, 3, center=c)   # 129 rows
    w_ref = ref.cclip_weights(ref.pairwise_sqdist(torch.cat([X[:128], c[None]])), 128, [0.0] * 128 + [1.0], None, 3, 3)
    assert w.shape == (129,) and (w.double() - w_ref).abs().max().item() < 1e-6
    g = X.double() @ X.double().T
    bad = torch.full((130,), math.nan)
    assert torch.equal(gar.cclip_weights_from_gram(g, 130, bad, None, 3, 3), gar.cclip_weights_from_gram(g, 130, None, None, 3, 3))


def impls(native):
    """The oracle and the C++ behind one signature (D, nw, a0, tau, f, iters) -> fp64 weights."""
    def cpp(D, nw, a0, tau, f, iters):
        a0 = None if a0 is None else torch.as_tensor(a0, dtype=torch.float64)
        return native.cpu_cclip_weights(D, nw, a0, 0.0 if tau is None else tau, f, iters).double()

    def vec(D, nw, a0, tau, f, iters):   # the vectorised path takes a Gram: one whose distances are D
        Dz = torch.where(torch.isfinite(D), D, torch.full_like(D, math.nan))
        Dz.fill_diagonal_(0.0)
        g = -0.5 * Dz
        a0 = None if a0 is None else torch.as_tensor(a0, dtype=torch.float64)
        return gar.cclip_weights_from_gram(g, nw, a0, tau, f, iters).double()

    return {"oracle": ref.cclip_weights, "cpp": cpp, "vectorised": vec}


@pytest.mark.parametrize("impl", ["oracle", "cpp", "vectorised"])
def test_one_round_with_a_huge_radius_is_exactly_uniform(native, impl):
    fn = impls(native)[impl]
    exact = (lambda w, v: torch.equal(w, v)) if impl == "oracle" else (lambda w, v: torch.equal(w.float(), v.float()))
    for n in (3, 8, 33):
        X, c, D, Dc = problem(n)
        uni = torch.full((n,), 1.0 / n, dtype=torch.float64)
        one_hot = [0.0] * n
        one_hot[1] = 1.0
        for a0 in (None, ref.krum_weights(D, 0), one_hot, torch.rand(n, generator=torch.Generator().manual_seed(n))):
            assert exact(fn(D, n, a0, 1e30, 0, 1), uni), (n, impl)
        wc = fn(Dc, n, [0.0] * n + [1.0], 1e30, 0, 1)
        assert exact(wc[:n], uni) and float(wc[n]) == 0.0


@pytest.mark.parametrize("tau", [0.5, 8.0, None])
@pytest.mark.parametrize("start", STARTS)
def test_the_centre_moves_by_at_most_iters_tau(start, tau):
    n, iters = 33, 3
    f = f_of(n)
    Xall, nw, a0, v0, D = start_of(n, start)
    radius = tau
    if tau is None:   # the data-derived radius never exceeds the largest distance met
        radius = max(float((Xall[:nw].double() - v).norm(dim=1).max())
                     for v in [v0] + [ref.combine(Xall, ref.cclip_weights(D, nw, a0, None, f, k)) for k in (1, 2)])
    out = ref.combine(Xall, ref.cclip_weights(D, nw, a0, tau, f, iters))
    moved = float((out - v0).norm())
    assert moved <= iters * radius * (1 + 1e-9)
    if tau == 0.5:   # every row is clipped every round, all from one side at first: it does move
        assert moved > 0.1


@pytest.mark.parametrize("impl", ["oracle", "cpp", "vectorised"])
def test_non_finite_rows(native, impl):
    fn = impls(native)[impl]
    X = separated(9, 500).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    D = ref.pairwise_sqdist(X)
    keep = [0, 1, 2, 3, 5, 7, 8]
    for tau in (TAU, None):
        w = fn(D, 9, None, tau, 2, 3)
        assert float(w[4]) == 0.0 and float(w[6]) == 0.0 and torch.isfinite(w).all()
        wk = ref.cclip_weights(ref.pairwise_sqdist(X[keep]), 7, None, tau, 2, 3)
        assert (w[keep] - wk).abs().max().item() < 1e-6
        # a start that lies entirely on an invalid row falls back to uniform on the valid rows
        on_bad = [0.0] * 9
        on_bad[4] = 1.0
        assert torch.equal(fn(D, 9, on_bad, tau, 2, 3), w)
    out = gar.cclip(X, 2)
    assert torch.isfinite(out).all()
    # all rows non-finite: uniform
    Y = separated(5, 40).clone()
    Y[:, 0] = math.nan
    w = fn(ref.pairwise_sqdist(Y), 5, None, None, 1, 3)
    assert torch.equal(w.float(), torch.full((5,), 0.2))
    assert torch.equal(gar.cclip_weights(Y, 1), torch.full((5,), 0.2))
    # one row alone
    assert torch.equal(gar.cclip_weights(separated(1, 40), 0), torch.ones(1))


def test_determinism(native):
    X = separated(33, 300)
    assert torch.equal(gar.cclip_weights(X, 3, start="krum"), gar.cclip_weights(X, 3, start="krum"))


def attack(seed=0):
    """10 rows, 3 Byzantine at 1e3 x the norm of the honest mean."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(64, generator=g)
    H = mu + 0.1 * torch.randn(7, 64, generator=g)
    B = (-1e3 * mu.norm() * torch.nn.functional.normalize(torch.randn(64, generator=g), dim=0)).expand(3, 64)
    B = B + 0.1 * torch.randn(3, 64, generator=g)
    return torch.cat([H, B]), H.double().mean(0)


def test_robust_start_and_data_radius_beat_the_average(native):
    X, honest = attack()
    out = gar.cclip(X, 3, None, 3, "krum").double()
    avg = X.double().mean(0)
    err, err_avg = float((out - honest).norm()), float((avg - honest).norm())
    print(f"cclip (krum start, data radius): {err:.3e} from the honest mean, the average {err_avg:.3e}")
    assert err * 100 <= err_avg
    assert (out - ref.cclip(X, 3, None, 3, "krum")).norm().item() <= 1e-5 * honest.norm().item()


def test_mean_start_with_a_small_radius_stays_near_the_poisoned_mean(native):
    """Why the robust start exists: from the plain mean, a fixed radius recovers by tau a round."""
    X, honest = attack()
    tau, iters = 1.0, 3
    out = gar.cclip(X, 3, tau, iters, "mean").double()
    avg = X.double().mean(0)
    assert float((out - avg).norm()) <= iters * tau * (1 + 1e-5)
    assert float((out - honest).norm()) > 100.0


def test_registry_and_errors(native):
    for name in ("cclip", "native-cclip", "nnm-cclip", "native-nnm-cclip"):
        assert name in aggregators.gars
        rule = aggregators.gars[name]
        assert callable(rule.check) and callable(rule.checked) and callable(rule.influence)
        assert rule.upper_bound is None
    check = aggregators.gars["cclip"].check
    G = separated(9, 50)
    assert "Byzantine" in check(gradients=G, f=5)
    assert check(gradients=G, f=4) is None
    assert "iterations" in check(gradients=G, f=2, iters=0)
    assert "radius" in check(gradients=G, f=2, tau=0)
    assert "radius" in check(gradients=G, f=2, tau=-1.0)
    assert check(gradients=G, f=2, tau=0.3, iters=5) is None
    assert "start" in check(gradients=G, f=2, start="median")
    assert check(gradients=G, f=3, start="krum") is None
    assert check(gradients=G, f=4, start="krum") is not None          # Krum's own n >= 2f + 3
    assert "selected" in check(gradients=G, f=2, start="krum", m=7)
    assert "both" in check(gradients=G, f=2, start="mean", center=G[0])
    assert check(gradients=G, f=2, start=torch.ones(9)) is None and check(gradients=G, f=2, start=torch.ones(8)) is not None
    assert aggregators.gars["nnm-cclip"].check(gradients=G, f=2, center=G[0]) is not None
    assert aggregators.gars["nnm-cclip"].check(gradients=G, f=2, start="krum") is None
    # the functional interface raises
    for bad in (lambda: gar.cclip_weights(G, 2, start="mean", center=G[0]), lambda: gar.cclip_weights(G, 2, tau=0.0),
                lambda: gar.cclip_weights(G, 2, iters=0), lambda: gar.cclip_weights(G, 4, start="krum"),
                lambda: gar.cclip_weights(G, 2, start="median"), lambda: gar.cclip_weights(G, 2, center=G[0], pre="nnm"),
                lambda: gar.cclip_weights(G, 2, center=torch.zeros(49)), lambda: gar.cclip_weights(G, 2, start=torch.ones(8)),
                lambda: gar.nnm_weights(G, 2, "cclip", start=torch.ones(9))):
        with pytest.raises(ValueError):
            bad()
    # the registry, the class registry and the gRPC names give the functional results
    rows = [G[i].clone() for i in range(9)]
    a = aggregators.gars["cclip"](gradients=G, f=2, start="krum", tau=0.7)
    assert torch.equal(a, gar.cclip(G, 2, 0.7, 3, "krum")) and torch.equal(a, aggregators.gars["cclip"](gradients=rows, f=2, start="krum", tau=0.7))
    assert all(a.data_ptr() != r.data_ptr() for r in rows)
    assert torch.equal(aggregators.gars["nnm-cclip"](gradients=G, f=2), gar.nnm(G, 2, "cclip"))
    assert torch.equal(gar.cclip(G, 2, pre="nnm"), gar.nnm(G, 2, "cclip"))
    assert torch.equal(gar.aggregate("nnm-cclip", G, f=2, start="krum"), gar.nnm(G, 2, "cclip", start="krum"))
    infl = aggregators.gars["cclip"].influence(rows[:7], rows[7:], f=2)
    assert 0.0 < infl < 1.0
    inst = aggregators.instantiate("cclip", 9, 2, ["start:krum", "tau:0.7"])
    assert torch.equal(inst.aggregate(G), a)
    assert torch.equal(aggregators.instantiate("nnm-cclip", 9, 2, []).aggregate(G), gar.nnm(G, 2, "cclip"))
    from garfield_amd.grpcnet.aggregator import Aggregator_tf

    out = Aggregator_tf("CClip", 9, 2).aggregate([r.numpy() for r in rows])
    assert torch.equal(torch.from_numpy(out), gar.cclip(rows, 2))
    out = Aggregator_tf("NNM-CClip", 9, 2).aggregate([r.numpy() for r in rows])
    assert torch.equal(torch.from_numpy(out), gar.nnm(rows, 2, "cclip"))


def test_nnm_cclip_matches_the_oracle_chain(native):
    X = separated(17, 300)
    D = ref.pairwise_sqdist(X)
    sets, Dm = ref.nnm_distances(D, 4)
    for start in ("mean", "krum"):
        for tau in (None, 2.0):
            a0 = ref.krum_weights(Dm, 4) if start == "krum" else None
            w_ref = ref.nnm_row_weights(sets, ref.cclip_weights(Dm, 17, a0, tau, 4, 3))
            w = gar.nnm_weights(X, 4, "cclip", tau=tau, start=start)
            assert (w.double() - w_ref.double()).abs().max().item() < 1e-6
            assert torch.equal(w_ref, ref.nnm_weights(D, 4, "cclip", tau=tau, start=start))


def make_engine(**kw):
    torch.manual_seed(0)
    return RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                              EngineConfig(gar="cclip", f=2, workers_per_rank=8, byzantine={7: "reverse"}, **kw))


@pytest.mark.parametrize("pre", [None, "nnm"])
@pytest.mark.parametrize("gkw", [{}, {"start": "krum"}, {"tau": 0.5, "iters": 2}])
def test_engine_cpu(pre, gkw):
    eng = make_engine(pre_aggregation=pre, gar_kwargs=gkw)
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    for _ in range(3):
        eng.step(b)
        w = eng.last_weights
        assert w is not None and w.shape == (8,)
        expect = gar.cclip_weights(eng.G.float(), 2, gkw.get("tau"), gkw.get("iters", 3), gkw.get("start", "mean"), pre=pre)
        assert torch.equal(w, expect)
        assert abs(float(w.double().sum()) - 1.0) < 1e-6
    assert torch.isfinite(eng.flat_model()).all()


def test_engine_layerwise_and_rows_cpu():
    eng = make_engine(layerwise=True, gar_kwargs={"start": "krum"})
    eng.step(synthetic_batches(8, 16, (1, 28, 28), 10, "cpu"))
    w = eng.last_weights
    assert w.dim() == 2 and w.shape[1] == 8 and ((w.double().sum(1) - 1.0).abs() < 1e-6).all()
    off, numel = eng._segments()[0]
    assert torch.equal(w[0], gar.cclip_weights(eng.G[:, off:off + numel].float(), 2, start="krum"))
    eng = make_engine()
    rows = [r.clone() for r in separated(6, eng.d, seed=8)]
    before = eng.flat_model().clone()
    eng._update_from_rows(rows)
    assert torch.equal(eng.last_weights, gar.cclip_weights(torch.stack(rows), 2))
    assert not torch.equal(before, eng.flat_model())


def test_engine_rejects_bad_arguments():
    with pytest.raises(ValueError, match="center"):
        make_engine(gar_kwargs={"center": torch.zeros(10)})
    with pytest.raises(ValueError, match="start"):
        make_engine(gar_kwargs={"start": "median"})
    with pytest.raises(ValueError, match="start"):
        make_engine(gar_kwargs={"start": torch.ones(8)})
    with pytest.raises(ValueError, match="radius"):
        make_engine(gar_kwargs={"tau": -1.0})
    with pytest.raises(ValueError, match="iterations"):
        make_engine(gar_kwargs={"iters": 0})
    with pytest.raises(ValueError):   # Krum's own check: 8 < 2 * 3 + 3
        RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                           EngineConfig(gar="cclip", f=3, workers_per_rank=8, gar_kwargs={"start": "krum"}))
    with pytest.raises(ValueError, match="layerwise"):
        make_engine(pre_aggregation="nnm", layerwise=True)
