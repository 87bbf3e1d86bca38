"""The pieces the engines' aggregate-and-update step shares: the resolved coordinate-wise rule
(gar.resolve_coord) against the public rules, and the host SGD update (parallel/update.py) applied to a
vector at once against the same update applied slice by slice. No GPU."""
import pytest
import torch

from garfield_amd.ops import gar
from garfield_amd.parallel.engine import EngineConfig
from garfield_amd.parallel.update import SgdUpdate

F, D = 2, 131
SEED = 4242


def rows(n: int) -> torch.Tensor:
    X = torch.randn((n, D), generator=torch.Generator().manual_seed(100 + n))
    X[1, 5], X[1, 77] = float("nan"), float("inf")
    return X


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equal, a NaN equal to a NaN."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.dtype == b.dtype and torch.equal(na, nb) and torch.equal(a.masked_fill(na, 0), b.masked_fill(nb, 0))


# rule, its own keyword arguments, the public call on (X, seed), the resolved (f, beta) for n rows
RULES = {
    "median": ("median", {}, lambda X, seed: gar.median(X), lambda n: (0, 0)),
    "trimmed-mean": ("trimmed-mean", {}, lambda X, seed: gar.trimmed_mean(X, F), lambda n: (F, 0)),
    "averaged-median": ("averaged-median", {}, lambda X, seed: gar.averaged_median(X, F), lambda n: (0, n - F)),
    "averaged-median-beta": ("averaged-median", {"beta": 3}, lambda X, seed: gar.averaged_median(X, F, beta=3),
                             lambda n: (0, 3)),
    "average-nan": ("average-nan", {}, lambda X, seed: gar.average_nan(X), lambda n: (0, 0)),
    "condense": ("condense", {}, lambda X, seed: gar.condense(X, seed=seed), lambda n: (0, 0)),
}


@pytest.mark.parametrize("n", [7, 9])
@pytest.mark.parametrize("case", sorted(RULES))
def test_resolved_rule_is_the_public_rule(case, n):
    rule, kw, public, args = RULES[case]
    X = rows(n)
    expect = public(X, SEED)
    assert expect.shape == (D,) and expect.dtype == torch.float32
    cr = gar.resolve_coord(rule, n, F, kw)
    assert (cr.rule, cr.n, cr.f, cr.beta) == (rule, n, *args(n))
    assert cr.takes_seed == (rule == "condense") and cr.p == (0.9 if rule == "condense" else 1.0)
    assert same_bits(gar._coord(gar.prepare(X), cr, SEED), expect)          # the resolved rule, run
    assert same_bits(gar.aggregate(rule, X, **cr.kwargs(SEED)), expect)     # by name, with its keyword arguments
    if rule == "condense":   # the seed is the call's: another one draws another mask
        assert not same_bits(gar.aggregate(rule, X, **cr.kwargs(SEED + 1)), expect)


def test_resolve_coord_rejects_what_the_kernels_cannot_run():
    for bad in (lambda: gar.resolve_coord("trimmed-mean", 4, 2), lambda: gar.resolve_coord("trimmed-mean", 7, -1),
                lambda: gar.resolve_coord("averaged-median", 7, 2, {"beta": 8}),
                lambda: gar.resolve_coord("krum", 7, 2)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("n", [7, 9])
def test_aksel_count_and_bulyan_sizes(n):
    assert gar.aksel_count(n, F, "mid") == gar.aksel_count(n, F) == (n + 1) // 2
    assert gar.aksel_count(n, F, "n-f") == n - F
    assert gar.bulyan_sizes(n, 1) == (n - 4, n - 6)


def test_aksel_weights_from_distances():
    """1 / c on the c closest, ties by index, non-finite last; batched over leading dimensions."""
    inf, nan = float("inf"), float("nan")
    D = torch.tensor([[3.0, 1.0, nan, 1.0, 0.5], [inf, 2.0, 2.0, 2.0, nan]], dtype=torch.float64)
    w = gar.aksel_weights_from_distances(D, 3)
    kept = torch.tensor([[0, 1, 0, 1, 1], [0, 1, 1, 1, 0]], dtype=torch.float32)
    assert w.dtype == torch.float32 and torch.equal(w, kept * torch.tensor(1.0 / 3, dtype=torch.float32))
    assert torch.equal(gar.aksel_weights_from_distances(D[0], 3), w[0])


HYPER = {"plain": dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
         "momentum": dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False),
         "dampening+wd": dict(momentum=0.9, dampening=0.1, weight_decay=5e-4, nesterov=False),
         "nesterov+wd": dict(momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=True)}


@pytest.mark.parametrize("case", sorted(HYPER))
def test_host_update_by_slices_is_the_update_at_once(case):
    """What sharded == redundant rests on: the update is elementwise, so three shards updated one after
    the other (highest first, as the buckets are ordered) leave the bits of one update of the whole vector."""
    d, ld = 1037, 1040
    hp = HYPER[case]
    up = SgdUpdate(EngineConfig(lr=0.05, **hp), None, torch.device("cpu"))

    def state():   # param, momentum, shadow
        return torch.randn(ld, generator=torch.Generator().manual_seed(1)), torch.zeros(ld), torch.zeros(ld)
    whole, parts = state(), state()
    gen = torch.Generator().manual_seed(7)
    for step in range(3):
        g = torch.randn(d, generator=gen)
        p, mom, sh = whole
        up.host(g, (p[:d], mom[:d], sh), step == 0)            # the engine's target: the shadow is the longer one
        p, mom, sh = parts
        for lo, hi in ((1000, 1037), (64, 1000), (0, 64)):      # the sharded targets: a slice of all three
            up.host(g[lo:hi], (p[lo:hi], mom[lo:hi], sh[lo:hi]), step == 0)
        for a, b in zip(whole, parts):
            assert torch.equal(a, b)
    p, mom, sh = whole
    assert torch.equal(sh[:d], p[:d]) and not sh[d:].any() and not torch.equal(p, state()[0])
    assert bool(mom.any()) == bool(hp["momentum"])
    q = p.clone()
    up.from_vector(g, (q[:d], mom[:d], None), False)           # without the extension: the same host update
    assert not torch.equal(q, p) and torch.equal(sh[:d], p[:d])
