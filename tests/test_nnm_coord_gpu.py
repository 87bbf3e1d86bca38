"""Nearest-neighbour mixing in front of a coordinate-wise rule on the GPU: the sets-only launch against
k_nnm_mix's masks, k_nnm_coord against the fp64 oracle on the vectors within the derived bound
(n + 1) 2^-22 A(x) (docs/GAR_SEMANTICS.md "Nearest-neighbour mixing before a coordinate-wise rule"), the
exact properties (f = 0, c = 1, list input, determinism), the non-finite policy, the shape edges, the
n > 128 path, the binding's checks and the engine."""
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

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
RULES = ("trimmed-mean", "median")
# 17: the second MFMA k-step; 33: the second 32-row set block; 64: the MFMA form's limits; 65: the second
# mask word and the LDS form for 16-bit rows; 130: the large path
SMALL = [(3, 100, 1), (8, 1000, 2), (16, 4096, 3), (17, 5003, 4), (33, 517, 8), (64, 777, 15), (65, 300, 16),
         (128, 2000, 31), (128, 2000, 1)]
LARGE = (130, 300, 20)
# Seeds (found on the CPU, on the oracle alone) at which every row's set is well separated: see case().
SEEDS = {(17, 5003, 4, torch.float32): 1, (17, 5003, 4, torch.bfloat16): 1, (17, 5003, 4, torch.float16): 1,
         (128, 2000, 31, torch.float32): 2, (128, 2000, 31, torch.bfloat16): 5, (128, 2000, 31, torch.float16): 2,
         (130, 300, 20, torch.float32): 1, (130, 300, 20, torch.bfloat16): 0, (130, 300, 20, torch.float16): 1}
GAP = 1e-4


def latent(n, d, dtype, seed=0):
    """A latent geometry (4 factors + small noise), on the CPU: neighbour sets differ from row to row
    (per-row noise scales would give every row the same low-noise neighbours)."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, 4, generator=g)
    P = torch.randn(4, d, generator=g)
    X = torch.randn(d, generator=g) + Z @ P + 0.05 * torch.randn(n, d, generator=g)
    return X.to(dtype)


def assert_gaps(D, f, tag, tainted=()):
    """The end-to-end precondition, ON THE ORACLE: for every row the c-th and (c + 1)-th nearest distances
    (the row itself first) differ by >= GAP relative, so that a set flipped by the fp32 Gram cannot pass
    as a tolerance problem. A row without a finite distance (``tainted``) has exact +inf ties, broken by
    index on every path; an infinite (c + 1)-th distance after a finite c-th is an infinite gap."""
    n = D.shape[0]
    c = n - f
    if f == 0:
        return
    for i in range(n):
        if i in tainted:
            continue
        o = sorted(float(D[i, j]) for j in range(n) if j != i)
        lo, hi = (o[c - 2] if c >= 2 else 0.0), o[c - 1]
        assert math.isfinite(lo), (tag, i)
        assert math.isinf(hi) or (hi - lo) / hi >= GAP, (tag, i)


def bound(X, n):
    """(n + 1) 2^-22 A(x), A(x) the largest finite |input| of the coordinate: twice the derived bound."""
    Xd = X.double()
    A = torch.where(torch.isfinite(Xd), Xd.abs(), torch.zeros_like(Xd)).max(0).values
    return (n + 1) * 2.0 ** -22 * A


def check(out, expect, X, n, tag):
    """|out - oracle| <= the bound per coordinate; prints the maximum of error / bound."""
    out = out.double().cpu()
    assert torch.isfinite(out).all(), tag
    b = bound(X, n)
    err = (out - expect).abs()
    ratio = torch.where(b > 0, err / b, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    r = ratio.max().item()
    print(f"nnm_coord {tag}: max error / bound = {r:.4f}"
          + ("  EXCEEDS THE UNDOUBLED BOUND (2n + 2) 2^-24 A" if r > 0.5 else ""))
    assert r <= 1.0, tag
    return r


@functools.lru_cache(maxsize=None)
def case(n, d, f, dtype):
    """(rows on the CPU, the oracle's sets, its output per rule): computed once, shared, never modified."""
    X = latent(n, d, dtype, SEEDS.get((n, d, f, dtype), 0))
    D = ref.pairwise_sqdist(X)
    assert_gaps(D, f, (n, d, f, dtype))
    return X, ref.nnm_sets(D, f), {r: ref.nnm_coord(X, f, r) for r in RULES}


def own_gram(native, G):
    rows = gar.prepare(G)
    return gar._gram_into(native, rows, gar.workspace(rows)).clone()


def sets_of(native, G, f):
    """masks [n, 2] of the sets-only launch on the kernel's own Gram of G."""
    n = len(G) if isinstance(G, (list, tuple)) else G.shape[0]
    masks = torch.zeros((n, 2), dtype=torch.int64, device=G[0].device)
    native.gpu_nnm_sets(own_gram(native, G), n, f, masks)
    return masks


def run(native, G, masks, f, rule, out_dtype=torch.float32):
    """The coordinate kernel alone on the rows G (a row pitch that is no multiple of 16 bytes is padded by
    gar.prepare, as on every GPU path) with the given sets."""
    rows = gar.prepare(G)
    out = torch.full((rows.d,), -777.0, dtype=out_dtype, device=rows.device)
    native.gpu_nnm_coord(rows.obj, masks, rows.n, f, rule, out)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", SMALL)
def test_sets_launch_equals_mix_masks(cuda, native, n, d, f, dtype):
    X, sets, _ = case(n, d, f, dtype)
    g = own_gram(native, X.to(cuda))
    np_ = native.gram_padded(n)
    H = torch.zeros(np_ * np_, device=cuda)
    m_mix = torch.zeros((n, 2), dtype=torch.int64, device=cuda)
    m_sets = torch.full((n, 2), -1, dtype=torch.int64, device=cuda)
    native.gpu_nnm_mix(g, n, f, H, m_mix)
    native.gpu_nnm_sets(g, n, f, m_sets)
    assert torch.equal(m_sets, m_mix)
    assert torch.equal(m_sets.cpu(), gar.masks_from_sets(sets))


def test_sets_launch_batched(cuda, native):
    n, f, L = 17, 4, 3
    np_ = native.gram_padded(n)
    grams = [own_gram(native, latent(n, 900 + 13 * s, torch.float32, seed=s).to(cuda)) for s in range(L)]
    batch = torch.cat(grams)
    Hb = torch.zeros(L * np_ * np_, device=cuda)
    m_mix = torch.zeros((L, n, 2), dtype=torch.int64, device=cuda)
    m_sets = torch.full((L, n, 2), -1, dtype=torch.int64, device=cuda)
    native.gpu_nnm_mix(batch, n, f, Hb, m_mix, L)
    native.gpu_nnm_sets(batch, n, f, m_sets, L)
    assert torch.equal(m_sets, m_mix) and not torch.equal(m_sets[0], m_sets[1])
    for s in range(L):
        one = torch.zeros((n, 2), dtype=torch.int64, device=cuda)
        native.gpu_nnm_sets(grams[s], n, f, one)
        assert torch.equal(one, m_sets[s])
    with pytest.raises(RuntimeError):
        native.gpu_nnm_sets(batch, n, f, m_sets[:2], L)     # masks too small for the batch
    with pytest.raises(RuntimeError):
        native.gpu_nnm_sets(batch, 129, f, m_sets, 1)
    with pytest.raises(RuntimeError):
        native.gpu_nnm_sets(batch, n, n, m_sets, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", SMALL)
def test_kernel_matches_oracle(cuda, native, n, d, f, dtype):
    X, sets, oracle = case(n, d, f, dtype)
    G = X.to(cuda)
    masks = sets_of(native, G, f)
    assert torch.equal(masks.cpu(), gar.masks_from_sets(sets))
    for rule in RULES:
        if rule == "trimmed-mean" and n < 2 * f + 1:
            continue
        out = run(native, G, masks, f, rule)
        check(out, oracle[rule], X, n, f"{rule} n={n} d={d} f={f} {dtype}")
        if dtype != torch.float32:   # the dtype-out form: the fp32 result rounded to nearest even
            assert torch.equal(run(native, G, masks, f, rule, dtype), out.to(dtype))
        # the functional interface: Gram -> sets -> kernel, in the input dtype
        o = gar.nnm_coord(G, f, rule)
        assert o.dtype == dtype and torch.equal(o, out.to(dtype))
        assert torch.equal(gar.aggregate("nnm-" + rule, G, f=f), o)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_path(cuda, native, dtype):
    """n = 130 > 128: the sets from the large Gram, the mixed rows through a bounded fp32 buffer."""
    n, d, f = LARGE
    X, sets, oracle = case(n, d, f, dtype)
    G = X.to(cuda)
    for rule in RULES:
        out = gar._large_nnm_coord(gar.prepare(G), f, rule)
        assert out.dtype == torch.float32 and out.shape == (d,)
        check(out, oracle[rule], X, n, f"{rule} n={n} d={d} f={f} {dtype} (large path)")
        assert torch.equal(gar.nnm_coord(G, f, rule), out.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(3, 100), (8, 1000), (17, 5003), (65, 300), (128, 2000)])
def test_f0_is_the_mean(cuda, native, n, d, dtype):
    X = latent(n, d, dtype)
    mean = X.double().sum(0) / n
    G = X.to(cuda)
    masks = sets_of(native, G, 0)
    assert torch.equal(masks.cpu(), gar.masks_from_sets([list(range(n))] * n))
    for rule in RULES:
        check(run(native, G, masks, 0, rule), mean, X, n, f"{rule} n={n} d={d} f=0 {dtype} (the mean)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d", [(8, 1000), (64, 777), (65, 300)])
def test_c1_median_is_the_median_bitwise(cuda, native, n, d, dtype):
    G = latent(n, d, dtype).to(cuda)
    assert torch.equal(sets_of(native, G, n - 1).cpu(), gar.masks_from_sets([[i] for i in range(n)]))
    assert torch.equal(gar.nnm_coord(G, n - 1, "median"), gar.median(G))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", [(8, 1000, 2), (33, 517, 8), (65, 300, 16)])
def test_list_input_and_determinism(cuda, native, n, d, f, dtype):
    X, _, _ = case(n, d, f, dtype)
    G = X.to(cuda)
    rows = [G[i].clone() for i in range(n)]
    masks = sets_of(native, G, f)
    assert torch.equal(sets_of(native, rows, f), masks)
    for rule in RULES:
        a = run(native, G, masks, f, rule)
        assert torch.equal(run(native, G, masks, f, rule), a)
        assert torch.equal(run(native, rows, masks, f, rule), a)
        assert torch.equal(gar.nnm_coord(rows, f, rule), gar.nnm_coord(G, f, rule))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_non_finite_rows(cuda, native, dtype):
    """f whole rows NaN / +inf / -inf: every finite row's set is the finite rows, exactly the non-finite
    rows' mixed values are non-finite, and both rules leave them out."""
    n, d, f = 16, 200, 3
    X = latent(n, d, dtype, 7).clone()
    X[2] = math.nan
    X[9] = math.inf
    X[13] = -math.inf
    D = ref.pairwise_sqdist(X)
    assert_gaps(D, f, ("rows", dtype), tainted=(2, 9, 13))
    sets = ref.nnm_sets(D, f)
    finite = [i for i in range(n) if i not in (2, 9, 13)]
    assert all(sets[i] == finite for i in finite)
    G = X.to(cuda)
    masks = sets_of(native, G, f)
    assert torch.equal(masks.cpu(), gar.masks_from_sets(sets))
    for rule in RULES:
        check(run(native, G, masks, f, rule), ref.nnm_coord(X, f, rule), X, n, f"{rule} three non-finite rows {dtype}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_single_nan_does_not_leak(cuda, native, dtype):
    """One NaN at one coordinate of an otherwise finite row: with the same sets, every other coordinate
    has the bits of the run without the NaN (0 * NaN inside the MFMA poisons only its own column, and only
    that column is redone), and the coordinate itself matches the oracle."""
    n, d, f, r, x = 16, 200, 3, 5, 77
    clean = latent(n, d, dtype, 7)
    X = clean.clone()
    X[r, x] = math.nan
    D = ref.pairwise_sqdist(X)
    assert_gaps(D, f, ("single", dtype), tainted=(r,))
    sets = ref.nnm_sets(D, f)
    assert all(r not in sets[i] for i in range(n) if i != r)
    G = X.to(cuda)
    masks = sets_of(native, G, f)
    assert torch.equal(masks.cpu(), gar.masks_from_sets(sets))
    others = torch.ones(d, dtype=torch.bool)
    others[x] = False
    for rule in RULES:
        out = run(native, G, masks, f, rule)
        base = run(native, clean.to(cuda), masks, f, rule)
        assert torch.equal(out.cpu()[others], base.cpu()[others])
        check(out, ref.nnm_coord(X, f, rule), X, n, f"{rule} single NaN {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 63, 64, 65])
def test_shape_edges(cuda, native, d, dtype):
    """Nothing outside out[0 : d] is written: sentinels on both sides."""
    n, f = 8, 2
    X = latent(n, d + 64, dtype, 3)
    D = ref.pairwise_sqdist(X[:, :d])
    sets = ref.nnm_sets(D, f)
    # the sets of such short rows come from the oracle: these cases check the coordinate kernel alone
    masks = gar.masks_from_sets(sets).to(cuda)
    G = gar.prepare(X.to(cuda)[:, :d]).obj
    for rule in RULES:
        buf = torch.full((d + 128,), -777.0, device=cuda)
        native.gpu_nnm_coord(G, masks, n, f, rule, buf[64:])
        assert (buf[:64] == -777.0).all() and (buf[64 + d:] == -777.0).all()
        check(buf[64:64 + d], ref.nnm_coord(X[:, :d], f, rule), X[:, :d], n, f"{rule} n={n} d={d} f={f} {dtype}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_grid_stride_wraps(cuda, native, dtype):
    """d beyond one sweep of the capped grid (4096 workgroups x 4 waves x 64 coordinates, or x 256 in the LDS
    form), plus a partial group. The reference here is the oracle's mixed rows with a vectorised fp64
    trimmed mean (sorted, f dropped at each end): the per-coordinate loop would take minutes."""
    n, f, d = 8, 2, 4096 * 4 * 64 + 77
    X = latent(n, d, dtype, 0)
    D = ref.pairwise_sqdist(X)
    assert_gaps(D, f, ("wrap", dtype))
    sets = ref.nnm_sets(D, f)
    Y = ref.nnm_mixed_rows(X, sets)
    expect = torch.sort(Y, dim=0).values[f:n - f].sum(0) / (n - 2 * f)
    G = gar.prepare(X.to(cuda)).obj
    masks = sets_of(native, G, f)
    assert torch.equal(masks.cpu(), gar.masks_from_sets(sets))
    buf = torch.full((d + 64,), -777.0, device=cuda)
    native.gpu_nnm_coord(G, masks, n, f, "trimmed-mean", buf)
    assert (buf[d:] == -777.0).all()
    check(buf[:d], expect, X, n, f"trimmed-mean n={n} d={d} f={f} {dtype} (grid-stride wrap)")


def test_binding_checks(cuda, native):
    n, d, f = 9, 300, 2
    G = gar.prepare(latent(n, d, torch.bfloat16).to(cuda)).obj
    masks = sets_of(native, G, f)
    out = torch.zeros(d, device=cuda)
    native.gpu_nnm_coord(G, masks, n, f, "median", out)
    big = latent(129, 64, torch.bfloat16).to(cuda)
    for bad in (lambda: native.gpu_nnm_coord(big, torch.zeros((129, 2), dtype=torch.int64, device=cuda), 129, f, "median", out[:64]),
                lambda: native.gpu_nnm_coord(G, masks, n, n, "median", out),            # f < n
                lambda: native.gpu_nnm_coord(G, masks, n, 5, "trimmed-mean", out),      # n >= 2f + 1
                lambda: native.gpu_nnm_coord(G, masks[:-1], n, f, "median", out),       # short masks
                lambda: native.gpu_nnm_coord(G, masks, n, f, "median", out[:-1]),       # short out
                lambda: native.gpu_nnm_coord(G, masks, n, f, "krum", out),              # the mode
                lambda: native.gpu_nnm_coord(G, masks.int(), n, f, "median", out),      # int64 masks
                lambda: native.gpu_nnm_coord(G, masks.cpu(), n, f, "median", out),      # device tensors
                lambda: native.gpu_nnm_coord(G, masks, n, f, "median", out.half())):    # fp32 or the rows' dtype
        with pytest.raises(RuntimeError):
            bad()
    native.gpu_nnm_coord(G, masks, n, 4, "trimmed-mean", out)
    native.gpu_nnm_coord(G, masks, n, 8, "median", out)
    torch.cuda.synchronize()


def _run(cuda, rule="trimmed-mean", steps=3, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar=rule, f=1, workers_per_rank=5, byzantine={4: "reverse"}, lr=0.05, pre_aggregation="nnm",
                       **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


def test_engine_graph_equals_eager(cuda):
    eager = _run(cuda, cuda_graph=False)
    graph = _run(cuda, cuda_graph=True)
    assert eager.last_weights is None and graph.last_weights is None
    assert torch.equal(eager.flat_model(), graph.flat_model())
    assert torch.isfinite(eager.flat_model()).all()
    # the aggregate of the last step is the functional interface's on the same rows, in fp32
    rows = gar.prepare(eager.G)
    g = torch.empty(eager.d, device=cuda)
    gar.nnm_coord_into(eager._C, gar.workspace(rows), rows.obj, gar._gram_into(eager._C, rows, gar.workspace(rows)),
                       5, 1, "trimmed-mean", g)
    assert torch.equal(g, eager._gagg[: eager.d])


def test_engine_sharded_one_rank_vs_unsharded(cuda):
    """The per-bucket partial Grams sum in another order than the whole-row Gram, and a bucket's groups of
    64 coordinates start elsewhere: within tolerance, not bitwise."""
    outs = []
    for shard in (False, True):
        eng = _run(cuda, shard_gar=shard, cuda_graph=False)
        assert (eng._shard is not None) == shard and eng.last_weights is None
        outs.append(eng.flat_model().clone())
    print("nnm-trimmed-mean sharded vs unsharded: models", float((outs[1] - outs[0]).abs().max()))
    torch.testing.assert_close(outs[1], outs[0], rtol=1e-5, atol=1e-7)


def test_engine_still_rejects(cuda):
    def make(**kw):
        return RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda),
                                  EngineConfig(f=1, pre_aggregation="nnm", **kw))

    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="median", workers_per_rank=5)
    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="trimmed-mean", workers_per_rank=5, layerwise=True)
    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="trimmed-mean", workers_per_rank=130, shard_gar=True)
