"""Nearest-neighbour mixing on the GPU: k_nnm_mix against the fp64 oracle on the kernel's own Gram
(sets, symmetry, exact zeros, D'), the folded weights and outputs end to end against the oracle on
the vectors, f = 0 and c = 1, the non-finite policy, batched launches, the n > 128 path and the
engine (HIP graph, sharded, a reversed worker)."""
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

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2e-3}
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 16 / 17: the wave-per-row wrap; 64 / 65: the second mask word and lane column; 128: the LDS maximum
SHAPES = [(1, 64, 0), (2, 100, 0), (3, 100, 1), (8, 1000, 2), (16, 4096, 3), (17, 5003, 4), (64, 777, 15),
          (65, 300, 16), (128, 2000, 31), (128, 2000, 1)]
# Seeds (found on the CPU, on the oracle alone) at which the oracle's own choices are well separated:
# see case(). Seed 0 unless listed.
SEEDS = {(16, 4096, 3, torch.bfloat16): 1, (17, 5003, 4, torch.float32): 1, (17, 5003, 4, torch.bfloat16): 1,
         (17, 5003, 4, torch.float16): 1, (128, 2000, 31, torch.float32): 2, (128, 2000, 31, torch.bfloat16): 5,
         (128, 2000, 31, torch.float16): 2, (128, 2000, 1, torch.float32): 2, (128, 2000, 1, torch.bfloat16): 2,
         (128, 2000, 1, torch.float16): 2, (130, 300, 20, torch.float32): 1, (130, 300, 20, torch.float16): 1}
GAP = 1e-4
# Krum after the mix: the weights are rationals k / (m c); only the fp32 rounding of a and w remains.
KRUM_RTOL = 1e-6
# Geometric median after the mix, per-weight relative bound against the fp64 oracle on the vectors:
# 20 x the maximum measured on an MI355X over SHAPES x DTYPES and the n = 130 case (the fp32 Gram's
# rounding of D; the mix and the iteration run in fp64). It may never exceed 1e-4: needing more means
# a bug. The measured maximum is 1.286e-7 (n = 3, d = 100, f = 1, fp32 and bf16; 1.03e-7 at n = 128,
# f = 31, bf16): profiles/r9/nnm/test_weights_error.log.
GEOMED_MEASURED = 1.286e-7
GEOMED_RTOL = 20 * GEOMED_MEASURED
assert GEOMED_RTOL <= 1e-4


def latent(n, d, dtype, seed=0):
    """A latent geometry (4 factors + small noise), on the CPU: neighbour sets differ from row to row
    (per-row noise scales would give every row the same low-noise neighbours)."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(n, 4, generator=g)
    P = torch.randn(4, d, generator=g)
    X = torch.randn(d, generator=g) + Z @ P + 0.05 * torch.randn(n, d, generator=g)
    return X.to(dtype)


def krum_ok(n, f):
    """Krum's own requirement (n >= 2f + 3): (1, 64, 0), (2, 100, 0) and (3, 100, 1) run the other rules."""
    return n >= 2 * f + 3


@functools.lru_cache(maxsize=None)
def case(n, d, f, dtype):
    """(rows on the CPU, oracle row weights and outputs per rule): computed once, shared, never
    modified. Asserts the end-to-end tests' precondition ON THE ORACLE: for every row the c-th and
    (c + 1)-th nearest distances differ by >= GAP relative, and so do the Krum scores on either side
    of the selection (unless they are exactly tied between rows with the same set, which does not
    change w): a set or a selection flipped by the fp32 Gram must not pass as a tolerance problem."""
    X = latent(n, d, dtype, SEEDS.get((n, d, f, dtype), 0))
    D = ref.pairwise_sqdist(X)
    c = n - f
    if f > 0:
        for i in range(n):
            o = sorted(float(D[i, j]) for j in range(n) if j != i)
            inner = o[c - 2] if c >= 2 else 0.0
            assert (o[c - 1] - inner) / o[c - 1] >= GAP, (n, d, f, dtype, i)
    sets, Dm = ref.nnm_distances(D, f)
    rules = ["geomed", "average"] + (["krum"] if krum_ok(n, f) else [])
    if krum_ok(n, f):
        sc = ref.krum_scores(Dm, f)
        o = ref._order(sc)
        lo, hi = o[n - f - 3], o[n - f - 2]
        assert (sc[lo] == sc[hi] and sets[lo] == sets[hi]) or (sc[hi] - sc[lo]) / sc[hi] >= GAP, (n, d, f, dtype)
    out = {}
    for rule in rules:
        w = ref.nnm_weights(D, f, rule)
        out[rule] = (w, ref.combine(X, w.double()))
    return X, out


def relerr(a, b):
    """Maximum relative error; where the reference is exactly zero the value must be too."""
    a, b = a.double().cpu(), b.double().cpu()
    zero = b == 0
    assert (a[zero] == 0).all()
    return ((a - b).abs()[~zero] / b.abs()[~zero]).max().item() if (~zero).any() else 0.0


def close(a, b, dtype):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() <= TOL[dtype] * max(b.abs().max().item(), 1.0)


def own_gram(native, G):
    """The kernel's own Gram of G (pitch gram_padded(n)), cloned out of the workspace."""
    rows = gar.prepare(G)
    return gar._gram_into(native, rows, gar.workspace(rows)).clone()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", SHAPES)
def test_mix_kernel_matches_oracle_on_its_own_gram(cuda, native, n, d, f, dtype):
    """k_nnm_mix alone: the oracle gets the distances of the kernel's own Gram."""
    G = latent(n, d, dtype, SEEDS.get((n, d, f, dtype), 0)).to(cuda)
    D = gar.distances_from_gram(gar.gram(G))
    H, masks = gar.nnm_mix(G, f)
    torch.cuda.synchronize()
    sets, Dm = ref.nnm_distances(D.cpu(), f)
    assert masks.dtype == torch.int64 and masks.shape == (n, 2)
    assert torch.equal(masks.cpu(), gar.masks_from_sets(sets))
    H = H[:n, :n].cpu()
    assert torch.equal(H, H.T) and (torch.diagonal(H) == 0).all()
    same = torch.tensor([[sets[i] == sets[j] for j in range(n)] for i in range(n)])
    assert (H[same] == 0).all()
    rec = -2.0 * H.double()
    m = ~same
    err = ((rec - Dm).abs()[m] / Dm[m]).max().item() if m.any() else 0.0
    print(f"nnm_mix n={n} d={d} f={f} {dtype}: {(int(same.sum()) - n) // 2} duplicate pairs, D' max relative error {err:.3e}")
    assert err <= 1e-6    # the arithmetic is fp64: only the final cast to fp32 rounds


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", SHAPES)
def test_weights_and_output_match_oracle(cuda, native, n, d, f, dtype):
    X, oracle = case(n, d, f, dtype)
    G = X.to(cuda)
    rows = [G[i].clone() for i in range(n)]
    for rule, (w_ref, out_ref) in oracle.items():
        w = gar.nnm_weights(G, f, rule).clone()
        out = gar.nnm(G, f, rule)
        torch.cuda.synchronize()
        assert w.dtype == torch.float32 and w.shape == (n,) and out.dtype == dtype and out.shape == (d,)
        err = relerr(w, w_ref)
        print(f"nnm-{rule} weights n={n} d={d} f={f} {dtype}: max relative error {err:.3e}")
        assert abs(float(w.double().sum()) - 1.0) < 1e-6
        assert err <= (GEOMED_RTOL if rule == "geomed" else KRUM_RTOL)
        assert close(out, out_ref, dtype)
        # list input: the same kernels on a row table
        assert torch.equal(gar.nnm_weights(rows, f, rule), w)
        assert torch.equal(gar.nnm(rows, f, rule), out)


@pytest.mark.parametrize("n,d", [(3, 100), (8, 1000), (17, 5003), (65, 300), (128, 2000)])
def test_f0_equals_average(cuda, native, n, d):
    """c = n: every set is everything, D' = 0 and the folded weights are exactly the average's."""
    G = latent(n, d, torch.float32).to(cuda)
    H, masks = gar.nnm_mix(G, 0)
    assert (H[:n, :n] == 0).all()
    uniform = torch.full((n,), 1.0 / n, device=cuda)
    for rule in ("krum", "geomed", "average"):
        assert torch.equal(gar.nnm_weights(G, 0, rule), uniform), rule
    assert torch.equal(gar.nnm(G, 0, "krum"), gar.average(G))


@pytest.mark.parametrize("n,d", [(8, 1000), (17, 5003), (65, 300), (128, 2000)])
def test_c1_krum_on_pseudo_gram_is_krum_on_gram(cuda, native, n, d):
    """c = 1: D' = D bit for bit, so Krum on H gives the bits of Krum on the Gram."""
    G = latent(n, d, torch.float32).to(cuda)
    g = own_gram(native, G)
    H, masks = gar.nnm_mix(G, n - 1)
    assert torch.equal(masks.cpu(), gar.masks_from_sets([[i] for i in range(n)]))
    res = []
    for src in (g, H.reshape(-1)):
        w = torch.full((n,), -1.0, device=cuda)
        order = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        scores = torch.full((n,), -1.0, device=cuda)
        native.gpu_krum_select(src, n, 2, n - 4, w, order, scores)
        res.append((w, order, scores))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("rule", ["krum", "geomed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(cuda, native, dtype, rule):
    X = latent(9, 500, dtype, 5).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    w_ref = ref.nnm_weights(ref.pairwise_sqdist(X), 2, rule)
    assert float(w_ref[4]) == 0.0 and float(w_ref[6]) == 0.0
    G = X.to(cuda)
    w = gar.nnm_weights(G, 2, rule).clone()
    out = gar.nnm(G, 2, rule)
    torch.cuda.synchronize()
    assert float(w[4]) == 0.0 and float(w[6]) == 0.0
    err = relerr(w, w_ref)
    print(f"nnm-{rule} weights with non-finite rows {dtype}: max relative error {err:.3e}")
    assert err <= (GEOMED_RTOL if rule == "geomed" else KRUM_RTOL)
    assert torch.isfinite(out).all()
    assert close(out, ref.combine(X[keep], w_ref[keep].double()), dtype)


def test_batched_launch_equals_single_launches(cuda, native):
    n, f, L = 17, 4, 5
    np_ = native.gram_padded(n)
    grams = [own_gram(native, latent(n, 900 + 13 * s, torch.float32, seed=s).to(cuda)) for s in range(L)]
    batch = torch.cat(grams)
    assert batch.numel() == L * np_ * np_
    Hb = torch.zeros(L * np_ * np_, device=cuda)
    mb = torch.zeros((L, n, 2), dtype=torch.int64, device=cuda)
    native.gpu_nnm_mix(batch, n, f, Hb, mb, L)
    g = torch.Generator().manual_seed(3)
    a = torch.rand((L, n), generator=g).to(cuda)
    a[:, 2] = 0.0
    wb = torch.full((L, n), -1.0, device=cuda)
    native.gpu_nnm_unmix(a, mb, n, f, wb, L)
    for s in range(L):
        H1 = torch.zeros(np_ * np_, device=cuda)
        m1 = torch.zeros((n, 2), dtype=torch.int64, device=cuda)
        native.gpu_nnm_mix(grams[s], n, f, H1, m1)
        assert torch.equal(H1, Hb[s * np_ * np_:(s + 1) * np_ * np_]) and torch.equal(m1, mb[s])
        w1 = torch.full((n,), -1.0, device=cuda)
        native.gpu_nnm_unmix(a[s].contiguous(), m1, n, f, w1)
        assert torch.equal(w1, wb[s])
        sets = [[j for j in range(n) if (int(m1[i, j >> 6]) >> (j & 63)) & 1] for i in range(n)]
        assert torch.equal(w1.cpu(), ref.nnm_row_weights(sets, a[s].cpu()))
    assert not torch.equal(mb[0], mb[1])
    with pytest.raises(RuntimeError):
        native.gpu_nnm_mix(batch, n, f, Hb[: np_ * np_], mb, L)        # H too small for the batch
    with pytest.raises(RuntimeError):
        native.gpu_nnm_mix(batch, 129, f, Hb, mb, 1)                   # beyond the LDS matrix
    with pytest.raises(RuntimeError):
        native.gpu_nnm_mix(batch, n, n, Hb, mb, 1)                     # f < n
    with pytest.raises(RuntimeError):
        native.gpu_nnm_unmix(a, mb, n, f, wb[:2], L)                   # weights too small for the batch


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_path(cuda, native, dtype):
    """n = 130 > 128: the large Gram kernel, the mix vectorised on the device, the large selection."""
    X, oracle = case(130, 300, 20, dtype)
    G = X.to(cuda)
    for rule, (w_ref, out_ref) in oracle.items():
        w = gar.nnm_weights(G, 20, rule)
        out = gar.nnm(G, 20, rule)
        assert w.is_cuda and w.dtype == torch.float32
        err = relerr(w, w_ref)
        print(f"nnm-{rule} weights n=130 d=300 f=20 {dtype} (large path): max relative error {err:.3e}")
        assert abs(float(w.double().sum()) - 1.0) < 1e-6
        assert err <= (GEOMED_RTOL if rule == "geomed" else KRUM_RTOL)
        assert close(out, out_ref, dtype)


def _run(cuda, rule, steps=3, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar=rule, f=1, workers_per_rank=5, byzantine={4: "reverse"}, lr=0.05, pre_aggregation="nnm",
                       **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("rule", ["krum", "geomed", "average"])
def test_engine_graph_equals_eager(cuda, rule):
    eager = _run(cuda, rule, cuda_graph=False)
    graph = _run(cuda, rule, cuda_graph=True)
    assert torch.equal(eager.last_weights, graph.last_weights)
    assert torch.equal(eager.flat_model(), graph.flat_model())
    assert torch.equal(eager.last_weights, gar.nnm_weights(eager.G, 1, rule))


@pytest.mark.parametrize("rule", ["krum", "geomed"])
def test_engine_reversed_worker(cuda, rule):
    """One reversed worker, f = 1: the weights sum to 1 (n fp32 roundings of values below 1: within
    n x 2^-24) and the Byzantine row weighs less than in the average."""
    eng = _run(cuda, rule, cuda_graph=False)
    w = eng.last_weights.cpu().double()
    print(f"nnm-{rule} engine weights", w.tolist())
    assert abs(float(w.sum()) - 1.0) <= 5 * 2.0 ** -24
    assert float(w[4]) < 1 / 5
    assert torch.isfinite(eng.flat_model()).all()


@pytest.mark.parametrize("rule", ["krum", "geomed", "average"])
def test_engine_sharded_one_rank_vs_unsharded(cuda, rule):
    """The per-bucket partial Grams sum in another order than the whole-row Gram: not bitwise."""
    outs = []
    for shard in (False, True):
        eng = _run(cuda, rule, shard_gar=shard, cuda_graph=False)
        assert (eng._shard is not None) == shard
        outs.append((eng.flat_model().clone(), eng.last_weights.clone().float()))
    (p0, w0), (p1, w1) = outs
    assert w0.shape == w1.shape == (5,)
    print(f"nnm-{rule} sharded vs unsharded: weights", relerr(w1, w0), "models", float((p1 - p0).abs().max()))
    assert relerr(w1, w0) <= (GEOMED_RTOL if rule == "geomed" else KRUM_RTOL)
    torch.testing.assert_close(p1, p0, rtol=1e-5, atol=1e-7)


def test_engine_rejects_sharded_large(cuda):
    with pytest.raises(ValueError, match="not yet supported"):
        RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda),
                           EngineConfig(gar="krum", f=2, workers_per_rank=130, shard_gar=True, pre_aggregation="nnm"))
