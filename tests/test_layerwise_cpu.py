"""The inputs of test_layerwise_gpu.py satisfy what its exact comparisons assume: the job tables are
those of the engines' rules, and every fp64 oracle value is one that the kernels' fp32 arithmetic
reaches without rounding. No GPU."""
from types import SimpleNamespace

import pytest
import torch

import _layerwise_common as lw
from garfield_amd.parallel.engine import LW_JOB
from garfield_amd.parallel.sharded import ShardedAggregator
from garfield_amd.parallel.update import lw_jobs


def fp32_exact(t: torch.Tensor) -> bool:
    return torch.equal(t.float().double(), t)


# ---------------------------------------------------------------------------------------------
# the table and its jobs

def test_table_properties():
    assert lw.OFFS == (0, 1, 4, 12, 19, 83, 92, 155, 220, 230, 360, 4457, 74458) and lw.D == 74458
    lens, starts = set(lw.LENS), lw.OFFS[:-1]
    assert 1 in lens and 8 in lens and {63, 64, 65} <= lens
    assert any(1 < n < 8 for n in lens) and any(n % 8 == 1 and n > 8 for n in lens) and any(n % 8 == 7 for n in lens)
    assert any(o % 2 == 1 for o in starts)                                   # 2-byte aligned 16-bit rows
    assert any(o % 4 != 0 for o in starts)                                   # fp32: 4-byte, not 16-byte aligned
    assert any(o % 2 == 0 and o % 8 != 0 for o in starts)                    # 16 bits: 4-byte, not 16-byte aligned
    assert any(o and o % 8 == 0 for o in starts)                             # 16-byte aligned for both sizes
    assert lw.LENS[lw.LONG] > 2 * LW_JOB and lw.OFFS[lw.LONG] % 2 == 1
    assert len([1 for a, e, s in lw.whole_cut()[0][2] if s == lw.LONG]) == 3
    assert lw.LD % 8 == 0 and lw.LD >= lw.D
    assert all(e % 64 == 0 for e in lw.SHARD_EDGES[:-1])


@pytest.mark.parametrize("kind", sorted(lw.CUTS))
def test_jobs_cover_each_range_once_inside_segments(kind):
    cut = lw.CUTS[kind]()
    owned = torch.zeros(lw.D, dtype=torch.int32)
    for o0, o1, jobs, seg_lo in cut:
        assert len(seg_lo) == lw.L + 1 and seg_lo[0] == 0 and seg_lo[-1] == len(jobs)
        hits = torch.zeros(o1 - o0, dtype=torch.int32)
        for j, (a, e, s) in enumerate(jobs):
            assert 0 <= a < e <= o1 - o0
            assert lw.OFFS[s] <= o0 + a and o0 + e <= lw.OFFS[s + 1]         # inside one segment
            assert seg_lo[s] <= j < seg_lo[s + 1]
            hits[a:e] += 1
            if kind != "arbitrary":                                           # the tail's contract
                assert o0 + a == lw.OFFS[s] or (o0 + a) % 64 == 0
                assert o0 + e == lw.OFFS[s + 1] or (o0 + e) % 64 == 0
        assert bool((hits == 1).all())
        owned[o0:o1] += 1
    assert bool((owned == 1).all())


def test_shard_cuts_split_groups():
    """The cut at 64 splits the 8-wide group [59, 67) of the segment that starts at 19, and every cut
    lies inside a group of some segment (no shard edge is a group edge of the segment it cuts)."""
    assert lw.seg_of(64) == 4 and (64 - lw.OFFS[4]) % 8 == 5
    for edge in lw.SHARD_EDGES[1:-1]:
        s = lw.seg_of(edge)
        assert lw.OFFS[s] < edge < lw.OFFS[s + 1] and (edge - lw.OFFS[s]) % 8 != 0


def test_arbitrary_cut_has_the_named_edges():
    jobs = lw.arbitrary_cut()[0][2]
    starts = {(a, s) for a, _, s in jobs}
    for s in range(lw.L):
        for k in (1, 5, 7):
            if k < lw.LENS[s]:
                assert (lw.OFFS[s] + k, s) in starts
    assert len(jobs) > 3 * lw.L and lw.arbitrary_cut()[0][2] == jobs       # fixed seed


def test_jobs_are_the_engines_rules():
    """The helper's tables against the engines' one builder (parallel/update.py): called as _layerwise_device
    calls it (the whole range) and as ShardedAggregator._lw_plan does (each owned range), and that plan
    itself, run on a stub engine."""
    segs = list(zip(lw.OFFS[:-1], lw.LENS))
    flat = SimpleNamespace(offsets=list(lw.OFFS[:-1]), numels=list(lw.LENS))
    for cut in (lw.whole_cut(), lw.shard_cuts()):
        buckets = [SimpleNamespace(lo=i, own=range(o0, o1), S=o1 - o0) for i, (o0, o1, _, _) in enumerate(cut)]
        stub = SimpleNamespace(e=SimpleNamespace(flat=flat, device=torch.device("cpu")), buckets=buckets)
        plan = ShardedAggregator._lw_plan(stub)
        assert plan["L"] == lw.L and plan["offs"] == list(lw.OFFS)
        for i, (o0, o1, jobs, seg_lo) in enumerate(cut):
            assert lw_jobs(segs, o0, o1) == (jobs, seg_lo)
            assert plan["buckets"][i] == (jobs, seg_lo)
            sid = plan["seg_id"][i]
            assert all(int(sid[a]) == s and int(sid[e - 1]) == s for a, e, s in jobs)
    assert lw_jobs(segs, 0, lw.D) == lw.whole_cut()[0][2:]                   # _layerwise_device
    # a range that is not at local 0: the same jobs, shifted
    o0, o1, jobs, seg_lo = lw.shard_cuts()[2]
    assert lw_jobs(segs, o0, o1, 5) == ([(a + 5, e + 5, s) for a, e, s in jobs], seg_lo)


# ---------------------------------------------------------------------------------------------
# exactness of the inputs

@pytest.mark.parametrize("n", lw.NS)
def test_gram_inputs_are_exact(n):
    X = lw.gram_exact_rows(n)
    for dt in lw.DTYPES:
        assert torch.equal(X.to(dt).float(), X)
    G = lw.gram_fp64(X)
    assert fp32_exact(G) and float(G.abs().max()) < 2 ** 24
    # every partial sum is an integer bounded by sum_k |x_ik x_jk| <= 9 K, below 2^24 as well
    assert 9 * max(lw.LENS) < 2 ** 24
    print(f"n={n}: largest fp64 Gram entry {float(G.abs().max()):.0f}")
    parts = sum(lw.gram_fp64(X, o0, o1) for o0, o1, _, _ in lw.shard_cuts())
    assert torch.equal(parts, G)


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("n", lw.NS)
def test_combine_inputs_are_exact(n, nesterov):
    w = lw.exact_weights(n)
    assert not w[lw.ZERO_SEG].any() and sorted(w[lw.ONE_SEG].tolist())[-2:] == [0.0, 1.0]
    assert all(int((w[s] != 0).sum()) == min(n - 1, 8) for s in range(lw.L) if s not in (lw.ZERO_SEG, lw.ONE_SEG))
    assert len({tuple(w[s].nonzero().flatten().tolist()) for s in range(lw.L)}) > lw.L // 2   # other subsets
    for k in range(2):
        X = lw.combine_exact_rows(n, k)
        for dt in lw.DTYPES:
            assert torch.equal(X.to(dt).float(), X)
    assert not torch.equal(lw.combine_exact_rows(n, 0), lw.combine_exact_rows(n, 1))
    steps, grads = lw.combine_exact_oracle(n, nesterov)
    # an fp32 emulation (one rounded operation at a time) gives the fp64 optimizer's values bit for bit
    p32, b32 = lw.exact_param(), None
    p64, b64 = lw.exact_param().double(), None
    for k, (p, buf) in enumerate(steps):
        g32 = lw.combined_grad(lw.combine_exact_rows(n, k), w, torch.float32)
        assert torch.equal(g32.double(), grads[k])
        p32, b32 = lw.sgd_formula(p32, b32, g32, lw.EXACT_HP, nesterov, k == 0)
        p64, b64 = lw.sgd_formula(p64, b64, grads[k], lw.EXACT_HP, nesterov, k == 0)
        assert p32.dtype == torch.float32 and b32.dtype == torch.float32
        assert torch.equal(p64, p) and torch.equal(b64, buf)                 # the formula is the optimizer's
        assert torch.equal(p32.double(), p) and torch.equal(b32.double(), buf)
        assert fp32_exact(p) and fp32_exact(buf)
    # a third step stays exact too (the margin of the two that the GPU tests run)
    g = lw.combined_grad(lw.combine_exact_rows(n, 0), w)
    p3, b3 = lw.sgd_formula(p64, b64, g, lw.EXACT_HP, nesterov, False)
    assert fp32_exact(p3) and fp32_exact(b3)


def test_momentum_zero_oracle_is_exact():
    steps, _ = lw.combine_exact_oracle(17, False, 0.0)
    assert all(buf is None and fp32_exact(p) for p, buf in steps)


def test_flat_combine_inputs_are_exact():
    for n in (7, 17):
        w = lw.exact_weights(n)[0]
        for k in range(2):
            assert fp32_exact(w.double() @ lw.combine_exact_rows(n, k)[:, :10007].double())


TAIL_SHAPES = lw.TAIL_MFMA + lw.TAIL_SCALAR_BF16


@pytest.mark.parametrize("n,t,beta", TAIL_SHAPES)
def test_tail_inputs_are_exact(n, t, beta):
    assert beta & (beta - 1) == 0
    X, W = lw.tail_exact_rows(n), lw.tail_exact_W(n, t)
    for dt in lw.DTYPES:
        assert torch.equal(X.to(dt).float(), X)
    assert not W[:, :, lw.bad_row(n)].any()
    for s in range(lw.L):
        for k in range(t):
            nz = W[s, k][W[s, k] != 0]
            assert nz.numel() in (1, 2, 4, 8) and bool((nz == 1.0 / nz.numel()).all())   # one common value per row
    assert not torch.equal(W[0], W[1])
    for s in range(lw.L):
        assert fp32_exact(lw.tail_means(X, W, s, lw.OFFS[s], lw.OFFS[s + 1]))
    out = lw.tail_exact_oracle(n, t, beta)
    assert fp32_exact(out)
    # the vectorised oracle is reference._closest_mean: every coordinate of the short segments and every
    # 16th of the long one
    xs = list(range(lw.OFFS[lw.LONG])) + list(range(lw.OFFS[lw.LONG], lw.D, 16))
    for s in range(lw.L):
        cols = [x for x in xs if lw.OFFS[s] <= x < lw.OFFS[s + 1]]
        V = (W[s].double() @ X[:, cols].double())
        assert torch.equal(lw.closest_mean_ref(V, beta), out[cols])


def test_tail_forms():
    for n, t, beta in lw.TAIL_MFMA:
        assert lw.tail_mfma_ok(n, t, beta, torch.bfloat16) and lw.tail_mfma_ok(n, t, beta, torch.float16)
        assert not lw.tail_mfma_ok(n, t, beta, torch.float32)
    assert [(n + 15) // 16 for n, _, _ in lw.TAIL_MFMA] == [1, 2, 3, 4]
    assert [lw.np_for(t) for _, t, _ in lw.TAIL_MFMA] == [8, 16, 32, 64]
    for n, t, beta in lw.TAIL_SCALAR_BF16:
        assert not lw.tail_mfma_ok(n, t, beta, torch.bfloat16)
    n, f = lw.TAIL_RANDN
    assert lw.tail_mfma_ok(n, n - 2 * f - 2, n - 4 * f - 2, torch.bfloat16)


def test_poison_only_touches_the_bad_row():
    n = 17
    X = lw.tail_exact_rows(n)
    P = lw.poison(X)
    bad = ~torch.isfinite(P)
    assert bool(bad[lw.bad_row(n)].any()) and not bool(bad[torch.arange(n) != lw.bad_row(n)].any())
    assert torch.equal(P[~bad], X[~bad])
    groups = set((bad[lw.bad_row(n)].nonzero().flatten() // 64).tolist())
    first, last = (lw.OFFS[lw.LONG] + 63) // 64, lw.D // 64
    assert {g for g in range(first, last) if g % 3 == 0} <= groups
    assert all(bool(bad[lw.bad_row(n), lw.OFFS[s]]) and bool(bad[lw.bad_row(n), lw.OFFS[s + 1] - 1]) for s in range(lw.L))
    kinds = P[lw.bad_row(n)][bad[lw.bad_row(n)]]
    assert bool(torch.isnan(kinds).any()) and bool((kinds == float("inf")).any()) and bool((kinds == float("-inf")).any())


def test_long_job_case():
    n, t, beta = lw.TAIL_MFMA[0]
    X = lw.tail_exact_rows(n, lw.TAIL_LONG_JOB)
    P = lw.poison_every_group(X)
    bad = ~torch.isfinite(P[lw.bad_row(n)])
    assert bool((bad.view(-1, 64).sum(1) == 1).all())
    # 16 workgroups of 4 waves share the job's groups: more than the 32 list slots each
    assert lw.TAIL_LONG_JOB // 64 // (16 * 4) > 32
    W = lw.tail_exact_W(n, t, 1)
    V = lw.tail_means(X, W, 0, 0, lw.TAIL_LONG_JOB)
    out, _ = lw.closest_mean(V, beta)
    assert fp32_exact(V) and fp32_exact(out)
    assert torch.equal(lw.closest_mean_ref(V[:, ::40], beta), out[::40])


def test_tail_randn_case_leaves_out_under_half_a_percent():
    X, W, t, beta, out, bound, keep = lw.tail_randn_case()
    n, f = lw.TAIL_RANDN
    assert (t, beta) == (n - 2 * f - 2, n - 4 * f - 2)
    assert sorted(int((W[0, k] != 0).sum()) for k in range(t)) == list(range(n - f - 2 - t + 1, n - f - 1))
    share = 1 - float(keep.double().mean())
    print(f"tail randn case: {100 * share:.4f} % of the coordinates left out")
    assert share <= 0.005
    xs = list(range(0, lw.D, 37))
    for s in range(lw.L):
        cols = [x for x in xs if lw.OFFS[s] <= x < lw.OFFS[s + 1]]
        if cols:
            V = W[s].double() @ X[:, cols].double()          # the two may sum the beta values in another order
            assert float((lw.closest_mean_ref(V, beta) - out[cols]).abs().max()) <= 2.0 ** -50
