"""Adaptive robust clipping on the GPU: k_arc_scale against the fp64 oracle on the kernel's own Gram (scales,
clipped rows, the clipped Gram, batches), k_arc_apply bit for bit against torch (list and matrix rows, strides,
unaligned ranges, sentinels, the grid-stride wrap), the folded weights and outputs end to end against the
oracle on the vectors, the coordinate-wise form, the non-finite policy, large norms, the n > 128 path, HIP
graph capture and the engine (graph, a reversed worker, sharded, refusals)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import test_cclip_gpu
import test_geomed_gpu
import test_nnm_gpu
from garfield_amd.models import build_model
from garfield_amd.ops import gar
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches
from test_nnm_gpu import DTYPES, GAP, close, latent, own_gram, relerr

pytestmark = pytest.mark.gpu

# 16 / 17: the wave-per-row wrap; 64 / 65: the second lane column; 128: the most rows; f = 63: the most clipped
SHAPES = [(1, 64, 0), (2, 100, 0), (3, 100, 1), (8, 1000, 2), (9, 1000, 3), (16, 4096, 3), (17, 5003, 4),
          (64, 777, 15), (65, 300, 16), (128, 2000, 31), (128, 2000, 63), (128, 2000, 1)]
LARGE = (130, 300, 20)
# Seeds (found on the CPU, on the oracle alone) at which the oracle's own choices are well separated: see case().
# Seed 0 unless listed. With 128 rows one of the 128 set gaps (f = 63) or the Krum gap behind the mixing
# (f = 1: the mixed rows are means of 127 of the 128 rows and all but coincide) is below GAP at most seeds.
SEEDS = {(130, 300, 20, torch.bfloat16): 3,
         (128, 2000, 63, torch.float32): 1, (128, 2000, 63, torch.bfloat16): 3, (128, 2000, 63, torch.float16): 1,
         (128, 2000, 1, torch.float32): 7, (128, 2000, 1, torch.bfloat16): 2, (128, 2000, 1, torch.float16): 10}
# The scales against the fp64 oracle on the vectors, relative: 20 x the maximum measured on an MI355X over
# SHAPES x DTYPES and the n = 130 case (the fp32 Gram's rounding of the two norms; the division, the root and the
# cast are correctly rounded). It may never exceed 1e-4: needing more means a bug. The measured maximum is
# 3.213e-7 (n = 128, d = 2000, f = 31, fp32; 2.09e-7 in bf16 there): profiles/r18/arc/test_scale_error.log.
SCALE_MEASURED = 3.213e-7
SCALE_RTOL = 20 * SCALE_MEASURED
assert SCALE_RTOL <= 1e-4
# A rule's weights: the scales' bound plus the rule's own, from its test module. Krum's, DnC's and the average's
# weights over the clipped rows are rationals (1 / m, 1 / kv, 1 / n): only their fp32 rounding remains.
RULE_RTOL = {(False, "krum"): test_nnm_gpu.KRUM_RTOL, (False, "dnc"): test_nnm_gpu.KRUM_RTOL,
             (False, "average"): test_nnm_gpu.KRUM_RTOL, (False, "geomed"): test_geomed_gpu.WEIGHT_RTOL,
             (False, "cclip"): test_cclip_gpu.WEIGHT_RTOL,
             (True, "krum"): test_nnm_gpu.KRUM_RTOL, (True, "average"): test_nnm_gpu.KRUM_RTOL,
             (True, "geomed"): test_nnm_gpu.GEOMED_RTOL, (True, "cclip"): test_cclip_gpu.NNM_RTOL}
COORD = ("trimmed-mean", "median")


def seed_of(n, d, f, dtype):
    return SEEDS.get((n, d, f, dtype), 0)


def sqnorms(X):
    X = X.double()
    return (X * X).sum(1)


@functools.lru_cache(maxsize=None)
def case(n, d, f, dtype):
    """(rows on the CPU, oracle scales, {(nnm, rule): (oracle row weights, oracle output)}): computed once,
    shared, never modified. Asserts the end-to-end tests' preconditions ON THE ORACLE, so that a flipped choice
    cannot pass as a tolerance problem: the squared norms on either side of the cut differ by >= GAP relative;
    after clipping, for every row the c-th and (c + 1)-th nearest distances differ by >= GAP relative, and so do
    the Krum scores on either side of the selection, plain and mixed (unless exactly tied between rows with the
    same set). DnC's own selection gap is asserted where DnC is compared."""
    X = latent(n, d, dtype, seed_of(n, d, f, dtype))
    s = sqnorms(X)
    k = ref.arc_count(n, f)
    if k:
        o = sorted(s.tolist(), reverse=True)
        assert (o[k - 1] - o[k]) / o[k - 1] >= GAP, (n, d, f, dtype)
    c = ref.arc_scales(s, f)
    assert len(ref.arc_clip_rows(c)) == k
    cd = c.double()
    D = ref.pairwise_sqdist(cd[:, None] * X.double())
    cnt = n - f
    if f > 0:
        for i in range(n):
            o = sorted(float(D[i, j]) for j in range(n) if j != i)
            inner = o[cnt - 2] if cnt >= 2 else 0.0
            assert (o[cnt - 1] - inner) / o[cnt - 1] >= GAP, (n, d, f, dtype, i)
    sets, Dm = ref.nnm_distances(D, f)
    krum = n >= 2 * f + 3
    if krum:
        for dist, tied in ((D, lambda a, b: False), (Dm, lambda a, b: sets[a] == sets[b])):
            sc = ref.krum_scores(dist, f)
            o = ref._order(sc)
            lo, hi = o[n - f - 3], o[n - f - 2]
            assert (sc[lo] == sc[hi] and tied(lo, hi)) or (sc[hi] - sc[lo]) / sc[hi] >= GAP, (n, d, f, dtype)
    a = {(False, "geomed"): ref.geomed_weights(D), (False, "cclip"): ref.cclip_weights(D, n, None, None, f, 3),
         (False, "average"): torch.full((n,), 1.0 / n, dtype=torch.float64),
         (True, "geomed"): ref.nnm_row_weights(sets, ref.geomed_weights(Dm)),
         (True, "cclip"): ref.nnm_row_weights(sets, ref.cclip_weights(Dm, n, None, None, f, 3)),
         (True, "average"): ref.nnm_row_weights(sets, torch.full((n,), 1.0 / n, dtype=torch.float64))}
    if krum:
        a[(False, "krum")] = ref.krum_weights(D, f)
        a[(True, "krum")] = ref.nnm_row_weights(sets, ref.krum_weights(Dm, f))
    if n >= 2 * f + 1 and n >= 2:
        m = n - f
        sc = sorted(ref.dnc_scores(D, 16).tolist())
        if m == n or sc[m] - sc[m - 1] >= GAP * sc[m]:   # the oracle's own selection is well separated
            a[(False, "dnc")] = ref.dnc_weights(D, m, 16)[0]
    out = {}
    for key, v in a.items():
        w = cd * v.double()
        out[key] = (w, ref.combine(X, w))
    return X, c, out


def scale(native, g, n, f, gram_out=True, batch=1):
    """(scales, clip_rows, G') of k_arc_scale on the device Gram(s) g, every output pre-filled with a sentinel."""
    np_ = native.gram_padded(n)
    scales = torch.full((batch * n,), -7.0, device=g.device)
    clip_rows = torch.full((batch * (n + 1),), -7, dtype=torch.int32, device=g.device)
    G2 = torch.full((batch * np_ * np_,), -7.0, device=g.device) if gram_out else None
    native.gpu_arc_scale(g, n, f, scales, clip_rows, G2, batch)
    return scales, clip_rows, G2


def clip_list(c, n):
    hit = ref.arc_clip_rows(c)
    return torch.tensor([len(hit)] + hit + [-1] * (n - len(hit)), dtype=torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", SHAPES)
def test_scale_kernel_matches_oracle_on_its_own_gram(cuda, native, n, d, f, dtype):
    """k_arc_scale alone: the oracle gets the kernel's own Gram; every operation is correctly rounded, so
    everything is bitwise."""
    G = latent(n, d, dtype, seed_of(n, d, f, dtype)).to(cuda)
    np_ = native.gram_padded(n)
    g = own_gram(native, G)
    g0 = g.clone()
    gm = g.view(np_, np_)[:n, :n].cpu()
    assert torch.equal(gm, gm.T)
    scales, clip_rows, G2 = scale(native, g, n, f)
    torch.cuda.synchronize()
    c = ref.arc_scales(torch.diagonal(gm), f)
    assert torch.equal(scales.cpu(), c)
    assert torch.equal(clip_rows.cpu(), clip_list(c, n))
    assert int(clip_rows[0]) <= ref.arc_count(n, f) and (f > 0 or int(clip_rows[0]) == 0)
    G2 = G2.view(np_, np_)
    assert torch.equal(G2[:n, :n].cpu(), ref.arc_gram(gm, c))
    assert torch.equal(G2[:n, :n], G2[:n, :n].T)
    one = c == 1
    assert torch.equal(G2[:n, :n].cpu()[one][:, one], gm[one][:, one])
    assert (G2[n:] == -7).all() and (G2[:, n:] == -7).all() and torch.equal(g, g0)   # nothing outside n x n, the input intact
    # without an output Gram: the same scales and list; the vectorised form: the same bits
    s1, c1, _ = scale(native, g, n, f, gram_out=False)
    assert torch.equal(s1, scales) and torch.equal(c1, clip_rows)
    assert torch.equal(gar.arc_scales_from_sqnorms(torch.diagonal(g.view(np_, np_)[:n, :n]), f), scales)
    assert torch.equal(gar.arc_scales(G, f), scales)
    # the fold: one fp64 product, rounded once
    a = torch.rand(n, generator=torch.Generator().manual_seed(1)).to(cuda)
    w = torch.full((n,), -7.0, device=cuda)
    native.gpu_arc_fold(a, scales, n, w)
    assert torch.equal(w.cpu(), (c.double() * a.cpu().double()).float())


def test_scale_hand_made_grams(cuda, native):
    """Ties, zero rows, non-finite rows and more than k of them, as diagonals of otherwise arbitrary Grams."""
    inf, nan = math.inf, math.nan
    for s, f in (([7.0, 5.0, 1.0, 5.0, 2.0], 2), ([3.0] * 6, 2), ([0.0, 0.0, 4.0, 0.0], 1), ([0.0] * 5, 2),
                 ([nan, 9.0, 1.0, 4.0, inf, 2.0, 3.0], 3), ([nan, 9.0, 1.0, 4.0, inf, 2.0, 3.0], 2),
                 ([nan, 9.0, inf, 4.0, inf, 2.0, 3.0], 2), ([1.0, 16.0, 4.0, 2.0], 1)):
        n = len(s)
        np_ = native.gram_padded(n)
        g = torch.rand((np_, np_), generator=torch.Generator().manual_seed(n))
        g = g + g.T
        g[range(n), range(n)] = torch.tensor(s)
        c = ref.arc_scales(torch.tensor(s), f)
        scales, clip_rows, G2 = scale(native, g.to(cuda).reshape(-1), n, f)
        assert torch.equal(scales.cpu(), c), (s, f)
        assert torch.equal(clip_rows.cpu(), clip_list(c, n)), (s, f)
        got, want = G2.view(np_, np_)[:n, :n].cpu(), ref.arc_gram(g[:n, :n], c)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))


def test_scale_batched_launch_equals_single_launches(cuda, native):
    n, f, L = 17, 4, 5
    np_ = native.gram_padded(n)
    grams = [own_gram(native, latent(n, 900 + 13 * s, torch.float32, seed=s).to(cuda)) for s in range(L)]
    batch = torch.cat(grams)
    sb, cb, Gb = scale(native, batch, n, f, batch=L)
    a = torch.rand((L, n), generator=torch.Generator().manual_seed(3)).to(cuda)
    wb = torch.full((L, n), -1.0, device=cuda)
    native.gpu_arc_fold(a, sb, n, wb, L)
    for s in range(L):
        s1, c1, G1 = scale(native, grams[s], n, f)
        assert torch.equal(s1, sb[s * n:(s + 1) * n]) and torch.equal(c1, cb[s * (n + 1):(s + 1) * (n + 1)])
        assert torch.equal(G1, Gb[s * np_ * np_:(s + 1) * np_ * np_])
        w1 = torch.full((n,), -1.0, device=cuda)
        native.gpu_arc_fold(a[s].contiguous(), s1, n, w1)
        assert torch.equal(w1, wb[s])
    assert not torch.equal(cb[: n + 1], cb[n + 1:2 * (n + 1)])
    clip32 = torch.zeros(L * (n + 1), dtype=torch.int32, device=cuda)
    for bad in (lambda: native.gpu_arc_scale(batch, n, f, sb[:n], clip32, None, L),            # scales too small for the batch
                lambda: native.gpu_arc_scale(batch, n, f, sb, clip32[: n + 1], None, L),       # the list too small
                lambda: native.gpu_arc_scale(batch, n, f, sb, clip32, Gb[: np_ * np_], L),     # the output Gram too small
                lambda: native.gpu_arc_scale(batch, 129, f, sb, clip32, None, 1),              # beyond the row table
                lambda: native.gpu_arc_scale(batch, n, n, sb, clip32, None, 1),                # f < n
                lambda: native.gpu_arc_scale(batch, n, -1, sb, clip32, None, 1),
                lambda: native.gpu_arc_scale(batch, n, f, sb, clip32.long(), None, 1),         # int32 list
                lambda: native.gpu_arc_scale(batch, n, f, sb.cpu(), clip32, None, 1),          # GPU tensors
                lambda: native.gpu_arc_scale(batch, n, f, sb, clip32, None, 0),
                lambda: native.gpu_arc_fold(a, sb, n, wb[:2], L),                              # weights too small for the batch
                lambda: native.gpu_arc_fold(a, sb, 129, wb, 1)):
        with pytest.raises(RuntimeError):
            bad()


# --------------------------------------------------------------------------- #
# k_arc_apply


def apply_case(cuda, native, n, d, f, dtype, seed=0):
    """(rows on the GPU, scales, clip_rows, the torch-clipped rows): the scales come from the kernel."""
    X = latent(n, d, dtype, seed).to(cuda)
    scales, clip_rows, _ = scale(native, own_gram(native, X), n, f, gram_out=False)
    want = X.clone()
    hit = (scales != 1).nonzero().flatten()
    want[hit] = (X[hit].float() * scales[hit][:, None]).to(dtype)
    return X, scales, clip_rows, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [1, 7, 63, 64, 65, 5003])
def test_apply_matches_torch(cuda, native, d, dtype):
    """Bitwise (x.float() * c).to(dtype) on the clipped rows, every other row and everything around the rows
    untouched: a matrix whose row stride is neither d nor a multiple of 16 bytes, and a list of rows."""
    n, f = 8, 2
    X, scales, clip_rows, want = apply_case(cuda, native, n, d, f, dtype)
    k = int(clip_rows[0])
    assert k == ref.arc_count(n, f) == 3
    pad = torch.full((n, d + 5), 77.0, dtype=dtype, device=cuda)     # stride d + 5: rows of every alignment
    M = pad[:, 2:2 + d]
    M.copy_(X)
    native.gpu_arc_apply(M, scales, clip_rows, f, 0, d)
    assert torch.equal(M, want)
    assert (pad[:, :2] == 77).all() and (pad[:, 2 + d:] == 77).all()
    rows = [X[i].clone() for i in range(n)]
    native.gpu_arc_apply(rows, scales, clip_rows, f, 0, d)
    assert torch.equal(torch.stack(rows), want)
    if d == 1:
        return
    # an unaligned range: nothing outside [lo, hi) is written
    lo, hi = 1, d - 1
    M.copy_(X)
    native.gpu_arc_apply(M, scales, clip_rows, f, lo, hi)
    assert torch.equal(M[:, lo:hi], want[:, lo:hi])
    assert torch.equal(M[:, :lo], X[:, :lo]) and torch.equal(M[:, hi:], X[:, hi:])
    assert (pad[:, :2] == 77).all() and (pad[:, 2 + d:] == 77).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lo,hi", [(3, 4999), (8, 16), (5, 6), (17, 17), (0, 5003), (4001, 5003)])
def test_apply_ranges_and_sentinels(cuda, native, lo, hi, dtype):
    n, d, f = 9, 5003, 3
    X, scales, clip_rows, want = apply_case(cuda, native, n, d, f, dtype)
    rows = [X[i].clone() for i in range(n)]
    native.gpu_arc_apply(rows, scales, clip_rows, f, lo, hi)
    got = torch.stack(rows)
    assert torch.equal(got[:, lo:hi], want[:, lo:hi])
    assert torch.equal(got[:, :lo], X[:, :lo]) and torch.equal(got[:, hi:], X[:, hi:])
    unclipped = (scales == 1).nonzero().flatten()
    assert unclipped.numel() == n - ref.arc_count(n, f) and torch.equal(got[unclipped], X[unclipped])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_apply_wraps_the_grid_stride_loop(cuda, native, dtype):
    """k = 8 clipped rows share the 4096 workgroups: 512 x 256 lanes x 2 trips x one vector per pass and row.
    d is one pass and a bit: the loop wraps once, with a ragged end."""
    n, f = 16, 8
    per_vec = 16 // torch.empty(0, dtype=dtype).element_size()
    d = 512 * 256 * 2 * per_vec + 70001
    g = torch.Generator(device=cuda).manual_seed(0)
    X = torch.randn((n, d), generator=g, device=cuda, dtype=torch.float32)
    X = (X * torch.linspace(0.5, 2.0, n, device=cuda)[:, None]).to(dtype)
    scales, clip_rows, _ = scale(native, own_gram(native, X), n, f, gram_out=False)
    assert int(clip_rows[0]) == ref.arc_count(n, f) == 8
    hit = clip_rows[1:9].long()
    want = X.clone()
    want[hit] = (X[hit].float() * scales[hit][:, None]).to(dtype)
    Y = X.clone()
    native.gpu_arc_apply(Y, scales, clip_rows, f, 0, d)
    assert torch.equal(Y, want)


def test_apply_writes_nothing_without_clipped_rows(cuda, native):
    n, d = 8, 1000
    X = latent(n, d, torch.bfloat16).to(cuda)
    # f = 0: k = 0, no launch at all
    scales, clip_rows, _ = scale(native, own_gram(native, X), n, 0, gram_out=False)
    assert int(clip_rows[0]) == 0 and (clip_rows[1:] == -1).all() and (scales == 1).all()
    Y = X.clone()
    native.gpu_arc_apply(Y, scales, clip_rows, 0, 0, d)
    assert torch.equal(Y, X)
    # equal rows: k = 3 workgroup rows are launched, the device's count is 0 and every one leaves
    E = X[:1].repeat(n, 1).contiguous()
    scales, clip_rows, _ = scale(native, own_gram(native, E), n, 2, gram_out=False)
    assert int(clip_rows[0]) == 0 and (scales == 1).all()
    Y = E.clone()
    native.gpu_arc_apply(Y, scales, clip_rows, 2, 0, d)
    assert torch.equal(Y, E)
    for bad in (lambda: native.gpu_arc_apply(Y, scales, clip_rows, 2, 0, d + 1),     # hi <= row length
                lambda: native.gpu_arc_apply(Y, scales, clip_rows, 2, 5, 4),
                lambda: native.gpu_arc_apply(Y, scales, clip_rows, n, 0, d),         # f < n
                lambda: native.gpu_arc_apply(Y, scales[:4], clip_rows, 2, 0, d),
                lambda: native.gpu_arc_apply(Y, scales, clip_rows[:4], 2, 0, d),
                lambda: native.gpu_arc_apply(Y, scales, clip_rows.long(), 2, 0, d),
                lambda: native.gpu_arc_apply(Y[:1].expand(n, d), scales, clip_rows, 2, 0, d),   # rows that overlap
                lambda: native.gpu_arc_apply(Y.cpu(), scales, clip_rows, 2, 0, d),
                lambda: native.gpu_arc_apply(Y.double(), scales, clip_rows, 2, 0, d)):
        with pytest.raises(RuntimeError):
            bad()


# --------------------------------------------------------------------------- #
# End to end


def check_weights(X, f, dtype, c_ref, oracle, cuda, tag):
    n, d = X.shape
    G = X.to(cuda)
    rows = [G[i].clone() for i in range(n)]
    before = G.clone()
    c = gar.arc_scales(G, f)
    err = relerr(c, c_ref)
    print(f"arc scales n={n} d={d} f={f} {dtype}{tag}: max relative error {err:.3e}")
    assert err <= SCALE_RTOL
    assert torch.equal((c != 1).cpu(), c_ref != 1)
    for (nnm, rule), (w_ref, out_ref) in oracle.items():
        w = gar.arc_weights(G, f, rule, nnm=nnm).clone()
        out = gar.arc(G, f, rule, nnm=nnm)
        torch.cuda.synchronize()
        assert w.dtype == torch.float32 and w.shape == (n,) and out.dtype == dtype and out.shape == (d,)
        werr = relerr(w, w_ref)
        print(f"arc{'-nnm' if nnm else ''}-{rule} weights n={n} d={d} f={f} {dtype}{tag}: max relative error {werr:.3e}")
        assert float(w.double().sum()) <= 1.0 + 1e-6
        assert werr <= SCALE_RTOL + RULE_RTOL[(nnm, rule)]
        assert close(out, out_ref, dtype)
        if n <= gar.MAX_ROWS:   # list input: the same kernels on a row table
            assert torch.equal(gar.arc_weights(rows, f, rule, nnm=nnm), w)
            assert torch.equal(gar.arc(rows, f, rule, nnm=nnm), out)
    assert torch.equal(G, before)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", SHAPES)
def test_weights_and_output_match_oracle(cuda, native, n, d, f, dtype):
    X, c_ref, oracle = case(n, d, f, dtype)
    check_weights(X, f, dtype, c_ref, oracle, cuda, "")


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_path(cuda, native, dtype):
    """n = 130 > 128: the large Gram kernel, the scales, the mix and the rules vectorised on the device."""
    n, d, f = LARGE
    X, c_ref, oracle = case(n, d, f, dtype)
    check_weights(X, f, dtype, c_ref, oracle, cuda, " (large path)")
    G = X.to(cuda)
    for rule in COORD:
        for nnm in (False, True):
            assert close(gar.arc_coord(G, f, rule, nnm), ref.arc_coord(X, f, rule, nnm), dtype)


@pytest.mark.parametrize("n,d", [(3, 100), (8, 1000), (17, 5003), (65, 300), (128, 2000)])
def test_f0_is_the_path_without_arc(cuda, native, n, d):
    G = latent(n, d, torch.bfloat16).to(cuda)
    before = G.clone()
    for rule in ("geomed", "cclip", "dnc", "average") + (("krum",) if n >= 3 else ()):
        plain = {"krum": lambda: gar.krum_weights(G, 0), "geomed": lambda: gar.geomed_weights(G),
                 "cclip": lambda: gar.cclip_weights(G, 0), "dnc": lambda: gar.dnc_weights(G, 0),
                 "average": lambda: torch.full((n,), 1.0 / n, device=cuda)}[rule]().clone()
        assert torch.equal(gar.arc_weights(G, 0, rule), plain), rule
        if rule != "dnc":
            assert torch.equal(gar.arc_weights(G, 0, rule, nnm=True), gar.nnm_weights(G, 0, rule).clone()), rule
    assert torch.equal(gar.arc(G, 0, "average"), gar.average(G))
    assert torch.equal(gar.arc_coord(G, 0, "median"), gar.median(G))
    assert torch.equal(gar.arc_coord(G, 0, "trimmed-mean"), gar.trimmed_mean(G, 0))
    assert torch.equal(gar.arc_coord(G, 0, "trimmed-mean", nnm=True), gar.nnm_coord(G, 0, "trimmed-mean"))
    assert torch.equal(G, before)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,f", [(3, 100, 1), (8, 1000, 2), (17, 5003, 4), (65, 300, 16), (128, 2000, 31)])
def test_coordinate_wise(cuda, native, n, d, f, dtype):
    """gar.arc_coord: bitwise the plain rule (or the mixing's, with the sets of the clipped Gram) on a copy
    clipped with torch from the kernel's own scales, within close() of the oracle on the vectors; the inputs
    are neither modified nor aliased."""
    X = case(n, d, f, dtype)[0]
    G = X.to(cuda)
    before = G.clone()
    np_ = native.gram_padded(n)
    scales, clip_rows, G2 = scale(native, own_gram(native, G), n, f)
    Y = G.clone()
    hit = (scales != 1).nonzero().flatten()
    Y[hit] = (G[hit].float() * scales[hit][:, None]).to(dtype)
    rows = [G[i].clone() for i in range(n)]
    for rule in COORD:
        out = gar.arc_coord(G, f, rule)
        plain = gar.trimmed_mean(Y, f) if rule == "trimmed-mean" else gar.median(Y)
        assert out.dtype == dtype and torch.equal(out, plain), rule
        assert close(out, ref.arc_coord(X, f, rule), dtype), rule
        assert torch.equal(gar.arc_coord(rows, f, rule), out)
        mixed = gar.arc_coord(G, f, rule, nnm=True)
        masks = torch.zeros((n, 2), dtype=torch.int64, device=cuda)
        native.gpu_nnm_sets(G2, n, f, masks)
        want = torch.empty(d, dtype=dtype, device=cuda)
        native.gpu_nnm_coord(gar.prepare(Y).obj, masks, n, f, rule, want)
        assert torch.equal(mixed, want), rule
        assert close(mixed, ref.arc_coord(X, f, rule, True), dtype), rule
        assert out.data_ptr() != G.data_ptr() and mixed.data_ptr() != G.data_ptr()
    assert torch.equal(G, before) and all(torch.equal(r, before[i]) for i, r in enumerate(rows))
    assert np_ >= n


@pytest.mark.parametrize("rule", ["krum", "geomed"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_non_finite_rows(cuda, native, dtype, rule):
    """A NaN row and an inf row take two of the k = 3 top slots, stay unclipped and get weight 0."""
    X = latent(9, 500, dtype, 5).clone()
    X[4, 17] = math.nan
    X[6, 3] = math.inf
    keep = [0, 1, 2, 3, 5, 7, 8]
    w_ref = ref.arc_weights(X, 2, rule)
    assert float(w_ref[4]) == 0.0 and float(w_ref[6]) == 0.0
    G = X.to(cuda)
    c = gar.arc_scales(G, 2)
    assert float(c[4]) == 1.0 and float(c[6]) == 1.0 and int((c != 1).sum()) == 1
    w = gar.arc_weights(G, 2, rule).clone()
    out = gar.arc(G, 2, rule)
    torch.cuda.synchronize()
    assert float(w[4]) == 0.0 and float(w[6]) == 0.0
    err = relerr(w, w_ref)
    print(f"arc-{rule} weights with non-finite rows {dtype}: max relative error {err:.3e}")
    assert err <= SCALE_RTOL + RULE_RTOL[(False, rule)]
    assert torch.isfinite(out).all()
    assert close(out, ref.combine(X[keep], w_ref[keep].double()), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_large_norms(cuda, native, dtype):
    """Two rows scaled by 1e3: arc-average matches the oracle, the plain average is nowhere near it."""
    X = latent(8, 1000, torch.float32, 3)
    X[6:] *= 1e3
    X = X.to(dtype)
    G = X.to(cuda)
    out_ref = ref.arc(X, 2, "average")
    out = gar.arc(G, 2, "average")
    assert close(out, out_ref, dtype)
    assert not close(gar.average(G), out_ref, dtype)
    assert float((gar.average(G).double().cpu() - out_ref).abs().max()) > 100 * float(out_ref.abs().max())
    assert torch.equal(out, gar.aggregate("arc-average", G, f=2))


def test_capture(cuda, native):
    """Gram -> k_arc_scale -> k_arc_apply captured once, replayed on two inputs that clip different rows: the
    scales and the list stay on the device, the grid is sized by the host's bound."""
    n, d, f = 8, 5003, 2
    rows = gar.prepare(torch.zeros((n, d), dtype=torch.bfloat16, device=cuda))
    X = rows.obj
    np_ = native.gram_padded(n)
    grid = native.gram_grid(d, torch.empty(0, dtype=torch.bfloat16), n)
    slabs = torch.empty((grid + native.GRAM_REDUCE_GROUPS) * native.gram_slab_floats(n), device=cuda)
    g = torch.empty(np_ * np_, device=cuda)
    scales = torch.empty(n, device=cuda)
    clip_rows = torch.empty(n + 1, dtype=torch.int32, device=cuda)

    def run():
        native.gpu_gram(X, slabs, g)
        native.gpu_arc_scale(g, n, f, scales, clip_rows, None)
        native.gpu_arc_apply(X, scales, clip_rows, f, 0, d)

    inputs = []
    for seed, big in ((0, (1, 4, 6)), (1, (0, 2, 7))):
        A = latent(n, d, torch.float32, seed)
        A = A / A.norm(dim=1, keepdim=True)
        A[list(big)] *= torch.tensor([2.0, 3.0, 4.0])[:, None]
        inputs.append(A.to(torch.bfloat16).to(cuda))
    eager = []
    for A in inputs:
        X.copy_(A)
        run()
        eager.append((X.clone(), scales.clone(), clip_rows.clone()))
    assert eager[0][2][:4].tolist() == [3, 1, 4, 6] and eager[1][2][:4].tolist() == [3, 0, 2, 7]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        X.copy_(inputs[0])
        run()
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    for A, (want, s_want, c_want) in zip(inputs, eager):
        X.copy_(A)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(X, want) and torch.equal(scales, s_want) and torch.equal(clip_rows, c_want)


# --------------------------------------------------------------------------- #
# The engine


def _run(cuda, rule, pre, steps=3, byzantine="reverse", **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(gar=rule, f=1, workers_per_rank=5, byzantine={4: byzantine}, lr=0.05, pre_aggregation=pre, **kw)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), cfg)
    for it in range(steps):
        eng.step(synthetic_batches(5, 8, (1, 28, 28), 10, cuda, seed=11 + it))
    eng.synchronize()
    torch.cuda.synchronize()
    return eng


ENGINE = [("arc", "krum"), ("arc", "geomed"), ("arc", "cclip"), ("arc", "dnc"), ("arc", "average"),
          ("arc+nnm", "krum"), ("arc+nnm", "average"), ("arc", "trimmed-mean"), ("arc", "median"),
          ("arc+nnm", "trimmed-mean")]


@pytest.mark.parametrize("pre,rule", ENGINE)
def test_engine_graph_equals_eager(cuda, pre, rule):
    eager = _run(cuda, rule, pre, cuda_graph=False)
    graph = _run(cuda, rule, pre, cuda_graph=True)
    assert torch.equal(eager.flat_model(), graph.flat_model())
    assert torch.isfinite(eager.flat_model()).all()
    if rule in COORD:
        assert eager.last_weights is None and graph.last_weights is None
        plain = _run(cuda, rule, "nnm" if pre == "arc+nnm" else None, cuda_graph=False)
        assert not torch.equal(plain.flat_model(), eager.flat_model())
        return
    assert torch.equal(eager.last_weights, graph.last_weights)
    assert torch.equal(eager.last_weights, gar.arc_weights(eager.G, 1, rule, nnm=pre == "arc+nnm"))


@pytest.mark.parametrize("rule", ["geomed", "average"])
def test_engine_reversed_loud_worker(cuda, rule):
    """One worker sends -100 x its gradient, f = 1: it is the row ARC clips, and it weighs less than without.
    (Krum gives it weight 0 with and without ARC: nothing to compare.)"""
    torch.manual_seed(0)
    outs = {}
    for pre in (None, "arc"):
        eng = _run(cuda, rule, pre, steps=1, byzantine="reverse", cuda_graph=False)
        outs[pre] = eng.last_weights.cpu().double()
        G = eng.G.float()
    print(f"arc-{rule} engine weights", outs["arc"].tolist(), "plain", outs[None].tolist())
    # the engine's reverse attack multiplies by -100 (runtime/attacks.py): the loudest row by far
    s = (G.double() ** 2).sum(1)
    assert int(s.argmax()) == 4 and float(s[4]) > 100 * float(s[:4].max())
    assert 0.0 < float(outs["arc"][4]) < float(outs[None][4])
    assert float(outs["arc"].sum()) <= 1.0 + 5 * 2.0 ** -24
    if rule == "average":
        assert float(outs["arc"][4]) < 0.2 / 10


@pytest.mark.parametrize("pre,rule", [("arc", "krum"), ("arc", "geomed"), ("arc", "average"), ("arc+nnm", "krum"),
                                      ("arc", "trimmed-mean"), ("arc+nnm", "trimmed-mean")])
def test_engine_sharded_one_rank_vs_unsharded(cuda, pre, rule):
    """The per-bucket partial Grams sum in another order than the whole-row Gram: not bitwise."""
    outs = []
    for shard in (False, True):
        eng = _run(cuda, rule, pre, shard_gar=shard, cuda_graph=False)
        assert (eng._shard is not None) == shard
        w = eng.last_weights
        outs.append((eng.flat_model().clone(), None if w is None else w.clone().float()))
    (p0, w0), (p1, w1) = outs
    if rule in COORD:
        assert w0 is None and w1 is None
    else:
        assert w0.shape == w1.shape == (5,)
        print(f"{pre} {rule} sharded vs unsharded: weights", relerr(w1, w0), "models", float((p1 - p0).abs().max()))
        assert relerr(w1, w0) <= SCALE_RTOL + (test_nnm_gpu.GEOMED_RTOL if rule == "geomed" else test_nnm_gpu.KRUM_RTOL)
    torch.testing.assert_close(p1, p0, rtol=1e-5, atol=1e-7)


def test_engine_refusals(cuda):
    def make(**kw):
        return RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda), EngineConfig(**kw))

    for pre in ("arc", "arc+nnm"):
        with pytest.raises(ValueError, match="not yet supported"):
            make(gar="krum", f=2, workers_per_rank=130, shard_gar=True, pre_aggregation=pre)
        with pytest.raises(ValueError, match="not yet supported with layerwise"):
            make(gar="krum", f=2, workers_per_rank=9, layerwise=True, pre_aggregation=pre)
        for rule in ("bulyan", "brute", "aksel"):
            with pytest.raises(ValueError, match="not yet supported"):
                make(gar=rule, f=2, workers_per_rank=11, pre_aggregation=pre)
    with pytest.raises(ValueError, match="unknown pre_aggregation"):
        make(gar="krum", f=2, workers_per_rank=9, pre_aggregation="bucketing")
    with pytest.raises(ValueError, match="not yet supported"):
        make(gar="median", f=2, workers_per_rank=9, pre_aggregation="nnm")
