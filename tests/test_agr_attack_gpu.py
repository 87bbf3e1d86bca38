"""The adaptive colluding attacks Min-Max / Min-Sum on the GPU (csrc/gar_agr_attack.hip: k_agr_stats, the
Gram, k_agr_solve, k_agr_write) against the fp64 oracle on the same stored rows.

Inputs: a +-1 offset per coordinate shared by the rows plus 0.1 N(0, 1) per element, cast to the dtype; the
oracle sees the rows after the cast. One coordinate is zero in every row (d >= 7). The `sgn` cases first
assert on the oracle that no other coordinate's mean is within 1e-3 of the largest input of a sign flip.

gamma: relative error against the oracle, bound = 20 x the maximum measured on an MI355X over every case of
this file (profiles/r17/agr_attack/test_agr_attack_gpu.log), never above 1e-4. The measured maximum is
2.496e-5 (minmax-sgn, fp32, k = 5, d = 2000), so the cap holds: GAMMA_RTOL = 1e-4. That maximum is above
1e-4 / 20, the project's mark of a defect. It is not in this feature's sums (b_i and c are fp64 sums of fp32
lane partials and agree with the oracle to 1e-6 of sqrt(c max a), see the log); it is the fp32 Gram: these
inputs share the +-1 offset, so the squared norms are 50 to 160 times the squared distances, and a distance
taken as G_ii + G_jj - 2 G_ij loses that factor against the Gram kernel's fp32 accumulation (one rounding of an
exact Gram to fp32 already gives 2.3e-5 at k = 2, d = 7, fp16; docs/GAR_SEMANTICS.md has the figures). Every
selection on the Gram shares it; on rows without a common offset the measured maximum is 1.9e-7
(test_gamma_error_without_a_common_offset).

Output: per element, twice the bound derived in docs/GAR_SEMANTICS.md "Adaptive colluding attacks", with
u = 2^-24, A = the coordinate's largest |input|, h = the half-ulp of the cast (0 for fp32, whose rounding is
the fused multiply-add's):
    gamma (GAMMA_RTOL + u) |p| + gamma (2k + 12) u A + k u A + (u + h) |m|   (+ 2^-25 for fp16 subnormals)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from garfield_amd.models import build_model
from garfield_amd.ops import agr_attack
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

pytestmark = pytest.mark.gpu

KINDS = ("minmax", "minmax-uv", "minmax-sgn", "minsum", "minsum-uv", "minsum-sgn")
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
KS = (2, 3, 5, 8, 17, 64, 128)
DS = (1, 7, 8, 9, 64, 2000)
GAMMA_ERR_MEASURED = 2.496e-5
GAMMA_RTOL = min(20 * GAMMA_ERR_MEASURED, 1e-4)
U = 2.0 ** -24
# half an ulp relative to the value is largest at the bottom of a binade: 2^-p for p significand bits
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def make_rows(k, d, dtype, seed=0):
    g = torch.Generator().manual_seed(100003 * k + 17 * d + seed)
    off = torch.randint(0, 2, (d,), generator=g).double() * 2 - 1
    X = off + 0.1 * torch.randn(k, d, generator=g, dtype=torch.float64)
    if d >= 7:
        X[:, 3] = 0.0
    return X.to(dtype)


@functools.lru_cache(maxsize=None)
def case(k, d, dtype, kind, seed=0):
    """(rows on the CPU, oracle m, oracle gamma, p, A): computed once, shared, never modified."""
    objective, pert = agr_attack.parse(kind)
    X = make_rows(k, d, dtype, seed)
    E = X.double()
    m, gamma = ref.agr_attack(E, objective, pert)
    mu, p = ref.agr_perturbation(E, pert)
    A = E.abs().max(0).values
    if pert == "sgn":
        live = A > 0
        assert float(mu[live].abs().min()) >= 1e-3 * float(A.max())
    return X, m, gamma, p, A


def device_rows(X, cuda, misalign=None):
    """The rows as separate device tensors (one upload, one device copy each); row `misalign` starts one
    element past a 16-byte boundary."""
    Xd = X.to(cuda)
    rows = []
    for i in range(X.shape[0]):
        if i == misalign:
            buf = torch.empty(X.shape[1] + 16, dtype=X.dtype, device=cuda)
            assert buf.data_ptr() % 16 == 0
            r = buf[1:1 + X.shape[1]]
            r.copy_(Xd[i])
        else:
            r = Xd[i].clone()
        rows.append(r)
    return rows


def out_bound(k, dtype, gamma, m, p, A):
    b = gamma * (GAMMA_RTOL + U) * p.abs() + gamma * (2 * k + 12) * U * A + k * U * A + (U + HALF_ULP[dtype]) * m.abs()
    return b + (2.0 ** -25 if dtype == torch.float16 else 0.0)


def check(rows, X, T, kind, dtype, gamma_dev, info, m, gamma, p, A, lo=0, hi=None):
    """gamma and the rows after the attack against the oracle; returns (gamma error, largest error / bound)."""
    k = X.shape[0]
    hi = X.shape[1] if hi is None else hi
    g64 = float(info[0])
    assert float(gamma_dev) == float(torch.tensor(g64).float())          # gamma rounded once to fp32
    gerr = abs(g64 - gamma) / gamma if gamma > 0 else abs(g64)
    after = torch.stack(list(rows)).cpu()
    assert torch.equal(after[:k - T], X[:k - T]), "an honest row was written"
    out = after[k - T]
    for t in range(1, T):
        assert torch.equal(after[k - T + t], out), "the target rows differ"
    err = (out[lo:hi].double() - m).abs()
    bound = out_bound(k, dtype, gamma, m, p, A)
    ratio = float(torch.where(err > 0, err / bound, torch.zeros_like(err)).max())   # 0 / 0: an all-zero coordinate
    return gerr, ratio


def stat_errors(info, X, kind):
    """Where the gamma error sits: (largest |a_i error| / R-or-S scale, largest |b_i error| / sqrt(c max a)):
    a comes from the fp32 Gram's distances, b from the statistics pass's own fp64 sums."""
    pert = agr_attack.parse(kind)[1]
    E, k = X.double(), X.shape[0]
    mu, p = ref.agr_perturbation(E, pert)
    a, b, c = ((mu - E) ** 2).sum(1), (p * (mu - E)).sum(1), float((p * p).sum())
    info = info.cpu()
    scale = max(float(a.max()), 1e-300)
    return (float((info[2:2 + k] - a).abs().max()) / scale,
            float((info[2 + k:2 + 2 * k] - b).abs().max()) / max((c * scale) ** 0.5, 1e-300))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_match_oracle(cuda, native, kind, dtype):
    worst_g, worst_r, where, worst_a, worst_b = 0.0, 0.0, None, 0.0, 0.0
    for k in KS:
        for d in DS:
            X, m, gamma, p, A = case(k, d, dtype, kind)
            for T, misalign in ((1, None), (3, 1), (3, None)):
                T = min(T, k)
                rows = device_rows(X, cuda, misalign)
                g, info = agr_attack.attack_rows(rows, k - T, kind, info=True)
                gerr, ratio = check(rows, X, T, kind, dtype, g, info, m, gamma, p, A)
                if gerr > worst_g:
                    worst_g, where = gerr, (k, d, T, misalign)
                worst_r = max(worst_r, ratio)
            ea, eb = stat_errors(info, X, kind)
            worst_a, worst_b = max(worst_a, ea), max(worst_b, eb)
    print(f"agr {kind} {dtype}: max gamma relative error {worst_g:.3e} at (k, d, T, misaligned row) = {where}; "
          f"max output error / derived bound {worst_r:.3f}; max a_i error / max a {worst_a:.3e} (Gram), "
          f"max b_i error / sqrt(c max a) {worst_b:.3e} (statistics pass)")
    assert worst_g <= GAMMA_RTOL, (worst_g, where)
    assert worst_r <= 2.0, worst_r


@pytest.mark.parametrize("dtype", DTYPES)
def test_gamma_error_without_a_common_offset(cuda, native, dtype):
    """Rows N(0, I) with no shared offset: squared norms and squared distances are of one size, the Gram's
    distances lose nothing, and gamma is inside 1e-4 / 20, the mark the inputs above miss."""
    worst = 0.0
    for kind in ("minmax", "minsum"):
        objective, pert = agr_attack.parse(kind)
        for k in (2, 5, 17, 128):
            for d in (7, 64, 2000):
                g = torch.Generator().manual_seed(k * 1000 + d)
                X = torch.randn(k, d, generator=g, dtype=torch.float64).to(dtype)
                gamma = ref.agr_attack(X.double(), objective, pert)[1]
                _, info = agr_attack.attack_rows(device_rows(X, cuda), k - 1, kind, info=True)
                worst = max(worst, abs(float(info[0]) - gamma) / gamma)
    print(f"agr N(0, I) rows {dtype}: max gamma relative error {worst:.3e}")
    assert worst <= 1e-4 / 20


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lo,hi", [(40, 1013), (37, 1000)])
def test_range_inside_rows_leaves_the_rest_untouched(cuda, native, dtype, lo, hi):
    """[lo, hi) strictly inside the rows: lo = 40 keeps the 16-byte loads (and a partial last vector), lo = 37
    takes the single-element path; sentinels outside the range stay what they were on every row."""
    k, T, d, kind = 5, 2, 1100, "minmax"
    X, m, gamma, p, A = case(k, hi - lo, dtype, kind, seed=lo)
    full = torch.full((k, d), 777.0, dtype=dtype)
    full[:, lo:hi] = X
    rows = device_rows(full, cuda)
    gram, part = agr_attack.agr_partials(rows, "std", lo, hi)
    g, info = agr_attack.agr_gamma(gram, part, "minmax", info=True)
    agr_attack.agr_write(rows, k - T, g, "std", lo, hi)
    for r in rows:
        assert bool((r[:lo] == 777.0).all()) and bool((r[hi:] == 777.0).all())
    gerr, ratio = check([r[lo:hi] for r in rows], X, T, kind, dtype, g, info, m, gamma, p, A)
    print(f"agr range [{lo}, {hi}) {dtype}: gamma relative error {gerr:.3e}, output error / bound {ratio:.3f}")
    assert gerr <= GAMMA_RTOL and ratio <= 2.0


def test_grid_stride_takes_more_than_one_trip(cuda, native):
    """d past 4096 workgroups x 2048 coordinates: the second trip of the grid-stride loops, partial tile last."""
    k, T, kind, dtype = 2, 1, "minsum", torch.bfloat16
    d = 4096 * 2048 + 3 * 2048 + 5
    assert native.agr_grid(d) == 4096
    X, m, gamma, p, A = case(k, d, dtype, kind)
    rows = device_rows(X, cuda)
    g, info = agr_attack.attack_rows(rows, k - T, kind, info=True)
    gerr, ratio = check(rows, X, T, kind, dtype, g, info, m, gamma, p, A)
    print(f"agr d={d} {dtype}: gamma relative error {gerr:.3e}, output error / bound {ratio:.3f}")
    assert gerr <= GAMMA_RTOL and ratio <= 2.0


@pytest.mark.parametrize("kind", ["minmax", "minsum-sgn"])
def test_deterministic_and_additive(cuda, native, kind):
    """The same inputs give the same bits twice; two half-range partials summed by the solve agree with the
    whole-range run within the gamma bound."""
    k, T, d, dtype = 17, 3, 2000, torch.bfloat16
    objective, pert = agr_attack.parse(kind)
    X = case(k, d, dtype, kind)[0]
    runs = []
    for _ in range(2):
        rows = device_rows(X, cuda)
        g, info = agr_attack.attack_rows(rows, k - T, kind, info=True)
        runs.append((g.clone(), info.clone(), torch.stack(rows).clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    rows = device_rows(X, cuda)
    g1, p1 = agr_attack.agr_partials(rows, pert, 0, 1000)
    g2, p2 = agr_attack.agr_partials(rows, pert, 1000, d)
    gh, infoh = agr_attack.agr_gamma(g1 + g2, torch.stack([p1, p2]), objective, info=True)
    whole = float(runs[0][1][0])
    print(f"agr {kind}: whole-range gamma {whole!r}, two half ranges {float(infoh[0])!r}")
    assert abs(float(infoh[0]) - whole) <= GAMMA_RTOL * whole


def test_capture_equals_eager(cuda, native):
    """stats -> Gram -> solve -> write in one captured graph, replayed on other row contents."""
    k, T, d, dtype, kind = 8, 2, 2000, torch.bfloat16, "minmax"
    objective, pert = agr_attack.parse(kind)
    X0, X1 = case(k, d, dtype, kind)[0], case(k, d, dtype, kind, seed=1)[0]

    def run(rows):
        gram, part = agr_attack.agr_partials(rows, pert, reduce=False)
        g = agr_attack.agr_gamma(gram, part, objective)
        agr_attack.agr_write(rows, k - T, g, pert)
        return g

    eager = device_rows(X1, cuda)
    g_eager = run(eager).clone()
    static = device_rows(X0, cuda)
    s = torch.cuda.Stream(cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        run([r.clone() for r in static])      # warm-up on the capture stream (workspaces)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g_static = run(static)
    torch.cuda.current_stream(cuda).wait_stream(s)
    for r, x in zip(static, X1):
        r.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_static, g_eager) and float(g_eager) > 0
    assert torch.equal(torch.stack(static), torch.stack(eager))
    assert not torch.equal(static[k - 1].cpu(), X1[k - 1])


def test_engine_sharded_one_rank_vs_unsharded(cuda, native):
    """The sharded step's order (per-bucket statistics summed, solve, write per bucket) against whole rows:
    another summation order, gamma within its bound; the attacked rows then differ by gamma's difference
    times |p| and a rounding of the cast."""
    out = []
    for shard in (False, True):
        torch.manual_seed(0)
        eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda),
                                 EngineConfig(gar="krum", f=2, workers_per_rank=8, byzantine={1: "minmax", 6: "minmax"},
                                              collusion="all", cuda_graph=False, shard_gar=shard,
                                              exchange_dtype=torch.float32))
        assert (eng._shard is not None) == shard
        eng.compute_local(synthetic_batches(8, 16, (1, 28, 28), 10, cuda))
        sigma = eng.X[:, 0, :eng.d].double().std(0)      # one rank: row j is slot j; collusion "all": E = every row
        eng.aggregate_and_update()
        torch.cuda.synchronize()
        out.append((float(eng.last_agr_gamma["minmax"]), eng.X[:, 0, :eng.d][[1, 6]].clone(), eng.last_weights.clone()))
    (g0, r0, w0), (g1, r1, w1) = out
    print(f"agr engine: gamma unsharded {g0!r} sharded {g1!r}")
    assert g0 > 0 and abs(g1 - g0) <= GAMMA_RTOL * g0
    assert torch.equal(r1[0], r1[1]) and torch.equal(w0, w1)
    # the two gammas' difference times |p| = sigma, and one fp32 rounding each way
    assert bool(((r1 - r0).abs() <= GAMMA_RTOL * g0 * sigma + 2.0 ** -22 * r0.abs()).all())


@pytest.mark.parametrize("rule,pre", [("krum", None), ("dnc", None), ("trimmed-mean", "nnm")])
def test_engine_step_with_minmax_colluders(cuda, native, rule, pre):
    """World 1, per-worker engine: the step completes with finite parameters and the attacked rows are the
    functional path's, bit for bit."""
    torch.manual_seed(0)
    byz = {1: "minmax", 6: "minmax"}
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(device=cuda),
                             EngineConfig(gar=rule, f=2, workers_per_rank=8, byzantine=byz, collusion="all",
                                          pre_aggregation=pre, cuda_graph=False, shard_gar=False))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, cuda)
    eng.compute_local(b)
    G0 = eng.G.clone()
    eng.aggregate_and_update()
    honest = [s for s in range(8) if s not in byz]
    rows = [G0[i].clone() for i in honest + [1, 6]]
    g = agr_attack.attack_rows(rows, len(honest), "minmax")
    torch.cuda.synchronize()
    assert float(g) > 0 and torch.equal(g, eng.last_agr_gamma["minmax"])
    assert torch.equal(eng.G[1], rows[-1]) and torch.equal(eng.G[6], rows[-1])
    assert torch.equal(eng.G[honest], G0[honest])
    for _ in range(2):
        eng.step(b)
    assert torch.isfinite(eng.flat_model()).all()
