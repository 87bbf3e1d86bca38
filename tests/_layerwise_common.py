"""Shared by test_layerwise_cpu.py and test_layerwise_gpu.py: an adversarial segment table for the
layer-wise GAR kernels (gar_layerwise.hip), the job tables of three kinds of cut, inputs on which
every fp32 operation of the kernels is exact, and the fp64 oracles. Pure torch: no GPU code is
imported here."""
import functools
import random

import torch

from garfield_amd.ops import reference as ref
from garfield_amd.parallel.engine import LW_JOB, lw_job_ranges

DTYPES = (torch.float32, torch.bfloat16, torch.float16)

# lengths 1, < 8, 8, 8k +- 1, 63 / 64 / 65; starts 0, 1, 4, 12, 19, 83, 92, 155, 220, 230, 360, 4457:
# odd ones, 4-byte but not 16-byte aligned ones (1, 19, 83, 155 in fp32; 230 in 16 bits), 16-byte
# aligned for both element sizes (0, 360); the last segment has an odd start and is longer than
# 2 LW_JOB, so it has three jobs whose inner edges are global multiples of LW_JOB.
LENS = (1, 3, 8, 7, 64, 9, 63, 65, 10, 130, 4097, 70001)
OFFS = tuple(sum(LENS[:i]) for i in range(len(LENS) + 1))
L = len(LENS)
D = OFFS[-1]                       # 74458
LD = (D + 7) // 8 * 8              # row stride: every row 16-byte aligned for both element sizes
LONG = L - 1                       # the segment with three jobs
SHARD_EDGES = (0, 64, 128, 4480, 32768, 65536, D)   # owned ranges of the shard cuts (multiples of 64)
NS = (7, 17, 40, 128)              # gram_nb 1, 2, 4, 8

EXACT_HP = dict(lr=0.5, momentum=0.5, dampening=0.25, weight_decay=0.25)
RANDN_HP = dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=5e-4)
ZERO_SEG, ONE_SEG = 6, 9           # combine: the segment with all-zero weights / with one row of weight 1

# (n, t, beta) of the tail: the MFMA form (KS 1..4, NP 8..64) and the shapes only the scalar form takes
TAIL_MFMA = ((7, 6, 4), (17, 10, 8), (40, 20, 16), (64, 40, 32))
TAIL_SCALAR_BF16 = ((100, 40, 32), (40, 36, 16))     # n > 64; t - beta > 16
TAIL_RANDN = (17, 2)               # n, f of the randn case: t = 11, beta = 7, |S_k| = 13, 12, ...
TAIL_LONG_JOB = 163840             # one job of 2560 groups: 40 per wave, more than the 32 list slots
SENTINEL = -777.25


def seg_of(x: int) -> int:
    return max(s for s in range(L) if OFFS[s] <= x)


# ---------------------------------------------------------------------------------------------
# job tables

def range_jobs(o0: int, o1: int, split=None):
    """(jobs, seg_lo) of the owned range [o0, o1) in local coordinates, by the rule of
    ShardedAggregator._lw_plan (o0 = 0, o1 = D: that of _layerwise_device). ``split(a, e, s)`` may cut
    a job further (global coordinates)."""
    jobs, seg_lo = [], [0]
    for s in range(L):
        x0, x1 = max(OFFS[s], o0), min(OFFS[s + 1], o1)
        for a, e in lw_job_ranges(x0, x1):
            pieces = split(a, e, s) if split else [(a, e)]
            jobs.extend((pa - o0, pe - o0, s) for pa, pe in pieces)
        seg_lo.append(len(jobs))
    return jobs, seg_lo


def whole_cut():
    return [(0, D) + range_jobs(0, D)]


def shard_cuts():
    return [(o0, o1) + range_jobs(o0, o1) for o0, o1 in zip(SHARD_EDGES, SHARD_EDGES[1:])]


def arbitrary_cut(seed: int = 1234):
    """base = 0; every job cut again 1, 5 and 7 elements past its segment's start and at seeded
    pseudo-random interior points (more of them in the long segment)."""
    rng = random.Random(seed)

    def split(a, e, s):
        pts = {OFFS[s] + k for k in (1, 5, 7)}
        if e - a > 1:
            pts |= {rng.randrange(a + 1, e) for _ in range(8 if s == LONG else 3)}
        cuts = [a] + sorted(p for p in pts if a < p < e) + [e]
        return list(zip(cuts, cuts[1:]))

    return [(0, D) + range_jobs(0, D, split)]


CUTS = {"whole": whole_cut, "shards": shard_cuts, "arbitrary": arbitrary_cut}


def job_tensors(jobs, seg_lo, device):
    return (torch.tensor(jobs, dtype=torch.int64, device=device).reshape(-1, 3),
            torch.tensor(seg_lo, dtype=torch.int32, device=device))


def seg_off_tensor(device):
    return torch.tensor(OFFS, dtype=torch.int64, device=device)


def describe(x: int, cut=None) -> str:
    """Where global coordinate x lies: its segment, its offset there modulo 8 and 64, its job."""
    s = seg_of(x)
    o = x - OFFS[s]
    txt = f"x={x} segment {s} (start {OFFS[s]}, length {LENS[s]}) offset {o} (mod 8: {o % 8}, mod 64: {o % 64}), x mod 64: {x % 64}"
    for o0, o1, jobs, _ in cut or ():
        for a, e, js in jobs:
            if o0 + a <= x < o0 + e:
                txt += f"; range [{o0}, {o1}) job [{o0 + a}, {o0 + e}) of segment {js}: {x - o0 - a} past its start, {o0 + e - x} before its end"
    return txt


_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float64: torch.int64}


def assert_same(got: torch.Tensor, want: torch.Tensor, what: str, cut=None, base: int = 0, bitwise: bool = False) -> None:
    """got == want element for element (1-D, on the CPU, same dtype and shape; ``bitwise``: the same
    bits, for two results of kernels); a failure names the first mismatching coordinates."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if bitwise:
        diff = got.contiguous().view(_BITS[got.dtype]) != want.contiguous().view(_BITS[want.dtype])
    else:
        diff = ~(got == want)
    if not bool(diff.any()):
        return
    bad = diff.nonzero().flatten().tolist()
    lines = [f"{describe(base + x, cut)}: got {got[x].item()!r}, want {want[x].item()!r}" for x in bad[:6]]
    raise AssertionError(f"{what}: {len(bad)} of {got.numel()} coordinates differ\n  " + "\n  ".join(lines))


# ---------------------------------------------------------------------------------------------
# A. Gram

@functools.lru_cache(maxsize=2)
def gram_exact_rows(n: int) -> torch.Tensor:
    """[n, LD] integers of {-3 .. 3} (exact in every dtype): every partial sum of a Gram entry is an
    integer below 2^24."""
    g = torch.Generator().manual_seed(100 + n)
    return torch.randint(-3, 4, (n, LD), generator=g).float()


@functools.lru_cache(maxsize=4)
def gram_randn_rows(n: int, dtype) -> torch.Tensor:
    g = torch.Generator().manual_seed(200 + n)
    return torch.randn((n, LD), generator=g).to(dtype)


def gram_fp64(X: torch.Tensor, x0: int = 0, x1: int = D) -> torch.Tensor:
    """[L, n, n]: per segment, the fp64 Gram of the segment's columns inside [x0, x1)."""
    out = torch.zeros((L, X.shape[0], X.shape[0]), dtype=torch.float64)
    for s in range(L):
        a, e = max(OFFS[s], x0), min(OFFS[s + 1], x1)
        if e > a:
            Y = X[:, a:e].double()
            out[s] = Y @ Y.t()
    return out


def gram_bound(X: torch.Tensor) -> torch.Tensor:
    """[L, n, n]: (K_s + 2) 2^-24 sum_k |x_ik x_jk|, the a-priori bound of an fp32 sum of K_s products."""
    out = torch.zeros((L, X.shape[0], X.shape[0]), dtype=torch.float64)
    for s in range(L):
        Y = X[:, OFFS[s]:OFFS[s + 1]].double().abs()
        out[s] = (LENS[s] + 2) * 2.0 ** -24 * (Y @ Y.t())
    return out


# ---------------------------------------------------------------------------------------------
# B. combine + SGD

@functools.lru_cache(maxsize=4)
def combine_exact_rows(n: int, step: int) -> torch.Tensor:
    """[n, LD] multiples of 1/8 in [-3, 3] (exact in every dtype), fresh for every step."""
    g = torch.Generator().manual_seed(300 + 10 * n + step)
    return torch.randint(-24, 25, (n, LD), generator=g).float() / 8


def exact_param() -> torch.Tensor:
    g = torch.Generator().manual_seed(301)
    return torch.randint(-16, 17, (D,), generator=g).float() / 8


def exact_weights(n: int) -> torch.Tensor:
    """[L, n]: dyadic weights on 8 of the n rows (6 of them at n = 7), another subset for every segment;
    ZERO_SEG has no row, ONE_SEG one row of weight 1."""
    g = torch.Generator().manual_seed(302 + n)
    vals = torch.tensor([.25, .25, .125, .125, .0625, .0625, .0625, .0625])[:min(n - 1, 8)]
    w = torch.zeros((L, n))
    for s in range(L):
        rows = torch.randperm(n, generator=g)[:vals.numel()]
        if s == ONE_SEG:
            w[s, rows[0]] = 1.0
        elif s != ZERO_SEG:
            w[s, rows] = vals[torch.randperm(vals.numel(), generator=g)]
    return w


@functools.lru_cache(maxsize=4)
def combine_randn_rows(n: int, step: int, dtype) -> torch.Tensor:
    g = torch.Generator().manual_seed(400 + 10 * n + step)
    return torch.randn((n, LD), generator=g).to(dtype)


def randn_param() -> torch.Tensor:
    return torch.randn((D,), generator=torch.Generator().manual_seed(401))


def randn_weights(n: int) -> torch.Tensor:
    """[L, n]: 1 + (5 s) % min(n, 11) non-dyadic weights per segment (counts 4k + r for every r, so
    the 4-row steps and the single-row steps of the gather both run)."""
    g = torch.Generator().manual_seed(402 + n)
    w = torch.zeros((L, n))
    for s in range(L):
        c = 1 + (5 * s) % min(n, 11)
        rows = torch.randperm(n, generator=g)[:c]
        v = torch.rand(c, generator=g) + 0.1
        w[s, rows] = v / v.sum()
    return w


def combined_grad(X: torch.Tensor, w: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """[D]: every coordinate's rows combined with its segment's weights, in ``dtype``."""
    g = torch.zeros(D, dtype=dtype)
    for s in range(L):
        g[OFFS[s]:OFFS[s + 1]] = w[s].to(dtype) @ X[:, OFFS[s]:OFFS[s + 1]].to(dtype)
    return g


def sgd_formula(p, buf, g, hp, nesterov: bool, first: bool):
    """One update in the dtype of its arguments, one rounded operation at a time: the arithmetic of
    sgd_one / sgd_apply. Returns (param, momentum buffer)."""
    if hp["weight_decay"] != 0:
        g = g + hp["weight_decay"] * p
    if hp["momentum"] != 0:
        buf = g.clone() if first else hp["momentum"] * buf + (1 - hp["dampening"]) * g
        g = g + hp["momentum"] * buf if nesterov else buf
    return p - hp["lr"] * g, buf


def sgd_fp64(p0: torch.Tensor, grads, hp, nesterov: bool):
    """torch.optim.SGD in fp64 on the per-coordinate gradients ``grads`` (one per step): the
    (param, momentum buffer or None) after every step."""
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.SGD([p], lr=hp["lr"], momentum=hp["momentum"], dampening=hp["dampening"],
                          weight_decay=hp["weight_decay"])
    # the constructor refuses Nesterov momentum with dampening; its step's arithmetic takes both
    opt.param_groups[0]["nesterov"] = nesterov
    out = []
    for g in grads:
        p.grad = g.double().clone()
        opt.step()
        buf = opt.state[p].get("momentum_buffer")
        out.append((p.detach().clone(), None if buf is None else buf.clone()))
    return out


@functools.lru_cache(maxsize=8)
def combine_exact_oracle(n: int, nesterov: bool, momentum: float = EXACT_HP["momentum"]):
    """Two steps of the exact inputs in fp64: [(param, mom)] per step and the two combined gradients."""
    hp = dict(EXACT_HP, momentum=momentum)
    w = exact_weights(n)
    grads = [combined_grad(combine_exact_rows(n, k), w) for k in range(2)]
    return sgd_fp64(exact_param(), grads, hp, nesterov), grads


# ---------------------------------------------------------------------------------------------
# C. Bulyan's tail

def np_for(k: int) -> int:
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128


def tail_mfma_ok(n: int, t: int, beta: int, dtype) -> bool:
    """The host rule that sends a tail launch to the MFMA form (lw_tail_mfma_ok)."""
    if dtype == torch.float32 or n > 64 or t > 64 or t < 1 or beta < 1 or t - beta > 16:
        return False
    p0 = (np_for(t) // 4) & ~3
    return t // 2 >= p0 and beta >= p0


def bad_row(n: int) -> int:
    """The row no set of the tail's exact inputs contains: it carries the non-finite values."""
    return n // 2


@functools.lru_cache(maxsize=2)
def tail_exact_rows(n: int, d: int = LD) -> torch.Tensor:
    g = torch.Generator().manual_seed(500 + n)
    return torch.randint(-24, 25, (n, d), generator=g).float() / 8


def tail_exact_W(n: int, t: int, nseg: int = L) -> torch.Tensor:
    """[nseg, t, n]: row k of segment s is 1 / |S| on a set S of 1, 2, 4 or 8 rows (at most n - 1, never
    bad_row(n)), 0 elsewhere: one common value per row, other sets for every segment."""
    g = torch.Generator().manual_seed(501 + 7 * n + t)
    ok = torch.tensor([j for j in range(n) if j != bad_row(n)])
    sizes = [c for c in (1, 2, 4, 8) if c <= ok.numel()]
    W = torch.zeros((nseg, t, n))
    for s in range(nseg):
        for k in range(t):
            c = sizes[(s + k) % len(sizes)]
            W[s, k, ok[torch.randperm(ok.numel(), generator=g)[:c]]] = 1.0 / c
    return W


def closest_mean(V: torch.Tensor, beta: int):
    """reference._closest_mean of every column of the finite [t, K] fp64 V at once: the mean of the
    beta values closest to the median s[t // 2], ties by the smaller value. Also returns the gap
    between the beta-th and the (beta + 1)-th distance to the median (inf at beta = t)."""
    t = V.shape[0]
    s = V.sort(dim=0).values
    key = (s - s[t // 2]).abs()
    order = key.argsort(dim=0, stable=True)          # s ascending: equal distances keep the smaller value first
    out = s.gather(0, order[:beta]).sum(0) / beta
    ks = key.gather(0, order)
    gap = ks[beta] - ks[beta - 1] if beta < t else torch.full_like(out, float("inf"))
    return out, gap


def closest_mean_ref(V: torch.Tensor, beta: int) -> torch.Tensor:
    return torch.tensor([ref._closest_mean(V[:, x].tolist(), beta) for x in range(V.shape[1])], dtype=torch.float64)


def tail_means(X: torch.Tensor, W: torch.Tensor, s: int, a: int, e: int) -> torch.Tensor:
    return W[s].double() @ X[:, a:e].double()


def tail_fp64(X: torch.Tensor, W: torch.Tensor, beta: int):
    """[D] oracle of the whole table (every coordinate with its segment's W), the distance gaps and
    max_k |V_k(x)|."""
    out, gap, vmax = (torch.zeros(D, dtype=torch.float64) for _ in range(3))
    for s in range(L):
        V = tail_means(X, W, s, OFFS[s], OFFS[s + 1])
        out[OFFS[s]:OFFS[s + 1]], gap[OFFS[s]:OFFS[s + 1]] = closest_mean(V, beta)
        vmax[OFFS[s]:OFFS[s + 1]] = V.abs().amax(0)
    return out, gap, vmax


@functools.lru_cache(maxsize=8)
def tail_exact_oracle(n: int, t: int, beta: int) -> torch.Tensor:
    return tail_fp64(tail_exact_rows(n), tail_exact_W(n, t), beta)[0]


def _nonfinite(i: int) -> float:
    return (float("inf"), float("-inf"), float("nan"))[i % 3]


def poison(X: torch.Tensor) -> torch.Tensor:
    """A copy of the [n, LD] rows with inf, -inf and NaN in bad_row(n): in every third 64-group of the
    long segment (at a varying column) and at the first and last element of every segment, which lie
    in the partial head and tail groups of the short ones."""
    X = X.clone()
    r, i = bad_row(X.shape[0]), 0
    for g in range((OFFS[LONG] + 63) // 64, D // 64):
        if g % 3 == 0:
            X[r, 64 * g + (7 * g) % 64] = _nonfinite(i)
            i += 1
    for s in range(L):
        for x in (OFFS[s], OFFS[s + 1] - 1):
            X[r, x] = _nonfinite(i)
            i += 1
    return X


def poison_every_group(X: torch.Tensor) -> torch.Tensor:
    """A copy with one non-finite value of bad_row(n) in every 64-group."""
    X = X.clone()
    r = bad_row(X.shape[0])
    for g in range(X.shape[1] // 64):
        X[r, 64 * g + (11 * g) % 64] = _nonfinite(g)
    return X


def bulyan_sized_W(n: int, f: int, seed: int = 600) -> torch.Tensor:
    """[L, t, n] with Bulyan's set sizes: row k is fp32(1 / (m - k)) on m - k rows, m = n - f - 2."""
    g = torch.Generator().manual_seed(seed)
    t, m = n - 2 * f - 2, n - f - 2
    W = torch.zeros((L, t, n))
    for s in range(L):
        for k in range(t):
            W[s, k, torch.randperm(n, generator=g)[:m - k]] = 1.0 / (m - k)
    return W


@functools.lru_cache(maxsize=1)
def tail_randn_case():
    """The randn case of the tail: bf16 rows, W, beta, the fp64 oracle, the per-coordinate bound
    (n + beta + 4) 2^-24 max_k |V_k(x)| and the mask of the coordinates kept (those whose beta-th and
    (beta + 1)-th distances to the median differ by more than twice the bound)."""
    n, f = TAIL_RANDN
    t, beta = n - 2 * f - 2, n - 4 * f - 2
    X = torch.randn((n, LD), generator=torch.Generator().manual_seed(601)).to(torch.bfloat16)
    W = bulyan_sized_W(n, f)
    out, gap, vmax = tail_fp64(X, W, beta)
    bound = (n + beta + 4) * 2.0 ** -24 * vmax
    return X, W, t, beta, out, bound, gap > 2 * bound


assert LW_JOB == 32768 and LENS[LONG] > 2 * LW_JOB and OFFS[LONG] % 2 == 1
