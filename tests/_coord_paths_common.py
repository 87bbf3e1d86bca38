"""Shared material of the coordinate-wise dispatch-path tests (test_coord_paths_cpu.py,
test_coord_paths_gpu.py, _coord_paths_child.py): exact-arithmetic inputs, Bulyan set tables built
by the test, a vectorised float64 oracle (sort / gather only, no project kernel), the tolerances
that follow from the construction, and the case table with the kernel family each case must reach.

Exactness. ``grid_rows`` values are k/4 with integer |k| <= 96: exact in bf16 (8 significant bits:
|k| <= 96 < 2^7 needs 7), fp16 and fp32. A sum of <= 128 of them is j/4 with |j| <= 12288 < 2^24 and a
set mean (a sum of s = 2^a <= 64 of them times 1/s) is j/(4 s) with |j| <= 96 s, so a sum of <= 128 set
means is an integer multiple of 1/(4 s) below 2^24 / (4 s) in magnitude: every set mean, the median,
every distance to it, every comparison and every sum is exact in fp32 (in any order, FMA or not, also
the running add / subtract of the incremental window kernel) and in fp64. What is left is the final
division (S / beta, S * fl(1 / beta), S / (n - 2f), S / cnt: at most 1.5 ulp of fp32 together) and
the round to the output dtype (0.5 ulp of it): a mean-valued result is within 2 ulp of the output
dtype of the float64 oracle; a median or condense result is an input value, bitwise.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch

from garfield_amd.ops import reference as ref

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MODES = {"median": 0, "trimmed-mean": 1, "averaged-median": 2, "average-nan": 3, "condense": 4, "bulyan-tail": 5}
FAMILIES = ("coord16", "coordwise", "coordwise_lds", "tail_window", "tail_window_direct", "tail_mfma", "tail_f32")
KNOBS = ("GARFIELD_COORD16", "GARFIELD_MFMA_TAIL", "GARFIELD_AVGMED_TAIL", "GARFIELD_COORD16_GRID",
         "GARFIELD_TAIL_GRID")
CONDENSE_P, CONDENSE_SEED = 0.6, 12345

# less than one vector, a d % VEC tail, the d % 64 partial MFMA group, the d % 256 last tile, exact multiples
SMALL_D = (1, 63, 64, 65, 255, 256, 257, 1027)
KNOB_D = 5000 + 37


# --------------------------------------------------------------------------- inputs

def poisoned_rows(n: int):
    """The two rows of the non-finite variant: row 1 (a member of some Bulyan sets) and row n - 1 (the row
    that belongs to no set)."""
    assert n >= 3
    return 1, n - 1


def grid_rows(n: int, d: int, dtype, seed: int, nonfinite: bool = False, device="cpu") -> torch.Tensor:
    """[n, d] (on the CPU unless ``device`` says otherwise: drawn where it lives, by that device's seeded
    generator): k/4, integer k in [-96, 96]. nonfinite: NaN / +inf / -inf (cycling, the two rows one step
    apart) at every 97th coordinate of the rows ``poisoned_rows(n)``."""
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 131 * n + d)
    X = torch.randint(-96, 97, (n, d), generator=g, dtype=torch.int32, device=device).to(torch.float32) * 0.25
    if nonfinite:
        cyc = torch.tensor([math.nan, math.inf, -math.inf], device=device)
        at = torch.arange(0, d, 97, device=device)
        for step, r in enumerate(poisoned_rows(n)):
            X[r, at] = cyc[(at // 97 + step) % 3]
    return X.to(dtype)


def bulyan_sets(n: int, t: int, seed: int):
    """(members, s): t sets of the same power-of-two size s over the rows 0 .. n - 2. Row n - 1 is in no
    set; row 1 is in exactly the sets k with k % 4 == 1 (so in some, never in most: the median of the set
    means stays finite when row 1 is poisoned); the other members are drawn per set from a seeded generator."""
    assert n >= 2 and t >= 1
    pool = [0] + list(range(2, n - 1))          # neither row 1 nor row n - 1
    s = 1
    while 2 * s <= min(len(pool), 64):
        s *= 2
    g = torch.Generator().manual_seed(7919 * seed + 31 * n + t)
    members = []
    for k in range(t):
        with_one = n >= 3 and k % 4 == 1
        take = s - 1 if with_one else s
        pick = [pool[i] for i in torch.randperm(len(pool), generator=g)[:take].tolist()]
        members.append(sorted(pick + ([1] if with_one else [])))
    return members, s


def bulyan_W(n: int, t: int, seed: int):
    """(W [t, n] fp32 on the CPU, members, s): weight 1 / s on the members of every set."""
    members, s = bulyan_sets(n, t, seed)
    W = torch.zeros((t, n), dtype=torch.float32)
    for k, m in enumerate(members):
        W[k, m] = 1.0 / s
    return W, members, s


# --------------------------------------------------------------------------- oracle (float64)

def _nan_inf(v: torch.Tensor) -> torch.Tensor:
    return torch.where(torch.isnan(v), torch.full_like(v, math.inf), v)


def _signed(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def _lsr(z: torch.Tensor, k: int) -> torch.Tensor:
    return (z >> k) & ((1 << (64 - k)) - 1)


def mix_hash_vec(seed: int, d: int, device="cpu") -> torch.Tensor:
    """ref.mix_hash(seed, x) for x = 0 .. d - 1 as an int64 tensor (two's-complement wrap = mod 2^64)."""
    x = torch.arange(d, dtype=torch.int64, device=device)
    z = x + _signed(seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019)
    z = (z ^ _lsr(z, 30)) * _signed(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _signed(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return _lsr(z, 32)


def set_means(X64: torch.Tensor, members, s: int) -> torch.Tensor:
    """[t, d] float64: the mean of every set over its members ONLY (a row outside a set never reaches its
    mean, whatever it holds)."""
    return torch.stack([X64[torch.tensor(m, device=X64.device)].sum(0) / s for m in members])


def closest_mean(V: torch.Tensor, beta: int) -> torch.Tensor:
    """Mean of the beta values of every column closest to its median (position len // 2 of the sorted
    column, NaN as +inf), ordered by (distance with NaN as +inf, value)."""
    S = torch.sort(_nan_inf(V), dim=0).values
    med = S[S.shape[0] // 2]
    key = _nan_inf((S - med).abs())
    idx = torch.sort(key, dim=0, stable=True).indices       # S is sorted by value: stable = (key, value)
    return torch.gather(S, 0, idx[:beta]).sum(0) / beta


def oracle(X: torch.Tensor, mode: str, f: int = 0, beta: int = 0, members=None, s: int = 1) -> torch.Tensor:
    """float64 [d] on X's device. Semantics of garfield_amd/ops/reference.py."""
    X64 = X.to(torch.float64)
    n, d = X64.shape
    if mode == "bulyan-tail":
        return closest_mean(set_means(X64, members, s), beta)
    if mode == "averaged-median":
        return closest_mean(X64, beta)
    if mode == "average-nan":
        fin = torch.isfinite(X64)
        cnt = fin.sum(0)
        tot = torch.where(fin, X64, torch.zeros_like(X64)).sum(0)
        return torch.where(cnt > 0, tot / cnt.clamp(min=1), torch.zeros_like(tot))
    if mode == "trimmed-mean":
        S = torch.sort(_nan_inf(X64), dim=0).values
        return S[f:n - f].sum(0) / (n - 2 * f)
    assert mode in ("median", "condense"), mode
    fin = torch.isfinite(X64)
    cnt = fin.sum(0)
    S = torch.sort(torch.where(fin, X64, torch.full_like(X64, math.inf)), dim=0).values
    med = torch.gather(S, 0, (cnt // 2).clamp(max=n - 1)[None]).squeeze(0)
    med = torch.where(cnt > 0, med, torch.zeros_like(med))
    if mode == "condense":
        keep = mix_hash_vec(CONDENSE_SEED, d, X64.device) < ref.bernoulli_threshold(CONDENSE_P)
        med = torch.where(keep, med, X64[0])
    return med


# --------------------------------------------------------------------------- tolerances

_FMT = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}


def ulp_out(want: torch.Tensor, dtype) -> torch.Tensor:
    """The spacing of ``dtype`` at |want| (float64; the subnormal spacing below the smallest normal)."""
    p, emin = _FMT[dtype]
    e = torch.frexp(want.abs())[1].to(torch.float64) - 1          # floor(log2 |want|); 0 -> clamped below
    e = torch.where(want == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.pow(torch.full_like(e, 2.0), e - (p - 1))


def mismatches(got: torch.Tensor, want: torch.Tensor, mode: str, dtype) -> torch.Tensor:
    """Indices of the coordinates where ``got`` (the output dtype) misses ``want`` (float64, same device).
    median / condense: the bits of want rounded to the output dtype (NaN equal to NaN). Mean-valued rules:
    |got - want| <= 2 ulp_out(want); non-finite results equal, NaN to NaN. No coordinate is excused."""
    assert got.dtype == dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    g = got.to(torch.float64)
    if mode in ("median", "condense"):
        w = want.to(dtype).to(torch.float64)
        ok = (g == w) | (torch.isnan(g) & torch.isnan(w))
        ok &= torch.signbit(g) == torch.signbit(w)
    else:
        fin = torch.isfinite(want)
        ok = torch.where(fin, torch.isfinite(g) & ((g - want).abs() <= 2 * ulp_out(want, dtype)),
                         (g == want) | (torch.isnan(g) & torch.isnan(want)))
    return torch.nonzero(~ok).flatten()


# --------------------------------------------------------------------------- cases

# f: trimmed-mean's f; beta: averaged-median / Bulyan; t: Bulyan's set count (0 otherwise)
# ds: the dimensions to run; env: the knob set ({} = default); family / np / bulyan: what coord_plan
# must answer (bulyan: the launch is Bulyan's tail, also for a rerouted averaged median);
# wrap: at every d of the case the grid-stride loop must wrap (grid * coords_per_pass < d)
Case = namedtuple("Case", "id mode dtype n f beta t ds nonfinite env family np bulyan wrap")

CASES: list[Case] = []


def _add(mode, dt, n, family, np_, f=0, beta=0, t=0, ds=SMALL_D, nonfinite=False, env=None, bulyan=None, wrap=False,
         tag=""):
    env = dict(env or {})
    if bulyan is None:
        bulyan = mode == "bulyan-tail"
    arg = {"trimmed-mean": f"-f{f}", "averaged-median": f"-b{beta}", "bulyan-tail": f"-t{t}-b{beta}"}.get(mode, "")
    cid = f"{mode}-{dt}-n{n}{arg}" + ("-nonfinite" if nonfinite else "") + (f"-{tag}" if tag else "")
    assert all(c.id != cid for c in CASES), cid
    CASES.append(Case(cid, mode, dt, n, f, beta, t, tuple(ds), nonfinite, env, family, np_, bulyan, wrap))


# rows n per padded count NP = 8, 16, 32, 64, 128 (odd sizes, one at a power of two)
_N_OF_NP = ((5, 8), (12, 16), (20, 32), (64, 64), (100, 128))

# ---- default knobs, small d ----------------------------------------------------------------------
for _dt in ("bf16", "f16"):
    # packed 16-bit keys: median / trimmed mean / condense at every NP (P = 4, 4, 2, 1, 1)
    for _n, _np in _N_OF_NP:
        _add("median", _dt, _n, "coord16", _np)
        _add("trimmed-mean", _dt, _n, "coord16", _np, f=(_n - 1) // 3)
        _add("condense", _dt, _n, "coord16", _np)
        _add("median", _dt, _n, "coord16", _np, nonfinite=True)
    _add("trimmed-mean", _dt, 20, "coord16", 32, f=4, nonfinite=True)
    _add("condense", _dt, 12, "coord16", 16, nonfinite=True)
    # average-NaN has no packed form: the generic kernels with 16-bit loaders
    _add("average-nan", _dt, 4, "coordwise", 8)
    _add("average-nan", _dt, 9, "coordwise", 16)
    _add("average-nan", _dt, 40, "coordwise_lds", 64)
    _add("average-nan", _dt, 100, "coordwise_lds", 128)
    _add("average-nan", _dt, 20, "coordwise_lds", 32, nonfinite=True)
    _add("average-nan", _dt, 9, "coordwise", 16, nonfinite=True)
    # averaged median, 16-bit: Bulyan's tail with W = I while n <= 64
    _add("averaged-median", _dt, 7, "tail_mfma", 8, beta=3, bulyan=True)
    _add("averaged-median", _dt, 13, "tail_mfma", 16, beta=9, bulyan=True)
    _add("averaged-median", _dt, 30, "tail_mfma", 32, beta=20, bulyan=True)
    _add("averaged-median", _dt, 64, "tail_mfma", 64, beta=50, bulyan=True)
    _add("averaged-median", _dt, 30, "tail_mfma", 32, beta=20, bulyan=True, nonfinite=True)
    _add("averaged-median", _dt, 13, "tail_window", 16, beta=2, bulyan=True)            # beta < wm_p0(16) = 4
    _add("averaged-median", _dt, 64, "coordwise_lds", 64, beta=40, bulyan=True)         # n - beta > 16
    _add("averaged-median", _dt, 64, "coordwise_lds", 64, beta=40, bulyan=True, nonfinite=True)
    _add("averaged-median", _dt, 100, "coordwise_lds", 128, beta=70)                    # n > 64: no reroute
    _add("averaged-median", _dt, 100, "coordwise_lds", 128, beta=70, nonfinite=True)
    # Bulyan's tail, 16-bit
    _add("bulyan-tail", _dt, 11, "tail_mfma", 8, t=5, beta=3)                           # KS = 1
    _add("bulyan-tail", _dt, 25, "tail_mfma", 16, t=15, beta=9)                         # KS = 2
    _add("bulyan-tail", _dt, 40, "tail_mfma", 32, t=30, beta=18)                        # KS = 3
    _add("bulyan-tail", _dt, 64, "tail_mfma", 64, t=46, beta=30)                        # KS = 4, two set blocks
    _add("bulyan-tail", _dt, 40, "tail_mfma", 32, t=30, beta=18, nonfinite=True)
    _add("bulyan-tail", _dt, 64, "tail_mfma", 64, t=46, beta=30, nonfinite=True)
    _add("bulyan-tail", _dt, 20, "tail_window", 16, t=12, beta=3)                       # the wm_p0 refusal, t in 9..16
    _add("bulyan-tail", _dt, 33, "tail_window", 32, t=21, beta=7)                       # t in 17..32, beta < 8
    _add("bulyan-tail", _dt, 33, "tail_window", 32, t=21, beta=7, nonfinite=True)
    _add("bulyan-tail", _dt, 32, "coordwise_lds", 32, t=32, beta=2)                     # t - beta > 16
    _add("bulyan-tail", _dt, 60, "coordwise_lds", 64, t=50, beta=20)
    _add("bulyan-tail", _dt, 100, "coordwise_lds", 128, t=88, beta=60)                  # ~82 KB static LDS
    _add("bulyan-tail", _dt, 32, "coordwise_lds", 32, t=32, beta=2, nonfinite=True)
    _add("bulyan-tail", _dt, 100, "coordwise_lds", 128, t=88, beta=60, nonfinite=True)
    _add("bulyan-tail", _dt, 70, "coordwise", 8, t=6, beta=2)                           # n > 64, n > NP
    _add("bulyan-tail", _dt, 70, "coordwise", 16, t=14, beta=6)
    _add("bulyan-tail", _dt, 70, "coordwise", 32, t=28, beta=12)
    _add("bulyan-tail", _dt, 70, "coordwise", 64, t=48, beta=20)
    _add("bulyan-tail", _dt, 70, "coordwise", 64, t=48, beta=20, nonfinite=True)

# fp32: the generic kernels for every plain rule
for _n, _np in _N_OF_NP:
    _fam = "coordwise_lds" if _np in (32, 64) else "coordwise"
    _add("median", "f32", _n, _fam, _np)
    _add("trimmed-mean", "f32", _n, _fam, _np, f=(_n - 1) // 3)
    _add("condense", "f32", _n, _fam, _np)
    _add("average-nan", "f32", _n, _fam, _np)
    _add("median", "f32", _n, _fam, _np, nonfinite=True)
    _add("average-nan", "f32", _n, _fam, _np, nonfinite=True)
_add("trimmed-mean", "f32", 20, "coordwise_lds", 32, f=4, nonfinite=True)
_add("condense", "f32", 12, "coordwise", 16, nonfinite=True)
# averaged median, fp32: the direct window kernel, or the generic ones
_add("averaged-median", "f32", 7, "tail_window_direct", 8, beta=3)
_add("averaged-median", "f32", 13, "tail_window_direct", 16, beta=2)
_add("averaged-median", "f32", 30, "tail_window_direct", 32, beta=20)
_add("averaged-median", "f32", 64, "tail_window_direct", 64, beta=50)
_add("averaged-median", "f32", 30, "tail_window_direct", 32, beta=20, nonfinite=True)
_add("averaged-median", "f32", 29, "coordwise_lds", 32, beta=10)
_add("averaged-median", "f32", 64, "coordwise_lds", 64, beta=40)
_add("averaged-median", "f32", 64, "coordwise_lds", 64, beta=40, nonfinite=True)
_add("averaged-median", "f32", 100, "coordwise", 128, beta=70)
_add("averaged-median", "f32", 100, "coordwise", 128, beta=70, nonfinite=True)
# Bulyan's tail, fp32
_add("bulyan-tail", "f32", 11, "tail_f32", 8, t=5, beta=3)                              # NR = 16
_add("bulyan-tail", "f32", 25, "tail_f32", 16, t=15, beta=9)                            # NR = 32
_add("bulyan-tail", "f32", 40, "tail_f32", 32, t=30, beta=18)                           # NR = 64
_add("bulyan-tail", "f32", 64, "tail_f32", 64, t=46, beta=30)
_add("bulyan-tail", "f32", 40, "tail_f32", 32, t=30, beta=18, nonfinite=True)
_add("bulyan-tail", "f32", 64, "tail_f32", 64, t=46, beta=30, nonfinite=True)
_add("bulyan-tail", "f32", 20, "tail_window", 16, t=12, beta=3)
_add("bulyan-tail", "f32", 33, "tail_window", 32, t=21, beta=7)
_add("bulyan-tail", "f32", 33, "tail_window", 32, t=21, beta=7, nonfinite=True)
_add("bulyan-tail", "f32", 32, "coordwise_lds", 32, t=32, beta=2)
_add("bulyan-tail", "f32", 60, "coordwise_lds", 64, t=50, beta=20)
_add("bulyan-tail", "f32", 32, "coordwise_lds", 32, t=32, beta=2, nonfinite=True)
_add("bulyan-tail", "f32", 70, "coordwise", 8, t=6, beta=2)
_add("bulyan-tail", "f32", 70, "coordwise", 16, t=14, beta=6)
_add("bulyan-tail", "f32", 70, "coordwise", 32, t=28, beta=12)
_add("bulyan-tail", "f32", 70, "coordwise", 64, t=48, beta=20)
_add("bulyan-tail", "f32", 100, "coordwise", 128, t=88, beta=60)                        # VEC = 1, 128 sets
_add("bulyan-tail", "f32", 70, "coordwise", 64, t=48, beta=20, nonfinite=True)
_add("bulyan-tail", "f32", 100, "coordwise", 128, t=88, beta=60, nonfinite=True)

# ---- wrap, default knobs: the two hard-coded caps, the smallest d that wraps plus an odd tail ----
_D_LDS = 2048 * 256 + 3 * 256 + 17
_add("median", "f32", 20, "coordwise_lds", 32, ds=(_D_LDS,), wrap=True, tag="wrap")
_add("bulyan-tail", "f32", 32, "coordwise_lds", 32, t=32, beta=2, ds=(_D_LDS,), wrap=True, tag="wrap")
_add("bulyan-tail", "bf16", 32, "coordwise_lds", 32, t=32, beta=2, ds=(_D_LDS,), wrap=True, nonfinite=True, tag="wrap")
_add("median", "f32", 65, "coordwise", 128, ds=(4096 * 256 + 256 + 3,), wrap=True, tag="wrap")          # VEC = 1
_add("trimmed-mean", "f32", 9, "coordwise", 16, f=2, ds=(4096 * 256 * 4 + 1024 + 3,), wrap=True, tag="wrap")   # VEC = 4
_add("median", "f32", 3, "coordwise", 8, ds=(4096 * 256 * 8 + 2048 + 5,), wrap=True, tag="wrap")         # VEC = 8
_add("average-nan", "bf16", 3, "coordwise", 8, ds=(4096 * 256 * 8 + 2048 + 5,), wrap=True, nonfinite=True, tag="wrap")

# ---- wrap, capped by knob (a child process): three passes and more at d = 5037 ----
GRID_ENV = {"GARFIELD_COORD16_GRID": "2", "GARFIELD_TAIL_GRID": "2"}
for _dt in ("bf16", "f16"):
    _add("median", _dt, 12, "coord16", 16, ds=(KNOB_D,), env=GRID_ENV, wrap=True, tag="grid2")          # P = 4
    _add("trimmed-mean", _dt, 20, "coord16", 32, f=4, ds=(KNOB_D,), env=GRID_ENV, wrap=True, tag="grid2")   # P = 2
    _add("condense", _dt, 64, "coord16", 64, ds=(KNOB_D,), env=GRID_ENV, wrap=True, nonfinite=True, tag="grid2")  # P = 1
    _add("bulyan-tail", _dt, 11, "tail_mfma", 8, t=5, beta=3, ds=(KNOB_D,), env=GRID_ENV, wrap=True, tag="grid2")     # KS = 1
    # KS = 4; the second d: 64 groups per wave with a non-finite value in two out of three, more than the
    # kernel's 32-slot list of groups to redo, so its redo-every-group path runs
    _add("bulyan-tail", _dt, 64, "tail_mfma", 64, t=46, beta=30, ds=(KNOB_D, 8 * 64 * 64 + 37), env=GRID_ENV, wrap=True,
         nonfinite=True, tag="grid2")
    _add("bulyan-tail", _dt, 33, "tail_window", 32, t=21, beta=7, ds=(KNOB_D,), env=GRID_ENV, wrap=True, tag="grid2")
_add("bulyan-tail", "f32", 11, "tail_f32", 8, t=5, beta=3, ds=(KNOB_D,), env=GRID_ENV, wrap=True, tag="grid2")        # NR = 16
_add("bulyan-tail", "f32", 64, "tail_f32", 64, t=46, beta=30, ds=(KNOB_D,), env=GRID_ENV, wrap=True, nonfinite=True,
     tag="grid2")                                                                                         # NR = 64
_add("bulyan-tail", "f32", 33, "tail_window", 32, t=21, beta=7, ds=(KNOB_D,), env=GRID_ENV, wrap=True, nonfinite=True,
     tag="grid2")
_add("averaged-median", "f32", 30, "tail_window_direct", 32, beta=20, ds=(KNOB_D,), env=GRID_ENV, wrap=True,
     nonfinite=True, tag="grid2")

# ---- fallback children ----
NO16_ENV = {"GARFIELD_COORD16": "0"}             # every rule and dtype on the generic kernels
for _dt in ("bf16", "f16", "f32"):
    _lds128 = "coordwise_lds" if _dt != "f32" else "coordwise"
    _add("median", _dt, 5, "coordwise", 8, env=NO16_ENV, nonfinite=True, tag="no16")
    _add("trimmed-mean", _dt, 12, "coordwise", 16, f=3, env=NO16_ENV, tag="no16")
    _add("condense", _dt, 20, "coordwise_lds", 32, env=NO16_ENV, nonfinite=True, tag="no16")
    _add("median", _dt, 64, "coordwise_lds", 64, env=NO16_ENV, tag="no16")
    _add("trimmed-mean", _dt, 100, _lds128, 128, f=30, env=NO16_ENV, nonfinite=True, tag="no16")
    _add("average-nan", _dt, 9, "coordwise", 16, env=NO16_ENV, nonfinite=True, tag="no16")
    _add("averaged-median", _dt, 7, "coordwise", 8, beta=3, env=NO16_ENV, bulyan=_dt != "f32", tag="no16")
    _add("averaged-median", _dt, 64, "coordwise_lds", 64, beta=50, env=NO16_ENV, bulyan=_dt != "f32", nonfinite=True,
         tag="no16")
    _add("bulyan-tail", _dt, 11, "coordwise", 8, t=5, beta=3, env=NO16_ENV, tag="no16")
    _add("bulyan-tail", _dt, 25, "coordwise", 16, t=15, beta=9, env=NO16_ENV, nonfinite=True, tag="no16")
    _add("bulyan-tail", _dt, 30, "coordwise_lds", 32, t=30, beta=18, env=NO16_ENV, nonfinite=True, tag="no16")
    _add("bulyan-tail", _dt, 64, "coordwise_lds", 64, t=46, beta=30, env=NO16_ENV, tag="no16")

NOMFMA_ENV = {"GARFIELD_MFMA_TAIL": "0", "GARFIELD_AVGMED_TAIL": "0"}
for _dt in ("bf16", "f16"):
    # 16-bit Bulyan on the incremental window kernel at shapes the MFMA kernel normally takes
    _add("bulyan-tail", _dt, 11, "tail_window", 8, t=5, beta=3, env=NOMFMA_ENV, tag="nomfma")
    _add("bulyan-tail", _dt, 25, "tail_window", 16, t=15, beta=9, env=NOMFMA_ENV, nonfinite=True, tag="nomfma")
    _add("bulyan-tail", _dt, 40, "tail_window", 32, t=30, beta=18, env=NOMFMA_ENV, tag="nomfma")
    _add("bulyan-tail", _dt, 64, "tail_window", 64, t=46, beta=30, env=NOMFMA_ENV, nonfinite=True, tag="nomfma")
    # 16-bit averaged median on the direct window kernel
    _add("averaged-median", _dt, 7, "tail_window_direct", 8, beta=3, env=NOMFMA_ENV, tag="nomfma")
    _add("averaged-median", _dt, 13, "tail_window_direct", 16, beta=9, env=NOMFMA_ENV, nonfinite=True, tag="nomfma")
    _add("averaged-median", _dt, 30, "tail_window_direct", 32, beta=20, env=NOMFMA_ENV, tag="nomfma")
    _add("averaged-median", _dt, 64, "tail_window_direct", 64, beta=50, env=NOMFMA_ENV, nonfinite=True, tag="nomfma")

CASE_BY_ID = {c.id: c for c in CASES}
ENVS = {"grid2": GRID_ENV, "no16": NO16_ENV, "nomfma": NOMFMA_ENV}


def cases_of(env: dict):
    return [c for c in CASES if c.env == env]


def case_seed(case: Case) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) % 9973


def plan_of(native, case: Case, d: int) -> dict:
    return native.coord_plan(DTYPES[case.dtype], MODES[case.mode], case.n, d, case.f, case.beta, case.t)


def plan_key(plan: dict, dt: str):
    return plan["family"], dt, plan["np"], bool(plan["bulyan"])


def check_plan(native, case: Case, d: int) -> dict:
    """coord_plan answers the case's expected family / NP (and wraps where the case says so)."""
    plan = plan_of(native, case, d)
    assert plan_key(plan, case.dtype) == (case.family, case.dtype, case.np, case.bulyan), (case.id, d, plan)
    if case.wrap:
        assert plan["grid"] * plan["coords_per_pass"] < d, (case.id, d, plan)
    return plan


def sweep(native, d: int = 100003) -> set:
    """Every (family, dtype, NP, Bulyan-or-not) coord_plan can answer under this process's knobs: every
    mode and dtype, n = 1 .. 128, every beta of the averaged median, and for Bulyan's tail every
    t = 1 .. n with beta at both ends, around window_mean's thresholds (wm_p0 = 4, 8, 16) and with
    t - beta on both sides of 16. (Trimmed mean's f does not enter the dispatch; both ends are asked.)"""
    keys = set()
    for dt, dtype in DTYPES.items():
        for n in range(1, 129):
            for mode in ("median", "condense", "average-nan"):
                keys.add(plan_key(native.coord_plan(dtype, MODES[mode], n, d, 0, 0, 0), dt))
            for f in {0, (n - 1) // 2}:
                keys.add(plan_key(native.coord_plan(dtype, MODES["trimmed-mean"], n, d, f, 0, 0), dt))
            for beta in range(1, n + 1):
                keys.add(plan_key(native.coord_plan(dtype, MODES["averaged-median"], n, d, 0, beta, 0), dt))
            for t in range(1, n + 1):
                betas = {1, 3, 4, 7, 8, 15, 16, t - 17, t - 16, t - 15, t - 1, t}
                for beta in sorted(b for b in betas if 1 <= b <= t):
                    keys.add(plan_key(native.coord_plan(dtype, MODES["bulyan-tail"], n, d, 0, beta, t), dt))
    return keys


def case_keys(cases) -> set:
    return {(c.family, c.dtype, c.np, c.bulyan) for c in cases}


def inputs(case: Case, d: int, device="cpu"):
    """(X [n, d] in the case's dtype, W (on the CPU) or None, members or None, s)."""
    X = grid_rows(case.n, d, DTYPES[case.dtype], case_seed(case), case.nonfinite, device)
    if case.mode != "bulyan-tail":
        return X, None, None, 1
    W, members, s = bulyan_W(case.n, case.t, case_seed(case))
    return X, W, members, s


def run_case(native, gar, case: Case, d: int, device) -> dict:
    """Run one (case, d) on the GPU against the oracle (float64, on the device). Returns a record with the
    number of mismatching coordinates and the first few of them."""
    check_plan(native, case, d)
    dtype = DTYPES[case.dtype]
    X, W, members, s = inputs(case, d, device if d > KNOB_D else "cpu")   # the wrap cases: drawn on the device
    G = X.to(device)
    want = oracle(G, case.mode, case.f, case.beta, members, s)
    rows = gar.prepare(G)
    Wd = W.to(device).reshape(-1) if W is not None else None

    def direct(out_dtype):
        out = torch.full((rows.d,), -777.0, dtype=out_dtype, device=device)
        native.gpu_coordwise(rows.obj, MODES[case.mode], case.f, case.beta, Wd, case.t, CONDENSE_SEED,
                             CONDENSE_P if case.mode == "condense" else 1.0, out)
        return out

    if case.mode == "bulyan-tail":
        got = direct(dtype)
    elif case.mode == "median":
        got = gar.median(G)
    elif case.mode == "trimmed-mean":
        got = gar.trimmed_mean(G, case.f)
    elif case.mode == "averaged-median":
        got = gar.averaged_median(G, beta=case.beta)
    elif case.mode == "average-nan":
        got = gar.average_nan(G)
    else:
        got = gar.condense(G, p=CONDENSE_P, seed=CONDENSE_SEED)
    # 16-bit rows also with an fp32 output (the same launch: the plan does not depend on the output dtype):
    # 2 ulp of bf16 would hide one wrong member of a large window, 2 ulp of fp32 does not
    got32 = direct(torch.float32) if dtype != torch.float32 else None
    torch.cuda.synchronize(device)
    bad = mismatches(got, want, case.mode, dtype)
    if got32 is not None:
        bad32 = mismatches(got32, want, case.mode, torch.float32)
        if bad32.numel():
            got, bad = got32, torch.cat([bad32, bad])
    rec = {"id": case.id, "d": d, "bad": int(bad.numel())}
    if bad.numel():
        i = bad[:5]
        rec["first"] = [(int(x), float(got[x]), float(want[x])) for x in i.tolist()]
    return rec
