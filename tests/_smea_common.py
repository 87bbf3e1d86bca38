"""What test_smea_cpu.py and test_smea_gpu.py share: the inputs, the rank of a subset and the oracle per case.

Inputs. ``plain``: rows N(0, I); nothing separates the subsets, the best and the runner-up can be close.
``planted``: attacked(n, f, d, dtype, seed) of tests/_caf_common.py (rows N(0, I), the last f rows shifted by one
common 3 N(0, I)): the subset without the shifted rows wins by far, so the winner is compared exactly. The
oracle sees the rows after the cast to dtype (bf16 / fp16 widen exactly).

``colluders(z, seed)``: the case the rule exists for. n = 12, f = 3, d = 200, honest rows N(0, I), the three
colluders identical at the honest mean + z along the first coordinate (σ = 1). Brute's diameter is blind to
them (they are closer to every honest row than two honest rows are to each other, and at distance 0 from each
other); the eigenvalue sees the direction they share. z = 17 and seed 9 were chosen on the CPU with the fp64
oracle and ``smea_dense_lambda``: a scan of z in {17, 17.5, ..., 20} x seeds 0..19 with C++ Brute and SMEA gave
(seed, z) = (0, 17), (9, 17), (10, 17), (12, 18.5), (13, 18), ... where Brute keeps all three colluders and SMEA
none; at (9, 17) the oracle's runner-up is 5.4 % above its best. Below z = 17 a single colluder (which sits at
the honest mean) is still cheaper than the ninth honest row: 8 z² / 81 < λ of the honest rows (about 30)."""
import functools
import math

import torch

from _caf_common import attacked
from garfield_amd.ops import reference as ref

COLLUDERS_Z = 17.0
COLLUDERS_SEED = 9
MARGIN = 1e-3   # the oracle's runner-up above its best, relative: beyond it the winner is compared exactly


def plain(n, d, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(7000 * n + d + seed)
    return torch.randn(n, d, generator=g).to(dtype)


def rows(kind, n, f, d, dtype=torch.float32):
    return plain(n, d, dtype) if kind == "plain" else attacked(n, f, d, dtype)


def colluders(z=COLLUDERS_Z, seed=COLLUDERS_SEED, n=12, f=3, d=200):
    g = torch.Generator().manual_seed(seed)
    H = torch.randn(n - f, d, generator=g, dtype=torch.float64)
    c = H.mean(0)
    c[0] += z
    return torch.cat([H, c[None, :].repeat(f, 1)])


def members_of(w):
    return [i for i, v in enumerate(w.tolist()) if v != 0.0]


def rank_of(members):
    """The position of the subset's mask among the masks of as many bits, in increasing numeric order."""
    return sum(math.comb(c, i + 1) for i, c in enumerate(sorted(members)))


def ulps(a, b):
    """The distance of two non-negative fp32 values in units in the last place (inf: one past the largest)."""
    a = torch.tensor(float(a), dtype=torch.float32).view(torch.int32)
    b = torch.tensor(float(b), dtype=torch.float32).view(torch.int32)
    return abs(int(a) - int(b))


def best_of(lams):
    """(key [C] fp32, rank of the smallest (key, rank), (runner-up - best) / best in fp64, inf with one subset)."""
    key = ref.smea_key(lams)
    rank = int(torch.where(key == key.min(), torch.arange(key.numel()), key.numel()).min())
    s = lams.sort().values
    margin = float((s[1] - s[0]) / s[0]) if s.numel() > 1 and float(s[0]) > 0 else math.inf
    return key, rank, margin


@functools.lru_cache(maxsize=None)
def case(kind, n, f, d, dtype):
    """(rows on the CPU, λ of every subset [C] fp64 on the vectors, their fp32 keys, the winner's rank, the
    margin) computed once, shared, never modified."""
    X = rows(kind, n, f, d, dtype)
    lams = ref.smea_lambdas(ref.pairwise_sqdist(X), f)
    return (X, lams) + best_of(lams)
