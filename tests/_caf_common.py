"""What test_caf_cpu.py and test_caf_gpu.py share: the inputs and the preconditions on the oracle.

Inputs: attacked(n, f, d, dtype, seed) of tests/test_dnc_gpu.py: rows N(0, I), the last f rows shifted by one
common 3 N(0, I); the oracle sees the rows after the cast to dtype.

Preconditions, asserted on the oracle's trace for every case with f >= 1, so that no discrete decision of
the filter (another pass or not, which pass is kept, which row gets the exact zero) hangs on rounding:
at every loop test |Σc - (n - 2f)| >= 1e-3; any two passes' λ differ by >= 1e-4 relative; at every pass the
two largest τ among the rows that still carry weight differ by >= 1e-4 relative.

Seeds: seed 0 holds over n in {3, 4, 5, 8, 16, 17, 33, 64, 65, 127, 128, 130} x d in {64, 2000} x
f in {(n - 1) // 4, (n - 1) // 2} x fp32 / bf16 / fp16 except at the (n, d, f) of SEEDS, where some dtype has
two λ or two τ closer than 1e-4 and seed 1 holds for all three dtypes."""
import functools

import torch

from garfield_amd.ops import reference as ref

SEEDS = {(128, 2000, 31): 1, (130, 2000, 32): 1, (130, 2000, 64): 1}


def attacked(n, f, d, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(1000 * n + d + seed)
    X = torch.randn(n, d, generator=g)
    if f:
        X[n - f:] += 3.0 * torch.randn(d, generator=g)
    return X.to(dtype)


def assert_preconditions(trace, n, f):
    for sc in trace["sums"]:
        assert abs(sc - (n - 2 * f)) >= 1e-3, (sc, n - 2 * f)
    lams = trace["lams"]
    for i in range(len(lams)):
        for j in range(i):
            assert abs(lams[i] - lams[j]) >= 1e-4 * max(lams[i], lams[j]), (j, i, lams[j], lams[i])
    for p, taus in enumerate(trace["taus"]):
        if len(taus) >= 2:
            assert taus[0] - taus[1] >= 1e-4 * taus[0], (p, taus[0], taus[1])


@functools.lru_cache(maxsize=None)
def case(n, d, dtype, f):
    """(rows on the CPU, the oracle's trace, its fp32 weights, its fp32 lams, its output) of
    attacked(n, f, d, dtype) with the seed of SEEDS: computed once, shared, never modified."""
    X = attacked(n, f, d, dtype, SEEDS.get((n, d, f), 0))
    D = ref.pairwise_sqdist(X)
    trace = ref.caf_trace(D, f)
    if f:
        assert_preconditions(trace, n, f)
    lams = torch.full((n,), float("inf"), dtype=torch.float64)   # as ref.caf_weights lays them out
    lams[:len(trace["lams"])] = torch.tensor(trace["lams"], dtype=torch.float64)
    return X, trace, trace["weights"].float(), lams.float(), ref.combine(X, trace["weights"])
