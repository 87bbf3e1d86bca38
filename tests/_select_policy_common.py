"""The validity policy that the iterated Gram selections share (docs/GAR_SEMANTICS.md: geometric median,
centered clipping, DnC), on crafted Gram matrices: the inputs, the oracle results and the comparison used
by test_select_policy_cpu.py and test_select_policy_gpu.py. Both sides see the same fp32 distances."""
import functools
import math

import torch

import test_cclip_gpu
import test_dnc_gpu
import test_geomed_gpu
from garfield_amd.ops import reference as ref
from garfield_amd.ops.selection import distances_from_gram

RULES = ["geomed", "cclip", "dnc"]
SIZES = [17, 65, 128]   # the wave-per-row wrap, the second lane column, the LDS maximum
# (a) one unusable pair; (b) and a row without a finite distance; (c) centered clipping: and a basis-only last row
CASES = [(r, c) for r in RULES for c in "ab"] + [("cclip", "c")]
F = 2   # centered clipping's f (data-derived radius, uniform start); DnC keeps m = n - 3 rows
# The per-weight / per-score bounds of the kernels' own tests, measured there with the fp32 Gram's rounding
# of D on one side only: test_geomed_gpu.WEIGHT_RTOL, test_cclip_gpu.WEIGHT_RTOL, test_dnc_gpu.SCORE_RTOL.
RTOL = {"geomed": test_geomed_gpu.WEIGHT_RTOL, "cclip": test_cclip_gpu.WEIGHT_RTOL, "dnc": test_dnc_gpu.SCORE_RTOL}


@functools.lru_cache(maxsize=None)
def gram(n, case):
    """The crafted fp32 Gram [n, n] on the CPU; (d): every entry NaN. Shared, never modified."""
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, 200, generator=g) * torch.linspace(0.5, 3, n)[:, None] + torch.randn(200, generator=g)
    G = X @ X.T
    G = torch.triu(G) + torch.triu(G, 1).T
    if case == "d":
        return torch.full_like(G, math.nan)
    G[0, 1] = G[1, 0] = math.nan   # both rows stay valid, the pair counts as 0
    if case in "bc":
        G[n - 2, :] = math.nan     # row n - 2 has no finite distance
        G[:, n - 2] = math.nan
    return G


def nw_of(rule, n, case):
    return n - 1 if rule == "cclip" and case in "cd" else n


@functools.lru_cache(maxsize=None)
def oracle(rule, n, case):
    """(weights, DnC's scores or None) of reference.py on fill_distances' fp32 distances of gram(n, case)."""
    D = distances_from_gram(gram(n, case))
    if rule == "geomed":
        return ref.geomed_weights(D), None
    if rule == "cclip":
        return ref.cclip_weights(D, nw_of(rule, n, case), None, None, F, 3), None
    return ref.dnc_weights(D, n - 3)


def check(rule, n, case, w, aux=None):
    """One implementation's weights [n] (aux: the kernel's dists / DnC's scores, when it has them) against
    the oracle. Exact zeros, the kept set and the uniform fallback are compared exactly."""
    w_ref, s_ref = oracle(rule, n, case)
    w = w.cpu()
    if case == "d":   # no valid row: the plain average (of the workers), dists / scores 0
        assert torch.equal(w, w_ref.float())
        assert aux is None or aux.tolist() == [0.0] * n
        return
    assert float(w[0]) > 0.0 and float(w[1]) > 0.0 and float(w_ref[0]) > 0.0 and float(w_ref[1]) > 0.0
    if case != "a":
        assert float(w[n - 2]) == 0.0 and (aux is None or float(aux[n - 2]) == math.inf)
    if rule == "dnc":
        assert int((w_ref > 0).sum()) == n - 3 and torch.equal(w, w_ref)   # (b): the invalid row is charged first
        if aux is not None:
            err = test_dnc_gpu.score_err(aux, s_ref)
            print(f"{rule} n={n} ({case}): max score error / largest score {err:.3e}")
            assert err <= RTOL[rule]
        return
    err = test_cclip_gpu.relerr(w, w_ref)   # where the oracle has an exact zero the value must be one too
    print(f"{rule} n={n} ({case}): max relative weight error {err:.3e}")
    assert abs(float(w.double().sum()) - 1.0) < 1e-6 and err <= RTOL[rule]
    if case == "c":
        assert float(w[n - 1]) == 0.0   # the basis-only row never gains weight from a uniform start
