"""The adaptive colluding attacks Min-Max / Min-Sum (Shejwalkar & Houmansadr, NDSS 2021), solved on the
Gram matrix of the colluders' estimates (docs/GAR_SEMANTICS.md "Adaptive colluding attacks").

Every Byzantine row becomes m = μ + γ p (μ the mean of the k estimate rows, p = -σ, -μ or -sign μ) with the
largest γ that keeps m inside the estimates' distance ball. γ has a closed form in a_i = ‖μ - e_i‖² (from
the pairwise distances, hence from the Gram), b_i = Σ_x p (μ - e_i) and c = Σ_x p², so the work is three
steps, each a function here:

* ``agr_partials``: the Gram and (b, c) of a coordinate range, both ADDITIVE over ranges (the sharded
  step sums them over buckets and ranks);
* ``agr_gamma``: γ from the summed statistics, on the device (no host round trip);
* ``agr_write``: the Byzantine rows in place, γ read from device memory.

GPU rows (fp32 / bf16 / fp16, at most ``MAX_ROWS``) run the gfx950 kernels of ``csrc/gar_agr_attack.hip``;
CPU tensors take the same steps in torch fp64.
"""
from __future__ import annotations

import math

import torch

from garfield_amd import _native
from garfield_amd.ops import gar
from garfield_amd.ops import reference as ref
from garfield_amd.ops.selection import MAX_ROWS

OBJECTIVES = ("minmax", "minsum")
PERTURBATIONS = ("std", "uv", "sgn")
KINDS = tuple(o + s for o in OBJECTIVES for s in ("", "-uv", "-sgn"))
_PERT = {"std": 0, "uv": 1, "sgn": 2}


def parse(kind: str) -> tuple:
    """``"minmax-uv"`` -> ``("minmax", "uv")``; no suffix means ``std``."""
    objective, _, perturbation = kind.partition("-")
    perturbation = perturbation or "std"
    if objective not in OBJECTIVES or perturbation not in PERTURBATIONS:
        raise ValueError(f"unknown adaptive attack {kind!r}; available: {KINDS}")
    return objective, perturbation


def _check(rows, perturbation: str, lo: int, hi) -> tuple:
    if perturbation not in _PERT:
        raise ValueError(f"unknown perturbation {perturbation!r}; available: {PERTURBATIONS}")
    rows = list(rows)
    if not rows:
        raise ValueError("expected a non-empty list of estimate rows")
    d = rows[0].numel()
    if any(r.dim() != 1 or r.numel() != d or r.device != rows[0].device or r.dtype != rows[0].dtype for r in rows):
        raise ValueError("the estimate rows must be 1-D tensors of one length, dtype and device")
    hi = d if hi is None else hi
    if not 0 <= lo <= hi <= d:
        raise ValueError(f"0 <= lo <= hi <= {d} expected, got [{lo}, {hi})")
    return rows, hi


def _native_for(rows):
    """The extension for GPU rows (mandatory there), None for the torch fp64 path of CPU tensors."""
    r = rows[0]
    if not r.is_cuda:
        return None
    if len(rows) > MAX_ROWS:
        raise ValueError(f"the adaptive attacks take at most {MAX_ROWS} estimate rows on the GPU, got {len(rows)}")
    if r.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"the adaptive attacks take fp32, bf16 or fp16 rows on the GPU, got {r.dtype}")
    if any(not t.is_contiguous() for t in rows):
        raise ValueError("the estimate rows must be contiguous")
    return _native.require_for(r.device)


def agr_partials(rows, perturbation: str = "std", lo: int = 0, hi: int | None = None, reduce: bool = True) -> tuple:
    """``(gram, partial)`` of the coordinates [lo, hi) of the k estimate ``rows``, both additive over
    coordinate ranges. GPU: ``gram`` the padded fp32 Gram (flat, as the selections take it) and ``partial``
    fp64 [k + 1] = (b_0..b_{k-1}, c); ``reduce=False`` leaves the workgroups' partial vectors [g, k + 1]
    for ``agr_gamma`` to sum (one launch less, not additive). CPU: fp64 [k, k] and [k + 1]."""
    rows, hi = _check(rows, perturbation, lo, hi)
    k = len(rows)
    C = _native_for(rows)
    if C is None:
        X = torch.stack([r[lo:hi] for r in rows]).double()
        mu, p = ref.agr_perturbation(X, perturbation)
        return X @ X.T, torch.cat([(p * (mu - X)).sum(1), (p * p).sum().reshape(1)])
    dev = rows[0].device
    np_ = C.gram_padded(k)
    parts = torch.empty((C.agr_grid(hi - lo), k + 1), dtype=torch.float64, device=dev)
    C.gpu_agr_stats(rows, _PERT[perturbation], lo, hi, parts)
    if reduce:
        out = torch.empty(k + 1, dtype=torch.float64, device=dev)
        C.gpu_agr_reduce(parts, parts.shape[0], k, out)
        parts = out
    if hi == lo:
        return torch.zeros(np_ * np_, dtype=torch.float32, device=dev), parts
    pr = gar.prepare([r[lo:hi] for r in rows])    # the existing Gram launch (copies a row that is not aligned)
    return gar._gram_into(C, pr, gar.workspace(pr)).clone(), parts


def _distances(gram: torch.Tensor) -> torch.Tensor:
    """fp64 squared distances from an fp64 Gram under the shared conventions: non-finite -> +inf, clamped
    at 0, a zero diagonal."""
    dg = torch.diagonal(gram)
    D = dg[:, None] + dg[None, :] - 2 * gram
    D = torch.where(torch.isfinite(D), D.clamp(min=0), torch.full_like(D, math.inf))
    D.fill_diagonal_(0.0)
    return D


def agr_gamma(gram: torch.Tensor, partial: torch.Tensor, objective: str, info: bool = False):
    """γ (a one-element tensor on the statistics' device: fp32 from the kernel, fp64 on the CPU) of the
    Min-Max or Min-Sum attack from the summed ``agr_partials``. ``info=True`` also returns the fp64 vector
    (γ, R or S, a_0..a_{k-1}, b_0..b_{k-1})."""
    if objective not in OBJECTIVES:
        raise ValueError(f"unknown objective {objective!r}; available: {OBJECTIVES}")
    k = partial.shape[-1] - 1
    if gram.is_cuda:
        C = _native.require_for(gram.device)
        parts = partial.contiguous()
        gamma = torch.empty(1, dtype=torch.float32, device=gram.device)
        inf_ = torch.empty(2 + 2 * k, dtype=torch.float64, device=gram.device)
        C.gpu_agr_solve(gram.contiguous().view(-1), k, parts, parts.numel() // (k + 1), objective == "minsum",
                        gamma, inf_)
        return (gamma, inf_) if info else gamma
    partial = partial.double().reshape(-1, k + 1).sum(0)
    D = _distances(gram.double())
    r = D.mean(1)
    a = r - r.mean() / 2
    b, c = partial[:k], partial[k]
    if objective == "minmax":
        bound = D.max()
        t = (bound - a).clamp(min=0)
        disc = torch.sqrt(b * b + c * t)
        g = torch.where(b > 0, t / (b + disc), (disc - b) / c).min()
    else:
        bound = D.sum(1).max()
        g = torch.sqrt((bound - a.sum()).clamp(min=0) / (k * c))
    ok = (c > 0) & torch.isfinite(c) & torch.isfinite(bound) & torch.isfinite(a).all() & torch.isfinite(b).all() \
        & torch.isfinite(g) & torch.tensor(k > 1)
    g = torch.where(ok, g, torch.zeros_like(g)).reshape(1)
    return (g, torch.cat([g, bound.reshape(1), a, b])) if info else g


def agr_write(rows, n_peers: int, gamma: torch.Tensor, perturbation: str = "std", lo: int = 0,
              hi: int | None = None) -> None:
    """``rows[n_peers:]`` <- μ + γ p on the coordinates [lo, hi), in place (μ, p over all the rows, read
    before anything is written); rows below ``n_peers`` and coordinates outside the range stay untouched."""
    rows, hi = _check(rows, perturbation, lo, hi)
    if not 0 <= n_peers <= len(rows):
        raise ValueError(f"0 <= n_peers <= {len(rows)} expected, got {n_peers}")
    C = _native_for(rows)
    if C is not None:
        C.gpu_agr_write(rows, n_peers, gamma, _PERT[perturbation], lo, hi)
        return
    X = torch.stack([r[lo:hi] for r in rows]).double()
    mu, p = ref.agr_perturbation(X, perturbation)
    g = gamma.double().reshape(())
    m = torch.where(g == 0, mu, mu + g * p)    # γ = 0 leaves μ whatever p is
    for r in rows[n_peers:]:
        r[lo:hi].copy_(m)


def attack_rows(rows, n_peers: int, kind: str, info: bool = False):
    """One attack ``kind`` on whole rows, in place: statistics, Gram, solve, write. Returns γ (and the
    solve's fp64 vector with ``info=True``)."""
    objective, perturbation = parse(kind)
    gram, parts = agr_partials(rows, perturbation, reduce=False)
    out = agr_gamma(gram, parts, objective, info)
    agr_write(rows, n_peers, out[0] if info else out, perturbation)
    return out


def attack(E: torch.Tensor, kind: str) -> torch.Tensor:
    """The attack vector of the estimates ``E`` [k, d] (runtime/attacks.py): a new [d] tensor of E's dtype."""
    rows = [E[i].contiguous() for i in range(E.shape[0] - 1)] + [E[-1].clone()]
    attack_rows(rows, len(rows) - 1, kind)
    return rows[-1]
