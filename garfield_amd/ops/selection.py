"""The distance-based selections, dispatched from one table.

Krum, the geometric median, centered clipping, DnC, CAF, Brute, SMEA and Bulyan all decide from the pairwise
squared distances of the gradients alone and end in a weight vector over the rows (Bulyan: ``W [t, n]``,
one row per selection round). "Which selection, with which arguments, on which backend" is decided here
and nowhere else:

* :func:`resolve` turns ``(rule, n, f, m, pre, gar_kwargs)`` into a :class:`Selection`: the rule's own
  arguments with the defaults applied and validated, once;
* a :class:`Selection` runs on one of three backends: :meth:`~Selection.on_device` (the one-workgroup
  ``gpu_*_select`` kernels on a device Gram, n <= MAX_ROWS, flat or batched over segments),
  :meth:`~Selection.on_host` (fp64 squared distances: the C++ functions, else the oracle of
  ``ops/reference.py``) and :meth:`~Selection.from_gram` (vectorised on the Gram's own device, any n);
* ``pre="nnm"`` wraps each of them in the mix -> selection on the mixed rows -> un-mix sandwich;
  ``pre="arc"`` in adaptive robust clipping (scale the Gram -> selection on the clipped rows -> fold the
  scales into the weights), ``pre="arc+nnm"`` in both, the clipping outermost.

A new distance rule is one ``_Rule`` entry in :data:`TABLE` plus its arguments in :func:`resolve`;
``ops/gar.py`` and the engines only pick the backend.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, NamedTuple

import torch

from garfield_amd import _native
from garfield_amd.ops import reference as ref

MAX_ROWS = 128
CCLIP_STARTS = ("mean", "krum")
NNM_RULES = ("krum", "geomed", "cclip", "average")
ARC_RULES = ("krum", "geomed", "cclip", "dnc", "caf", "average")
# the pre-aggregations: the rules each takes, and its prefix in the registry's names and in messages
PRE_RULES = {"nnm": NNM_RULES, "arc": ARC_RULES, "arc+nnm": NNM_RULES}
PRE_TAGS = {"nnm": "nnm", "arc": "arc", "arc+nnm": "arc-nnm"}
BRUTE_MAX_SUBSETS = 2 ** 32
# SMEA scores a subset by iters * k^2 multiply-adds where Brute takes k^2 / 2 compares: the most subsets one
# k_smea_search launch may enumerate. Measured on one MI355X (profiles/r20/smea/): the worst case it admits at
# n = 32, (n, f) = (32, 8) with 10 518 300 subsets of k = 24, takes 39.0 ms per launch with 16 rounds (3.7 ns per
# subset; per_n/kernel_stats_n32.csv), far below the one second a launch may hold a shared device: the cap stays at 2^24.
SMEA_MAX_SUBSETS = 2 ** 24


# --------------------------------------------------------------------------- #
# Selections vectorised on a Gram matrix (any n, on the Gram's device, no host round trip)


def large_select(g: torch.Tensor, f: int, m: int, bulyan: bool = False) -> torch.Tensor:
    """Multi-Krum weights [n] (or Bulyan's W [t, n]) from a GPU fp32 Gram of up to LARGE_ROWS rows, on
    device (gar_large.hip: per-row neighbourhoods by an LDS bitonic sort, the selection rounds in one
    workgroup; fp64 distances): no host round trip."""
    n = g.shape[0]
    rounds = n - 2 * f - 2 if bulyan else 1
    W = torch.empty((rounds, n), dtype=torch.float32, device=g.device)
    _native.native().gpu_large_select(g.float().contiguous(), f, m, rounds, bulyan, W)
    return W if bulyan else W[0]


def distances_from_gram(g: torch.Tensor) -> torch.Tensor:
    """Squared distances [n, n] from a Gram matrix: +inf on the diagonal and where non-finite."""
    dg = torch.diagonal(g)
    D = (dg[:, None] + dg[None, :] - 2 * g)
    D = torch.where(torch.isfinite(D), D.clamp(min=0), torch.full_like(D, math.inf))
    D.fill_diagonal_(math.inf)
    return D


def krum_weights_from_gram(g: torch.Tensor, f: int, m: int) -> torch.Tensor:
    """Multi-Krum weights [n] (fp32, g's device) from a Gram matrix (vectorised, any n)."""
    n = g.shape[0]
    D = distances_from_gram(g)
    q = n - f - 2
    near = torch.sort(D, dim=1, stable=True).values[:, :q]
    scores = near.sum(1)
    scores = torch.where(torch.isnan(scores), torch.full_like(scores, math.inf), scores)
    order = torch.sort(scores, stable=True).indices
    w = torch.zeros(n, dtype=torch.float32, device=g.device)
    w[order[:m]] = 1.0 / m
    return w


def geomed_weights_from_gram(g: torch.Tensor, iters: int = 32, nu: float = 1e-6) -> torch.Tensor:
    """Geometric-median weights [n] (fp32, g's device) from a Gram matrix (vectorised, any n):
    reference.geomed_weights with the distances built as the selection kernels build them."""
    n = g.shape[0]
    D = distances_from_gram(g).double()
    D.fill_diagonal_(0.0)
    fin = torch.isfinite(D)
    fin.fill_diagonal_(False)
    valid = fin.any(1)
    D = torch.where(fin, D, torch.zeros_like(D))
    nv = valid.sum()
    # no valid row (n == 1, every pair non-finite): uniform 1/n, without a host branch on device data
    a = torch.where(valid, 1.0 / nv.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=g.device))
    for _ in range(iters):
        s = (D * a[None, :]).sum(1)
        q = 0.5 * (a * s).sum()
        b = torch.where(valid, 1.0 / (s - q).clamp(min=0).sqrt().clamp(min=nu), torch.zeros_like(s))
        a = b / b.sum().clamp(min=torch.finfo(torch.float64).tiny)
    a = torch.where(nv > 0, a, torch.full_like(a, 1.0 / n))
    return a.float()


def dnc_weights_from_gram(g: torch.Tensor, m: int, iters: int = 16, with_scores: bool = False):
    """DnC weights [n] (fp32, g's device; with the fp32 scores when ``with_scores``) from a Gram matrix
    (vectorised in fp64, any n, no host round trip): reference.dnc_weights with the distances built as
    the selection kernels build them, and rank masks in place of a host-side kv."""
    n = g.shape[0]
    dev = g.device
    D = distances_from_gram(g).double()
    D.fill_diagonal_(0.0)
    fin = torch.isfinite(D)
    fin.fill_diagonal_(False)
    valid = fin.any(1)
    D = torch.where(fin, D, torch.zeros_like(D))   # invalid rows and columns: all zero
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    nv = valid.sum()
    nvd = nv.clamp(min=1).double()
    ids = torch.arange(n, device=dev)
    r = D.sum(1) / nvd
    gm = r.sum() / nvd
    kappa = torch.where(valid, r - 0.5 * gm, torch.full_like(r, -math.inf))
    star = torch.where(kappa == kappa.max(), ids, torch.full_like(ids, n - 1)).min().reshape(1)
    b = torch.where(valid, -0.5 * (D.index_select(1, star)[:, 0] - r - r.index_select(0, star) + gm), zero)
    u = torch.zeros_like(b)
    tiny = torch.finfo(torch.float64).tiny
    for _ in range(iters):
        nu = (b * b).sum().sqrt()
        u = torch.where(nu > 0, b / nu.clamp(min=tiny), zero)
        c = u.sum() / nvd
        t = (D * torch.where(valid, u - c, zero)[None, :]).sum(1)
        b = torch.where(valid, -0.5 * (t - t.sum() / nvd), zero)
    lam = (u * b).sum()
    s = torch.where(lam > 0, b * b / lam.clamp(min=tiny), zero).float()
    s = torch.where(valid, s, torch.full_like(s, math.inf))
    # rank by (fp32 score, index); invalid rows carry +inf and kv <= |V| keeps them out
    before = (s[None, :] < s[:, None]) | ((s[None, :] == s[:, None]) & (ids[None, :] < ids[:, None]))
    kv = nv.clamp(max=m)
    keep = valid & (before.sum(1) < kv)
    w = torch.where(keep, 1.0 / kv.clamp(min=1).double(), zero).float()
    # no valid row (n == 1, every pair non-finite): uniform 1/n and zero scores, without a host branch
    w = torch.where(nv > 0, w, torch.full_like(w, 1.0 / n))
    s = torch.where(nv > 0, s, torch.zeros_like(s))
    return (w, s) if with_scores else w


def cclip_weights_from_gram(g: torch.Tensor, nw: int | None = None, a0: torch.Tensor | None = None,
                            tau: float | None = None, f: int = 0, iters: int = 3) -> torch.Tensor:
    """Centered-clipping weights [n] (fp32, g's device) from a Gram matrix (vectorised in fp64, any n, no
    host round trip): reference.cclip_weights with the distances built as the selection kernels build
    them. Rows nw..n-1 are basis-only; ``a0`` None: uniform on the workers; ``tau`` None: from the data."""
    n = g.shape[0]
    nw = n if nw is None else nw
    D = distances_from_gram(g).double()
    D.fill_diagonal_(0.0)
    fin = torch.isfinite(D)
    fin.fill_diagonal_(False)
    valid = fin.any(1)
    D = torch.where(fin, D, torch.zeros_like(D))
    zero = torch.zeros((), dtype=torch.float64, device=g.device)
    is_worker = torch.arange(n, device=g.device) < nw
    V = valid & is_worker
    nv = V.sum()
    nvd = nv.clamp(min=1).double()
    uniform = torch.where(V, 1.0 / nvd, zero)
    if a0 is None:
        a = uniform
    else:
        a = torch.where(valid, a0.to(g.device, torch.float64).reshape(-1), zero)
        tot = a.sum()
        ok = torch.isfinite(tot) & (tot > 0)
        a = torch.where(ok, a / torch.where(ok, tot, torch.ones_like(tot)), uniform)
    k = (nv - f).clamp(min=1)
    for _ in range(iters):
        s = (D * a[None, :]).sum(1)
        q = 0.5 * (a * s).sum()
        r = (s - q).clamp(min=0).sqrt()
        if tau is None:   # the k-th smallest r over V: only its value is used
            t = torch.sort(torch.where(V, r, torch.full_like(r, math.inf))).values.gather(0, (k - 1).reshape(1))[0]
        else:
            t = torch.full((), float(tau), dtype=torch.float64, device=g.device)
        lam = torch.where(V & (r > t), t / r, V.double())
        a = a * (1.0 - lam.sum() / nvd) + lam / nvd
    # no valid worker (n == 1, every pair non-finite): uniform on the workers, without a host branch on device data
    a = torch.where(nv > 0, a, torch.where(is_worker, 1.0 / nw, zero))
    return a.float()


def nan_inf(X: torch.Tensor) -> torch.Tensor:
    return torch.where(torch.isnan(X), torch.full_like(X, math.inf), X)


def large_bulyan_weights(D: torch.Tensor, f: int, m: int) -> torch.Tensor:
    """reference.bulyan_weights vectorised over n (fp64, CPU: t sequential tiny steps):
    each gradient's q nearest-neighbour distances P, scores = row sums, then t rounds of
    'weights over the mk best scores; remove the best; subtract its column of P'."""
    D = D.double().cpu()
    n = D.shape[0]
    t, q = n - 2 * f - 2, n - f - 2
    Dn = nan_inf(D.clone())
    Dn.fill_diagonal_(math.inf)
    near = torch.sort(Dn, dim=1, stable=True).indices[:, :q]
    P = torch.zeros((n, n), dtype=torch.float64)
    P.scatter_(1, near, D.gather(1, near))
    scores = P.sum(1)
    W = torch.zeros((t, n), dtype=torch.float64)
    for k in range(t):
        mk = max(m - k, 1)
        order = torch.sort(nan_inf(scores), stable=True).indices   # by (value, index), NaN last: reference._order
        W[k, order[:mk]] = 1.0 / mk
        best = int(order[0])
        scores -= P[:, best]
        scores[best] = ref.FLT_MAX
    return W


def nnm_from_gram(g: torch.Tensor, f: int) -> tuple:
    """(H, S) from a Gram matrix, vectorised in fp64 on g's device (any n, no host round trip): the
    fp32 pseudo-Gram H of the mixed rows (H_ii = 0, H_ij = -D'_ij / 2, so that distances_from_gram(H)
    = D') and the membership matrix S [n, n] (bool, S_ij: j ∈ S_i). reference.nnm_distances with
    matrix products for the sums; equal sets give an exact zero."""
    n = g.shape[0]
    c = n - f
    D = distances_from_gram(g).double()
    key = D.clone()
    key.fill_diagonal_(-1.0)   # row i itself first, then (distance, index)
    near = torch.sort(key, dim=1, stable=True).indices[:, :c]
    S = torch.zeros((n, n), dtype=torch.bool, device=g.device)
    S.scatter_(1, near, torch.ones_like(near, dtype=torch.bool))
    Sd = S.double()
    D.fill_diagonal_(0.0)
    fin = torch.isfinite(D)
    M = Sd @ torch.where(fin, D, torch.zeros_like(D)) @ Sd.T / float(c * c)
    M = torch.triu(M) + torch.triu(M, 1).T
    bad = (Sd @ (~fin).double() @ Sd.T) > 0    # an infinite pair inside S_i x S_j
    taint = torch.diagonal(bad)
    dm = torch.diagonal(M)
    Dm = (M - 0.5 * dm[:, None] - 0.5 * dm[None, :]).clamp(min=0)
    Dm = torch.where((Sd @ Sd.T) == c, torch.zeros_like(Dm), Dm)
    Dm = torch.where(bad | bad.T | taint[:, None] | taint[None, :], torch.full_like(Dm, math.inf), Dm)
    H = (-0.5 * Dm).float()
    H.fill_diagonal_(0.0)
    return H, S


def nnm_fold(S: torch.Tensor, a: torch.Tensor, c: int) -> torch.Tensor:
    """w_j = (1/c) Σ_{i : j∈S_i} a_i / Σ_i a_i in fp64 (zero a_i add nothing), as fp32."""
    a = a.to(S.device, torch.float64)
    acc = torch.where(S, a[:, None], torch.zeros((), dtype=torch.float64, device=S.device)).sum(0)
    return (acc / a.sum().clamp(min=torch.finfo(torch.float64).tiny) / c).float()


def arc_count(n: int, f: int) -> int:
    """Rows adaptive robust clipping may clip: k = (2 f (n - f)) // n (< n; 0 exactly when f = 0)."""
    return (2 * f * (n - f)) // n


def arc_scales_from_sqnorms(s: torch.Tensor, f: int) -> torch.Tensor:
    """The ARC scales [n] (fp32, s's device) from the squared norms ``s`` (a Gram's diagonal), vectorised, any n,
    no host round trip: reference.arc_scales with the rank counted as k_arc_scale counts it. From the same
    fp32 diagonal: the kernel's bits (fp64 ``/`` and ``sqrt``, rounded once)."""
    n = s.numel()
    k = arc_count(n, f)
    if k == 0:
        return torch.ones(n, dtype=torch.float32, device=s.device)
    key = torch.where(torch.isfinite(s), s, torch.full_like(s, math.inf))
    ids = torch.arange(n, device=s.device)
    before = (key[None, :] > key[:, None]) | ((key[None, :] == key[:, None]) & (ids[None, :] < ids[:, None]))
    c2 = torch.where(before.sum(1) == k, key, torch.full_like(key, -math.inf)).max()
    clip = torch.isfinite(s) & torch.isfinite(c2) & (s > c2)
    one = torch.ones((), dtype=torch.float64, device=s.device)
    return torch.where(clip, (c2.double() / torch.where(clip, s.double(), one)).sqrt(), one).float()


def arc_gram(g: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """The clipped rows' Gram G'_ij = (c_i c_j) G_ij in g's dtype (the product in fp64, rounded once)."""
    cc = c.double()[:, None] * c.double()[None, :]
    return torch.where(cc == 1.0, g, (cc * g.double()).to(g.dtype))


def arc_fold(c: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
    """w_j = c_j a_j (fp64 product, as fp32): the weights over the clipped rows onto the original rows."""
    return (c.to(a.device).double() * a.double()).float()


def arc_distances(D: torch.Tensor, s: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """The clipped rows' squared distances (fp64, +inf diagonal) from the rows' distances ``D``, their squared
    norms ``s`` and the scales ``c``: G_ij = (s_i + s_j - D_ij) / 2, D'_ij = c_i² s_i + c_j² s_j - 2 c_i c_j G_ij.
    Squared distances lose the norms, so the host backend carries ``s`` beside ``D``; both are additive over
    coordinate shards. A pair of unclipped rows keeps its entry bit for bit."""
    D, s, c = D.double().cpu(), s.double().cpu(), c.double().cpu()
    G = 0.5 * (s[:, None] + s[None, :] - D)
    cc = c[:, None] * c[None, :]
    sc = c * c * s
    Dc = (sc[:, None] + sc[None, :] - 2.0 * cc * G)
    Dc = torch.where(torch.isfinite(Dc), Dc.clamp(min=0), torch.full_like(Dc, math.inf))
    Dc = torch.where((cc == 1.0) | ~torch.isfinite(D), D, Dc)
    Dc.fill_diagonal_(math.inf)
    return Dc


# --------------------------------------------------------------------------- #
# The table: per rule, the selection on each backend. ``s`` is the resolved Selection.
#   device(s, C, gram, ws, batch) -> w [batch * n] in the buffers of ``ws`` (Bulyan: W [batch * t * n])
#   host(s, C, D)                 -> w [n] fp32 on the CPU from fp64 squared distances (Bulyan: [t, n])
#   gram(s, g)                    -> w [n] fp32 on g's device (Bulyan: [t, n]); None: no such form


class _Rule(NamedTuple):
    device: Callable
    host: Callable
    gram: Callable | None
    device_rows: int = MAX_ROWS    # the most rows the device selection takes
    gram_on_cpu: bool = True       # whether ``gram`` also runs on a CPU Gram


def _buf(ws, batch: int, name: str, k: int, dtype=torch.float32) -> torch.Tensor:
    """``ws``'s buffer ``name`` of ``k`` elements per batch entry: [k], or [batch, k]."""
    t = ws.get(name, batch * k, dtype)
    return t if batch == 1 else t.view(batch, k)


def _const(ws, name: str, make) -> torch.Tensor:
    """A constant of ``ws``, made on first use (before any capture) and kept."""
    t = ws.tensors.get(name)
    if t is None:
        t = ws.tensors[name] = make()
    return t


def _one_hot_last(n: int, device) -> torch.Tensor:
    e = torch.zeros(n, dtype=torch.float32, device=device)
    e[-1] = 1.0
    return e


def _krum_device(s, C, g, ws, batch):
    w = _buf(ws, batch, "weights", s.n)
    C.gpu_krum_select(g, s.n, s.f, s.m, w, _buf(ws, batch, "order", s.n, torch.int32), _buf(ws, batch, "scores", s.n),
                      batch)
    return w


def _krum_host(s, C, D):
    return ref.krum_weights(D, s.f, s.m).float() if C is None else C.cpu_krum_weights(D, s.f, s.m)[0]


def _krum_gram(s, g):
    return large_select(g, s.f, s.m) if g.is_cuda else krum_weights_from_gram(g, s.f, s.m)


def _geomed_device(s, C, g, ws, batch):
    w = _buf(ws, batch, "weights", s.n)
    C.gpu_geomed_select(g, s.n, s.iters, s.nu, w, _buf(ws, batch, "dists", s.n), batch)
    return w


def _geomed_host(s, C, D):
    return ref.geomed_weights(D, s.iters, s.nu).float() if C is None else C.cpu_geomed_weights(D, s.iters, s.nu)


def _geomed_gram(s, g):
    return geomed_weights_from_gram(g, s.iters, s.nu)


def _dnc_device(s, C, g, ws, batch):
    w = _buf(ws, batch, "weights", s.n)
    C.gpu_dnc_select(g, s.n, s.m, s.iters, w, _buf(ws, batch, "scores", s.n), batch)
    return w


def _dnc_host(s, C, D):
    return (ref.dnc_weights if C is None else C.cpu_dnc_weights)(D, s.m, s.iters)[0]


def _dnc_gram(s, g):
    return dnc_weights_from_gram(g, s.m, s.iters)


def _caf_device(s, C, g, ws, batch):
    """The λ of every pass lands in the workspace's ``scores`` buffer."""
    w = _buf(ws, batch, "weights", s.n)
    C.gpu_caf_select(g, s.n, s.f, s.iters, s.max_passes, w, _buf(ws, batch, "scores", s.n), batch)
    return w


def _caf_host(s, C, D):
    if C is None:
        return ref.caf_weights(D, s.f, s.iters, s.max_passes or None)[0]
    return C.cpu_caf_weights(D, s.f, s.iters, s.max_passes)[0]


def _cclip_device(s, C, g, ws, batch):
    """For ``start="krum"`` k_krum_select writes the start into the weights buffer, then k_cclip_select
    iterates in place. Rows nw..n-1 are basis-only; ``tau <= 0``: from the data."""
    w = _buf(ws, batch, "weights", s.n)
    a0 = None
    if isinstance(s.start, torch.Tensor):
        a0 = ws.get("cclip_a0", s.n)
        a0.copy_(s.start.reshape(-1))
    elif s.start == "center":   # all the start weight on the appended centre row
        a0 = _const(ws, "cclip_center", lambda: _one_hot_last(s.n, g.device))
    elif s.start == "krum":
        a0 = _krum_device(s, C, g, ws, batch)
    C.gpu_cclip_select(g, s.n, s.nw, a0, s.tau, s.f, s.iters, w, _buf(ws, batch, "dists", s.n), batch)
    return w


def _cclip_host(s, C, D):
    a0 = None
    if isinstance(s.start, torch.Tensor):
        a0 = s.start.reshape(-1).double().cpu()
    elif s.start == "center":
        a0 = _one_hot_last(s.n, "cpu").double()
    elif s.start == "krum":   # the oracle's start stays in its own fp64
        a0 = ref.krum_weights(D, s.f, s.m) if C is None else _krum_host(s, C, D).double()
    if C is None:
        return ref.cclip_weights(D, s.nw, a0, s.tau if s.tau > 0 else None, s.f, s.iters).float()
    return C.cpu_cclip_weights(D, s.nw, a0, s.tau, s.f, s.iters)


def _cclip_gram(s, g):
    a0 = s.start if isinstance(s.start, torch.Tensor) else None
    if isinstance(s.start, str) and s.start == "center":
        a0 = _one_hot_last(s.n, g.device)
    elif isinstance(s.start, str) and s.start == "krum":
        a0 = _krum_gram(s, g)
    return cclip_weights_from_gram(g, s.nw, a0, s.tau if s.tau > 0 else None, s.f, s.iters)


def _brute_device(s, C, g, ws, batch):
    """The device-wide subset search has no batched launcher: one launch per segment."""
    w = _buf(ws, batch, "weights", s.n)
    best = ws.get("brute_best", 1, torch.int64)
    np2 = C.gram_padded(s.n) ** 2
    for i in range(batch):
        C.gpu_brute_select(g[i * np2:(i + 1) * np2], s.n, s.f, best, w.view(batch, s.n)[i])
    return w


def _brute_host(s, C, D):
    if C is None or s.n > 64:
        return ref.brute_weights(D, s.f).float()
    return C.cpu_brute_weights(D, s.f)


def _smea_device(s, C, g, ws, batch):
    """As Brute, the subset search has no batched launcher: one launch per segment. The winning λ lands in
    slot 0 of the workspace's ``scores`` buffer (per segment: slot 0 of its row)."""
    w = _buf(ws, batch, "weights", s.n)
    lam = _buf(ws, batch, "scores", s.n)
    best = ws.get("smea_best", 1, torch.int64)
    np2 = C.gram_padded(s.n) ** 2
    for i in range(batch):
        C.gpu_smea_select(g[i * np2:(i + 1) * np2], s.n, s.f, s.iters, best, w.view(batch, s.n)[i],
                          lam.view(batch, s.n)[i])
    return w


def _smea_host(s, C, D):
    if C is None or s.n > 64:
        return ref.smea_weights(D, s.f, s.iters)[0]
    return C.cpu_smea_weights(D, s.f, s.iters)[0]


def _bulyan_device(s, C, g, ws, batch):
    W = _buf(ws, batch, "bulyan_W", s.t * s.n)
    C.gpu_bulyan_select(g, s.n, s.f, s.m, s.t, W, batch)
    return W.view(s.t, s.n) if batch == 1 else W.view(batch, s.t, s.n)


def _bulyan_host(s, C, D):
    if s.n > MAX_ROWS:
        return large_bulyan_weights(D, s.f, s.m).float()
    if C is None:
        return ref.bulyan_weights(D, s.f, s.m).float()
    return C.cpu_bulyan_weights(D, s.f, s.m, s.t)


def _bulyan_gram(s, g):
    return large_select(g, s.f, s.m, bulyan=True)


TABLE = {
    "krum": _Rule(_krum_device, _krum_host, _krum_gram),
    "geomed": _Rule(_geomed_device, _geomed_host, _geomed_gram),
    "cclip": _Rule(_cclip_device, _cclip_host, _cclip_gram),
    "dnc": _Rule(_dnc_device, _dnc_host, _dnc_gram),
    # no vectorised Gram form: the pass count depends on the data, and that form may not sync with the host
    "caf": _Rule(_caf_device, _caf_host, None),
    "brute": _Rule(_brute_device, _brute_host, None, device_rows=64),
    # the mask is one word, as Brute's; no vectorised Gram form (C(n, f) blocks of k x k)
    "smea": _Rule(_smea_device, _smea_host, None, device_rows=64),
    "bulyan": _Rule(_bulyan_device, _bulyan_host, _bulyan_gram, gram_on_cpu=False),
}

# the average behind the mixing: the uniform weights as the sandwich's "selection"
_UNIFORM = _Rule(
    lambda s, C, g, ws, batch: _const(ws, "avg_w", lambda: torch.full((s.n,), 1.0 / s.n, dtype=torch.float32,
                                                                      device=g.device)),
    lambda s, C, D: torch.full((s.n,), 1.0 / s.n, dtype=torch.float32),
    lambda s, g: torch.full((s.n,), 1.0 / s.n, dtype=torch.float32, device=g.device))


# --------------------------------------------------------------------------- #
# The resolved selection


@dataclass(frozen=True, eq=False)
class Selection:
    """A rule with its arguments resolved for ``n`` rows (see :func:`resolve`). Arguments a rule does not
    take stay None."""

    rule: str
    n: int
    f: int
    m: int | None = None       # krum, bulyan: rows kept per round; dnc: rows kept; cclip: of its Krum start
    iters: int | None = None   # geomed, cclip, dnc; caf: power rounds per pass; smea: per subset
    max_passes: int = 0        # caf: the most passes, as the launchers take it, 0 = n
    nu: float | None = None    # geomed
    tau: float = 0.0           # cclip: the radius as the launchers take it, 0 = from the data
    start: object = "mean"     # cclip: "mean", "krum", "center" (the appended row nw) or an [n] weight tensor
    nw: int | None = None      # cclip: rows 0..nw-1 are workers, the rest basis-only
    pre: str | None = None     # "nnm": the rule runs on the rows mixed over their n - f nearest; "arc": on the rows
                               # clipped to the (k + 1)-th largest norm; "arc+nnm": clipped, then mixed

    @property
    def t(self) -> int:
        """Bulyan's selection rounds."""
        return self.n - 2 * self.f - 2

    @property
    def _entry(self) -> _Rule:
        return TABLE.get(self.rule, _UNIFORM)

    @property
    def device_rows(self) -> int:
        """The most rows :meth:`on_device` takes."""
        return self._entry.device_rows

    def has_gram_form(self, cuda: bool) -> bool:
        """Whether :meth:`from_gram` exists for a Gram on that kind of device."""
        e = self._entry
        return e.gram is not None and (cuda or e.gram_on_cpu)

    @property
    def mixes(self) -> bool:
        """Whether nearest-neighbour mixing runs in front of the rule."""
        return self.pre in ("nnm", "arc+nnm")

    @property
    def clips(self) -> int:
        """The rows adaptive robust clipping may clip in front of everything else (0: no clipping, and no
        trace of it: with f = 0 every path is the path without ARC, bit for bit)."""
        return arc_count(self.n, self.f) if self.pre in ("arc", "arc+nnm") else 0

    def on_device(self, C, gram: torch.Tensor, ws, batch: int = 1) -> torch.Tensor:
        """Weights [n] ([batch, n]; Bulyan: W [t, n] / [batch, t, n]) from ``batch`` device Grams (pitch
        gram_padded(n), n <= device_rows) by the ``gpu_*_select`` launches. Every buffer comes from ``ws``
        (a ``gar.Workspace``, allocated on the first call: capture-safe after it). The sandwich around the
        rule: k_arc_scale (``pre`` "arc" / "arc+nnm") -> k_nnm_mix ("nnm" / "arc+nnm") -> the rule's selection
        on the Gram it is handed -> k_nnm_unmix -> k_arc_fold."""
        n, f = self.n, self.f
        np_ = C.gram_padded(n)
        scales = None
        if self.clips:
            scales = _buf(ws, batch, "arc_scales", n)
            G2 = _buf(ws, batch, "arc_gram", np_ * np_)
            C.gpu_arc_scale(gram, n, f, scales, _buf(ws, batch, "arc_clip_rows", n + 1, torch.int32), G2, batch)
            gram = G2
        if self.mixes:
            H = _buf(ws, batch, "nnm_H", np_ * np_)
            masks = _buf(ws, batch, "nnm_masks", 2 * n, torch.int64)
            C.gpu_nnm_mix(gram, n, f, H, masks, batch)
            a = self._entry.device(self, C, H, ws, batch)
            w = _buf(ws, batch, "nnm_w", n)
            C.gpu_nnm_unmix(a, masks, n, f, w, batch)
        else:
            w = self._entry.device(self, C, gram, ws, batch)
        if scales is not None:
            a, w = w, _buf(ws, batch, "arc_w", n)
            C.gpu_arc_fold(a, scales, n, w, batch)
        return w

    def on_host(self, C, D: torch.Tensor, sqnorms: torch.Tensor | None = None) -> torch.Tensor:
        """Weights [n] (fp32, CPU; Bulyan: W [t, n]) from fp64 squared distances: the C++ functions of the
        extension ``C``, else (``C`` None, or more rows than they take) the oracle. ARC needs the rows'
        squared norms ``sqnorms`` [n] beside ``D`` (distances lose them)."""
        n, f = self.n, self.f
        c = None
        if self.clips:
            if sqnorms is None:
                raise ValueError("arc: the host selection needs the rows' squared norms beside their distances")
            c = arc_scales_from_sqnorms(sqnorms.detach().cpu(), f)
            D = arc_distances(D, sqnorms, c)
        if not self.mixes:
            w = self._entry.host(self, C, D)
        elif C is None or n > MAX_ROWS:   # the C++ sets are two mask words
            w = ref.nnm_weights(D, f, self.rule, m=self.m, iters=self.iters, nu=self.nu,
                                tau=self.tau if self.tau > 0 else None, start=self.start)
        else:
            Dm, masks = C.cpu_nnm_mix(D, f)
            w = C.cpu_nnm_unmix(self._entry.host(self, C, Dm), masks, n - f)
        return w if c is None else arc_fold(c, w)

    def from_gram(self, g: torch.Tensor) -> torch.Tensor:
        """Weights [n] (fp32; Bulyan: W [t, n]) vectorised on the device of the Gram ``g`` (any n, no host
        round trip; Krum and Bulyan on the GPU: gar_large.hip)."""
        c = None
        if self.clips:
            c = arc_scales_from_sqnorms(torch.diagonal(g), self.f)
            g = arc_gram(g, c)
        if self.mixes:
            H, S = nnm_from_gram(g, self.f)
            w = nnm_fold(S, self._entry.gram(self, H), self.n - self.f)
        else:
            w = self._entry.gram(self, g)
        return w if c is None else arc_fold(c, w)


def resolve(rule: str, n: int, f: int, m: int | None = None, pre: str | None = None,
            gar_kwargs: dict | None = None) -> Selection:
    """The :class:`Selection` of ``rule`` over ``n`` rows: defaults applied, arguments validated (ValueError).
    ``gar_kwargs``: the rule's own keyword arguments (``iters``, ``nu``, ``tau``, ``start``, ``max_passes``); others are ignored."""
    kw = gar_kwargs or {}
    start = kw.get("start")
    start = "mean" if start is None else start
    if pre is not None:
        tag = PRE_TAGS.get(pre, "nnm")
        if rule == "cclip" and not isinstance(start, str):
            raise ValueError(f"{tag}-cclip: start must be one of {CCLIP_STARTS}")
        if pre not in PRE_RULES:
            raise ValueError(f"unknown pre-aggregation {pre!r}; available: {tuple(PRE_RULES)}")
        if rule not in PRE_RULES[pre]:
            raise ValueError(f"{tag}: unsupported rule {rule!r}; available: {PRE_RULES[pre]}")
        if not 0 <= f < n:
            raise ValueError(f"{tag}: expected 0 <= f < n, got f = {f}, n = {n}")
    elif rule not in TABLE:
        raise ValueError(f"unknown distance-based rule {rule!r}; available: {tuple(TABLE)}")
    if rule in ("krum", "bulyan"):
        m = n - f - 2 if m is None else m
        if pre is not None and (n < 2 * f + 3 or not 1 <= m <= n - f - 2):   # Krum's own requirement, as on every other path
            raise ValueError(f"{PRE_TAGS[pre]}-krum: expected n >= 2f + 3 and 1 <= m <= n - f - 2, got n = {n}, f = {f}, "
                             f"m = {m}")
        return Selection(rule, n, f, m=m, pre=pre)
    if rule == "geomed":
        return Selection(rule, n, f, iters=int(kw.get("iters", 32)), nu=float(kw.get("nu", 1e-6)), pre=pre)
    if rule == "dnc":
        iters = kw.get("iters", 16)
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise ValueError(f"dnc: expected an int iters >= 1, got {iters!r}")
        if f < 0 or n < 2 * f + 1:
            raise ValueError(f"dnc: expected 0 <= f and n >= 2f + 1, got n = {n}, f = {f}")
        m = n - f if m is None else m
        if not 1 <= m <= n:
            raise ValueError(f"dnc: expected 1 <= m <= n, got m = {m}, n = {n}")
        return Selection(rule, n, f, m=int(m), iters=iters, pre=pre)
    if rule == "caf":
        iters, max_passes = kw.get("iters", 16), kw.get("max_passes")
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise ValueError(f"caf: expected an int iters >= 1, got {iters!r}")
        if max_passes is not None and (isinstance(max_passes, bool) or not isinstance(max_passes, int) or max_passes < 1):
            raise ValueError(f"caf: expected max_passes None (n) or an int >= 1, got {max_passes!r}")
        if isinstance(f, bool) or not isinstance(f, int) or f < 0 or n < 2 * f + 1:
            raise ValueError(f"caf: expected 0 <= f and n >= 2f + 1, got n = {n}, f = {f!r}")
        return Selection(rule, n, f, iters=iters, max_passes=0 if max_passes is None else min(max_passes, n), pre=pre)
    if rule == "cclip":
        iters, tau = kw.get("iters", 3), kw.get("tau")
        if iters is None or int(iters) < 1:
            raise ValueError(f"cclip: expected iters >= 1, got {iters}")
        if tau is not None and not float(tau) > 0.0:
            raise ValueError(f"cclip: expected tau None (from the data) or > 0, got {tau}")
        if f < 0:
            raise ValueError(f"cclip: expected f >= 0, got {f}")
        if isinstance(start, str):
            if start not in CCLIP_STARTS:
                raise ValueError(f"cclip: unknown start {start!r}; available: {CCLIP_STARTS} or an [n] weight tensor")
            if start == "krum":
                m = n - f - 2 if m is None else m
                if n < 2 * f + 3 or not 1 <= m <= n - f - 2:   # Krum's own requirement, as on every other path
                    raise ValueError(f"cclip: start='krum' expects n >= 2f + 3 and 1 <= m <= n - f - 2, got n = {n}, "
                                     f"f = {f}, m = {m}")
        elif not isinstance(start, torch.Tensor) or start.numel() != n:
            raise ValueError(f"cclip: start must be one of {CCLIP_STARTS} or an [n] weight tensor (n = {n})")
        return Selection(rule, n, f, m=m, iters=int(iters), tau=0.0 if tau is None else float(tau), start=start,
                         nw=n, pre=pre)
    if rule == "smea":
        iters = kw.get("iters", 16)
        if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
            raise ValueError(f"smea: expected an int iters >= 1, got {iters!r}")
        if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < n:
            raise ValueError(f"smea: expected 0 <= f < n, got n = {n}, f = {f!r}")
        subsets = math.comb(n, n - f)
        if subsets > SMEA_MAX_SUBSETS:
            raise ValueError(f"smea: C({n}, {n - f}) = {subsets} subsets exceeds {SMEA_MAX_SUBSETS} (2^"
                             f"{SMEA_MAX_SUBSETS.bit_length() - 1}); use a smaller f or a spectral filter (caf, dnc)")
        return Selection(rule, n, f, iters=iters, pre=pre)
    if rule == "brute":
        # the device search keys each subset by its 32-bit rank (gar_gram.hip k_brute_*): refuse
        # what it cannot index (C(64, 56) is 4.4e9 subsets: infeasible on any device anyway)
        subsets = math.comb(n, n - f) if 0 <= f <= n else 0
        if subsets > BRUTE_MAX_SUBSETS:
            raise ValueError(f"brute: C({n}, {n - f}) = {subsets} subsets exceeds 2^32; use a smaller f "
                             "or another rule")
    return Selection(rule, n, f, pre=pre)   # brute; the average behind the mixing
