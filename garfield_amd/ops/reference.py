"""Plain-PyTorch fp64 reference ("oracle") implementations of every GAR.

These are the specification the native CPU and HIP kernels are tested against
(SURVEY.md §4 "GAR oracle tests"), written for clarity, not speed. They follow
the native-reference semantics documented in ``docs/GAR_SEMANTICS.md``:

* distances are SQUARED L2 (``py_krum/krum.cu:92-94``), non-finite -> +inf;
* Krum score = sum of the ``n - f - 2`` nearest (``py_krum/krum.cpp:86-97``);
* every ranking is by ``(value with NaN as +inf, index)``;
* median = upper median of the finite values, 0 if none (``py_median/median.cpp:42-77``);
* Bulyan follows ``py_bulyan/bulyan.cpp:53-193`` (pruned-score selection loop,
  then averaged-median with beta = t - 2f);
* Brute enumerates (n-f)-subsets as bit masks in increasing numeric order.

All functions take ``G`` as an ``[n, d]`` tensor (any dtype / device) and return
a 1-D fp64 CPU tensor unless stated otherwise.
"""
from __future__ import annotations

import math
from itertools import combinations

import torch

FLT_MAX = 3.4028234663852886e38
_MASK64 = (1 << 64) - 1


def _g(G) -> torch.Tensor:
    if isinstance(G, (list, tuple)):
        G = torch.stack([g.reshape(-1) for g in G])
    return G.detach().to(device="cpu", dtype=torch.float64)


def _key(v: float) -> float:
    return math.inf if v != v else v


def _order(values, ids=None):
    ids = list(range(len(values))) if ids is None else list(ids)
    return sorted(ids, key=lambda i: (_key(float(values[i])), i))


def pairwise_sqdist(G) -> torch.Tensor:
    X = _g(G)
    n = X.shape[0]
    D = torch.full((n, n), math.inf, dtype=torch.float64)
    for i in range(n):
        for j in range(i + 1, n):
            v = float(((X[i] - X[j]) ** 2).sum())
            if not math.isfinite(v):
                v = math.inf
            D[i, j] = D[j, i] = v
    return D


def krum_scores(D: torch.Tensor, f: int) -> list[float]:
    n = D.shape[0]
    q = n - f - 2
    scores = []
    for i in range(n):
        near = _order(D[i].tolist(), [j for j in range(n) if j != i])[:q]
        scores.append(sum(float(D[i, j]) for j in near))
    return scores


def krum_weights(D: torch.Tensor, f: int, m: int | None = None) -> torch.Tensor:
    n = D.shape[0]
    m = n - f - 2 if m is None else m
    order = _order(krum_scores(D, f))
    w = torch.zeros(n, dtype=torch.float64)
    for i in order[:m]:
        w[i] = 1.0 / m
    return w


def combine(G, w: torch.Tensor) -> torch.Tensor:
    X = _g(G)
    out = torch.zeros(X.shape[1], dtype=torch.float64)
    for j in range(X.shape[0]):
        if float(w[j]) != 0.0:
            out += float(w[j]) * X[j]
    return out


def average(G) -> torch.Tensor:
    return _g(G).mean(dim=0)


def krum(G, f: int, m: int | None = None) -> torch.Tensor:
    return combine(G, krum_weights(pairwise_sqdist(G), f, m))


def geomed_weights(D: torch.Tensor, iters: int = 32, nu: float = 1e-6) -> torch.Tensor:
    """Weights [n] (fp64) of the smoothed-Weiszfeld geometric median, iterated on the squared
    distances alone (docs/GAR_SEMANTICS.md "Geometric median"): the iterate z = Σ a_j x_j has
    ||x_i - z||² = Σ_j a_j D_ij - ½ Σ_jk a_j a_k D_jk. Exactly ``iters`` rounds, sums in index order."""
    D = D.detach().to(device="cpu", dtype=torch.float64)
    n = D.shape[0]
    fin = [[i != j and math.isfinite(float(D[i, j])) for j in range(n)] for i in range(n)]
    V = [i for i in range(n) if any(fin[i])]
    if not V:
        return torch.full((n,), 1.0 / n, dtype=torch.float64)
    dist = [[float(D[i, j]) if fin[i][j] else 0.0 for j in range(n)] for i in range(n)]
    a = [0.0] * n
    for i in V:
        a[i] = 1.0 / len(V)
    for _ in range(iters):
        s = {}
        for i in V:
            acc = 0.0
            for j in V:
                acc += a[j] * dist[i][j]
            s[i] = acc
        q = 0.0
        for i in V:
            q += a[i] * s[i]
        q *= 0.5
        b, tot = {}, 0.0
        for i in V:
            b[i] = 1.0 / max(math.sqrt(max(s[i] - q, 0.0)), nu)
            tot += b[i]
        for i in V:
            a[i] = b[i] / tot
    return torch.tensor(a, dtype=torch.float64)


def geomed(G, iters: int = 32, nu: float = 1e-6) -> torch.Tensor:
    return combine(G, geomed_weights(pairwise_sqdist(G), iters, nu))


def cclip_weights(D: torch.Tensor, nw: int | None = None, a0=None, tau: float | None = None, f: int = 0,
                  iters: int = 3) -> torch.Tensor:
    """Weights [n] (fp64) of centered clipping, iterated on the squared distances alone
    (docs/GAR_SEMANTICS.md "Centered clipping"): the centre v = Σ a_j x_j has
    ||x_i - v||² = Σ_j a_j D_ij - ½ Σ_jk a_j a_k D_jk, and one round is
    a_j <- a_j (1 - Λ/|V|) + λ_j/|V| with λ_i = min(1, τ / r_i) on the valid workers. Rows nw..n-1 are
    basis-only. ``a0``: the start weights (None: uniform on the workers); ``tau``: the radius (None: the
    max(|V| - f, 1)-th smallest r of the round). Exactly ``iters`` rounds, sums in index order."""
    D = D.detach().to(device="cpu", dtype=torch.float64)
    n = D.shape[0]
    nw = n if nw is None else nw
    fin = [[i != j and math.isfinite(float(D[i, j])) for j in range(n)] for i in range(n)]
    valid = [i for i in range(n) if any(fin[i])]
    V = [i for i in valid if i < nw]
    if not V:
        return torch.tensor([1.0 / nw if i < nw else 0.0 for i in range(n)], dtype=torch.float64)
    dist = [[float(D[i, j]) if fin[i][j] else 0.0 for j in range(n)] for i in range(n)]
    a = [0.0] * n
    tot = 0.0
    if a0 is not None:
        for i in valid:
            a[i] = float(a0[i])
            tot += a[i]
    if a0 is not None and math.isfinite(tot) and tot > 0.0:
        a = [x / tot for x in a]
    else:
        a = [1.0 / len(V) if i in V else 0.0 for i in range(n)]
    k = max(len(V) - f, 1)
    for _ in range(iters):
        s = [0.0] * n
        for i in valid:
            acc = 0.0
            for j in valid:
                acc += a[j] * dist[i][j]
            s[i] = acc
        q = 0.0
        for i in valid:
            q += a[i] * s[i]
        q *= 0.5
        r = {i: math.sqrt(max(s[i] - q, 0.0)) for i in V}
        t = sorted(r.values())[k - 1] if tau is None else float(tau)
        lam, Lam = [0.0] * n, 0.0
        for i in V:
            lam[i] = 1.0 if r[i] <= t else t / r[i]
            Lam += lam[i]
        keep = 1.0 - Lam / len(V)
        a = [a[i] * keep + lam[i] / len(V) for i in range(n)]
    return torch.tensor(a, dtype=torch.float64)


def cclip(G, f: int = 0, tau: float | None = None, iters: int = 3, start="mean", center=None,
          m: int | None = None) -> torch.Tensor:
    """Centered clipping of the rows G: ``start`` "mean", "krum" (the Multi-Krum weights, f and m) or an
    [n] weight vector; ``center``: a d-vector appended as a basis-only row that carries the start."""
    X = _g(G)
    n = X.shape[0]
    if center is not None:
        X = torch.cat([X, center.detach().reshape(1, -1).to(device="cpu", dtype=torch.float64)])
    D = pairwise_sqdist(X)
    if center is not None:
        a0 = [0.0] * n + [1.0]
    elif isinstance(start, str):
        a0 = {"mean": lambda: None, "krum": lambda: krum_weights(D, f, m)}[start]()
    else:
        a0 = start
    return combine(X, cclip_weights(D, n, a0, tau, f, iters))


def _dnc_power(dist, V, iters: int) -> tuple:
    """(λ, b): exactly ``iters`` power rounds on K = -½ J D J over the rows ``V`` (indices into the usable
    distances ``dist``, a list of rows with zeros where unusable), from the column of K at the row farthest from
    the mean, sums in index order; λ = u·b after the last round, b = K u on ``V`` (0 elsewhere). The loop of
    :func:`dnc_scores`, shared with :func:`smea_lambda`."""
    n = len(dist)
    nv = len(V)
    r = [0.0] * n
    for i in V:
        acc = 0.0
        for j in V:
            acc += dist[i][j]
        r[i] = acc / nv
    g = 0.0
    for i in V:
        g += r[i]
    g /= nv
    star = V[0]   # the lowest index in V that attains max κ, κ_i = r_i - g/2
    for i in V:
        if r[i] - 0.5 * g > r[star] - 0.5 * g:
            star = i
    b = [0.0] * n
    for i in V:
        b[i] = -0.5 * (dist[i][star] - r[i] - r[star] + g)
    u = [0.0] * n
    for _ in range(iters):
        nu = 0.0
        for i in V:
            nu += b[i] * b[i]
        nu = math.sqrt(nu)
        c = 0.0
        for i in V:
            u[i] = b[i] / nu if nu > 0.0 else 0.0
            c += u[i]
        c /= nv
        t = [0.0] * n
        tm = 0.0
        for i in V:
            acc = 0.0
            for j in V:
                acc += dist[i][j] * (u[j] - c)
            t[i] = acc
            tm += acc
        tm /= nv
        for i in V:
            b[i] = -0.5 * (t[i] - tm)
    lam = 0.0
    for i in V:
        lam += u[i] * b[i]
    return lam, b


def dnc_scores(D: torch.Tensor, iters: int = 16) -> torch.Tensor:
    """Outlier scores [n] (fp64, before the cast to fp32) of the DnC spectral filter on the squared distances
    alone (docs/GAR_SEMANTICS.md "Spectral filtering"). With the rows centred at their mean, C Cᵀ = K = -½ J D J,
    and the score of row i, its squared projection on the top right singular vector of C, is λ u_i² for the
    top eigenpair (λ, u) of K. Exactly ``iters`` power rounds from the column of K at the row farthest from
    the mean, sums in index order. +inf on rows without a finite off-diagonal distance; 0 if there is none."""
    D = D.detach().to(device="cpu", dtype=torch.float64)
    n = D.shape[0]
    fin = [[i != j and math.isfinite(float(D[i, j])) for j in range(n)] for i in range(n)]
    V = [i for i in range(n) if any(fin[i])]
    if not V:
        return torch.zeros(n, dtype=torch.float64)
    dist = [[float(D[i, j]) if fin[i][j] else 0.0 for j in range(n)] for i in range(n)]
    lam, b = _dnc_power(dist, V, iters)
    s = torch.full((n,), math.inf, dtype=torch.float64)
    for i in V:
        s[i] = b[i] * b[i] / lam if lam > 0.0 else 0.0
    return s


def dnc_weights(D: torch.Tensor, m: int, iters: int = 16) -> tuple:
    """(w [n], s [n]), both fp32: the scores of :func:`dnc_scores` cast to fp32, and weight 1 / kv on the
    kv = min(m, |V|) valid rows lowest by (fp32 score, index), 0 elsewhere; no valid row: uniform 1/n."""
    n = D.shape[0]
    s = dnc_scores(D, iters).float()
    Df = D.detach().to(device="cpu", dtype=torch.float64)
    V = [i for i in range(n) if any(j != i and math.isfinite(float(Df[i, j])) for j in range(n))]
    if not V:
        return torch.full((n,), 1.0 / n, dtype=torch.float64).float(), s
    kv = min(m, len(V))
    w = torch.zeros(n, dtype=torch.float64)
    for i in _order(s.tolist(), V)[:kv]:
        w[i] = 1.0 / kv
    return w.float(), s


def dnc_svd_scores(G) -> torch.Tensor:
    """The paper's outlier scores [n] (fp64) on the vectors themselves: the squared projection of every
    centred row on the top right singular vector of the centred matrix (all coordinates, finite rows)."""
    X = _g(G)
    C = X - X.mean(dim=0, keepdim=True)
    v = torch.linalg.svd(C, full_matrices=False).Vh[0]
    return (C @ v) ** 2


def dnc(G, f: int, m: int | None = None, iters: int = 16) -> torch.Tensor:
    X = _g(G)
    m = X.shape[0] - f if m is None else m
    return combine(X, dnc_weights(pairwise_sqdist(X), m, iters)[0].double())


# CAF, the covariance filter (docs/GAR_SEMANTICS.md "Covariance filter"): the rows are down-weighted along
# the top principal direction of their weighted covariance, pass after pass, and the weighted mean whose
# covariance had the smallest top eigenvalue is kept. With μ_a = Σ a_i x_i and K_ij = (x_i - μ_a)·(x_j - μ_a),
# the n x n matrix M = A^½ K A^½ has the non-zero eigenvalues of the d x d covariance Σ_i a_i (x_i - μ_a)(x_i - μ_a)ᵀ,
# and K comes from the squared distances alone: everything below works on D.


def _caf_distances(D: torch.Tensor) -> tuple:
    """(usable distances [n, n] fp64 with zeros on the diagonal, on invalid rows and where infinite; valid [n])."""
    D = D.detach().to(device="cpu", dtype=torch.float64)
    fin = torch.isfinite(D)
    fin.fill_diagonal_(False)
    return torch.where(fin, D, torch.zeros_like(D)), fin.any(1)


def caf_pass(D: torch.Tensor, valid: torch.Tensor, a: torch.Tensor, iters: int = 16) -> tuple:
    """One pass of the covariance filter on the usable distances ``D`` with the weights ``a`` (fp64, Σ a = 1,
    zero on invalid rows): ``(λ, τ [n])``, the top eigenvalue of the weighted covariance after exactly ``iters``
    power rounds on M = A^½ K A^½ from its column at the row of largest a_i ‖x_i - μ_a‖², and the squared
    projections of the centred rows on the top eigenvector (0 on invalid rows, and everywhere if λ <= 0)."""
    n = D.shape[0]
    ra = a.sqrt()
    s = D @ a
    q = float(a @ s)
    zero = torch.zeros(n, dtype=torch.float64)

    def K(p):
        sp = float(p.sum())
        return torch.where(valid, -0.5 * (D @ p - s * sp - float(s @ p) + q * sp), zero)

    v = (a * (s - 0.5 * q)).tolist()
    star = 0   # the lowest index that attains the maximum
    for i in range(n):
        if v[i] > v[star]:
            star = i
    p = zero.clone()
    p[star] = ra[star]
    b = ra * K(p)
    u, kp = zero, zero
    for _ in range(iters):
        nb = math.sqrt(float(b @ b))
        u = b / nb if nb > 0.0 else zero
        kp = K(ra * u)
        b = ra * kp
    lam = float(u @ b)
    return lam, (kp * kp / lam if lam > 0.0 else zero)


def caf_trace(D: torch.Tensor, f: int, iters: int = 16, max_passes: int | None = None) -> dict:
    """The covariance filter with its decisions laid open (all fp64): ``weights`` [n] (the a of the pass of
    smallest λ), ``lams`` (λ per pass), ``sums`` (Σc at every loop test), ``taus`` (per pass, τ on the rows that
    still carry weight, descending) and ``best`` (the pass kept; None when no pass ran)."""
    n = D.shape[0]
    D, valid = _caf_distances(D)
    out = {"lams": [], "sums": [], "taus": [], "best": None}
    if not bool(valid.any()):
        out["weights"] = torch.full((n,), 1.0 / n, dtype=torch.float64)
        return out
    c = valid.double()
    best, best_a = math.inf, c / float(c.sum())
    limit = n if max_passes is None else max_passes
    while True:
        sc = float(c.sum())
        out["sums"].append(sc)
        if not (sc > n - 2 * f and len(out["lams"]) < limit):
            break
        a = c / sc
        lam, tau = caf_pass(D, valid, a, iters)
        if lam < best:   # strict: the first pass wins a tie
            best, best_a, out["best"] = lam, a, len(out["lams"])
        out["lams"].append(lam)
        live = c > 0
        out["taus"].append(sorted(tau[live].tolist(), reverse=True))
        tmax = float(tau[live].max())
        if not (lam > 0.0 and tmax > 0.0):
            break
        c = torch.where(live, c * (1.0 - (tau / tmax).clamp(max=1.0)), c)
    out["weights"] = best_a
    return out


def caf_weights(D: torch.Tensor, f: int, iters: int = 16, max_passes: int | None = None) -> tuple:
    """(w [n], lams [n]), both fp32: the weights of the covariance filter on the squared distances ``D`` and
    the λ of pass p at index p, +inf beyond the last pass. No valid row: uniform 1/n."""
    n = D.shape[0]
    t = caf_trace(D, f, iters, max_passes)
    lams = torch.full((n,), math.inf, dtype=torch.float64)
    lams[:len(t["lams"])] = torch.tensor(t["lams"], dtype=torch.float64)
    return t["weights"].float(), lams.float()


def caf_dense_pass(X, a) -> tuple:
    """The check on the vectors themselves: (λ, τ [n]) from the d x d weighted covariance
    Σ_i a_i (x_i - μ_a)(x_i - μ_a)ᵀ, its top eigenvalue and the squared projections of the centred rows on
    its top eigenvector (``torch.linalg.eigh``)."""
    X = _g(X)
    a = torch.as_tensor(a, dtype=torch.float64)
    C = X - (a[:, None] * X).sum(0, keepdim=True)
    ev, vec = torch.linalg.eigh(C.T @ (a[:, None] * C))
    return float(ev[-1]), (C @ vec[:, -1]) ** 2


def caf(G, f: int, iters: int = 16, max_passes: int | None = None) -> torch.Tensor:
    X = _g(G)
    return combine(X, caf_weights(pairwise_sqdist(X), f, iters, max_passes)[0].double())


# Nearest-neighbour mixing (docs/GAR_SEMANTICS.md "Nearest-neighbour mixing"): every gradient is
# replaced by the mean of its c = n - f nearest gradients, itself included, before a rule runs.
# Mixing is linear, so everything below works on the squared distances alone.


def nnm_sets(D: torch.Tensor, f: int) -> list[list[int]]:
    """S_i (ascending indices): the first c = n - f indices j by the key (j != i, D_ij, j)."""
    n = D.shape[0]
    if not 0 <= f < n:
        raise ValueError(f"nnm: expected 0 <= f < n, got f = {f}, n = {n}")
    c = n - f
    sets = []
    for i in range(n):
        row = D[i].tolist()
        order = sorted(range(n), key=lambda j: (j != i, _key(float(row[j])) if j != i else 0.0, j))
        sets.append(sorted(order[:c]))
    return sets


def nnm_distances(D: torch.Tensor, f: int):
    """(sets, D'): the neighbour sets and the squared distances [n, n] (fp64, +inf diagonal) of the
    mixed rows y_i = (1/c) Σ_{j∈S_i} x_j, from D alone: with D⁰ = D with a zero diagonal and
    M_ij = (1/c²) Σ_{k∈S_i} Σ_{l∈S_j} D⁰_kl, ||y_i - y_j||² = M_ij - ½M_ii - ½M_jj (clamped at 0).
    +inf when i or j is tainted (two members of its set at distance +inf) or a cross pair is +inf.
    Sums run over the set members in ascending index, the inner sum (over l) first."""
    D = D.detach().to(device="cpu", dtype=torch.float64)
    n = D.shape[0]
    sets = nnm_sets(D, f)
    c = n - f
    d0 = [[0.0 if k == l else _key(float(v)) for l, v in enumerate(row)] for k, row in enumerate(D.tolist())]
    # R[j][k] = Σ_{l∈S_j} D⁰_kl ; distances are >= 0 or +inf, so a sum is +inf iff a term is
    R = []
    for j in range(n):
        col = []
        for k in range(n):
            acc, row = 0.0, d0[k]
            for l in sets[j]:
                acc += row[l]
            col.append(acc)
        R.append(col)

    def m_of(i, j):
        acc, col = 0.0, R[j]
        for k in sets[i]:
            acc += col[k]
        return acc / (c * c)

    diag = [m_of(i, i) for i in range(n)]
    out = torch.full((n, n), math.inf, dtype=torch.float64)
    for i in range(n):
        for j in range(i + 1, n):
            mij = m_of(i, j)
            if math.isinf(mij) or math.isinf(diag[i]) or math.isinf(diag[j]):
                v = math.inf
            else:
                v = max(mij - 0.5 * diag[i] - 0.5 * diag[j], 0.0)
            out[i, j] = out[j, i] = v
    return sets, out


def nnm_row_weights(sets, a) -> torch.Tensor:
    """Fold weights a over the mixed rows back into weights over the original rows (fp32):
    w_j = (1/c) Σ_{i : j∈S_i} a_i / Σ_i a_i, i ascending in fp64, terms with a_i == 0 skipped. The
    division by Σ_i a_i (1 up to the rounding of a) makes equal sets give exactly 1/n."""
    n = len(sets)
    c = len(sets[0])
    acc, tot = [0.0] * n, 0.0
    for i in range(n):
        ai = float(a[i])
        if ai == 0.0:
            continue
        tot += ai
        for j in sets[i]:
            acc[j] += ai
    if tot == 0.0:
        return torch.zeros(n, dtype=torch.float32)
    return torch.tensor([v / tot / c for v in acc], dtype=torch.float64).float()


def nnm_weights(D: torch.Tensor, f: int, rule: str = "krum", **kw) -> torch.Tensor:
    """Row weights [n] (fp32) of ``rule`` (krum / geomed / average) applied after the mixing."""
    sets, Dm = nnm_distances(D, f)
    n = D.shape[0]
    if rule == "krum":
        a = krum_weights(Dm, f, kw.get("m"))
    elif rule == "geomed":
        a = geomed_weights(Dm, kw.get("iters", 32), kw.get("nu", 1e-6))
    elif rule == "cclip":   # start "mean" or "krum", on the mixed rows
        a0 = krum_weights(Dm, f, kw.get("m")) if kw.get("start", "mean") == "krum" else None
        a = cclip_weights(Dm, n, a0, kw.get("tau"), f, kw.get("iters", 3))
    elif rule == "average":
        a = torch.full((n,), 1.0 / n, dtype=torch.float64)
    else:
        raise ValueError(f"nnm: unsupported rule {rule!r} (krum, geomed, cclip, average)")
    return nnm_row_weights(sets, a)


def nnm(G, f: int, rule: str = "krum", **kw) -> torch.Tensor:
    return combine(G, nnm_weights(pairwise_sqdist(G), f, rule, **kw).double())


def nnm_mixed_rows(X, sets) -> torch.Tensor:
    """The mixed rows [n, d] (fp64): y_i[x] = (1/c) Σ_{j∈S_i} x_j[x], plain IEEE sums over the members in
    ascending index. A non-finite member makes exactly the mixed values of the sets that hold it
    non-finite."""
    X = _g(X)
    out = torch.empty((len(sets), X.shape[1]), dtype=torch.float64)
    for i, s in enumerate(sets):
        acc = torch.zeros(X.shape[1], dtype=torch.float64)
        for j in s:   # one fp64 addition per member and coordinate, members ascending
            acc = acc + X[j]
        out[i] = acc / len(s)
    return out


def nnm_coord(G, f: int, rule: str = "trimmed-mean") -> torch.Tensor:
    """A coordinate-wise rule (trimmed-mean with the same f, or median) over the rows mixed over their
    n - f nearest: pairwise_sqdist -> nnm_sets -> nnm_mixed_rows -> the plain rule."""
    X = _g(G)
    n = X.shape[0]
    if rule not in ("trimmed-mean", "median"):
        raise ValueError(f"nnm: unsupported coordinate-wise rule {rule!r} (trimmed-mean, median)")
    if rule == "trimmed-mean" and n < 2 * f + 1:
        raise ValueError(f"nnm-trimmed-mean: expected n >= 2f + 1, got n = {n}, f = {f}")
    Y = nnm_mixed_rows(X, nnm_sets(pairwise_sqdist(X), f))
    return trimmed_mean(Y, f) if rule == "trimmed-mean" else median(Y)


def arc_count(n: int, f: int) -> int:
    """Rows adaptive robust clipping may clip: k = (2 f (n - f)) // n (< n; 0 exactly when f = 0)."""
    if not 0 <= f < n:
        raise ValueError(f"arc: expected 0 <= f < n, got f = {f}, n = {n}")
    return (2 * f * (n - f)) // n


def arc_scales(sqnorms, f: int) -> torch.Tensor:
    """The ARC scales [n] (fp32) from the squared norms s (docs/GAR_SEMANTICS.md "Adaptive robust clipping"):
    C² = s of the row at position k of the order (s descending with a non-finite s as +inf, index
    ascending); c_i = sqrt(C² / s_i) in fp64, rounded once to fp32, where s_i and C² are finite and
    s_i > C²; 1 elsewhere."""
    s = [float(v) for v in torch.as_tensor(sqnorms).detach().double().cpu().reshape(-1)]
    n = len(s)
    k = arc_count(n, f)
    key = [v if math.isfinite(v) else math.inf for v in s]
    c2 = key[sorted(range(n), key=lambda i: (-key[i], i))[k]]
    c = [math.sqrt(c2 / s[i]) if math.isfinite(s[i]) and math.isfinite(c2) and s[i] > c2 else 1.0 for i in range(n)]
    return torch.tensor(c, dtype=torch.float64).float()


def arc_clip_rows(scales) -> list[int]:
    """The rows ARC writes: those whose fp32 scale is not 1, ascending."""
    return [i for i, c in enumerate(torch.as_tensor(scales).tolist()) if c != 1.0]


def arc_gram(G: torch.Tensor, scales) -> torch.Tensor:
    """The clipped rows' Gram (fp32): G'_ij = (c_i c_j) G_ij, the products in fp64 in that order, rounded once."""
    c = torch.as_tensor(scales).detach().double().cpu()
    cc = c[:, None] * c[None, :]
    G = G.detach().cpu()
    return torch.where(cc == 1.0, G.float(), (cc * G.double()).float())


def arc_clip(X, f: int) -> torch.Tensor:
    """The clipped rows y_i = c_i x_i [n, d] (fp64), the scales from the rows' own fp64 squared norms."""
    X = _g(X)
    return arc_scales((X * X).sum(1), f).double()[:, None] * X


def arc_weights(X, f: int, rule: str = "krum", nnm: bool = False, **kw) -> torch.Tensor:
    """Weights [n] (fp64) over the ORIGINAL rows of ``rule`` (krum / geomed / cclip / dnc / caf / average) over the
    clipped rows, behind the mixing when ``nnm``: w_j = c_j a_j."""
    X = _g(X)
    n = X.shape[0]
    c = arc_scales((X * X).sum(1), f).double()
    D = pairwise_sqdist(c[:, None] * X)
    if nnm:
        a = nnm_weights(D, f, rule, **kw).double()
    elif rule == "krum":
        a = krum_weights(D, f, kw.get("m"))
    elif rule == "geomed":
        a = geomed_weights(D, kw.get("iters", 32), kw.get("nu", 1e-6))
    elif rule == "cclip":
        a0 = krum_weights(D, f, kw.get("m")) if kw.get("start", "mean") == "krum" else None
        a = cclip_weights(D, n, a0, kw.get("tau"), f, kw.get("iters", 3))
    elif rule == "dnc":
        a = dnc_weights(D, n - f if kw.get("m") is None else kw["m"], kw.get("iters", 16))[0]
    elif rule == "caf":
        a = caf_weights(D, f, kw.get("iters", 16), kw.get("max_passes"))[0]
    elif rule == "average":
        a = torch.full((n,), 1.0 / n, dtype=torch.float64)
    else:
        raise ValueError(f"arc: unsupported rule {rule!r} (krum, geomed, cclip, dnc, caf, average)")
    return c * a.double()


def arc(X, f: int, rule: str = "krum", nnm: bool = False, **kw) -> torch.Tensor:
    return combine(X, arc_weights(X, f, rule, nnm, **kw))


def arc_coord(X, f: int, rule: str = "trimmed-mean", nnm: bool = False) -> torch.Tensor:
    """A coordinate-wise rule (trimmed-mean with the same f, or median) over the clipped rows, behind the
    mixing when ``nnm``."""
    Y = arc_clip(X, f)
    if nnm:
        return nnm_coord(Y, f, rule)
    return trimmed_mean(Y, f) if rule == "trimmed-mean" else median(Y)


def bulyan_weights(D: torch.Tensor, f: int, m: int | None = None) -> torch.Tensor:
    n = D.shape[0]
    m = n - f - 2 if m is None else m
    t = n - 2 * f - 2
    q = n - f - 2
    scores, P = [], torch.zeros((n, n), dtype=torch.float64)
    for i in range(n):
        near = _order(D[i].tolist(), [j for j in range(n) if j != i])[:q]
        scores.append(sum(float(D[i, j]) for j in near))
        for j in near:
            P[i, j] = D[i, j]
    W = torch.zeros((t, n), dtype=torch.float64)
    for k in range(t):
        mk = max(m - k, 1)
        order = _order(scores)
        for i in order[:mk]:
            W[k, i] = 1.0 / mk
        best = order[0]
        for i in range(n):
            if i != best:
                scores[i] -= float(P[i, best])
        scores[best] = FLT_MAX
    return W


def _closest_mean(vals: list[float], beta: int) -> float:
    s = sorted(_key(v) for v in vals)
    med = s[len(s) // 2]
    kv = sorted((_key(abs(v - med)), v) for v in s)
    return sum(v for _, v in kv[:beta]) / beta


def bulyan(G, f: int, m: int | None = None) -> torch.Tensor:
    X = _g(G)
    n = X.shape[0]
    t = n - 2 * f - 2
    beta = t - 2 * f
    W = bulyan_weights(pairwise_sqdist(X), f, m)
    V = W @ X  # [t, d]
    return torch.tensor([_closest_mean(V[:, x].tolist(), beta) for x in range(X.shape[1])], dtype=torch.float64)


def median(G) -> torch.Tensor:
    X = _g(G)
    out = torch.zeros(X.shape[1], dtype=torch.float64)
    for x in range(X.shape[1]):
        v = sorted(a for a in X[:, x].tolist() if math.isfinite(a))
        out[x] = v[len(v) // 2] if v else 0.0
    return out


def trimmed_mean(G, f: int) -> torch.Tensor:
    X = _g(G)
    n = X.shape[0]
    out = torch.zeros(X.shape[1], dtype=torch.float64)
    for x in range(X.shape[1]):
        v = sorted(_key(a) for a in X[:, x].tolist())
        out[x] = sum(v[f:n - f]) / (n - 2 * f)
    return out


def averaged_median(G, beta: int) -> torch.Tensor:
    X = _g(G)
    return torch.tensor([_closest_mean(X[:, x].tolist(), beta) for x in range(X.shape[1])], dtype=torch.float64)


def average_nan(G) -> torch.Tensor:
    X = _g(G)
    fin = torch.isfinite(X)
    cnt = fin.sum(0)
    s = torch.where(fin, X, torch.zeros_like(X)).sum(0)
    return torch.where(cnt > 0, s / cnt.clamp(min=1), torch.zeros_like(s))


def mix_hash(seed: int, x: int) -> int:
    """Bit-exact Python twin of ``garfield::mix_hash`` (csrc/gar_common.hpp)."""
    z = (seed * 0x9E3779B97F4A7C15 + x + 0x632BE59BD9B4E019) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    z ^= z >> 31
    return z >> 32


def bernoulli_threshold(p: float) -> int:
    if p >= 1.0:
        return 1 << 32
    if p <= 0.0:
        return 0
    return int(p * 4294967296.0)


def condense(G, p: float, seed: int) -> torch.Tensor:
    X = _g(G)
    med = median(X)
    thr = bernoulli_threshold(p)
    out = med.clone()
    for x in range(X.shape[1]):
        if not mix_hash(seed, x) < thr:
            out[x] = X[0, x]
    return out


def brute_weights(D: torch.Tensor, f: int) -> torch.Tensor:
    n = D.shape[0]
    k = n - f
    Df = torch.where(torch.isfinite(D), D.clamp(min=0), torch.full_like(D, FLT_MAX)).float().double()
    best, best_mask = None, None
    # numeric order of k-bit masks == colexicographic order of the subsets
    subsets = sorted(combinations(range(n), k), key=lambda c: sum(1 << i for i in c))
    for c in subsets:
        diam = 0.0
        for a, b in combinations(c, 2):
            diam = max(diam, float(Df[a, b]))
        if best is None or diam < best:
            best, best_mask = diam, c
    w = torch.zeros(n, dtype=torch.float64)
    for i in best_mask:
        w[i] = 1.0 / k
    return w


def brute(G, f: int) -> torch.Tensor:
    return combine(G, brute_weights(pairwise_sqdist(G), f))


# SMEA, smallest maximum eigenvalue averaging (docs/GAR_SEMANTICS.md "SMEA"): Brute's enumeration of the
# (n - f)-subsets, each scored by the top eigenvalue of its members' empirical covariance instead of its
# diameter. The eigenvalue comes from the power rounds of the DnC filter on the subset's block of the squared
# distances, so everything below works on D alone.


def _smea_distances(D: torch.Tensor) -> torch.Tensor:
    """Squared distances [n, n] (fp64, CPU) as the selections build them: clamped at 0, a zero diagonal and
    +inf where non-finite (kept, not zeroed: a subset with such a pair is invalid)."""
    D = D.detach().to(device="cpu", dtype=torch.float64)
    D = torch.where(torch.isfinite(D), D.clamp(min=0), torch.full_like(D, math.inf))
    D.fill_diagonal_(0.0)
    return D


def smea_subsets(n: int, k: int) -> torch.Tensor:
    """The C(n, k) subsets as ascending member indices [C(n, k), k] (int64), row ``rank`` = the subset whose
    k-bit mask is the rank-th smallest: Brute's enumeration order."""
    lex = torch.tensor(list(combinations(range(n), k)), dtype=torch.int64).reshape(-1, k)
    # numeric order of the masks compares the largest member first: the reverse of the lexicographic
    # order of the mirrored tuples
    return (n - 1 - lex).flip(1).flip(0).contiguous()


def smea_lambda(D: torch.Tensor, members, iters: int = 16) -> float:
    """λ of one subset (fp64): the top eigenvalue of the members' empirical covariance (1/k) Σ (x_i - μ)(x_i - μ)ᵀ
    after exactly ``iters`` power rounds on K_S = -½ J D_S J, members in increasing index, sums in index
    order (the loop of :func:`dnc_scores` on the sub-matrix, λ / k). +inf if any pair of members has a
    non-finite distance; 0 for a single member."""
    D = _smea_distances(D)
    S = sorted(int(i) for i in members)
    k = len(S)
    dist = [[float(D[a, b]) for b in S] for a in S]
    if any(not math.isfinite(v) for row in dist for v in row):
        return math.inf
    if k == 1:
        return 0.0
    return _dnc_power(dist, list(range(k)), iters)[0] / k


def smea_lambdas(D: torch.Tensor, f: int, iters: int = 16, chunk: int | None = None) -> torch.Tensor:
    """λ of every (n - f)-subset [C(n, n - f)] (fp64) in rank order: :func:`smea_lambda` vectorised over the
    subsets (gathered [B, k, k] blocks, batched power rounds, ``chunk`` subsets at a time: None, 32 MB blocks)."""
    D = _smea_distances(D)
    n = D.shape[0]
    k = n - f
    chunk = max(64, (1 << 22) // (k * k)) if chunk is None else chunk
    subsets = smea_subsets(n, k)
    out = torch.empty(subsets.shape[0], dtype=torch.float64)
    ids = torch.arange(k)
    for lo in range(0, subsets.shape[0], chunk):
        S = subsets[lo:lo + chunk]
        B = torch.arange(S.shape[0])
        Ds = D[S[:, :, None], S[:, None, :]]
        bad = ~torch.isfinite(Ds).all(2).all(1)
        Ds = torch.where(bad[:, None, None], torch.zeros_like(Ds), Ds)
        if k == 1:
            out[lo:lo + chunk] = torch.where(bad, math.inf, 0.0)
            continue
        r = Ds.sum(2) / k
        g = r.sum(1, keepdim=True) / k
        kappa = r - 0.5 * g
        star = torch.where(kappa == kappa.max(1, keepdim=True).values, ids[None, :], k).min(1).values
        b = -0.5 * (Ds[B, :, star] - r - r[B, star][:, None] + g)
        u = torch.zeros_like(b)
        for _ in range(iters):
            nu = (b * b).sum(1, keepdim=True).sqrt()
            u = torch.where(nu > 0, b / nu, torch.zeros_like(b))
            c = u.sum(1, keepdim=True) / k
            t = (Ds * (u - c)[:, None, :]).sum(2)
            b = -0.5 * (t - t.sum(1, keepdim=True) / k)
        lam = (u * b).sum(1) / k
        out[lo:lo + chunk] = torch.where(bad, torch.full_like(lam, math.inf), lam)
    return out


def smea_key(lams: torch.Tensor) -> torch.Tensor:
    """The fp32 score the winner is chosen by: λ cast to fp32, negative values 0 (NaN: +inf)."""
    s = lams.float().clamp(min=0)
    return torch.where(torch.isnan(s), torch.full_like(s, math.inf), s)


def smea_weights(D: torch.Tensor, f: int, iters: int = 16) -> tuple:
    """(w [n] fp32, λ fp32 scalar tensor): 1 / (n - f) on the members of the subset of smallest
    (fp32 λ, rank), 0 elsewhere, and that λ."""
    n = D.shape[0]
    k = n - f
    s = smea_key(smea_lambdas(D, f, iters))
    rank = int(torch.where(s == s.min(), torch.arange(s.numel()), s.numel()).min())
    w = torch.zeros(n, dtype=torch.float64)
    w[smea_subsets(n, k)[rank]] = 1.0 / k
    return w.float(), s[rank]


def smea_dense_lambda(X, members) -> float:
    """The check on the vectors themselves: the top eigenvalue (``torch.linalg.eigvalsh``) of the members'
    d x d empirical covariance (1/k) Σ (x_i - μ)(x_i - μ)ᵀ."""
    X = _g(X)[sorted(int(i) for i in members)]
    C = X - X.mean(dim=0, keepdim=True)
    return float(torch.linalg.eigvalsh(C.T @ C / X.shape[0])[-1])


def smea(G, f: int, iters: int = 16) -> torch.Tensor:
    X = _g(G)
    return combine(X, smea_weights(pairwise_sqdist(X), f, iters)[0].double())


def worker_momentum(X, M, beta: float, first: bool, lo: int = 0, hi: int | None = None):
    """Worker-side momentum on coordinates [lo, hi) of the rows ``X`` [k, >= hi] with the state ``M``
    [k, >= hi] (docs/GAR_SEMANTICS.md "Worker momentum"): ``(state, finite)``, both [k, hi - lo]. The
    new state in exact fp64 arithmetic, m <- g on the first step and beta * m + (1 - beta) * g later,
    with g the row's value; where g is not finite (``finite`` False) the state stays what it was and
    the row keeps g. The row a native implementation leaves is ITS fp32 state rounded to nearest even
    into the row's dtype, never this fp64 value rounded."""
    X, M = _g(X), _g(M)
    hi = X.shape[1] if hi is None else hi
    g, m = X[:, lo:hi], M[:, lo:hi]
    finite = torch.isfinite(g)
    new = g if first else beta * m + (1.0 - beta) * g
    return torch.where(finite, new, m), finite


def agr_perturbation(X: torch.Tensor, perturbation: str) -> tuple:
    """(μ, p) of the estimate rows ``X`` [k, d] (fp64): p = -σ (unbiased, 0 for k = 1), -μ or -sign μ."""
    mu = X.mean(0)
    if perturbation == "std":
        p = -X.std(0, unbiased=True) if X.shape[0] > 1 else torch.zeros_like(mu)
    elif perturbation == "uv":
        p = -mu
    elif perturbation == "sgn":
        p = -torch.sign(mu)
    else:
        raise ValueError(f"unknown perturbation {perturbation!r}; available: 'std', 'uv', 'sgn'")
    return mu, p


def agr_attack(E, objective: str, perturbation: str = "std") -> tuple:
    """The Min-Max / Min-Sum colluding attacks (docs/GAR_SEMANTICS.md "Adaptive colluding attacks") on the
    estimate rows ``E`` [k, d], on the vectors: ``(m, γ)`` with m = μ + γ p and γ the largest value with
    max_i ‖m - e_i‖² <= R = max_ij ‖e_i - e_j‖² (``objective`` "minmax") or Σ_i ‖m - e_i‖² <= S =
    max_i Σ_j ‖e_i - e_j‖² ("minsum"), in closed form from ‖m - e_i‖² = a_i + 2 γ b_i + γ² c. γ = 0 for
    k = 1, c = 0 or any non-finite quantity. Returns (fp64 [d], float)."""
    if objective not in ("minmax", "minsum"):
        raise ValueError(f"unknown objective {objective!r}; available: 'minmax', 'minsum'")
    X = _g(E)
    k = X.shape[0]
    mu, p = agr_perturbation(X, perturbation)
    D = torch.zeros((k, k), dtype=torch.float64)
    for i in range(k):
        D[i] = ((X - X[i]) ** 2).sum(1)
    a = ((mu - X) ** 2).sum(1)
    b = (p * (mu - X)).sum(1)
    c = float((p * p).sum())
    bound = float(D.max()) if objective == "minmax" else float(D.sum(1).max())
    gamma = 0.0
    if k > 1 and c > 0 and math.isfinite(c) and math.isfinite(bound) and bool(torch.isfinite(a).all()) \
            and bool(torch.isfinite(b).all()):
        if objective == "minmax":
            gamma = float(((-b + torch.sqrt(b * b + c * (bound - a).clamp(min=0))) / c).min())
        else:
            gamma = math.sqrt(max(bound - float(a.sum()), 0.0) / (k * c))
        if not math.isfinite(gamma):
            gamma = 0.0
    if gamma == 0.0:
        return mu.clone(), 0.0      # also keeps a non-finite p out of m
    return mu + gamma * p, gamma


def aksel(G, f: int, mode: str = "mid") -> torch.Tensor:
    X = _g(G)
    n = X.shape[0]
    med = median(X)
    dist = [((X[j] - med) ** 2).sum().item() for j in range(n)]
    dist = [d if math.isfinite(d) else math.inf for d in dist]
    c = (n + 1) // 2 if mode == "mid" else n - f
    w = torch.zeros(n, dtype=torch.float64)
    for j in _order(dist)[:c]:
        w[j] = 1.0 / c
    return combine(X, w)
