"""Device-dispatching front-end of the robust gradient aggregation rules (GARs).

Every rule accepts the gradient set either as an ``[n, d]`` tensor (rows may be
views of a padded exchange buffer) or as a list of ``n`` 1-D tensors (the
reference's ``gradients=[...]`` calling convention, ``PT/libs/aggregators/
__init__.py:15-31``), and returns a NEW 1-D tensor of the input dtype.

GPU path (``garfield_amd._C``, gfx950 HIP), all launches asynchronous on the
current stream, nothing copied to the host:

* Krum / Multi-Krum: split-K MFMA Gram -> one-workgroup selection -> combine;
* Geometric median: Gram -> one-workgroup smoothed Weiszfeld on the n x n distances -> combine;
* Centered clipping: Gram -> (Krum selection as the robust start) -> one-workgroup clipping rounds on the
  n x n distances -> combine;
* Nearest-neighbour mixing before Krum / geometric median / centered clipping / average: Gram -> one-workgroup mix
  (neighbour sets + the mixed rows' pseudo-Gram) -> the rule's selection -> un-mix -> combine;
* Adaptive robust clipping before any of those (and before the mixing): Gram -> one-workgroup scales + the clipped
  rows' Gram -> (mix ->) the rule's selection -> (un-mix ->) fold the scales into the weights -> combine; before the
  coordinate-wise trimmed mean / median: the clipped rows rewritten on a private copy -> the rule;
* Bulyan: Gram -> on-device selection loop -> W[t, n] -> fused W·G averaged-median;
* Brute: Gram -> device-wide subset search (atomicMin on (diameter, rank)) -> combine;
* Median / Trimmed-Mean / Averaged-Median / Average-NaN / Condense: register
  sorting-network kernels;
* Aksel: median kernel -> squared distance to it -> selection -> combine.

CPU path: the C++ thread-pool implementations in the same extension.

More than ``MAX_ROWS`` (128) gradients (the reference's gar_bench sweeps n to 512): on
the GPU, up to ``LARGE_ROWS`` (1024) rows run on ``gar_large.hip`` as one [n, d] matrix
(combine with fp32 accumulation; median / trimmed-mean / averaged-median and the Bulyan
tail by LDS radix select; the Krum/Bulyan Gram as a split-K MFMA kernel with fp32 output and
Bulyan's W·X on fp32 MFMA);
everything else, and the CPU, uses a vectorised PyTorch implementation.

The distance-based selections (Krum, geometric median, centered clipping, DnC, CAF, Brute, SMEA, Bulyan, and the
mixing in front of them) are resolved and dispatched in ``ops/selection.py``; :func:`selection_weights`
picks the backend for a gradient set.
"""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass, field, replace

import torch

from garfield_amd import _native
from garfield_amd.ops import reference as ref
# the distance-based selections live in ops/selection.py; their Gram forms keep their names here
from garfield_amd.ops.selection import (ARC_RULES, BRUTE_MAX_SUBSETS, CCLIP_STARTS, MAX_ROWS, NNM_RULES,  # noqa: F401
                                        SMEA_MAX_SUBSETS,
                                        Selection, arc_count, arc_distances, arc_gram, arc_scales_from_sqnorms,
                                        cclip_weights_from_gram, distances_from_gram,
                                        dnc_weights_from_gram, geomed_weights_from_gram, krum_weights_from_gram,
                                        large_bulyan_weights as _large_bulyan_weights, large_select,
                                        nan_inf as _nan_inf, nnm_from_gram, resolve)

LARGE_ROWS = 1024
_LARGE_MODE = {"median": 0, "trimmed-mean": 1, "averaged-median": 2}

_MODE = {"median": 0, "trimmed-mean": 1, "averaged-median": 2, "average-nan": 3, "condense": 4, "bulyan-tail": 5}


# --------------------------------------------------------------------------- #
# Input normalisation


@dataclass
class Rows:
    """A gradient set ready for the native layer."""

    obj: object  # [n, d] tensor or list of 1-D tensors
    n: int
    d: int
    dtype: torch.dtype
    device: torch.device
    out_dtype: torch.dtype  # dtype of the returned aggregate

    def stacked(self) -> torch.Tensor:
        if isinstance(self.obj, torch.Tensor):
            return self.obj
        return torch.stack(list(self.obj))


_SUPPORTED_GPU = (torch.float32, torch.bfloat16, torch.float16)


def _aligned(t: torch.Tensor) -> bool:
    return t.data_ptr() % 16 == 0


def prepare(gradients) -> Rows:
    """Validate and normalise a gradient set (list of tensors or [n, d] tensor; prepared rows pass through)."""
    if isinstance(gradients, Rows):
        return gradients
    if isinstance(gradients, torch.Tensor):
        if gradients.dim() == 1:
            gradients = gradients.unsqueeze(0)
        if gradients.dim() != 2:
            raise ValueError(f"expected an [n, d] gradient tensor, got shape {tuple(gradients.shape)}")
        G = gradients
        out_dtype = G.dtype
        if G.device.type == "cpu":
            if G.dtype not in (torch.float32, torch.float64):
                G = G.float()
            if G.stride(1) != 1:
                G = G.contiguous()
        else:
            if G.dtype not in _SUPPORTED_GPU:
                G = G.float()
            esz = G.element_size()
            if G.stride(1) != 1 or (G.stride(0) * esz) % 16 != 0 or not _aligned(G):
                G = _padded_copy(G)
        return Rows(G, G.shape[0], G.shape[1], G.dtype, G.device, out_dtype)
    if not isinstance(gradients, (list, tuple)) or len(gradients) == 0:
        raise ValueError("expected a non-empty list of gradients")
    first = gradients[0]
    dev, dt = first.device, first.dtype
    d = first.numel()
    rows = []
    for g in gradients:
        if g.device != dev:
            raise ValueError("all gradients must be on the same device")
        if g.numel() != d:
            raise ValueError(f"all gradients must have the same size ({g.numel()} != {d})")
        rows.append(g.reshape(-1))
    out_dtype = dt
    if dev.type == "cpu":
        if dt not in (torch.float32, torch.float64):
            rows = [r.float() for r in rows]
        rows = [r if r.is_contiguous() else r.contiguous() for r in rows]
        if any(r.dtype != rows[0].dtype for r in rows):
            rows = [r.float() for r in rows]
    else:
        if dt not in _SUPPORTED_GPU or any(r.dtype != dt for r in rows):
            rows = [r.float() for r in rows]
        rows = [r if (r.is_contiguous() and _aligned(r)) else r.clone(memory_format=torch.contiguous_format)
                for r in rows]
        rows = [r if _aligned(r) else _aligned_clone(r) for r in rows]
    return Rows(rows, len(rows), d, rows[0].dtype, dev, out_dtype)


def _aligned_clone(t: torch.Tensor) -> torch.Tensor:
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    off = (-(buf.data_ptr() % 16) // t.element_size()) % (16 // t.element_size())
    v = buf[off:off + t.numel()]
    v.copy_(t)
    return v


def _padded_copy(G: torch.Tensor) -> torch.Tensor:
    n, d = G.shape
    esz = G.element_size()
    align = 16 // esz
    ld = ((d + align - 1) // align) * align
    buf = torch.empty((n, ld), dtype=G.dtype, device=G.device)
    buf[:, :d].copy_(G)
    return buf[:, :d]


# --------------------------------------------------------------------------- #
# Device workspaces (allocated once per shape/stream, reused: capture-safe)


@dataclass
class Workspace:
    n: int
    d: int
    device: torch.device
    tensors: dict = field(default_factory=dict)

    def get(self, name: str, numel: int, dtype=torch.float32) -> torch.Tensor:
        t = self.tensors.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(max(numel, 1), dtype=dtype, device=self.device)
            self.tensors[name] = t
        return t[:numel]


_WS: dict = {}
_WS_LOCK = threading.Lock()


def workspace(rows: Rows) -> Workspace:
    stream = torch.cuda.current_stream(rows.device).cuda_stream if rows.device.type == "cuda" else 0
    key = (str(rows.device), rows.n, rows.d, stream)
    with _WS_LOCK:
        ws = _WS.get(key)
        if ws is None:
            if len(_WS) > 64:
                _WS.clear()
            ws = Workspace(rows.n, rows.d, rows.device)
            _WS[key] = ws
    return ws


def _C_for(rows: Rows):
    return _native.require_for(rows.device)


def _finish(out: torch.Tensor, rows: Rows) -> torch.Tensor:
    return out if out.dtype == rows.out_dtype else out.to(rows.out_dtype)


# --------------------------------------------------------------------------- #
# Building blocks


def gram(gradients) -> torch.Tensor:
    """G·Gᵀ (fp32 [n, n]) on the GPU; fp64 pairwise squared distances are in pairwise_distances."""
    rows = prepare(gradients)
    if rows.device.type != "cuda":
        X = rows.stacked().double()
        return X @ X.T
    if rows.n > MAX_ROWS:
        return _large_gram(rows)
    C = _C_for(rows)
    ws = workspace(rows)
    g = _gram_into(C, rows, ws)
    np_ = C.gram_padded(rows.n)
    return g.view(np_, np_)[: rows.n, : rows.n].clone()


def _gram_into(C, rows: Rows, ws: Workspace) -> torch.Tensor:
    grid = C.gram_grid(rows.d, _dtype_probe(rows), rows.n)
    slabs = ws.get("slabs", (grid + C.GRAM_REDUCE_GROUPS) * C.gram_slab_floats(rows.n))
    np_ = C.gram_padded(rows.n)
    g = ws.get("gram", np_ * np_)
    C.gpu_gram(rows.obj, slabs, g)
    return g


_PROBES: dict = {}


def _dtype_probe(rows: Rows) -> torch.Tensor:
    p = _PROBES.get(rows.dtype)
    if p is None:
        p = torch.empty(0, dtype=rows.dtype)
        _PROBES[rows.dtype] = p
    return p


def pairwise_distances(gradients) -> torch.Tensor:
    """Squared L2 distance matrix [n, n] (+inf on the diagonal and for non-finite pairs)."""
    rows = prepare(gradients)
    if rows.device.type == "cuda":
        g = gram(rows.obj).double()
        dg = torch.diagonal(g)
        D = dg[:, None] + dg[None, :] - 2 * g
        D = torch.where(torch.isfinite(D), D.clamp(min=0), torch.full_like(D, math.inf))
        D.fill_diagonal_(math.inf)
        return D.cpu()
    C = _C_for(rows)
    if C is None:
        return ref.pairwise_sqdist(rows.stacked())
    return C.cpu_pairwise(rows.obj)


def combine(gradients, weights: torch.Tensor) -> torch.Tensor:
    rows = prepare(gradients)
    if _large(rows):
        X = _matrix(rows)
        out = torch.empty(rows.d, dtype=X.dtype, device=X.device)
        _native.native().gpu_large_combine(X, weights.to(X.device, torch.float32).contiguous(), out)
        return _finish(out, rows)
    if rows.n > MAX_ROWS:
        return _finish((weights.to(rows.device, torch.float32)[:, None] * rows.stacked().float()).sum(0), rows)
    C = _C_for(rows)
    if rows.device.type == "cuda":
        out = torch.empty(rows.d, dtype=rows.dtype, device=rows.device)
        C.gpu_combine(rows.obj, weights.to(rows.device, torch.float32).contiguous(), out)
        return _finish(out, rows)
    if C is None:
        return ref.combine(rows.stacked(), weights.double()).to(rows.out_dtype)
    return _finish(C.cpu_combine(rows.obj, weights.float().cpu()), rows)


def combine_into(gradients, weights: torch.Tensor, out: torch.Tensor) -> None:
    """out (fp32, [d]) = Σ_j w_j g_j in fp32 (the GPU combine kernel's arithmetic, no rounding to
    the gradients' dtype): the layer-wise loop's per-segment combine."""
    rows = prepare(gradients)
    if rows.device.type == "cuda" and rows.n <= MAX_ROWS:
        dst = out if (out.is_contiguous() and _aligned(out)) else torch.empty_like(out)
        _C_for(rows).gpu_combine(rows.obj, weights.to(rows.device, torch.float32).contiguous(), dst)
        if dst is not out:
            out.copy_(dst)
        return
    X = rows.stacked().double() if rows.dtype == torch.float64 else rows.stacked().float()
    out.copy_((weights.to(X.device, X.dtype)[:, None] * X).sum(0))


def _large(rows: Rows) -> bool:
    """GPU set of MAX_ROWS < n <= LARGE_ROWS gradients: the gar_large.hip kernels."""
    return rows.device.type == "cuda" and MAX_ROWS < rows.n <= LARGE_ROWS


def _matrix(rows: Rows) -> torch.Tensor:
    X = rows.stacked()
    return X if X.stride(1) == 1 else X.contiguous()


# --------------------------------------------------------------------------- #
# Rules


def average(gradients, **_) -> torch.Tensor:
    rows = prepare(gradients)
    if rows.device.type == "cuda" and rows.n <= MAX_ROWS:
        ws = workspace(rows)
        w = ws.tensors.get("avg_w")
        if w is None:
            w = torch.full((rows.n,), 1.0 / rows.n, dtype=torch.float32, device=rows.device)
            ws.tensors["avg_w"] = w
        return combine(rows, w)
    if _large(rows):
        return combine(rows, torch.full((rows.n,), 1.0 / rows.n, dtype=torch.float32, device=rows.device))
    return _finish(rows.stacked().float().mean(0) if rows.dtype != torch.float64 else rows.stacked().mean(0), rows)


def selection_weights(gradients, sel: Selection) -> torch.Tensor:
    """The weights of the resolved selection ``sel`` over a gradient set ([n] fp32 on the gradients' device;
    Bulyan: W [t, n]). The one place the backend is picked, by (n, device, extension): the device kernels on
    the workspace's Gram; beyond their rows the form vectorised on the Gram where the rule has one; else
    fp64 squared distances into the C++ functions or the oracle."""
    rows = prepare(gradients)
    C = _C_for(rows)
    cuda = rows.device.type == "cuda"
    if cuda and rows.n <= sel.device_rows:
        ws = workspace(rows)
        return sel.on_device(C, _gram_into(C, rows, ws), ws)
    if rows.n > MAX_ROWS and sel.has_gram_form(cuda):   # the Gram's own device: large_gram on the GPU, no host round trip
        return sel.from_gram(_large_gram(rows))
    if cuda:
        D = pairwise_distances(rows.obj)
    else:
        # the C++ distances take MAX_ROWS rows; beyond them (a rule without a Gram form: caf) the oracle's
        host = C is None or rows.n > MAX_ROWS
        D = ref.pairwise_sqdist(rows.stacked()) if host else C.cpu_pairwise(rows.obj)
    if sel.clips:   # distances lose the norms ARC decides from: they travel beside D
        return sel.on_host(C, D, _sqnorms(rows)).to(rows.device)
    return sel.on_host(C, D).to(rows.device)


def _sqnorms(rows: Rows) -> torch.Tensor:
    """The rows' squared norms [n] (fp64, CPU): the Gram's diagonal on the GPU, fp64 sums on the CPU."""
    if rows.device.type == "cuda":
        return torch.diagonal(gram(rows)).double().cpu()
    X = rows.stacked().double()
    return (X * X).sum(1)


def krum_weights(gradients, f: int, m: int | None = None, pre: str | None = None) -> torch.Tensor:
    """Selection weights of Multi-Krum ([n] fp32 on the gradients' device); ``pre="nnm"``: the row
    weights of Krum applied after nearest-neighbour mixing (:func:`nnm_weights`)."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve("krum", rows.n, f, m, pre))


def krum(gradients, f: int, m: int | None = None, **_) -> torch.Tensor:
    rows = prepare(gradients)
    return combine(rows, krum_weights(rows, f, m))


def geomed_weights(gradients, iters: int = 32, nu: float = 1e-6, pre: str | None = None, f: int = 0) -> torch.Tensor:
    """Weights of the geometric median ([n] fp32 on the gradients' device): ``iters`` rounds of
    smoothed Weiszfeld (RFA) iterated on the pairwise distances alone. ``pre="nnm"``: the row weights
    of the geometric median of the rows mixed over their ``n - f`` nearest (:func:`nnm_weights`)."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve("geomed", rows.n, f, None, pre, {"iters": iters, "nu": nu}))


def geomed(gradients, f: int = 0, iters: int = 32, nu: float = 1e-6, **_) -> torch.Tensor:
    """Geometric median (minimiser of the sum of L2 distances; breakdown point 1/2, so ``f`` only
    enters the registry's check): Σ_i a_i g_i with the weights of :func:`geomed_weights`."""
    rows = prepare(gradients)
    return combine(rows, geomed_weights(rows, iters, nu))


# DnC spectral filtering (docs/GAR_SEMANTICS.md): the squared projection of every centred row on the top
# principal direction equals λ u_i² for the top eigenpair of K = -½ J D J, so the scores come from a
# fixed number of power rounds on the Gram's distances alone and end in a weight vector (1 / kv on the
# kv lowest scores) for the combine kernels.


def dnc_weights(gradients, f: int, m: int | None = None, iters: int = 16, pre: str | None = None) -> torch.Tensor:
    """Selection weights of DnC spectral filtering ([n] fp32 on the gradients' device): 1 / m on the
    ``m`` (default ``n - f``) rows of lowest outlier score, the squared projection on the top principal
    direction of the centred rows, from ``iters`` power rounds on the pairwise distances alone. ``pre="arc"``:
    the row weights of DnC over the adaptively clipped rows (:func:`arc_weights`)."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve("dnc", rows.n, f, m, pre, {"iters": iters}))


def dnc(gradients, f: int = 0, m: int | None = None, iters: int = 16, **_) -> torch.Tensor:
    """DnC spectral filtering (Shejwalkar & Houmansadr, 2021; all coordinates, one filter): the average
    of the rows kept by :func:`dnc_weights`."""
    rows = prepare(gradients)
    return combine(rows, dnc_weights(rows, f, m, iters))


# CAF, the covariance filter (docs/GAR_SEMANTICS.md): the top eigenpair of the weighted covariance
# Σ_i a_i (x_i - μ_a)(x_i - μ_a)ᵀ comes from power rounds on the n x n matrix A^½ K A^½ of the Gram's distances,
# every row is down-weighted by its squared projection on the top direction, pass after pass, and the
# weights of the pass of smallest top eigenvalue go to the combine kernels.


def caf_weights(gradients, f: int, iters: int = 16, max_passes: int | None = None,
                pre: str | None = None) -> torch.Tensor:
    """Weights of the CAF covariance filter ([n] fp32 on the gradients' device): while more than n - 2f rows'
    worth of weight is left (at most ``max_passes`` passes, None: n), ``iters`` power rounds on the pairwise
    distances alone and a soft down-weighting along the top principal direction of the weighted covariance; the
    weights of the pass whose covariance had the smallest top eigenvalue. ``pre="arc"``: the row weights of
    CAF over the adaptively clipped rows (:func:`arc_weights`)."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve("caf", rows.n, f, None, pre, {"iters": iters, "max_passes": max_passes}))


def caf(gradients, f: int = 0, iters: int = 16, max_passes: int | None = None, **_) -> torch.Tensor:
    """CAF, the covariance-bound agnostic filter (Allouah et al.): Σ_i a_i g_i with the weights of
    :func:`caf_weights`."""
    rows = prepare(gradients)
    return combine(rows, caf_weights(rows, f, iters, max_passes))


# Centered clipping (CC; docs/GAR_SEMANTICS.md): v <- v + (1/n) Σ_i (x_i - v) min(1, tau / ||x_i - v||). The
# centre stays an affine combination of the rows, so the rounds run on the Gram's distances alone and
# end in a weight vector for the combine kernels. tau=None: the radius from the data, every round (the
# (|V| - f)-th smallest distance of the centre to a worker).


def _with_center(rows: Rows, center: torch.Tensor) -> Rows:
    """The row table with ``center`` appended as row n (cast to the rows' dtype; the rows are not copied)."""
    c = center.detach().reshape(-1)
    if c.numel() != rows.d:
        raise ValueError(f"cclip: center has {c.numel()} elements, the gradients {rows.d}")
    c = c.to(device=rows.device, dtype=rows.dtype)
    table = list(rows.obj.unbind(0)) if isinstance(rows.obj, torch.Tensor) else list(rows.obj)
    out = prepare(table + [c])
    out.out_dtype = rows.out_dtype
    return out


def _cclip_rows_w(gradients, f, tau, iters, start, center, m, pre) -> tuple:
    rows = prepare(gradients)
    kw = {"tau": tau, "iters": iters, "start": start}
    if center is None:
        return rows, selection_weights(rows, resolve("cclip", rows.n, f, m, pre, kw))
    if start is not None:
        raise ValueError("cclip: give either center or start, not both")
    if pre is not None:
        raise ValueError("cclip: a center is not supported under nearest-neighbour mixing")
    sel = resolve("cclip", rows.n, f, m, None, kw)   # the centre is row n, basis-only, and carries the start weight
    rows = _with_center(rows, center)
    return rows, selection_weights(rows, replace(sel, n=rows.n, start="center"))


def cclip_weights(gradients, f: int = 0, tau: float | None = None, iters: int = 3, start=None, center=None,
                  m: int | None = None, pre: str | None = None) -> torch.Tensor:
    """Weights of centered clipping ([n] fp32 on the gradients' device; [n + 1] with a ``center``, whose
    row is the last): ``iters`` clipping rounds iterated on the pairwise distances alone. ``tau``: the
    absolute L2 radius, None: from the data (the (n - f)-th smallest distance to the centre, every round).
    ``start``: "mean" (default), "krum" (the Multi-Krum weights with ``f`` and ``m``: the robust start) or an
    [n] weight tensor; ``center``: a d-vector to start from instead. ``pre="nnm"``: the row weights of
    centered clipping on the rows mixed over their ``n - f`` nearest (:func:`nnm_weights`)."""
    return _cclip_rows_w(gradients, f, tau, iters, start, center, m, pre)[1]


def cclip(gradients, f: int = 0, tau: float | None = None, iters: int = 3, start=None, center=None,
          m: int | None = None, pre: str | None = None, **_) -> torch.Tensor:
    """Centered clipping (Karimireddy et al., 2021): Σ_i a_i g_i (+ a_n center) with the weights of
    :func:`cclip_weights`."""
    rows, w = _cclip_rows_w(gradients, f, tau, iters, start, center, m, pre)
    return combine(rows, w)


# Nearest-neighbour mixing (NNM; docs/GAR_SEMANTICS.md): every row is replaced by the mean of its
# n - f nearest rows, itself included, before the rule runs. Mixing is linear: the mixed rows' distances
# follow from the Gram, the rule's weights fold back onto the original rows, and the combine kernels
# consume those: no pass over the d-length rows, no [n, d] buffer of mixed gradients.


def nnm_mix(gradients, f: int) -> tuple:
    """The mixing alone: ``(H, masks)`` on the GPU for n <= MAX_ROWS (the pseudo-Gram [np, np] the
    selection kernels take, and the sets as [n, 2] int64 mask words), ``(D', masks)`` on the CPU
    (fp64 distances of the mixed rows), ``(H, S)`` of :func:`nnm_from_gram` for n > MAX_ROWS.
    Any 0 <= f < n."""
    rows = prepare(gradients)
    if not 0 <= f < rows.n:
        raise ValueError(f"nnm: expected 0 <= f < n, got f = {f}, n = {rows.n}")
    if rows.n > MAX_ROWS:
        return nnm_from_gram(_large_gram(rows), f)
    C = _C_for(rows)
    if rows.device.type == "cuda":
        ws = workspace(rows)
        g = _gram_into(C, rows, ws)
        np_ = C.gram_padded(rows.n)
        H = torch.zeros(np_ * np_, dtype=torch.float32, device=rows.device)
        masks = torch.empty((rows.n, 2), dtype=torch.int64, device=rows.device)
        C.gpu_nnm_mix(g, rows.n, f, H, masks)
        return H.view(np_, np_), masks
    if C is None:
        sets, Dm = ref.nnm_distances(ref.pairwise_sqdist(rows.stacked()), f)
        return Dm, masks_from_sets(sets)
    return C.cpu_nnm_mix(C.cpu_pairwise(rows.obj), f)


def masks_from_sets(sets) -> torch.Tensor:
    """[n, 2] int64 mask words of neighbour sets given as index lists (n <= 128)."""
    out = []
    for s in sets:
        v = sum(1 << j for j in s)
        out.append([((v >> (64 * k)) & ((1 << 64) - 1)) for k in range(2)])
    return torch.tensor([[x - (1 << 64) if x >= (1 << 63) else x for x in r] for r in out], dtype=torch.int64)


def nnm_weights(gradients, f: int, rule: str = "krum", **kw) -> torch.Tensor:
    """Weights over the ORIGINAL rows ([n] fp32 on the gradients' device) of ``rule`` (krum: ``m``;
    geomed: ``iters``, ``nu``; cclip: ``tau``, ``iters``, ``start`` "mean" / "krum", ``m``; average) applied to the rows mixed over their n - f nearest."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve(rule, rows.n, f, kw.pop("m", None), "nnm", kw))


def nnm(gradients, f: int, rule: str = "krum", **kw) -> torch.Tensor:
    """``rule`` after nearest-neighbour mixing: Σ_j w_j g_j with the weights of :func:`nnm_weights`."""
    rows = prepare(gradients)
    return combine(rows, nnm_weights(rows, f, rule, **kw))


# NNM before a coordinate-wise rule (docs/GAR_SEMANTICS.md "Nearest-neighbour mixing before a
# coordinate-wise rule"): there is no weight vector to fold the mixing into, so per coordinate the n set
# means are formed and the rule runs over them, in one pass over the rows; the mixed rows are never stored.

NNM_COORD_RULES = ("trimmed-mean", "median")


def _nnm_coord_args(n: int, f: int, rule: str) -> None:
    if rule not in NNM_COORD_RULES:
        raise ValueError(f"nnm: unsupported coordinate-wise rule {rule!r}; available: {NNM_COORD_RULES}")
    if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < n:
        raise ValueError(f"nnm: expected 0 <= f < n, got f = {f!r}, n = {n}")
    if rule == "trimmed-mean" and n < 2 * f + 1:
        raise ValueError(f"nnm-trimmed-mean: expected n >= 2f + 1, got n = {n}, f = {f}")


def nnm_coord_into(C, ws: Workspace, G, g: torch.Tensor, n: int, f: int, rule: str, out: torch.Tensor) -> None:
    """``out`` (fp32 or the rows' dtype, >= d elements) = ``rule`` over the rows ``G`` mixed over their
    n - f nearest, from a device Gram ``g`` (pitch gram_padded(n), n <= MAX_ROWS): the sets launch, then
    k_nnm_coord. Every buffer comes from ``ws`` (capture-safe)."""
    masks = ws.get("nnm_masks", 2 * n, torch.int64)
    C.gpu_nnm_sets(g, n, f, masks)
    C.gpu_nnm_coord(G, masks, n, f, rule, out)


def nnm_coord_from_distances(C, X: torch.Tensor, D: torch.Tensor, f: int, rule: str) -> torch.Tensor:
    """``rule`` over the CPU rows ``X`` [n, d'] mixed by the sets of the squared distances ``D`` (which
    may come from more coordinates than X holds: a shard of the rows with the distances summed over
    ranks). The C++ path for n <= MAX_ROWS, else the oracle. A coordinate's result does not depend on
    which other coordinates X holds."""
    n = X.shape[0]
    if C is None or n > MAX_ROWS:
        Y = ref.nnm_mixed_rows(X, ref.nnm_sets(D, f))
        return (ref.trimmed_mean(Y, f) if rule == "trimmed-mean" else ref.median(Y)).to(X.dtype)
    _, masks = C.cpu_nnm_mix(D, f)
    return C.cpu_mixed_coordwise(X, masks, n - f, rule, f)


def _large_nnm_coord(rows: Rows, f: int, rule: str) -> torch.Tensor:
    """MAX_ROWS < n <= LARGE_ROWS on the GPU, as Bulyan's large case: the sets from the Gram, the mixed
    rows V = (S / c) · X column chunk by chunk into a bounded fp32 buffer, the radix-select rule on each."""
    n, c = rows.n, rows.n - f
    X = _matrix(rows)
    _, S = nnm_from_gram(_large_gram(rows), f)
    Wd = (S.float() / float(c)).contiguous()
    out = torch.empty(rows.d, dtype=torch.float32, device=rows.device)
    step = max(1, (1 << 28) // (4 * n))
    Vbuf = torch.empty((n, min(step, rows.d)), dtype=torch.float32, device=rows.device)
    for c0 in range(0, rows.d, step):
        w = min(step, rows.d - c0)
        Xc = X[:, c0:c0 + w]
        V = large_wx(Wd, Xc, Vbuf[:, :w])
        bad = (~torch.isfinite(Xc)).any(0).nonzero().flatten()
        if bad.numel():   # 0 * inf poisoned every set of these coordinates: plain sums over the members
            Xb = Xc[:, bad].float()
            V[:, bad] = torch.where(S[:, :, None], Xb[None], torch.zeros((), device=X.device)).sum(1) / float(c)
        _native.native().gpu_large_coord(V, _LARGE_MODE[rule], f, 0, out[c0:c0 + w])
    return out


def nnm_coord(gradients, f: int, rule: str = "trimmed-mean") -> torch.Tensor:
    """``rule`` ("trimmed-mean" with the same ``f``, or "median") over the rows mixed over their n - f
    nearest, in the gradients' dtype. GPU, n <= MAX_ROWS: Gram -> sets -> k_nnm_coord, one pass over the
    rows; CPU: the C++ path (the oracle without the extension); beyond MAX_ROWS the mixed rows go
    through a bounded buffer (GPU) or torch (CPU)."""
    rows = prepare(gradients)
    n = rows.n
    _nnm_coord_args(n, f, rule)
    if _large(rows):
        return _finish(_large_nnm_coord(rows, f, rule), rows)
    if n > MAX_ROWS:
        X = rows.stacked()
        X = X.double() if X.dtype == torch.float64 else X.float()
        _, S = nnm_from_gram(X.double() @ X.double().T, f)
        zero = torch.zeros((), dtype=X.dtype, device=X.device)
        step = max(1, (1 << 24) // (n * n))   # the [n, n, step] member tensor stays bounded
        outs = []
        for c0 in range(0, rows.d, step):
            Y = torch.where(S[:, :, None], X[None, :, c0:c0 + step], zero).sum(1) / float(n - f)
            outs.append(_torch_coord(Y, rule, f, 0, 0, 1.0))
        return _finish(torch.cat(outs), rows)
    C = _C_for(rows)
    if rows.device.type == "cuda":
        ws = workspace(rows)
        out = torch.empty(rows.d, dtype=rows.dtype, device=rows.device)
        nnm_coord_into(C, ws, rows.obj, _gram_into(C, rows, ws), n, f, rule, out)
        return _finish(out, rows)
    if C is None:
        return ref.nnm_coord(rows.stacked(), f, rule).to(rows.out_dtype)
    _, masks = C.cpu_nnm_mix(C.cpu_pairwise(rows.obj), f)
    return _finish(C.cpu_mixed_coordwise(rows.obj, masks, n - f, rule, f), rows)   # rows.obj may be a list


# Adaptive robust clipping (ARC; docs/GAR_SEMANTICS.md): the k = 2f(n - f) // n rows of largest norm are
# scaled down to the (k + 1)-th largest norm before anything else runs. The decision needs the Gram's diagonal
# alone and clipping is linear per row: for the weighted rules the scales fold into the Gram and into the
# weights (no pass over the d-length rows); the coordinate-wise rules get the few clipped rows rewritten.

ARC_COORD_RULES = NNM_COORD_RULES


def _arc_pre(nnm: bool) -> str:
    return "arc+nnm" if nnm else "arc"


def _arc_args(n: int, f: int) -> None:
    if isinstance(f, bool) or not isinstance(f, int) or not 0 <= f < n:
        raise ValueError(f"arc: expected 0 <= f < n, got f = {f!r}, n = {n}")


def arc_scales(gradients, f: int) -> torch.Tensor:
    """The scales alone ([n] fp32 on the gradients' device): sqrt(C² / ||g_i||²) on the rows whose norm is
    above the (k + 1)-th largest, 1 elsewhere. GPU, n <= MAX_ROWS: Gram -> k_arc_scale; else vectorised
    on the Gram's diagonal (GPU) or on fp64 squared norms (CPU). Any 0 <= f < n."""
    rows = prepare(gradients)
    _arc_args(rows.n, f)
    if rows.device.type != "cuda":
        return arc_scales_from_sqnorms(_sqnorms(rows), f)
    if rows.n > MAX_ROWS:
        return arc_scales_from_sqnorms(torch.diagonal(_large_gram(rows)), f)
    C = _C_for(rows)
    ws = workspace(rows)
    scales = torch.empty(rows.n, dtype=torch.float32, device=rows.device)
    C.gpu_arc_scale(_gram_into(C, rows, ws), rows.n, f, scales, ws.get("arc_clip_rows", rows.n + 1, torch.int32))
    return scales


def arc_weights(gradients, f: int, rule: str = "krum", nnm: bool = False, **kw) -> torch.Tensor:
    """Weights over the ORIGINAL rows ([n] fp32 on the gradients' device) of ``rule`` (krum: ``m``; geomed:
    ``iters``, ``nu``; cclip: ``tau``, ``iters``, ``start`` "mean" / "krum", ``m``; dnc: ``m``, ``iters``;
    caf: ``iters``, ``max_passes``; average) applied to the adaptively clipped rows; ``nnm``: to those rows mixed
    over their n - f nearest (not dnc, caf). The weights sum to at most 1: a clipped row counts with its scale."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve(rule, rows.n, f, kw.pop("m", None), _arc_pre(nnm), kw))


def arc(gradients, f: int, rule: str = "krum", nnm: bool = False, **kw) -> torch.Tensor:
    """``rule`` after adaptive robust clipping (and mixing, with ``nnm``): Σ_j w_j g_j with the weights of
    :func:`arc_weights`; nothing is rounded to the gradients' dtype in between."""
    rows = prepare(gradients)
    return combine(rows, arc_weights(rows, f, rule, nnm, **kw))


def arc_apply_into(C, ws: Workspace, G, g: torch.Tensor, n: int, f: int, lo: int, hi: int,
                   gram_out: torch.Tensor | None = None) -> torch.Tensor:
    """Clip the device rows ``G`` (a list or an [n, ld] matrix, n <= MAX_ROWS) in place on the coordinates
    [lo, hi) from their device Gram ``g``: k_arc_scale, then k_arc_apply on the clipped rows only. Returns the
    scales; ``gram_out``: the clipped rows' Gram as well. Every buffer comes from ``ws`` (capture-safe)."""
    scales = ws.get("arc_scales", n)
    clip_rows = ws.get("arc_clip_rows", n + 1, torch.int32)
    C.gpu_arc_scale(g, n, f, scales, clip_rows, gram_out)
    C.gpu_arc_apply(G, scales, clip_rows, f, lo, hi)
    return scales


def _clipped_copy(rows: Rows, c: torch.Tensor) -> torch.Tensor:
    """A private [n, d] copy of the rows with the rows of scale != 1 as cast(c · float(x)) (torch)."""
    X = rows.stacked().clone() if isinstance(rows.obj, torch.Tensor) else rows.stacked()
    c = c.to(X.device)
    hit = (c != 1).nonzero().flatten()
    if hit.numel():
        wide = torch.float64 if X.dtype == torch.float64 else torch.float32
        X[hit] = (c[hit].to(wide)[:, None] * X[hit].to(wide)).to(X.dtype)
    return X


def arc_coord(gradients, f: int, rule: str = "trimmed-mean", nnm: bool = False) -> torch.Tensor:
    """``rule`` ("trimmed-mean" with the same ``f``, or "median") over the adaptively clipped rows, in the
    gradients' dtype; ``nnm``: over those rows mixed over their n - f nearest (the sets from the clipped
    rows' Gram). The clipped rows are written as cast(c · float(x)) on a private copy: the inputs are never
    modified. GPU, n <= MAX_ROWS: Gram -> k_arc_scale -> k_arc_apply on the copy -> the plain rule (or
    k_nnm_coord); elsewhere the copy is clipped with torch."""
    rows = prepare(gradients)
    n = rows.n
    _arc_args(n, f)
    if nnm:
        _nnm_coord_args(n, f, rule)
    elif rule not in ARC_COORD_RULES:
        raise ValueError(f"arc: unsupported coordinate-wise rule {rule!r}; available: {ARC_COORD_RULES}")
    plain = resolve_coord(rule, n, f)   # the rule's own requirement (trimmed-mean: 2f < n)
    if arc_count(n, f) == 0:            # f = 0: the path without ARC, bit for bit
        return nnm_coord(rows, f, rule) if nnm else _coord(rows, plain)
    C = _C_for(rows)
    if rows.device.type == "cuda" and n <= MAX_ROWS:
        ws = workspace(rows)
        g = _gram_into(C, rows, ws)
        Y = _padded_copy(rows.stacked())
        np_ = C.gram_padded(n)
        g2 = ws.get("arc_gram", np_ * np_) if nnm else None
        arc_apply_into(C, ws, Y, g, n, f, 0, rows.d, g2)
        out = torch.empty(rows.d, dtype=rows.dtype, device=rows.device)
        if nnm:
            nnm_coord_into(C, ws, Y, g2, n, f, rule, out)
        else:
            plain.into(C, Y, out)
        return _finish(out, rows)
    if rows.device.type == "cuda":      # beyond MAX_ROWS: the large kernels on the clipped copy
        Y = _clipped_copy(rows, arc_scales_from_sqnorms(torch.diagonal(_large_gram(rows)), f))
        if nnm:
            return nnm_coord(replace(rows, obj=Y), f, rule)
        if Y.dtype == torch.float16:
            # gar_large.hip's radix select keys 16-bit rows by their top 16 bits, which is all of a bf16 but
            # cuts an fp16's last 3 mantissa bits: the clipped fp16 values go in widened (exactly) instead
            return _coord(replace(rows, obj=Y.float(), dtype=torch.float32), plain)
        return _coord(replace(rows, obj=Y), plain)
    s = _sqnorms(rows)
    c = arc_scales_from_sqnorms(s, f)
    Y = _clipped_copy(rows, c)
    if not nnm:
        return _coord(replace(rows, obj=Y), plain)
    D = distances_from_gram(gram(rows)) if C is None or n > MAX_ROWS else C.cpu_pairwise(rows.obj)
    return _finish(nnm_coord_from_distances(C, Y, arc_distances(D, s, c), f, rule), rows)


def bulyan_weights(gradients, f: int, m: int | None = None) -> torch.Tensor:
    rows = prepare(gradients)
    return selection_weights(rows, resolve("bulyan", rows.n, f, m))


def bulyan_sizes(n: int, f: int) -> tuple:
    """(t, beta) of Bulyan over n rows: t = n - 2f - 2 selection rounds, then per coordinate the mean of
    the beta = t - 2f selection means closest to their median."""
    t = n - 2 * f - 2
    return t, t - 2 * f


def bulyan_tail_into(C, rows, W: torch.Tensor, n: int, f: int, out: torch.Tensor, jobs=None) -> torch.Tensor:
    """``out`` = Bulyan's tail over device rows (n <= MAX_ROWS) with the selection weights ``W`` [t, n]; with
    a job table ``jobs`` the segmented tail (gar_layerwise.hip), each job with its segment's W of [L, t, n]."""
    t, beta = bulyan_sizes(n, f)
    if jobs is not None:
        C.gpu_lw_bulyan_tail(rows, jobs, W, t, beta, out)
    else:
        C.gpu_coordwise(rows, _MODE["bulyan-tail"], f, beta, W.reshape(-1), t, 0, 1.0, out)
    return out


def bulyan_tail_large(V: torch.Tensor, n: int, f: int, out: torch.Tensor) -> torch.Tensor:
    """``out`` = Bulyan's tail of the selection means ``V`` = W·X [t, d'] (fp32, GPU): their averaged median."""
    _native.native().gpu_large_coord(V, _LARGE_MODE["averaged-median"], 0, bulyan_sizes(n, f)[1], out)
    return out


def bulyan_tail_host(C, X: torch.Tensor, W: torch.Tensor, n: int, f: int) -> torch.Tensor:
    """Bulyan's tail over CPU rows ``X`` [n, d'] with ``W`` [t, n]: the C++ function, else torch."""
    t, beta = bulyan_sizes(n, f)
    if C is not None:
        return C.cpu_coordwise(X, _MODE["bulyan-tail"], f, beta, W.reshape(-1), t, 0, 1.0)
    return _torch_closest_mean(W @ X, beta)


def bulyan(gradients, f: int, m: int | None = None, **_) -> torch.Tensor:
    rows = prepare(gradients)
    n = rows.n
    m = n - f - 2 if m is None else m
    t, beta = bulyan_sizes(n, f)
    W = bulyan_weights(rows, f, m)
    if _large(rows):   # V = W·X column chunk by chunk (bounded fp32 memory), then the radix-select tail
        X, Wd = _matrix(rows), W.to(rows.device, torch.float32)
        out = torch.empty(rows.d, dtype=torch.float32, device=rows.device)
        step = max(1, (1 << 28) // (4 * max(n, t)))
        Vbuf = torch.empty((t, min(step, rows.d)), dtype=torch.float32, device=rows.device)
        for c0 in range(0, rows.d, step):
            w = min(step, rows.d - c0)
            bulyan_tail_large(large_wx(Wd, X[:, c0:c0 + w], Vbuf[:, :w]), n, f, out[c0:c0 + w])
        return _finish(out, rows)
    if n > MAX_ROWS:
        V = W.to(rows.device) @ rows.stacked().float()
        return _finish(_torch_closest_mean(V, beta), rows)
    C = _C_for(rows)
    if rows.device.type == "cuda":
        out = torch.empty(rows.d, dtype=rows.dtype, device=rows.device)
        return _finish(bulyan_tail_into(C, rows.obj, W, n, f, out), rows)
    if C is None:
        return ref.bulyan(rows.stacked(), f, m).to(rows.out_dtype)
    return _finish(bulyan_tail_host(C, rows.obj, W, n, f), rows)


# --------------------------------------------------------------------------- #
# The resolved coordinate-wise rule


@dataclass(frozen=True, eq=False)
class CoordRule:
    """A coordinate-wise rule with its kernel arguments resolved for ``n`` rows (see :func:`resolve_coord`).
    An argument the rule does not read is passed as the kernels' neutral value. Condense's seed is an
    argument of each run (it changes every step), not of the rule."""

    rule: str
    n: int
    mode: int                  # the mode code of gpu_coordwise / cpu_coordwise
    large_mode: int | None     # that of gpu_large_coord; None: the rule has no large form
    f: int                     # trimmed-mean: values cut at each end
    beta: int                  # averaged-median: values averaged around the median
    p: float                   # condense: probability of keeping the median
    takes_seed: bool           # condense
    kw: dict                   # the rule's keyword arguments for :func:`aggregate`, the seed aside

    def into(self, C, rows, out: torch.Tensor, seed: int = 0) -> torch.Tensor:
        """``out`` (fp32 or the rows' dtype) = the rule over device rows (n <= MAX_ROWS), one launch."""
        C.gpu_coordwise(rows, self.mode, self.f, self.beta, None, 0, seed if self.takes_seed else 0, self.p, out)
        return out

    def large_into(self, X: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """``out`` = the rule over a GPU [n, d'] matrix of up to LARGE_ROWS rows (gar_large.hip)."""
        _native.native().gpu_large_coord(X, self.large_mode, self.f, self.beta, out)
        return out

    def kwargs(self, seed: int = 0) -> dict:
        """The keyword arguments with which ``aggregate(rule, ...)`` runs the rule (a seed among its own wins)."""
        return {"seed": seed, **self.kw} if self.takes_seed else self.kw


def resolve_coord(rule: str, n: int, f: int = 0, gar_kwargs: dict | None = None) -> CoordRule:
    """The :class:`CoordRule` of ``rule`` over ``n`` rows: defaults applied, arguments validated (ValueError).
    ``gar_kwargs``: the rule's own keyword arguments (``beta``, ``p``, ``seed``); others only travel in ``kw``."""
    if rule not in _MODE or rule == "bulyan-tail":
        raise ValueError(rule)
    kw = dict(gar_kwargs or {})
    if rule not in ("median", "average-nan"):
        kw["f"] = f
    beta = (kw.get("beta") or n - f) if rule == "averaged-median" else 0
    if rule == "trimmed-mean" and not 0 <= 2 * f < n:
        raise ValueError(f"trimmed-mean: expected 0 <= 2f < n, got n = {n}, f = {f}")
    if rule == "averaged-median" and not 1 <= beta <= n:
        raise ValueError(f"averaged-median: expected 1 <= beta <= n, got beta = {beta}, n = {n}")
    condense = rule == "condense"
    return CoordRule(rule, n, _MODE[rule], _LARGE_MODE.get(rule), f if rule == "trimmed-mean" else 0, beta,
                     float(kw.get("p", 0.9)) if condense else 1.0, condense, kw)


def _coord(rows: Rows, cr: CoordRule, seed: int = 0) -> torch.Tensor:
    if _large(rows) and cr.large_mode is not None:
        X = _matrix(rows)
        return _finish(cr.large_into(X, torch.empty(rows.d, dtype=X.dtype, device=X.device)), rows)
    if rows.n > MAX_ROWS:
        return _finish(_torch_coord(rows.stacked().float(), cr.rule, cr.f, cr.beta, seed, cr.p), rows)
    C = _C_for(rows)
    if rows.device.type == "cuda":
        return _finish(cr.into(C, rows.obj, torch.empty(rows.d, dtype=rows.dtype, device=rows.device), seed), rows)
    if C is None:
        X = rows.stacked()
        r = {"median": lambda: ref.median(X), "trimmed-mean": lambda: ref.trimmed_mean(X, cr.f),
             "averaged-median": lambda: ref.averaged_median(X, cr.beta), "average-nan": lambda: ref.average_nan(X),
             "condense": lambda: ref.condense(X, cr.p, seed)}[cr.rule]()
        return r.to(rows.out_dtype)
    return _finish(C.cpu_coordwise(rows.obj, cr.mode, cr.f, cr.beta, None, 0, seed, cr.p), rows)


def median(gradients, **_) -> torch.Tensor:
    rows = prepare(gradients)
    return _coord(rows, resolve_coord("median", rows.n))


def trimmed_mean(gradients, f: int, **_) -> torch.Tensor:
    rows = prepare(gradients)
    return _coord(rows, resolve_coord("trimmed-mean", rows.n, f))


def averaged_median(gradients, f: int = 0, beta: int | None = None, **_) -> torch.Tensor:
    rows = prepare(gradients)
    return _coord(rows, resolve_coord("averaged-median", rows.n, f, {"beta": beta}))


def average_nan(gradients, **_) -> torch.Tensor:
    rows = prepare(gradients)
    return _coord(rows, resolve_coord("average-nan", rows.n))


def condense(gradients, p: float = 0.9, seed: int | None = None, **_) -> torch.Tensor:
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,)).item())
    rows = prepare(gradients)
    return _coord(rows, resolve_coord("condense", rows.n, gar_kwargs={"p": p}), seed)


def brute_weights(gradients, f: int) -> torch.Tensor:
    rows = prepare(gradients)
    return selection_weights(rows, resolve("brute", rows.n, f))


def brute(gradients, f: int, **_) -> torch.Tensor:
    rows = prepare(gradients)
    return combine(rows, brute_weights(rows, f))


# SMEA, smallest maximum eigenvalue averaging (docs/GAR_SEMANTICS.md): Brute's subset search with every
# (n - f)-subset scored by the top eigenvalue of its members' covariance, which power rounds on the subset's
# block of the Gram's distances give without touching the d-length rows.


def smea_weights(gradients, f: int, iters: int = 16, pre: str | None = None) -> torch.Tensor:
    """Weights of SMEA ([n] fp32 on the gradients' device): 1 / (n - f) on the members of the (n - f)-subset
    whose empirical covariance has the smallest top eigenvalue (``iters`` power rounds per subset on the
    pairwise distances alone, ties to the lowest rank in Brute's order), 0 elsewhere. ``pre`` is refused:
    no pre-aggregation runs in front of SMEA yet."""
    rows = prepare(gradients)
    return selection_weights(rows, resolve("smea", rows.n, f, None, pre, {"iters": iters}))


def smea(gradients, f: int = 0, iters: int = 16, **_) -> torch.Tensor:
    """SMEA (Allouah et al., ICML 2023): the mean of the subset chosen by :func:`smea_weights`."""
    rows = prepare(gradients)
    return combine(rows, smea_weights(rows, f, iters))


def aksel_count(n: int, f: int, mode: str = "mid") -> int:
    """The rows Aksel keeps: the closer half (``mode`` "mid"), else all but f."""
    return (n + 1) // 2 if mode == "mid" else n - f


def aksel_weights_from_distances(D: torch.Tensor, c: int) -> torch.Tensor:
    """Aksel's weights ([..., n] fp32 on D's device) from the squared distances to the median ``D`` [..., n]:
    1 / c on the c closest rows, ties by index, a non-finite distance counting as +inf."""
    D = torch.where(torch.isfinite(D), D, torch.full_like(D, math.inf))
    idx = torch.sort(D, dim=-1, stable=True).indices[..., :c]
    return torch.zeros(D.shape, dtype=torch.float32, device=D.device).scatter_(-1, idx, 1.0 / c)


def aksel_sqdist_slabs(C, ws: Workspace, median: CoordRule, rows, d: int) -> torch.Tensor:
    """[grid, n] partial squared distances of the device rows (n <= MAX_ROWS, length d) to their coordinate-wise
    median (``median``: the resolved rule): its launch, then gpu_sqdist. Additive over coordinate blocks."""
    med = median.into(C, rows, ws.get("aksel_med", d))
    grid = C.sqdist_grid(d)
    slabs = ws.get("aksel_slabs", grid * median.n)
    C.gpu_sqdist(rows, med, slabs)
    return slabs.view(grid, median.n)


def aksel_weights(gradients, f: int, mode: str = "mid") -> torch.Tensor:
    rows = prepare(gradients)
    c = aksel_count(rows.n, f, mode)
    C = _C_for(rows)
    if rows.device.type == "cuda" and rows.n <= MAX_ROWS:
        ws = workspace(rows)
        w = ws.get("weights", rows.n)
        slabs = aksel_sqdist_slabs(C, ws, resolve_coord("median", rows.n), rows.obj, rows.d)
        C.gpu_aksel_select(slabs.view(-1), rows.n, c, w, ws.get("aksel_dists", rows.n))
        return w
    if C is None or rows.n > MAX_ROWS:
        X = rows.stacked().double()
        med = _torch_coord(X, "median", 0, 0, 0, 1.0) if rows.n > MAX_ROWS else ref.median(X)
        dist = ((X - med.to(X.device)) ** 2).sum(1).cpu()
        return aksel_weights_from_distances(dist, c).to(rows.device)
    med = C.cpu_coordwise(rows.obj, _MODE["median"], 0, 0, None, 0, 0, 1.0)
    return C.cpu_aksel_weights(C.cpu_sqdist(rows.obj, med), c)


def aksel(gradients, f: int, mode: str = "mid", **_) -> torch.Tensor:
    rows = prepare(gradients)
    return combine(rows, aksel_weights(rows, f, mode))


# --------------------------------------------------------------------------- #
# Vectorised PyTorch implementations for n > MAX_ROWS (same semantics).


def large_gram(X: torch.Tensor) -> torch.Tensor:
    """fp32 Gram matrix [n, n] of a GPU [n, d] matrix of up to LARGE_ROWS rows on the MFMA kernel of
    gar_large.hip (split-K 64 x 64 tiles, fixed-order sums; no library GEMM)."""
    C = _native.native()
    if X.stride(1) != 1 or (X.stride(0) * X.element_size()) % 16 or X.data_ptr() % 16:
        X = X.contiguous()
        if (X.shape[1] * X.element_size()) % 16:   # pad the rows to 16 bytes (zeros add nothing)
            X = torch.nn.functional.pad(X, (0, (-X.shape[1]) % (16 // X.element_size())))
    n, d = X.shape
    slabs = torch.empty(max(C.large_gram_slab_floats(n, d, X), 1), dtype=torch.float32, device=X.device)
    g = torch.empty((n, n), dtype=torch.float32, device=X.device)
    C.gpu_large_gram(X, slabs, g)
    return g


def large_wx(W: torch.Tensor, X: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """V [t, d] = W [t, n] · X [n, d] in fp32 on the MFMA kernel of gar_large.hip."""
    if X.stride(1) != 1:
        X = X.contiguous()
    V = out if out is not None else torch.empty((W.shape[0], X.shape[1]), dtype=torch.float32, device=X.device)
    _native.native().gpu_large_wx(W.contiguous(), X, V)
    return V


def _large_gram(rows: Rows) -> torch.Tensor:
    """fp32 Gram matrix of a large set: the MFMA kernel on the GPU, fp32 matmul on the CPU."""
    if rows.device.type == "cuda":
        return large_gram(_matrix(rows))
    X = rows.stacked().float()
    return X @ X.T


def _torch_closest_mean(V: torch.Tensor, beta: int) -> torch.Tensor:
    V = torch.sort(_nan_inf(V), dim=0).values
    med = V[V.shape[0] // 2]
    key = _nan_inf((V - med).abs())
    # (key, value) order: stable sort by value first, then by key
    idx = torch.sort(key, dim=0, stable=True).indices
    return torch.gather(V, 0, idx[:beta]).sum(0) / beta


def _torch_coord(X: torch.Tensor, mode: str, f: int, beta: int, seed: int, p: float) -> torch.Tensor:
    n = X.shape[0]
    if mode == "average-nan":
        fin = torch.isfinite(X)
        cnt = fin.sum(0)
        return torch.where(cnt > 0, torch.where(fin, X, 0).sum(0) / cnt.clamp(min=1), torch.zeros_like(X[0]))
    if mode in ("median", "condense"):
        fin = torch.isfinite(X)
        cnt = fin.sum(0)
        S = torch.sort(torch.where(fin, X, torch.full_like(X, math.inf)), dim=0).values
        med = torch.gather(S, 0, (cnt // 2).clamp(max=n - 1)[None]).squeeze(0)
        med = torch.where(cnt > 0, med, torch.zeros_like(med))
        if mode == "condense":
            thr = ref.bernoulli_threshold(p)
            keep = torch.tensor([ref.mix_hash(seed, x) < thr for x in range(X.shape[1])], device=X.device)
            med = torch.where(keep, med, X[0])
        return med
    if mode == "trimmed-mean":
        S = torch.sort(_nan_inf(X), dim=0).values
        return S[f:n - f].sum(0) / (n - 2 * f)
    if mode == "averaged-median":
        return _torch_closest_mean(X, beta)
    raise ValueError(mode)


# --------------------------------------------------------------------------- #

RULES = {
    "average": average,
    "median": median,
    "krum": krum,
    "bulyan": bulyan,
    "brute": brute,
    "aksel": aksel,
    "geomed": geomed,
    "cclip": cclip,
    "dnc": dnc,
    "caf": caf,
    "smea": smea,
    "nnm-cclip": lambda gradients, f=0, tau=None, iters=3, start="mean", m=None, **_: nnm(
        gradients, f, "cclip", tau=tau, iters=iters, start=start, m=m),
    "nnm-krum": lambda gradients, f, m=None, **_: nnm(gradients, f, "krum", m=m),
    "nnm-geomed": lambda gradients, f=0, iters=32, nu=1e-6, **_: nnm(gradients, f, "geomed", iters=iters, nu=nu),
    "nnm-average": lambda gradients, f=0, **_: nnm(gradients, f, "average"),
    "nnm-trimmed-mean": lambda gradients, f, **_: nnm_coord(gradients, f, "trimmed-mean"),
    "nnm-median": lambda gradients, f=0, **_: nnm_coord(gradients, f, "median"),
    "arc-krum": lambda gradients, f, m=None, **_: arc(gradients, f, "krum", m=m),
    "arc-geomed": lambda gradients, f=0, iters=32, nu=1e-6, **_: arc(gradients, f, "geomed", iters=iters, nu=nu),
    "arc-cclip": lambda gradients, f=0, tau=None, iters=3, start="mean", m=None, **_: arc(
        gradients, f, "cclip", tau=tau, iters=iters, start=start, m=m),
    "arc-dnc": lambda gradients, f=0, m=None, iters=16, **_: arc(gradients, f, "dnc", m=m, iters=iters),
    "arc-caf": lambda gradients, f=0, iters=16, max_passes=None, **_: arc(gradients, f, "caf", iters=iters,
                                                                          max_passes=max_passes),
    "arc-average": lambda gradients, f=0, **_: arc(gradients, f, "average"),
    "arc-nnm-krum": lambda gradients, f, m=None, **_: arc(gradients, f, "krum", True, m=m),
    "arc-nnm-geomed": lambda gradients, f=0, iters=32, nu=1e-6, **_: arc(gradients, f, "geomed", True, iters=iters,
                                                                         nu=nu),
    "arc-nnm-cclip": lambda gradients, f=0, tau=None, iters=3, start="mean", m=None, **_: arc(
        gradients, f, "cclip", True, tau=tau, iters=iters, start=start, m=m),
    "arc-nnm-average": lambda gradients, f=0, **_: arc(gradients, f, "average", True),
    "arc-trimmed-mean": lambda gradients, f, **_: arc_coord(gradients, f, "trimmed-mean"),
    "arc-median": lambda gradients, f=0, **_: arc_coord(gradients, f, "median"),
    "arc-nnm-trimmed-mean": lambda gradients, f, **_: arc_coord(gradients, f, "trimmed-mean", True),
    "arc-nnm-median": lambda gradients, f=0, **_: arc_coord(gradients, f, "median", True),
    "condense": condense,
    "trimmed-mean": trimmed_mean,
    "averaged-median": averaged_median,
    "average-nan": average_nan,
}


def aggregate(rule: str, gradients, **kwargs) -> torch.Tensor:
    """Apply the named rule (see RULES) to the gradient set."""
    try:
        fn = RULES[rule]
    except KeyError:
        raise KeyError(f"unknown aggregation rule {rule!r}; available: {sorted(RULES)}") from None
    return fn(gradients, **kwargs)
