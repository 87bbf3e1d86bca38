"""Worker-side momentum: every logical worker sends its momentum, not its gradient.

The rules of "Learning from History" (Karimireddy, He, Jaggi 2021: centered clipping) and "Fixing by
Mixing" (Allouah et al. 2023: nearest-neighbour mixing) are robust to time-coupled attacks when each
worker i sends m_i, an average of its gradients over the steps, which shrinks the honest variance
those attacks hide in. ``update`` is that step on the exchange rows, in place, before any simulated
attack and before the rule (docs/GAR_SEMANTICS.md "Worker momentum"; the fp64 specification:
``ops.reference.worker_momentum``):

    first step:   m <- g                 later steps:   m <- fmaf(beta, m, omega * g)
    row <- m rounded to nearest even into the row's dtype

with g the row widened to fp32 and omega = 1 - beta rounded once to fp32. A non-finite g stays in the
row and leaves the state unchanged.

GPU rows run on ``worker_mom.hip`` (one streaming pass, mandatory: no PyTorch fallback on the GPU), CPU
rows on the C++ thread pool with the same ``fmaf`` formula (bit-equal state); without an extension the
CPU uses PyTorch, whose unfused ``beta * m + omega * g`` may differ from the fused form by one rounding.
"""
from __future__ import annotations

import struct

import torch

from garfield_amd import _native

DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def omega_of(beta: float) -> float:
    """1 - beta rounded once to fp32 (the kernels take it as a float argument)."""
    return struct.unpack("f", struct.pack("f", 1.0 - float(beta)))[0]


def _check(X: torch.Tensor, M: torch.Tensor, beta: float, lo: int, hi: int) -> None:
    if X.dim() != 2 or M.dim() != 2 or X.shape[0] != M.shape[0] or X.shape[0] < 1:
        raise ValueError(f"worker momentum: rows [k, >= hi] and state [k, ld] with the same k, got "
                         f"{tuple(X.shape)} and {tuple(M.shape)}")
    if X.dtype not in DTYPES:
        raise ValueError(f"worker momentum: fp32, bf16 or fp16 rows, got {X.dtype}")
    if M.dtype != torch.float32 or not M.is_contiguous():
        raise ValueError("worker momentum: the state must be contiguous fp32")
    if X.device != M.device:
        raise ValueError("worker momentum: rows and state must be on the same device")
    if X.shape[1] and X.stride(1) != 1:
        raise ValueError("worker momentum: the rows must have unit element stride")
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"worker momentum: 0 <= beta < 1, got {beta}")
    if not (0 <= lo <= hi <= X.shape[1] and hi <= M.shape[1]):
        raise ValueError(f"worker momentum: 0 <= lo <= hi <= row length, got [{lo}, {hi}) on rows of "
                         f"{X.shape[1]} and a state of {M.shape[1]}")


def update_torch(X: torch.Tensor, M: torch.Tensor, beta: float, first: bool, lo: int = 0, hi: int | None = None) -> None:
    """``update`` in plain PyTorch (CPU without an extension): the product and the sum are rounded
    separately, so the state may differ from the fused form by one rounding."""
    hi = X.shape[1] if hi is None else int(hi)
    _check(X, M, float(beta), int(lo), hi)
    if hi <= lo:
        return
    with torch.no_grad():
        row, m = X[:, lo:hi], M[:, lo:hi]
        g = row.float()
        ok = torch.isfinite(g)
        if first:
            new = g
        else:
            new = float(beta) * m + omega_of(beta) * g   # fp32 scalars: both products round to fp32
        new = torch.where(ok, new, m)
        m.copy_(new)
        row.copy_(torch.where(ok, new.to(row.dtype), row))


def update(X_rows: torch.Tensor, M: torch.Tensor, beta: float, first: bool, lo: int = 0, hi: int | None = None) -> None:
    """Worker momentum in place on coordinates [lo, hi) of the k rows ``X_rows`` [k, >= hi] (a view of
    the exchange buffer: any row stride, fp32 / bf16 / fp16) with the fp32 state ``M`` [k, ld].
    Asynchronous on the current stream on the GPU; nothing outside [lo, hi) is read or written."""
    hi = X_rows.shape[1] if hi is None else int(hi)
    lo, beta = int(lo), float(beta)
    _check(X_rows, M, beta, lo, hi)
    if hi <= lo:
        return
    C = _native.require_for(X_rows.device)
    if X_rows.is_cuda:
        C.gpu_worker_momentum(X_rows, M, lo, hi, beta, bool(first))
    elif C is not None:
        C.cpu_worker_momentum(X_rows, M, lo, hi, beta, bool(first))
    else:
        update_torch(X_rows, M, beta, first, lo, hi)
