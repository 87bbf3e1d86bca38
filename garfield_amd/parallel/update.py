"""What the redundant (``engine.py``) and the sharded (``sharded.py``) aggregate-and-update step share: the SGD
update of a slice of the master weights, and the job tables of the layer-wise (segmented) kernels.

A *target* is ``(param, mom, shadow)``: the slice of the fp32 master weights to update, its momentum buffer, and
the working-weight copy the same pass refreshes (None: no copy; of a longer one the first ``param.numel()``
elements are written). The engine's target is its whole vector, the sharded aggregator's one bucket's owned shard.
"""
from __future__ import annotations

import torch

LW_JOB = 32768   # coordinates per job of the segmented kernels (a multiple of 64)


class SgdUpdate:
    """SGD with momentum, dampening, weight decay and Nesterov (torch.optim.SGD's update rule), with the
    hyper-parameters of an ``EngineConfig`` read at every call (``set_lr``). On a device the update is fused
    into the combine kernels (``C``: the extension); without one (``C`` None) it is :meth:`host`.
    ``first``: the first step, when the momentum buffer takes the gradient as it is."""

    def __init__(self, cfg, C, device):
        self.cfg, self.C = cfg, C
        self.one = torch.ones(1, dtype=torch.float32, device=device)   # the weight of an aggregate that is one vector

    def _args(self, first: bool) -> tuple:
        cfg = self.cfg
        return cfg.lr, cfg.momentum, cfg.dampening, cfg.weight_decay, cfg.nesterov, first

    def from_rows(self, rows, w: torch.Tensor, target, first: bool) -> None:
        """The update from Σ_j w_j rows_j (rows: [n, d] or a list of n vectors), one launch."""
        p, mom, shadow = target
        self.C.gpu_combine_sgd(rows, w, p, mom, None, shadow, *self._args(first))

    def from_vector(self, g: torch.Tensor, target, first: bool) -> None:
        """The update from the aggregate ``g`` itself."""
        if self.C is None:
            return self.host(g, target, first)
        self.from_rows([g], self.one, target, first)

    def segmented(self, rows, jobs: torch.Tensor, seg_off: torch.Tensor, base: int, w: torch.Tensor, target,
                  first: bool) -> None:
        """The update from each segment's own combine Σ_j w[s, j] rows_j (``jobs``, ``seg_off``: the tables of
        :func:`lw_device_tables`; ``base``: the global coordinate of the rows' coordinate 0), one launch."""
        p, mom, shadow = target
        self.C.gpu_lw_combine_sgd(rows, jobs, seg_off, base, w, p, mom, shadow, *self._args(first))

    def host(self, g: torch.Tensor, target, first: bool) -> None:
        """The update in torch. Elementwise, so applying it slice by slice equals applying it at once."""
        lr, momentum, dampening, weight_decay, nesterov, _ = self._args(first)
        p, buf, shadow = target
        with torch.no_grad():
            if weight_decay:
                g = g + weight_decay * p
            if momentum:
                if first:
                    buf.copy_(g)
                else:
                    buf.mul_(momentum).add_(g, alpha=1 - dampening)
                g = g + momentum * buf if nesterov else buf
            p.add_(g, alpha=-lr)
            if shadow is not None:
                shadow[: p.numel()].copy_(p)


# --------------------------------------------------------------------------- #
# Job tables of the layer-wise kernels (gar_layerwise.hip)


def lw_job_ranges(x0: int, x1: int, origin: int = 0) -> list:
    """[x0, x1) cut at the multiples of LW_JOB of the global coordinate (``origin``: the global
    coordinate of local 0): every job boundary inside a segment is then a multiple of 64 whatever the
    sharding, so the layer-wise tail's MFMA / exact split of the coordinates is sharding-invariant."""
    out, a = [], x0
    while a < x1:
        e = min(((a + origin) // LW_JOB + 1) * LW_JOB - origin, x1)
        out.append((a, e))
        a = e
    return out


def lw_jobs(segs: list, o0: int, o1: int, local: int = 0) -> tuple:
    """``(jobs, seg_lo)`` of the owned coordinates [o0, o1) under the segments ``segs`` (sorted
    ``(offset, numel)``): every segment's piece of the range cut by :func:`lw_job_ranges` into jobs
    ``(begin, end, segment)`` in local coordinates (``local``: that of o0), and ``seg_lo[s]`` the first job
    of segment s (``seg_lo[L]``: the job count). The unsharded engine owns [0, d), a shard its bucket slice."""
    jobs, seg_lo = [], [0]
    for s, (off, numel) in enumerate(segs):
        x0, x1 = max(off, o0), min(off + numel, o1)
        jobs.extend((a - o0 + local, e - o0 + local, s) for a, e in lw_job_ranges(x0, x1))
        seg_lo.append(len(jobs))
    return jobs, seg_lo


def lw_device_tables(C, n: int, L: int, jobs: list, seg_lo: list, device) -> dict:
    """What the segmented kernels take for one owned range of n rows: ``J`` jobs as an int64 [J, 3] tensor,
    ``seg_lo``, the Gram slabs and the [L, np, np] Gram buffer. A range that meets no segment (J == 0: a
    shard of padding) keeps a one-row placeholder table and its launches are skipped by the caller."""
    J, np_ = len(jobs), C.gram_padded(n)
    return dict(J=J,
                jobs=torch.tensor(jobs if jobs else [(0, 0, 0)], dtype=torch.int64, device=device),
                seg_lo=torch.tensor(seg_lo, dtype=torch.int32, device=device),
                slabs=torch.empty(max(J, 1) * C.gram_slab_floats(n), dtype=torch.float32, device=device),
                gram=torch.empty(L * np_ * np_, dtype=torch.float32, device=device))
