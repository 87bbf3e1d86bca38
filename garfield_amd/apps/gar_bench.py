"""GAR micro-benchmark: latency and achieved bandwidth of every rule.

Reference: ``pytorch_impl/applications/benchmarks/gar_bench.py:41-89`` (one
wall-clock call per GAR on ``torch.rand(d)`` CUDA tensors, sweeping n, d and f,
bulyan skipped for n > 23). Here each rule is timed with HIP events over several
back-to-back calls on an ``[n, d]`` gradient buffer (the engine's exchange
layout), optionally also from a list of separate tensors, and the effective
bandwidth (gradient bytes read / time) is reported next to the ~6.3 TB/s HBM3E
streaming ceiling of one MI355X.

Usage::

    python -m garfield_amd.apps.gar_bench --n 8 16 32 64 --d 23528522 --dtype bf16
"""
from __future__ import annotations

import argparse
import json
import time

import torch

from garfield_amd.ops import gar

RULES = ["average", "krum", "bulyan", "median", "trimmed-mean", "averaged-median", "aksel", "brute", "condense",
         "average-nan", "geomed", "nnm-krum", "nnm-geomed", "nnm-average", "cclip", "cclip-krum", "nnm-cclip",
         "nnm-trimmed-mean", "nnm-median", "dnc", "caf", "smea",
         "arc-krum", "arc-geomed", "arc-cclip", "arc-dnc", "arc-caf", "arc-average", "arc-nnm-krum", "arc-nnm-geomed",
         "arc-nnm-cclip", "arc-nnm-average", "arc-trimmed-mean", "arc-median", "arc-nnm-trimmed-mean", "arc-nnm-median"]
# "cclip-krum": centered clipping from the Multi-Krum start (start="krum"), Krum's f


def default_f(rule: str, n: int) -> int | None:
    if rule.startswith("arc-"):   # adaptive robust clipping in front: the f of what it stands in front of
        rule = rule[4:] if rule.startswith("arc-nnm-") else "nnm-" + rule[4:]
    if rule.startswith("nnm-"):   # the f of the plain rule (average: as geomed, median: as the trimmed mean:
        # the plain median takes no f, the mixing and the clipping need one), so the pair is comparable
        rule = {"nnm-average": "geomed", "nnm-median": "trimmed-mean"}.get(rule, rule[4:])
    if rule == "cclip-krum":
        rule = "krum"
    if rule in ("average", "average-nan", "median"):
        return None
    if rule == "bulyan":
        f = (n - 3) // 4
    elif rule == "krum":
        f = (n - 3) // 2
    elif rule == "condense":
        f = (n - 2) // 2
    else:
        f = (n - 1) // 2
    f = min(f, 2) if rule != "bulyan" else min(f, 3)
    return f if f >= 1 else None


def bench_rule(rule, G, f, iters, warmup):
    kw = {} if f is None else {"f": f}
    if rule == "averaged-median":
        kw = {"f": f or 0}
    if rule == "cclip-krum":
        rule, kw = "cclip", dict(kw, start="krum")
    for _ in range(warmup):
        gar.aggregate(rule, G, **kw)
    dev = G.device if isinstance(G, torch.Tensor) else G[0].device
    if dev.type == "cuda":
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(iters):
            gar.aggregate(rule, G, **kw)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters
    t0 = time.perf_counter()
    for _ in range(iters):
        gar.aggregate(rule, G, **kw)
    return 1000 * (time.perf_counter() - t0) / iters


def bench_worker_momentum(k: int, d: int, dt, beta: float, device, iters: int, warmup: int) -> dict:
    """The worker-momentum pass alone (``ops.worker_momentum.update``, later-step form) on k exchange rows
    of d coordinates: ms per call and the bytes it moves (row read + written, fp32 state read + written)."""
    from garfield_amd.ops import worker_momentum

    ld = ((d + 63) // 64) * 64
    X = torch.randn(k, ld, device=device, dtype=dt)
    M = torch.randn(k, ld, device=device, dtype=torch.float32)

    def run(times):
        for _ in range(times):
            worker_momentum.update(X, M, beta, False, 0, d)

    run(warmup)
    if X.is_cuda:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        run(iters)
        e.record()
        torch.cuda.synchronize()
        ms = s.elapsed_time(e) / iters
    else:
        t0 = time.perf_counter()
        run(iters)
        ms = 1000 * (time.perf_counter() - t0) / iters
    nbytes = k * d * (2 * X.element_size() + 8)
    return {"op": "worker_momentum", "k": k, "d": d, "beta": beta, "ms": round(ms, 4), "bytes": nbytes,
            "GBps": round(nbytes / ms / 1e6, 1)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, nargs="+", default=[8, 16, 32, 64])
    p.add_argument("--d", type=int, nargs="+", default=[11173962, 23528522])
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp16"])
    p.add_argument("--rules", nargs="+", default=RULES)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    p.add_argument("--list-input", action="store_true", help="pass a list of n tensors instead of [n, d]")
    p.add_argument("--f", type=int, default=None,
                   help="the f of every rule that takes one, instead of the sweep's default (at most 2, 3 for bulyan); "
                        "also lifts the sweep's n <= 20 limit on the subset searches brute and smea")
    p.add_argument("--worker_momentum", type=float, default=None, metavar="BETA",
                   help="time the worker-momentum pass alone instead of the rules, on --n rows (as k) of --d coordinates")
    a = p.parse_args(argv)
    dt = {"bf16": torch.bfloat16, "fp32": torch.float32, "fp16": torch.float16}[a.dtype]
    if a.worker_momentum is not None:
        for d in a.d:
            for n in a.n:
                res = bench_worker_momentum(n, d, dt, a.worker_momentum, a.device, a.iters, a.warmup)
                print(json.dumps(dict(res, dtype=a.dtype)), flush=True)
        return
    for d in a.d:
        for n in a.n:
            ld = ((d + 63) // 64) * 64
            G = torch.randn(n, ld, device=a.device, dtype=dt)[:, :d]
            inp = [G[i].clone() for i in range(n)] if a.list_input else G
            for rule in a.rules:
                f = default_f(rule, n)
                if a.f is not None and f is not None:
                    f = a.f
                if rule in ("krum", "nnm-krum", "cclip-krum", "bulyan", "brute", "smea", "aksel", "trimmed-mean", "condense",
                            "nnm-trimmed-mean", "nnm-median") + tuple(r for r in RULES if r.startswith("arc-")) and f is None:
                    continue
                if rule in ("brute", "smea") and n > 20 and a.f is None:
                    continue
                ms = bench_rule(rule, inp, f, a.iters, a.warmup)
                nbytes = n * d * G.element_size()
                print(json.dumps({"rule": rule, "n": n, "d": d, "f": f, "dtype": a.dtype, "ms": round(ms, 4),
                                  "GBps_read": round(nbytes / ms / 1e6, 1)}), flush=True)
            del G, inp
            if a.device == "cuda":
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
