"""Micro-benchmark of the batched 1x1 weight gradients (gpu_iwgrad_multi) against the same jobs launched
one by one (gpu_iwgrad): the wide-kernel job sets of the grouped ResNet-50 CIFAR step's layer2, layer3 and
layer4 (8 workers x 250 images, the splits the step uses), every job on its own tensors. Device time per set
from a HIP graph of 20 repetitions; the outputs of both forms are compared bit for bit.
Results: profiles/r7/wgrad_batch/."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garfield_amd import _native  # noqa: E402

G, N = 8, 2000
# (count, H of x, C, Cout, stride, splits) in the backward's order
SETS = {
    "layer4": [(1, 1, 512, 2048, 1, 1), (1, 1, 2048, 512, 1, 1), (1, 1, 512, 2048, 1, 1), (1, 1, 2048, 512, 1, 1),
               (1, 1, 512, 2048, 1, 1), (1, 2, 1024, 2048, 2, 1), (1, 2, 1024, 512, 1, 1)],
    "layer4 (< 512 workgroups)": [(1, 2, 1024, 512, 1, 1)],
    "layer3": [(1, 2, 256, 1024, 1, 1)] + [(1, 2, 1024, 256, 1, 1), (1, 2, 256, 1024, 1, 1)] * 5
              + [(1, 4, 512, 1024, 2, 1), (1, 4, 512, 256, 1, 4)],
    "layer2": [(1, 4, 128, 512, 1, 4)] + [(1, 4, 512, 128, 1, 4), (1, 4, 128, 512, 1, 4)] * 3
              + [(1, 8, 256, 512, 2, 4), (1, 8, 256, 128, 1, 16)],
}


def bench(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / iters * 1e6)
    return best


def make(dev, H, C, Co, s, S):
    x = torch.randn(N, C, H, H, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    Ho = (H - 1) // s + 1
    dy = torch.randn(N, Co, Ho, Ho, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

    def out():
        if S == 1:
            return torch.empty(G, Co, C, dtype=torch.bfloat16, device=dev)
        return torch.empty(S, G, Co, C, dtype=torch.float32, device=dev)

    wgs = (C // 128) * (Co // 128) * G * S
    return dict(x=x, dy=dy, geom=[1, 1, s, s, 0, 0, 1, 1], S=S, one=out(), multi=out(), wgs=wgs)


def main():
    C_ = _native.native()
    dev = torch.device("cuda")
    for name, spec in SETS.items():
        jobs = [make(dev, H, C, Co, s, S) for n, H, C, Co, s, S in spec for _ in range(n)]

        def one_by_one():
            for j in jobs:
                C_.gpu_iwgrad(j["x"], j["dy"], *j["geom"], G, j["one"], j["S"])

        def batched():
            C_.gpu_iwgrad_multi([j["x"] for j in jobs], [j["dy"] for j in jobs], [j["geom"] for j in jobs], G,
                                [j["multi"] for j in jobs], [j["S"] for j in jobs])

        t1, tm = bench(one_by_one), bench(batched)
        same = all(torch.equal(j["one"], j["multi"]) for j in jobs)
        print(f"{name:28s} {len(jobs):2d} jobs {sum(j['wgs'] for j in jobs):5d} workgroups: one by one {t1:7.1f} us, "
              f"batched {tm:7.1f} us ({t1 / tm:4.2f}x){'' if same else '  MISMATCH'}", flush=True)


if __name__ == "__main__":
    main()
