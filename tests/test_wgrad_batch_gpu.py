"""Batched 1x1 weight gradients on MI355X: ``gpu_iwgrad_multi`` (several layers' 128 x 128-tile
weight gradients in one launch) against the same jobs through ``gpu_iwgrad``, bit for bit, and the
ResNet-50 step with the GradSink's deferred queue (``WGRAD_BATCH``) against the one-by-one step."""
import pytest
import torch
import torch.nn.functional as F

from garfield_amd.models import build_model
from garfield_amd.ops.grouped import GradSink
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches

pytestmark = pytest.mark.gpu

G = 3
GUARD = 40          # bf16 guard elements before the first row
PAD = 100           # ... and between rows
# (B, C, Cout, H, stride, splits, bf16 row view)
JOBS = [(7, 128, 256, 8, 2, 4, False),    # fp32 slabs, ragged splits (28 of 112 pixels each)
        (5, 256, 512, 6, 1, 1, True),     # bf16 strided row view
        (2, 512, 128, 3, 1, 8, False),    # depth-2 ring, splits 6 and 7 empty (18 pixels, 3 per split)
        (20, 128, 256, 8, 1, 1, False)]   # depth-3 ring (20 stages of 64 pixels)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _job(cuda, B, C, Co, H, s, S, bf16, seed):
    """Inputs, geometry and a fresh poisoned out (with its backing buffer) of one job."""
    gen = torch.Generator(device=cuda).manual_seed(seed)
    x = torch.randn(G * B, C, H, H, device=cuda, generator=gen).to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    Ho = (H - 1) // s + 1
    dy = torch.randn(G * B, Co, Ho, Ho, device=cuda, generator=gen).to(torch.bfloat16)
    dy = dy.contiguous(memory_format=torch.channels_last)
    return x, dy, [1, 1, s, s, 0, 0, 1, 1]


def _out(cuda, C, Co, S, bf16):
    if bf16:
        flat = torch.full((GUARD + G * (Co * C + PAD),), 7.0, dtype=torch.bfloat16, device=cuda)
        return flat.as_strided((G, Co, C), (Co * C + PAD, C, 1), GUARD), flat
    flat = torch.full((S, G, Co, C), 7.0, device=cuda)
    return flat, flat


def _guards_untouched(flat, C, Co):
    rows = flat[GUARD:].view(G, Co * C + PAD)
    return bool((flat[:GUARD] == 7).all()) and bool((rows[:, Co * C:] == 7).all())


@pytest.fixture(scope="module")
def jobs(cuda, native):
    """The four jobs with their one-by-one (gpu_iwgrad) results and fp32 references, computed once."""
    out = []
    for i, (B, C, Co, H, s, S, bf16) in enumerate(JOBS):
        x, dy, geom = _job(cuda, B, C, Co, H, s, S, bf16, 100 + i)
        one, flat = _out(cuda, C, Co, S, bf16)
        native.gpu_iwgrad(x, dy, *geom, G, one, S)
        ref = torch.stack([torch.nn.grad.conv2d_weight(x[g * B:(g + 1) * B].float(), (Co, C, 1, 1),
                                                       dy[g * B:(g + 1) * B].float(), s, 0).reshape(Co, C)
                           for g in range(G)])
        out.append(dict(x=x, dy=dy, geom=geom, S=S, bf16=bf16, C=C, Co=Co, one=flat.clone(), ref=ref))
    torch.cuda.synchronize()
    return out


def _run_multi(cuda, native, js):
    outs, flats = zip(*[_out(cuda, j["C"], j["Co"], j["S"], j["bf16"]) for j in js])
    native.gpu_iwgrad_multi([j["x"] for j in js], [j["dy"] for j in js], [j["geom"] for j in js], G, list(outs),
                            [j["S"] for j in js])
    torch.cuda.synchronize()
    return outs, flats


def _check(js, outs, flats):
    for j, out, flat in zip(js, outs, flats):
        assert torch.equal(flat, j["one"])     # the whole backing buffer: results and guard elements
        if j["bf16"]:
            assert _guards_untouched(flat, j["C"], j["Co"])
            assert rel(out.float(), j["ref"]) < 1e-2
        else:
            assert rel(out.sum(0), j["ref"]) < 1e-2


def test_multi_launch_equals_single_launches_bitwise(cuda, native, jobs):
    """Four jobs, each with its own batch, in one launch (depth-3 ring: the last job has 20 stages):
    fp32 slabs with ragged and empty splits, a bf16 strided row view with guard elements, equal to
    gpu_iwgrad bit for bit and within rel < 1e-2 of fp32 conv2d_weight."""
    _check(jobs, *_run_multi(cuda, native, jobs))


def test_multi_launch_depth2_ring(cuda, native, jobs):
    """Jobs whose splits all have at most four 64-pixel stages take the depth-2 ring."""
    js = [jobs[0], jobs[2]]
    _check(js, *_run_multi(cuda, native, js))


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_one_job_call(cuda, native, jobs, i):
    _check([jobs[i]], *_run_multi(cuda, native, [jobs[i]]))


def test_seventeen_jobs_take_two_launches(cuda, native, jobs):
    js = [jobs[i % 4] for i in range(17)]
    _check(js, *_run_multi(cuda, native, js))


def test_multi_rejects_jobs_the_wide_kernel_does_not_take(cuda, native):
    x, dy, geom = _job(cuda, 2, 64, 128, 4, 1, 1, False, 7)        # C % 128 != 0
    with pytest.raises(RuntimeError):
        native.gpu_iwgrad_multi([x], [dy], [geom], G, [torch.empty(1, G, 128, 64, device=cuda)], [1])
    x, dy, geom = _job(cuda, 2, 128, 128, 4, 1, 1, False, 8)
    with pytest.raises(RuntimeError):                               # slab of the wrong split count
        native.gpu_iwgrad_multi([x], [dy], [geom], G, [torch.empty(1, G, 128, 128, device=cuda)], [2])
    with pytest.raises(RuntimeError):                               # lists of different lengths
        native.gpu_iwgrad_multi([x], [dy, dy], [geom], G, [torch.empty(1, G, 128, 128, device=cuda)], [1])


def _steps(cuda, monkeypatch, on, steps, **cfg):
    """Exchange rows and loss after each of ``steps`` ResNet-50 steps (G = 2, 2 images per worker)."""
    import garfield_amd.ops.grouped as grouped

    monkeypatch.setattr(grouped, "WGRAD_BATCH", on)
    queued, flushes = [], []
    q0, f0 = GradSink.queue_wgrad, GradSink.flush_splits

    def queue(self, *a, **k):
        queued.append(1)
        q0(self, *a, **k)

    def flush(self):
        f0(self)
        flushes.append(1)
        assert not self._wq and self._wq_wgs == 0     # the queue is empty after flush_splits()

    monkeypatch.setattr(GradSink, "queue_wgrad", queue)
    monkeypatch.setattr(GradSink, "flush_splits", flush)
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("resnet50", 10), F.cross_entropy, DistContext(device=cuda),
                             EngineConfig(gar="average", f=0, workers_per_rank=2, lr=0.01, **cfg))
    b = synthetic_batches(2, 2, (3, 32, 32), 10, cuda, seed=3)
    out = []
    for _ in range(steps):
        loss = eng.step(b)
        torch.cuda.synchronize()
        out.append((eng.X.clone(), loss.clone()))
    assert flushes
    assert bool(queued) == on
    return eng, out


def _same(a, b):
    assert len(a) == len(b)
    for (xa, la), (xb, lb) in zip(a, b):
        assert torch.equal(xa, xb)
        assert torch.equal(la, lb)


def test_step_eager_bitwise(cuda, monkeypatch):
    _, off = _steps(cuda, monkeypatch, False, 2, cuda_graph=False)
    _, on = _steps(cuda, monkeypatch, True, 2, cuda_graph=False)
    _same(on, off)


def test_step_hip_graph_bitwise(cuda, monkeypatch):
    """Step 0 eager, step 1 captured and replayed, step 2 replayed."""
    e0, off = _steps(cuda, monkeypatch, False, 3, cuda_graph=True)
    e1, on = _steps(cuda, monkeypatch, True, 3, cuda_graph=True)
    assert e0._ggraph is not None and e1._ggraph is not None
    _same(on, off)


def test_step_sharded_bucket_marks_flush_the_queue(cuda, monkeypatch):
    """shard_gar with the exchange machinery of a multi-rank step on one rank (comm stream, bucket signals
    recorded inside the backward, stage graphs): the bucket marks call flush_splits(), which launches the
    queue first, so every bucket's rows are complete when its signal fires."""
    monkeypatch.setenv("GARFIELD_LOOPBACK_EXCHANGE", "1")
    monkeypatch.setenv("GARFIELD_OVERLAP", "1")
    e0, off = _steps(cuda, monkeypatch, False, 3, cuda_graph=True, shard_gar=True)
    e1, on = _steps(cuda, monkeypatch, True, 3, cuda_graph=True, shard_gar=True)
    for e in (e0, e1):
        assert e._gexec.marks and e._gexec.mark_events() is not None
        assert isinstance(e._ggraph, list) and len(e._ggraph) == 3
    _same(on, off)
