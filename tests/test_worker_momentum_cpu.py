"""Worker-side momentum on the CPU: the C++ thread-pool implementation and the PyTorch stand-in against
the fp64 oracle (``ops.reference.worker_momentum``), and the engine around it (the identity with server
momentum under plain averaging, sharded == redundant over two gloo ranks, checkpoint / resume,
construction errors)."""
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import _worker_momentum_common as wc
from garfield_amd.models import build_model
from garfield_amd.ops import worker_momentum as wm
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches


def _native_update(native):
    return lambda X, M, beta, first, lo, hi: native.cpu_worker_momentum(X, M, lo, hi, beta, first)


def _torch_update(X, M, beta, first, lo, hi):
    wm.update_torch(X, M, beta, first, lo, hi)


@pytest.fixture(params=["native", "torch"])
def impl(request, native):
    return _native_update(native) if request.param == "native" else _torch_update


@pytest.mark.parametrize("beta", wc.BETAS)
@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("dtype", wc.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_one_step_against_the_oracle(impl, dtype, first, beta):
    for k in wc.KS:
        for d in wc.DS:
            for lo, hi in wc.ranges(d):
                X0, M0 = wc.inputs(k, d, dtype, seed=1000 * k + d)
                X1, M1 = X0.clone(), M0.clone()
                impl(X1, M1, beta, first, lo, hi)
                wc.check(X0, M0, X1, M1, beta, first, lo, hi)


def test_dispatcher_takes_strided_rows_and_default_range(native):
    """``update`` on rows that are a view of a [k, world, ld] exchange buffer, whole row by default;
    the C++ and the dispatcher agree bit for bit."""
    X, M0 = wc.inputs(3, 2 * 1000, torch.bfloat16, seed=5)
    X = X.view(3, 2, 1000)
    M0 = M0[:, :1000].contiguous()
    Xa, Ma, Xb, Mb = X.clone(), M0.clone(), X.clone(), M0.clone()
    wm.update(Xa[:, 1], Ma, 0.9, False)
    native.cpu_worker_momentum(Xb[:, 1], Mb, 0, 1000, 0.9, False)
    assert wc.same_bits(Xa, Xb) and wc.same_bits(Ma, Mb)
    assert wc.same_bits(Xa[:, 0], X[:, 0])
    wc.check(X[:, 1], M0, Xa[:, 1], Ma, 0.9, False, 0, 1000)
    with pytest.raises(ValueError):
        wm.update(Xa[:, 1], Ma, 1.0, False)
    with pytest.raises(ValueError):
        wm.update(Xa[:, 1], Ma, 0.9, False, 0, 1001)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bfloat16", "float16"])
def test_beta_zero_on_16_bit_rows(impl, dtype):
    X0, M0 = wc.inputs(3, 1000, dtype, seed=7)
    X1, M1 = X0.clone(), M0.clone()
    impl(X1, M1, 0.0, False, 0, 1000)
    assert wc.same_bits(M1, X0.float())
    assert wc.same_bits(X1, X0)


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("dtype", wc.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_non_finite_gradient_stays_in_the_row_and_out_of_the_state(impl, dtype, first):
    X0, M0 = wc.inputs(3, 1000, dtype, seed=11)
    for r, x, v in ((0, 0, float("nan")), (0, 999, float("inf")), (1, 8, float("-inf")), (2, 500, float("nan")),
                    (2, 501, float("inf"))):
        X0[r, x] = v
    X1, M1 = X0.clone(), M0.clone()
    impl(X1, M1, 0.9, first, 0, 1000)
    bad = ~torch.isfinite(X0.float())
    assert int(bad.sum()) == 5
    assert wc.same_bits(X1[bad], X0[bad]) and wc.same_bits(M1[bad], M0[bad])
    wc.check(X0, M0, X1, M1, 0.9, first, 0, 1000)   # every other coordinate as without them


# ---------------------------------------------------------------------------------------------- engine


def _mlp_engine(ctx=None, **kw):
    torch.manual_seed(0)
    cfg = EngineConfig(**{**dict(workers_per_rank=4, lr=0.05, exchange_dtype=torch.float32, autocast_dtype=None), **kw})
    return RobustDataParallel(build_model("mlp"), F.nll_loss, ctx or DistContext(), cfg)


def _batches(step: int, k: int = 4, seed: int = 0):
    return synthetic_batches(k, 8, (1, 28, 28), 10, "cpu", seed=100 * seed + step)


# the run shows 1.7e-8 (two fp32 sums of the same terms in different orders, over 6 steps); bound = 20 x
IDENTITY_REL = 3.4e-7


def test_engine_identity_with_server_momentum_under_averaging():
    """With plain averaging the mean of the worker momenta is the momentum of the mean, first step
    included: worker_momentum=beta, momentum=0 trains as momentum=beta, dampening=beta does."""
    beta = 0.9
    a = _mlp_engine(gar="average", f=0, weight_decay=0.0, worker_momentum=beta, momentum=0.0)
    b = _mlp_engine(gar="average", f=0, weight_decay=0.0, worker_momentum=0.0, momentum=beta, dampening=beta)
    assert a.wmom is not None and b.wmom is None
    for it in range(6):
        a.step(_batches(it))
        b.step(_batches(it))
        mean = a.wmom[:, : a.d].mean(0)
        rel_m = float((mean - b.mom[: b.d]).norm() / b.mom[: b.d].norm())
        assert rel_m <= 1e-5, (it, rel_m)
    pa, pb = a.flat_model(), b.flat_model()
    rel = float((pa - pb).norm() / pb.norm())
    print(f"worker momentum identity: parameters relative difference {rel:.3e} after 6 steps")
    assert rel <= IDENTITY_REL, rel


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_rank_worker(rank, world, port, outdir, shard):
    from garfield_amd.parallel.comm import init_distributed, shutdown

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    ctx = init_distributed(backend="gloo", device="cpu")
    eng = _mlp_engine(ctx, gar="krum", f=1, byzantine={3: "lie"}, shard_gar=shard, worker_momentum=0.9,
                      exchange_dtype=torch.bfloat16)
    assert (eng._shard is not None) == shard
    for it in range(4):
        eng.step(_batches(it, seed=rank + 1))
    torch.save({"flat": eng.flat_model().clone(), "sum": eng.replica_checksum(),
                "wmom": eng.wmom[:, : eng.d].clone()},   # without the row padding, which differs
               os.path.join(outdir, f"{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_two_rank_sharded_equals_redundant_bitwise():
    """Krum over 2 gloo ranks x 4 workers with a colluding ``lie`` slot and beta = 0.9: the bucketed
    application of the sharded step is the whole-row one of the redundant step, bit for bit."""
    world = 2
    with tempfile.TemporaryDirectory() as d:
        for shard in (False, True):
            mp.spawn(_two_rank_worker, args=(world, _port(), d, shard), nprocs=world, join=True)
        res = {(s, r): torch.load(os.path.join(d, f"{s}r{r}.pt"), weights_only=True) for s in (0, 1) for r in range(world)}
    ref = res[(0, 0)]
    for s in (0, 1):
        for r in range(world):
            assert res[(s, r)]["sum"] == ref["sum"], (s, r)
            assert torch.equal(res[(s, r)]["flat"], ref["flat"]), (s, r)
    for r in range(world):
        assert wc.same_bits(res[(1, r)]["wmom"], res[(0, r)]["wmom"]), r
        assert float(res[(0, r)]["wmom"].abs().max()) > 0


def test_checkpoint_resumes_bit_identically(tmp_path):
    from garfield_amd.utils.checkpoint import load_engine, save_engine

    kw = dict(gar="krum", f=1, workers_per_rank=5, byzantine={2: "reverse"}, worker_momentum=0.9, momentum=0.0)
    whole = _mlp_engine(**kw)
    for it in range(5):
        whole.step(_batches(it, k=5))
    part = _mlp_engine(**kw)
    for it in range(3):
        part.step(_batches(it, k=5))
    path = save_engine(str(tmp_path / "ck.pt"), part)
    state = torch.load(path, weights_only=True)
    assert tuple(state["worker_momentum"].shape) == (5, part.d) and state["worker_momentum_beta"] == 0.9
    torch.manual_seed(99)   # other initial weights: everything must come from the checkpoint
    resumed = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(), part.cfg)
    load_engine(path, resumed)
    assert resumed.step_count == 3 and wc.same_bits(resumed.wmom, part.wmom)
    for it in range(3, 5):
        resumed.step(_batches(it, k=5))
    assert torch.equal(resumed.flat_model(), whole.flat_model())
    assert wc.same_bits(resumed.wmom, whole.wmom)


def test_checkpoint_without_worker_momenta_loads_with_zero_state(tmp_path):
    """A checkpoint written with worker_momentum=0 resumes with zero state and ``first`` from its step
    count: the first resumed step gives m = (1 - beta) * g."""
    from garfield_amd.utils.checkpoint import load_engine, save_engine

    old = _mlp_engine(gar="average", f=0, momentum=0.0)
    old.step(_batches(0))
    path = save_engine(str(tmp_path / "old.pt"), old)
    assert "worker_momentum" not in torch.load(path, weights_only=True)
    new = _mlp_engine(gar="average", f=0, momentum=0.0, worker_momentum=0.5)
    load_engine(path, new)
    assert new.step_count == 1 and float(new.wmom.abs().max()) == 0.0
    old.step(_batches(1))          # leaves the gradients of step 1 in old.X
    new.step(_batches(1))
    assert wc.same_bits(new.wmom[:, : new.d], 0.5 * old.X[:, 0, : old.d])


def test_construction_errors():
    from dataclasses import asdict

    from garfield_amd.parallel.byzps import ByzantinePSDataParallel, ByzPSConfig
    from garfield_amd.parallel.quorum import QuorumConfig, QuorumDataParallel

    for beta in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="worker_momentum"):
            _mlp_engine(gar="average", f=0, worker_momentum=beta)
    base = asdict(EngineConfig(gar="average", f=0, workers_per_rank=4, worker_momentum=0.9))
    with pytest.raises(ValueError, match="worker_momentum"):
        ByzantinePSDataParallel(build_model("mlp"), F.nll_loss, DistContext(), ByzPSConfig(**base, num_ps=1))
    with pytest.raises(ValueError, match="worker_momentum"):
        QuorumDataParallel(build_model("mlp"), F.nll_loss, DistContext(), QuorumConfig(**base))
    off = _mlp_engine(gar="average", f=0)
    assert off.cfg.worker_momentum == 0.0 and off.wmom is None
    assert _mlp_engine(gar="average", f=0, worker_momentum=0.9).wmom.shape == (4, off.ld)


def test_command_line_flags(capsys):
    import json

    from garfield_amd.apps import gar_bench, garfield_cc

    assert garfield_cc.parse([]).worker_momentum == 0.0
    assert garfield_cc.parse(["--worker_momentum", "0.9"]).worker_momentum == 0.9
    gar_bench.main(["--worker_momentum", "0.9", "--n", "3", "--d", "1001", "--dtype", "bf16", "--device", "cpu",
                    "--iters", "2", "--warmup", "1"])
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["op"] == "worker_momentum" and rec["k"] == 3 and rec["bytes"] == 3 * 1001 * 12 and rec["ms"] > 0
