"""The adaptive colluding attacks Min-Max / Min-Sum on the CPU: the fp64 oracle against the definition on
the vectors, the tensor functions of runtime/attacks.py against the oracle, the engine's redundant path and
the sharded step against it (docs/GAR_SEMANTICS.md "Adaptive colluding attacks")."""
import os
import socket
import tempfile

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from garfield_amd.models import build_model
from garfield_amd.ops import agr_attack
from garfield_amd.ops import reference as ref
from garfield_amd.parallel.comm import DistContext
from garfield_amd.parallel.engine import EngineConfig, RobustDataParallel, synthetic_batches
from garfield_amd.runtime import attacks

KINDS = ("minmax", "minmax-uv", "minmax-sgn", "minsum", "minsum-uv", "minsum-sgn")
KS = (2, 3, 5, 8, 17, 64, 128)
DS = (1, 7, 64, 2000)

# The sharded and the redundant step take the same fp64 statistics in another order (per bucket and rank,
# then summed): b_i, c and the Gram differ by a few fp64 roundings of sums of d ~ 8e4 terms, with
# cancellation in the distances (‖e‖² / D ~ 1e2 at most here), so γ agrees far inside 1e-9 relative. The
# attacked rows are fp32: one ulp (2^-23 relative to the element, plus the γ difference times |p|) where a
# rounding falls the other way.
GAMMA_SHARD_RTOL = 1e-9


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(k, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(k, d, generator=g, dtype=torch.float64) * 0.3 + torch.randn(d, generator=g, dtype=torch.float64)


def _constraint(E, m, objective):
    dist = ((m - E) ** 2).sum(1)
    D = ((E[:, None, :] - E[None, :, :]) ** 2).sum(-1) if E.shape[0] * E.shape[0] * E.shape[1] < 1 << 24 else \
        torch.stack([((E - e) ** 2).sum(1) for e in E])
    if objective == "minmax":
        return float(dist.max()), float(D.max())
    return float(dist.sum()), float(D.sum(1).max())


def test_names_are_registered():
    for kind in KINDS:
        assert kind in attacks.WORKER_ATTACKS and kind in attacks.NEEDS_ESTIMATES
        assert kind not in attacks.SERVER_ATTACKS
    assert agr_attack.parse("minsum") == ("minsum", "std") and agr_attack.parse("minmax-sgn") == ("minmax", "sgn")
    with pytest.raises(ValueError):
        agr_attack.parse("minmax-foo")


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_constraint_is_tight(kind):
    """γ is the limit of the paper's search: the constraint holds with equality to 1e-9 relative and is
    violated at γ (1 + 1e-6)."""
    objective, pert = agr_attack.parse(kind)
    worst = 0.0
    for k in KS:
        for d in DS:
            E = _rows(k, d, 1000 * k + d)
            m, gamma = ref.agr_attack(E, objective, pert)
            mu, p = ref.agr_perturbation(E, pert)
            assert gamma > 0 and torch.equal(m, mu + gamma * p)
            got, bound = _constraint(E, m, objective)
            worst = max(worst, abs(got - bound) / bound)
            assert abs(got - bound) <= 1e-9 * bound, (k, d, got, bound)
            over, _ = _constraint(E, mu + gamma * (1 + 1e-6) * p, objective)
            assert over > bound, (k, d, over, bound)
    print(f"{kind}: largest relative slack of the constraint {worst:.2e}")


@pytest.mark.parametrize("objective", ["minmax", "minsum"])
def test_oracle_uv_is_scale_invariant(objective):
    """μ + γ p does not depend on the scale of p: the paper's unit vector -μ/‖μ‖ gives the same m as -μ."""
    for k in KS:
        for d in DS:
            E = _rows(k, d, 7 * k + d)
            m, gamma = ref.agr_attack(E, objective, "uv")
            mu = E.mean(0)
            u = -mu / mu.norm()
            # the same closed form with the unit vector as p
            a, b, c = ((mu - E) ** 2).sum(1), (u * (mu - E)).sum(1), float(u @ u)
            _, bound = _constraint(E, mu, objective)
            if objective == "minmax":
                gu = float(((-b + torch.sqrt(b * b + c * (bound - a).clamp(min=0))) / c).min())
            else:
                gu = (max(bound - float(a.sum()), 0.0) / (k * c)) ** 0.5
            assert torch.allclose(mu + gu * u, m, rtol=1e-9, atol=1e-12 * float(mu.abs().max()))
            assert abs(gu - gamma * float(mu.norm())) <= 1e-9 * gu


@pytest.mark.parametrize("kind", KINDS)
def test_edges(kind):
    objective, pert = agr_attack.parse(kind)
    e1 = _rows(1, 33, 1)
    m, gamma = ref.agr_attack(e1, objective, pert)                        # k = 1
    assert gamma == 0.0 and torch.equal(m, e1[0])
    same = e1.repeat(5, 1)
    m, gamma = ref.agr_attack(same, objective, pert)                      # identical rows
    assert gamma == 0.0 and torch.allclose(m, e1[0], rtol=1e-15, atol=0)
    E = _rows(6, 40, 2)
    E[:, 11] = 0.0                                                        # an all-zero coordinate
    m, gamma = ref.agr_attack(E, objective, pert)
    assert gamma > 0 and float(m[11]) == 0.0
    if pert == "sgn":
        assert float(ref.agr_perturbation(E, pert)[1][11]) == 0.0
    E[2, 5] = float("nan")                                                # a NaN estimate: γ = 0, no raise
    m, gamma = ref.agr_attack(E, objective, pert)
    assert gamma == 0.0
    for fn_rows in (E, E.float()):
        out = attacks.apply_attack(kind, fn_rows[0], fn_rows)
        assert out.shape == fn_rows[0].shape
        g = agr_attack.attack_rows([r.clone() for r in fn_rows], 5, kind)
        assert float(g) == 0.0
    # the functional path on the same edges
    assert float(agr_attack.attack_rows([e1[0].clone()], 0, kind)) == 0.0
    rows = [r.clone() for r in same]
    assert float(agr_attack.attack_rows(rows, 3, kind)) == 0.0
    assert torch.allclose(rows[4], e1[0], rtol=1e-15, atol=0) and torch.equal(rows[0], e1[0])


@pytest.mark.parametrize("kind", KINDS)
def test_tensor_functions_match_the_oracle(kind):
    """runtime/attacks.py (γ from the Gram of the estimates) against the oracle (on the vectors), fp32
    rows: γ within 1e-6 relative, the vector within fp32 rounding of the oracle's."""
    objective, pert = agr_attack.parse(kind)
    for k, d in ((2, 7), (5, 64), (17, 2000), (128, 300)):
        E = _rows(k, d, 31 * k + d).float()
        m, gamma = ref.agr_attack(E, objective, pert)
        rows = [r.clone() for r in E]
        g, info = agr_attack.attack_rows(rows, k - 1, kind, info=True)
        assert abs(float(g) - gamma) <= 1e-6 * gamma, (k, d, float(g), gamma)
        assert float(info[0]) == float(g) and info.numel() == 2 + 2 * k
        out = attacks.apply_attack(kind, E[0], E)
        assert out.dtype == torch.float32 and torch.equal(out, rows[-1])
        assert torch.equal(out, attacks.WORKER_ATTACKS[kind](E[0], estimates=list(E)))
        tol = 2.0 ** -23 * m.abs() + 1e-6 * gamma * ref.agr_perturbation(E.double(), pert)[1].abs()
        assert bool(((out.double() - m).abs() <= tol).all())
        for i in range(k - 1):
            assert torch.equal(rows[i], E[i])       # the peers' rows are never written


def test_partials_are_additive_and_ranges_are_respected():
    E = _rows(6, 500, 3).float()
    for pert in ("std", "uv", "sgn"):
        rows = [r.clone() for r in E]
        g, p = agr_attack.agr_partials(rows, pert)
        g1, p1 = agr_attack.agr_partials(rows, pert, 0, 123)
        g2, p2 = agr_attack.agr_partials(rows, pert, 123, 500)
        assert torch.allclose(g1 + g2, g, rtol=1e-12) and torch.allclose(p1 + p2, p, rtol=1e-9, atol=1e-9)
        gamma = agr_attack.agr_gamma(g1 + g2, p1 + p2, "minmax")
        agr_attack.agr_write(rows, 4, gamma, pert, 100, 200)
        for i, r in enumerate(rows):
            assert torch.equal(r[:100], E[i, :100]) and torch.equal(r[200:], E[i, 200:])
            assert torch.equal(r[100:200], E[i, 100:200]) == (i < 4)
        assert torch.equal(rows[4][100:200], rows[5][100:200])


@pytest.mark.parametrize("collusion", ["fw", "all"])
def test_engine_targets_get_the_oracle_vector(collusion):
    """All targets receive one vector: the oracle's on {peers' rows} + {every target's honest row}."""
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="krum", f=3, workers_per_rank=10, collusion=collusion,
                                          exchange_dtype=torch.float32, byzantine={1: "minmax", 5: "minmax", 8: "minmax"}))
    b = synthetic_batches(10, 16, (1, 28, 28), 10, "cpu")
    eng.compute_local(b)
    G0 = eng.G.clone()
    honest = [0, 2, 3, 4, 6, 7, 9]
    peers = honest[:2] if collusion == "fw" else honest
    eng.aggregate_and_update()
    m, gamma = ref.agr_attack(G0[peers + [1, 5, 8]], "minmax", "std")
    assert gamma > 0 and abs(float(eng.last_agr_gamma["minmax"]) - gamma) <= 1e-6 * gamma
    assert torch.equal(eng.G[1], eng.G[5]) and torch.equal(eng.G[1], eng.G[8])
    sigma = G0[peers + [1, 5, 8]].double().std(0)
    assert bool(((eng.G[1].double() - m).abs() <= 2.0 ** -23 * m.abs() + 1e-6 * gamma * sigma).all())
    assert torch.equal(eng.G[honest], G0[honest])
    print(f"collusion={collusion}: gamma {gamma:.4f}, multi-Krum weights on the targets "
          f"{[float(eng.last_weights[s]) for s in (1, 5, 8)]}")     # reported, not asserted
    assert torch.isfinite(eng.flat_model()).all()


def test_engine_kinds_compose_with_lie():
    """Two adaptive kinds and lie in one step: each kind sees the honest rows and its own targets only."""
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                             EngineConfig(gar="median", f=3, workers_per_rank=8, collusion="all",
                                          exchange_dtype=torch.float32, byzantine={1: "minsum-uv", 2: "lie", 6: "minmax-sgn"}))
    b = synthetic_batches(8, 16, (1, 28, 28), 10, "cpu")
    eng.compute_local(b)
    G0 = eng.G.clone()
    honest = [0, 3, 4, 5, 7]
    eng.aggregate_and_update()
    for s, kind in ((1, "minsum-uv"), (6, "minmax-sgn")):
        want = attacks.apply_attack(kind, G0[s], torch.stack([*G0[honest], G0[s]]))
        assert torch.equal(eng.G[s], want)
    want = attacks.lie_attack(G0[2], torch.stack([G0[2], *G0[honest]]))
    assert torch.allclose(eng.G[2], want, rtol=1e-6, atol=1e-7)


def test_too_many_estimate_rows_raise_at_construction():
    with pytest.raises(ValueError, match="estimate rows"):
        RobustDataParallel(build_model("mlp"), F.nll_loss, DistContext(),
                           EngineConfig(gar="median", f=1, workers_per_rank=130, collusion="all",
                                        byzantine={0: "minmax"}))


def _worker(rank, world, port, outdir, shard, attack):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from garfield_amd.parallel.comm import init_distributed, shutdown

    ctx = init_distributed(backend="gloo", device="cpu")
    torch.manual_seed(0)
    eng = RobustDataParallel(build_model("mlp"), F.nll_loss, ctx,
                             EngineConfig(gar="median", f=2, workers_per_rank=4, byzantine={1: attack, 6: attack},
                                          shard_gar=shard, lr=0.05, collusion="all", momentum=0.0,
                                          exchange_dtype=torch.float32))
    assert (eng._shard is not None) == shard
    b = synthetic_batches(4, 8, (1, 28, 28), 10, "cpu", seed=rank)
    eng.compute_local(b)
    eng.aggregate_and_update()
    out = {"gamma": {k: float(v) for k, v in eng.last_agr_gamma.items()}}
    if shard:   # this rank's coordinate shard of the two attacked rows, per bucket
        out["rows"] = {b_.lo: (b_.own.start, torch.stack([b_.rows[1], b_.rows[6]]).clone()) for b_ in eng._shard.buckets}
    else:
        out["rows"] = eng.G[[1, 6]].clone()
    for _ in range(2):
        eng.step(b)
    out["flat"], out["sum"] = eng.flat_model().clone(), eng.replica_checksum()
    torch.save(out, os.path.join(outdir, f"{attack}{int(shard)}r{rank}.pt"))
    shutdown(ctx)


def test_two_rank_sharded_matches_redundant():
    """The sharded step (per-bucket partials, one all-gather, solve, write) against the redundant one: γ and
    the attacked rows within the bound (another summation order), replicas bit-identical; lie as before."""
    with tempfile.TemporaryDirectory() as d:
        for attack in ("minmax", "lie"):
            for shard in (False, True):
                mp.spawn(_worker, args=(2, free_port(), d, shard, attack), nprocs=2, join=True)
        r = {k: torch.load(os.path.join(d, f"{k}.pt"), weights_only=False)
             for k in [f"{a}{s}r{q}" for a in ("minmax", "lie") for s in (0, 1) for q in (0, 1)]}
        for a in ("minmax", "lie"):
            for s in (0, 1):
                assert torch.equal(r[f"{a}{s}r0"]["flat"], r[f"{a}{s}r1"]["flat"])
                assert r[f"{a}{s}r0"]["sum"] == r[f"{a}{s}r1"]["sum"]            # replica_checksum()
        g0, g1 = r["minmax0r0"]["gamma"]["minmax"], r["minmax1r0"]["gamma"]["minmax"]
        assert g0 > 0 and r["minmax1r1"]["gamma"]["minmax"] == g1 and r["minmax0r1"]["gamma"]["minmax"] == g0
        print(f"gamma redundant {g0!r} sharded {g1!r} relative difference {abs(g1 - g0) / g0:.2e}")
        assert abs(g1 - g0) <= GAMMA_SHARD_RTOL * g0
        full = r["minmax0r0"]["rows"]
        assert torch.equal(full[0], full[1])
        for q in (0, 1):
            for lo, (start, rows) in r[f"minmax1r{q}"]["rows"].items():
                want = full[:, start:start + rows.shape[1]]
                have = rows[:, :want.shape[1]]
                assert torch.equal(have[0], have[1])
                assert bool(((have - want).abs() <= 2.0 ** -23 * want.abs() + 1e-30).all()), (q, lo)
        # lie: the per-bucket path is untouched. On the CPU it goes through torch's mean / std, whose
        # vectorisation depends on where a slice starts, so a shard's fp32 row is within an fp32 rounding of the
        # whole row's (the tolerances of test_engine_cpu.py's collusion tests), replicas bit-identical (above)
        a = r["lie0r0"]["flat"]
        for name in ("lie0r1", "lie1r0", "lie1r1"):
            assert torch.allclose(a, r[name]["flat"], rtol=1e-5, atol=1e-6), name
        lie_full = r["lie0r0"]["rows"]
        for q in (0, 1):
            for lo, (start, rows) in r[f"lie1r{q}"]["rows"].items():
                want = lie_full[:, start:start + rows.shape[1]]
                assert torch.allclose(rows[:, :want.shape[1]], want, rtol=1e-6, atol=1e-7), (q, lo)
