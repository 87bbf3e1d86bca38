"""The coordinate-wise dispatch-path tests' own ground, checked without a GPU: the float64 oracle of
_coord_paths_common against ops/reference.py on inputs full of exact ties, the exactness premise of the
inputs, and the coverage of the case table against _C.coord_plan (the pure host function the launchers
obey): every kernel family x dtype x NP x Bulyan-or-not that the dispatcher can reach has a case, and
every case reaches the family it names. The knobs are static per process: each knob set is asked in a
fresh child."""
import json
import os
import subprocess
import sys

import pytest
import torch

import _coord_paths_common as cp
from garfield_amd.ops import reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "_coord_paths_child.py")


@pytest.fixture(scope="module")
def reachable(native):
    assert not any(k in os.environ for k in cp.KNOBS), "the default-knob tests need the knobs unset"
    return cp.sweep(native)


def child_env(env):
    e = {k: v for k, v in os.environ.items() if k not in cp.KNOBS}
    e.update(env)
    return e


# ---- the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("dt", list(cp.DTYPES))
@pytest.mark.parametrize("n", [5, 9, 33, 70])
def test_oracle_equals_reference(n, dt, nonfinite):
    d = 257
    X = cp.grid_rows(n, d, cp.DTYPES[dt], seed=n, nonfinite=nonfinite)
    f, beta = (n - 1) // 3, max(1, n // 2 - 1)

    def same(got, want, what):
        assert got.dtype == torch.float64 and want.dtype == torch.float64
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin), what
        assert torch.equal(torch.isnan(got), torch.isnan(want)), what
        assert torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)]), what
        err = (got[fin] - want[fin]).abs().max().item() if fin.any() else 0.0
        assert err <= 1e-12, (what, err)

    same(cp.oracle(X, "median"), ref.median(X), "median")
    same(cp.oracle(X, "trimmed-mean", f=f), ref.trimmed_mean(X, f), "trimmed-mean")
    same(cp.oracle(X, "averaged-median", beta=beta), ref.averaged_median(X, beta), "averaged-median")
    same(cp.oracle(X, "average-nan"), ref.average_nan(X), "average-nan")
    same(cp.oracle(X, "condense"), ref.condense(X, cp.CONDENSE_P, cp.CONDENSE_SEED), "condense")
    t = n - 2
    for b in (1, max(1, t - 2), t):
        W, members, s = cp.bulyan_W(n, t, seed=n)
        # a row outside a set never reaches its mean: masked sums, not W @ X (0 * inf)
        V = cp.set_means(X.double(), members, s)
        if not nonfinite:
            assert torch.equal(V, W.double() @ X.double())
        want = torch.tensor([ref._closest_mean(V[:, x].tolist(), b) for x in range(d)], dtype=torch.float64)
        same(cp.oracle(X, "bulyan-tail", beta=b, members=members, s=s), want, f"closest mean beta={b}")


def test_mix_hash_vectorised():
    for seed in (0, 1, cp.CONDENSE_SEED, 2**62 - 1):
        got = cp.mix_hash_vec(seed, 300).tolist()
        assert got == [ref.mix_hash(seed, x) for x in range(300)]


def test_inputs_are_what_the_issue_says():
    X = cp.grid_rows(9, 400, torch.float32, 3, nonfinite=True)
    bad = ~torch.isfinite(X)
    assert set(torch.nonzero(bad)[:, 0].tolist()) == set(cp.poisoned_rows(9))
    assert torch.nonzero(bad)[:, 1].unique().tolist() == list(range(0, 400, 97))
    assert torch.isnan(X[1, 0]) and X[1, 97] == float("inf") and X[1, 194] == float("-inf") and X[8, 0] == float("inf")
    fin = X[torch.isfinite(X)] * 4
    assert torch.equal(fin, fin.round()) and fin.abs().max() <= 96
    # exact ties are frequent: nearly every coordinate of 64 rows holds a repeated value (193 levels)
    Y = cp.grid_rows(64, 400, torch.float32, 3)
    ties = sum(int(Y[:, x].unique().numel() < 64) for x in range(400))
    assert ties >= 390, ties
    for n, t in ((2, 1), (3, 1), (11, 5), (64, 46), (100, 88), (128, 128)):
        W, members, s = cp.bulyan_W(n, t, 5)
        assert s & (s - 1) == 0 and 1 <= s <= n - 1
        assert all(len(m) == s == len(set(m)) for m in members)
        assert not W[:, n - 1].any()                                   # one row belongs to no set
        assert torch.equal(W.sum(1), torch.ones(t))
        if n >= 3 and t >= 2:
            assert 0 < int((W[:, 1] != 0).sum()) <= (t + 2) // 4     # the other poisoned row: some sets, a minority


def test_mismatches_notices():
    """The comparison itself: 2 ulp of the output dtype pass, 3 do not; median results are compared bit for
    bit; a non-finite result must be the same non-finite; no coordinate is excused."""
    inf, nan = float("inf"), float("nan")
    for dtype, eps in ((torch.float32, 2.0 ** -23), (torch.bfloat16, 2.0 ** -7), (torch.float16, 2.0 ** -10)):
        want = torch.tensor([1.0, 1.5, -3.0, 0.0, inf, -inf, nan, 20.25, 2.0 ** -130], dtype=torch.float64)
        good = want.to(dtype)
        assert cp.mismatches(good, want, "trimmed-mean", dtype).numel() == 0
        assert cp.mismatches(good, want, "median", dtype).numel() == 0
        near = torch.tensor([1.0 + 2 * eps, 1.5 - 2 * eps, -3.0 - 4 * eps, 0.0, inf, -inf, nan, 20.25 + 32 * eps],
                            dtype=torch.float64).to(dtype)
        assert cp.mismatches(near, want[:8], "averaged-median", dtype).numel() == 0
        assert cp.mismatches(near, want[:8], "median", dtype).tolist() == [0, 1, 2, 7]
        far = torch.tensor([1.0 + 3 * eps, 1.5 - 3 * eps, -3.0 - 6 * eps, 2.0 ** -20, -inf, nan, inf, 20.25 - 48 * eps],
                           dtype=torch.float64).to(dtype)
        assert cp.mismatches(far, want[:8], "bulyan-tail", dtype).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
        assert cp.mismatches(far, want[:8], "condense", dtype).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    assert cp.mismatches(torch.tensor([-0.0]), torch.tensor([0.0], dtype=torch.float64), "median", torch.float32).numel() == 1


def test_inputs_tell_the_tie_orders_apart():
    """The (distance, value) order of the window is visible in the cases' own inputs: an oracle that takes
    the LARGER value first among equally distant ones differs from the right one, beyond the tolerance of
    the strictest comparison (fp32 output), at some coordinate of the cases of every (family, dtype, knob
    set) that runs a window, so a kernel with that tie order cannot pass."""
    told = {}
    for case in cp.CASES:
        if case.mode not in ("bulyan-tail", "averaged-median") or case.beta >= (case.t or case.n):
            continue
        d = min(max(case.ds), cp.KNOB_D)
        X, W, members, s = cp.inputs(case, d)
        V = cp.set_means(X.double(), members, s) if members is not None else X.double()
        want = cp.closest_mean(V, case.beta)
        S = torch.sort(cp._nan_inf(V), dim=0, descending=True).values
        med = S[S.shape[0] - 1 - S.shape[0] // 2]
        idx = torch.sort(cp._nan_inf((S - med).abs()), dim=0, stable=True).indices
        other = torch.gather(S, 0, idx[:case.beta]).sum(0) / case.beta
        key = (case.family, case.dtype, tuple(sorted(case.env)))
        told[key] = told.get(key, 0) + cp.mismatches(other.float(), want, case.mode, torch.float32).numel()
    print(told)
    assert told and all(v > 0 for v in told.values()), {k: v for k, v in told.items() if not v}


# ---- the exactness premise -------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in cp.CASES if max(c.ds) <= cp.KNOB_D], ids=lambda c: c.id)
def test_sums_are_exact_in_fp32(case):
    """For the case's inputs, the fp32 and fp64 column sums of every set (the whole finite column for the
    plain rules), and of the set means themselves, are identical: the premise of the tolerances."""
    d = max(c for c in case.ds)
    X, W, members, s = cp.inputs(case, d)
    X = torch.where(torch.isfinite(X), X, torch.zeros_like(X))        # the finite values: a sum with a non-finite term is not finite
    X32, X64 = X.float(), X.double()
    if members is None:
        members, s = [list(range(case.n))], 1
    V32 = torch.stack([X32[m].sum(0) * (1.0 / s) for m in members])
    V64 = torch.stack([X64[m].sum(0) / s for m in members])
    assert torch.equal(V32.double(), V64)
    assert torch.equal(V32.sum(0).double(), V64.sum(0))
    rev = list(range(len(members) - 1, -1, -1))
    assert torch.equal(V32[rev].cumsum(0)[-1].double(), V64.sum(0))     # any order


# ---- coverage ------------------------------------------------------------------------------------------

def test_default_cases_cover_every_reachable_path(native, reachable):
    default = cp.cases_of({})
    for c in default:
        for d in c.ds:
            cp.check_plan(native, c, d)
    missing = sorted(reachable - cp.case_keys(default))
    assert not missing, f"reachable (family, dtype, NP, Bulyan) without a case: {missing}"
    assert {k[0] for k in reachable} == set(cp.FAMILIES)
    # the non-finite variants: every Bulyan / averaged-median family
    need = {(c.family, c.dtype) for c in default if c.mode in ("bulyan-tail", "averaged-median")}
    have = {(c.family, c.dtype) for c in default if c.mode in ("bulyan-tail", "averaged-median") and c.nonfinite}
    assert need == have, sorted(need - have)
    # every small-d case runs the whole list; the wrap cases wrap
    for c in default:
        assert c.wrap or c.ds == cp.SMALL_D, c.id


def test_plan_answers(native):
    """Spot values of the plan itself: grids, caps and the per-workgroup pass size, as the launchers had them."""
    bf, f32 = torch.bfloat16, torch.float32
    P = native.coord_plan
    assert P(bf, 0, 8, 23_500_000, 0, 0, 0) == {"family": "coord16", "np": 8, "grid": 11475, "coords_per_pass": 2048,
                                                 "sub": 4, "bulyan": False}
    assert P(bf, 0, 64, 23_500_000, 0, 0, 0)["grid"] == 4096 and P(bf, 0, 8, 10**9, 0, 0, 0)["grid"] == 16384
    assert P(f32, 0, 20, 23_500_000, 0, 0, 0) == {"family": "coordwise_lds", "np": 32, "grid": 2048,
                                                  "coords_per_pass": 256, "sub": 0, "bulyan": False}
    assert P(f32, 3, 3, 0, 0, 0, 0)["grid"] == 1 and P(f32, 3, 40, 100, 0, 0, 0)["grid"] == 1
    assert P(f32, 1, 9, 1000, 2, 0, 0) == {"family": "coordwise", "np": 16, "grid": 1, "coords_per_pass": 1024,
                                           "sub": 4, "bulyan": False}
    assert P(bf, 5, 25, 23_500_000, 0, 9, 15) == {"family": "tail_mfma", "np": 16, "grid": 4096, "coords_per_pass": 256,
                                                  "sub": 2, "bulyan": True}
    assert P(f32, 5, 25, 1027, 0, 9, 15) == {"family": "tail_f32", "np": 16, "grid": 5, "coords_per_pass": 256,
                                             "sub": 32, "bulyan": True}
    assert P(f32, 5, 25, 23_500_000, 0, 9, 15)["grid"] == 2048
    assert P(f32, 5, 20, 1027, 0, 3, 12) == {"family": "tail_window", "np": 16, "grid": 5, "coords_per_pass": 256,
                                             "sub": 0, "bulyan": True}
    assert P(bf, 2, 64, 1027, 0, 50, 0)["family"] == "tail_mfma" and P(bf, 2, 65, 1027, 0, 50, 0)["bulyan"] is False
    for bad in (lambda: P(torch.float64, 0, 8, 10, 0, 0, 0), lambda: P(bf, 6, 8, 10, 0, 0, 0),
                lambda: P(bf, 0, 129, 10, 0, 0, 0), lambda: P(bf, 5, 8, 10, 0, 1, 0), lambda: P(bf, 5, 8, 10, 0, 1, 129)):
        with pytest.raises(RuntimeError):
            bad()


@pytest.mark.parametrize("knobs", sorted(cp.ENVS))
def test_knob_cases_cover_what_the_knobs_add(native, reachable, knobs, tmp_path):
    """In a fresh child under the knob set: every case of the set reaches the family it names (and wraps
    where it says so), and every (family, dtype, NP, Bulyan) that the knobs make reachable beyond the
    default set has a case. (The fallbacks add no kernel that the default dispatch cannot reach through
    another rule or dtype, except the window kernels of GARFIELD_MFMA_TAIL=0 / GARFIELD_AVGMED_TAIL=0;
    what they add is other rules on the same kernels, which the cases name rule by rule.)"""
    out = str(tmp_path / "plan.json")
    r = subprocess.run([sys.executable, CHILD, "--knobs", knobs, "--out", out, "--plan-only"],
                       env=child_env(cp.ENVS[knobs]), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as fh:
        rec = json.load(fh)
    cases = cp.cases_of(cp.ENVS[knobs])
    assert cases and set(rec["cases"]) == {c.id for c in cases}
    wrong = {k: v for k, v in rec["cases"].items() if v}
    assert not wrong, wrong
    here = {(f, dt, np_, b) for f, dt, np_, b in rec["reachable"]}
    missing = sorted(here - reachable - cp.case_keys(cases))
    assert not missing, f"reachable only under {knobs}, without a case: {missing}"
    if knobs == "no16":
        assert {k[0] for k in here} == {"coordwise", "coordwise_lds"}
    if knobs == "nomfma":
        assert "tail_mfma" not in {k[0] for k in here} and ("tail_window_direct", "bf16", 64, False) in here
        assert ("tail_window", "bf16", 64, True) in here - reachable
    if knobs == "grid2":
        assert here == reachable and all(c.wrap for c in cases)
        # at least three passes of the fp32 tail, so its prefetch chain (load(gi + gstep)) runs
        for c in cases:
            if c.family in ("tail_f32", "tail_mfma"):
                p = cp.plan_of(native, c, cp.KNOB_D)        # this process: default caps
                assert 3 * 2 * p["coords_per_pass"] < cp.KNOB_D
