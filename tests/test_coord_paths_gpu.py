"""Every dispatch path of the coordinate-wise GAR kernels against a float64 oracle, on exact-arithmetic
inputs full of ties (tests/_coord_paths_common.py): each case first asks _C.coord_plan that it reaches the
kernel family it names (so the table cannot go stale silently), then compares every coordinate.

Default knobs: every reachable (family, dtype, NP, Bulyan-or-not) at d in {1, 63, 64, 65, 255, 256, 257,
1027}, the non-finite variants, and the grid-stride wraps of the two hard-coded caps (coordwise 4096
workgroups, coordwise_lds 2048 tiles) at the smallest wrapping d. The knobs are read once per process, so
the capped-grid wraps (GARFIELD_COORD16_GRID=2, GARFIELD_TAIL_GRID=2) and the A/B fallbacks
(GARFIELD_COORD16=0; GARFIELD_MFMA_TAIL=0 with GARFIELD_AVGMED_TAIL=0) run in one fresh child each.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import _coord_paths_common as cp
from garfield_amd.ops import gar

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "_coord_paths_child.py")
DEFAULT = cp.cases_of({})
# child time limits: each child measured 2.7 s on an MI355X (interpreter start, imports and the first
# launch of every kernel included); ten times that, for a cold file cache
CHILD_TIMEOUT = {"grid2": 30, "no16": 30, "nomfma": 30}
FATAL = {134, 139, 124, 137}


def report(recs):
    bad = [r for r in recs if r["bad"]]
    assert not bad, "coordinates that miss the oracle (index, got, want): " + json.dumps(bad)


@pytest.fixture(scope="module", autouse=True)
def default_knobs():
    assert not any(k in os.environ for k in cp.KNOBS), "the default-knob cases need the knobs unset"


@pytest.mark.parametrize("case", [c for c in DEFAULT if not c.wrap], ids=lambda c: c.id)
def test_small_d(cuda, native, case):
    report([cp.run_case(native, gar, case, d, cuda) for d in case.ds])


@pytest.mark.parametrize("case", [c for c in DEFAULT if c.wrap], ids=lambda c: c.id)
def test_grid_stride_wraps(cuda, native, case):
    """The capped grids of k_coordwise (4096 workgroups) and k_coordwise_lds (2048 tiles) wrap: the
    smallest d beyond one pass, plus an odd tail. The oracle runs in float64 on the device."""
    report([cp.run_case(native, gar, case, d, cuda) for d in case.ds])
    torch.cuda.empty_cache()


def test_nothing_outside_out_is_written(cuda, native):
    """Sentinels on both sides of out[0 : d] for one Bulyan case of every family and dtype at a partial last
    group (the other rules allocate their own output)."""
    seen = set()
    for case in DEFAULT:
        if case.wrap or case.mode != "bulyan-tail" or (case.family, case.dtype) in seen:
            continue
        seen.add((case.family, case.dtype))
        d = 257
        cp.check_plan(native, case, d)
        X, W, members, s = cp.inputs(case, d)
        rows = gar.prepare(X.to(cuda))
        dtype = cp.DTYPES[case.dtype]
        buf = torch.full((d + 256,), -777.0, dtype=dtype, device=cuda)
        native.gpu_coordwise(rows.obj, cp.MODES[case.mode], 0, case.beta, W.to(cuda).reshape(-1), case.t, 0, 1.0,
                             buf[128:128 + d])
        torch.cuda.synchronize()
        assert (buf[:128] == -777.0).all() and (buf[128 + d:] == -777.0).all(), case.id
        want = cp.oracle(X.to(cuda), case.mode, case.f, case.beta, members, s)
        assert cp.mismatches(buf[128:128 + d].clone(), want, case.mode, dtype).numel() == 0, case.id


@pytest.mark.parametrize("knobs", ["grid2", "no16", "nomfma"])
def test_knob_child(cuda, knobs, tmp_path):
    """One fresh child per knob set, one at a time. A child that ends by a signal, an abort, a segmentation
    fault or its time limit ends the whole session: nothing further is started on the GPU."""
    out = str(tmp_path / "result.json")
    env = {k: v for k, v in os.environ.items() if k not in cp.KNOBS}
    env.update(cp.ENVS[knobs])
    try:
        r = subprocess.run([sys.executable, CHILD, "--knobs", knobs, "--out", out], env=env, capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT[knobs])
    except subprocess.TimeoutExpired:
        pytest.exit(f"coord paths child {knobs} ran into its time limit; in flight: {_in_flight(out)}", returncode=3)
    if r.returncode < 0 or r.returncode in FATAL:
        pytest.exit(f"coord paths child {knobs} ended with status {r.returncode}; in flight: {_in_flight(out)}\n"
                    + r.stderr[-2000:], returncode=3)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as fh:
        rec = json.load(fh)
    assert rec["done"]
    cases = cp.cases_of(cp.ENVS[knobs])
    assert {(x["id"], x["d"]) for x in rec["results"]} == {(c.id, d) for c in cases for d in c.ds}
    report(rec["results"])
    if knobs == "grid2":
        assert len(rec["nnm"]) == 4 and all(v <= 1.0 for v in rec["nnm"].values()), rec["nnm"]


def _in_flight(path):
    try:
        with open(path) as fh:
            return json.load(fh).get("running")
    except (OSError, ValueError):
        return None
