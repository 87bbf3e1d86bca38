"""Child process of the coordinate-wise dispatch-path tests: the knobs (GARFIELD_COORD16, GARFIELD_MFMA_TAIL,
GARFIELD_AVGMED_TAIL, GARFIELD_COORD16_GRID, GARFIELD_TAIL_GRID) are read once per process, so every knob
set runs in a fresh interpreter started by the parent test with the knobs in ``env=``.

    python tests/_coord_paths_child.py --knobs NAME --out FILE [--plan-only] [case ids ...]

NAME is a key of _coord_paths_common.ENVS; the child refuses to run when its environment does not hold
exactly that knob set. Without ids: every case of the knob set. Writes a JSON to FILE after every case
(``running`` names the case in flight, so a child that dies leaves the culprit on record):

  --plan-only  no GPU: {"reachable": [...the sweep under these knobs...], "cases": {id: error or null}}
  otherwise    {"results": [{"id", "d", "bad", "first"?}, ...], "nnm": {...}, "done": true}
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import _coord_paths_common as cp  # noqa: E402


def dump(path, rec):
    tmp = path + ".tmp"
    with open(tmp, "w") as fh:
        json.dump(rec, fh)
    os.replace(tmp, path)


def nnm_under_tail_cap(native, device):
    """gar.nnm_coord shares tail_grid_cap: bf16 n = 16 (MFMA form) and fp32 n = 16 (LDS form) at d = 5037
    under GARFIELD_TAIL_GRID=2, compared as tests/test_nnm_coord_gpu.py compares (same inputs, sets
    checked against the oracle's, same derived bound)."""
    import test_nnm_coord_gpu as nn
    from garfield_amd.ops import gar
    from garfield_amd.ops import reference as ref

    out = {}
    n, f, d = 16, 3, cp.KNOB_D
    for dtype in (torch.bfloat16, torch.float32):
        X = nn.latent(n, d, dtype, 1)
        D = ref.pairwise_sqdist(X)
        nn.assert_gaps(D, f, ("tail cap", dtype))
        sets = ref.nnm_sets(D, f)
        G = X.to(device)
        masks = nn.sets_of(native, G, f)
        assert torch.equal(masks.cpu(), gar.masks_from_sets(sets))
        for rule in nn.RULES:
            got = nn.run(native, G, masks, f, rule)
            r = nn.check(got, ref.nnm_coord(X, f, rule), X, n, f"{rule} n={n} d={d} f={f} {dtype} (tail cap 2)")
            assert torch.equal(gar.nnm_coord(G, f, rule), got.to(dtype))
            out[f"{rule}-{dtype}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knobs", required=True, choices=sorted(cp.ENVS))
    ap.add_argument("--out", required=True)
    ap.add_argument("--plan-only", action="store_true")
    ap.add_argument("ids", nargs="*")
    a = ap.parse_args()
    env = cp.ENVS[a.knobs]
    have = {k: os.environ[k] for k in cp.KNOBS if k in os.environ}
    if have != env:
        sys.exit(f"knob set {a.knobs} wants {env}, the environment holds {have}")
    cases = [cp.CASE_BY_ID[i] for i in a.ids] if a.ids else cp.cases_of(env)
    assert all(c.env == env for c in cases)

    from garfield_amd import _native
    native = _native.native()

    if a.plan_only:
        rec = {"reachable": sorted(map(list, cp.sweep(native))), "cases": {}}
        for c in cases:
            err = None
            try:
                for d in c.ds:
                    cp.check_plan(native, c, d)
            except AssertionError as e:
                err = str(e)
            rec["cases"][c.id] = err
        dump(a.out, rec)
        return 0

    from garfield_amd.ops import gar
    device = torch.device("cuda", 0)
    rec = {"results": [], "running": None, "done": False}
    for c in cases:
        for d in c.ds:
            rec["running"] = [c.id, d]
            dump(a.out, rec)
            rec["results"].append(cp.run_case(native, gar, c, d, device))
    if a.knobs == "grid2" and not a.ids:
        rec["running"] = ["nnm_coord", cp.KNOB_D]
        dump(a.out, rec)
        rec["nnm"] = nnm_under_tail_cap(native, device)
    rec["running"], rec["done"] = None, True
    dump(a.out, rec)
    return 0


if __name__ == "__main__":
    sys.exit(main())
