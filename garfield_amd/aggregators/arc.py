"""Adaptive robust clipping (ARC; Allouah et al., "Boosting Robustness by Clipping Gradients in Distributed
Learning") in front of a rule (new, absent from the reference): the ``2f(n - f) // n`` gradients of largest
norm are scaled down to the norm of the next one, then the rule runs, optionally behind nearest-neighbour
mixing (``arc-nnm-*``: ARC, then NNM, then the rule). For the rules that end in weights the clipping is folded
into the Gram and into the weights (``docs/GAR_SEMANTICS.md`` "Adaptive robust clipping"): the aggregate is
Σ_j w_j g_j over the ORIGINAL gradients with Σ w <= 1. The coordinate-wise trimmed mean and median have no
weights to fold into: the clipped gradients are rewritten on a private copy and the plain rule (or the
mixing's) runs on it."""
from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import n_of
from garfield_amd.aggregators.average import check as _average_check
from garfield_amd.aggregators.caf import check as _caf_check
from garfield_amd.aggregators.cclip import check as _cclip_check
from garfield_amd.aggregators.dnc import check as _dnc_check
from garfield_amd.aggregators.geomed import check as _geomed_check
from garfield_amd.aggregators.krum import check as _krum_check
from garfield_amd.aggregators.median import check as _median_check
from garfield_amd.aggregators.trimmed_mean import check as _trimmed_mean_check
from garfield_amd.ops import gar


def _check_clip(gradients, f):
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or not 0 <= f < n:
        return f"Invalid number of Byzantine gradients to clip for, got f = {f!r}, expected 0 <= f <= {n - 1}"
    return None


def _rule_kwargs(rule, m=None, iters=None, nu=1e-6, tau=None, start=None, max_passes=None, **kwargs):
    if rule == "caf":
        return {"iters": 16 if iters is None else iters, "max_passes": max_passes}
    if rule == "cclip":
        return {"m": m, "iters": 3 if iters is None else iters, "tau": tau, "start": "mean" if start is None else start}
    return {"krum": {"m": m}, "geomed": {"iters": 32 if iters is None else iters, "nu": nu},
            "dnc": {"m": m, "iters": 16 if iters is None else iters}, "average": {}}[rule]


def _make(rule, own_check, nnm):
    name = ("arc-nnm-" if nnm else "arc-") + rule

    def aggregate(gradients, f=0, **kwargs):
        return gar.arc(gradients, f, rule, nnm, **_rule_kwargs(rule, **kwargs))

    aggregate.__doc__ = (f"{rule} of the adaptively clipped gradients" + (" mixed over their n - f nearest" if nnm else "")
                         + ": Σ_j w_j g_j with the folded weights.")

    def check(gradients, f=0, **kwargs):
        msg = own_check(gradients=gradients, f=f, **kwargs)
        if msg:
            return msg
        start = kwargs.get("start")
        if rule == "cclip" and (kwargs.get("center") is not None or not (start is None or isinstance(start, str))):
            return "Invalid start, expected 'mean' or 'krum' (computed on the clipped gradients) and no center"
        return _check_clip(gradients, f)

    def influence(honests, attacks, f=0, **kwargs):
        """Total weight of the attack gradients (a clipped gradient counts with its scale)."""
        w = gar.arc_weights(list(honests) + list(attacks), f, rule, nnm, **_rule_kwargs(rule, **kwargs))
        return float(w.detach().double().cpu()[len(honests):].sum())

    # no variance-to-norm bound is claimed: upper_bound stays None
    register(name, aggregate, check, influence=influence)


def _make_coord(rule, own_check, nnm):
    """ARC before a coordinate-wise rule: no weights to fold, the clipped gradients are rewritten on a private
    copy (``gar.arc_coord``); one ``f`` serves the clipping, the mixing and the trimming."""
    def aggregate(gradients, f=0, **kwargs):
        return gar.arc_coord(gradients, f, rule, nnm)

    aggregate.__doc__ = (f"Coordinate-wise {rule} of the adaptively clipped gradients"
                         + (" mixed over their n - f nearest." if nnm else "."))

    def check(gradients, f=0, **kwargs):
        msg = own_check(gradients=gradients, f=f, **kwargs)
        if msg:
            return msg
        return _check_clip(gradients, f)

    # as for the plain coordinate-wise rules there is no weight vector: no influence; no bound is claimed
    register(("arc-nnm-" if nnm else "arc-") + rule, aggregate, check)


for _nnm in (False, True):
    _make("krum", _krum_check, _nnm)
    _make("geomed", _geomed_check, _nnm)
    _make("cclip", _cclip_check, _nnm)
    _make("average", _average_check, _nnm)
    _make_coord("trimmed-mean", _trimmed_mean_check, _nnm)
    _make_coord("median", _median_check, _nnm)
_make("dnc", _dnc_check, False)
_make("caf", _caf_check, False)
