"""Nearest-neighbour mixing (NNM; Allouah et al., "Fixing by Mixing", AISTATS 2023) in front of a
rule (new, absent from the reference): every gradient is replaced by the mean of its ``n - f``
nearest gradients, itself included, then Krum, the geometric median, centered clipping or the average
runs on the mixed gradients. The mixing is folded into the rule's weights (``docs/GAR_SEMANTICS.md``
"Nearest-neighbour mixing"): the aggregate is Σ_j w_j g_j over the ORIGINAL gradients. The coordinate-wise
trimmed mean and median have no weights to fold into: they run per coordinate over the n set means, which
are never stored ("Nearest-neighbour mixing before a coordinate-wise rule")."""
from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import n_of
from garfield_amd.aggregators.average import check as _average_check
from garfield_amd.aggregators.cclip import check as _cclip_check
from garfield_amd.aggregators.geomed import check as _geomed_check
from garfield_amd.aggregators.krum import check as _krum_check
from garfield_amd.aggregators.median import check as _median_check
from garfield_amd.aggregators.trimmed_mean import check as _trimmed_mean_check
from garfield_amd.ops import gar


def _check_mix(gradients, f):
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or not 0 <= f < n:
        return f"Invalid number of Byzantine gradients to mix out, got f = {f!r}, expected 0 <= f <= {n - 1}"
    return None


def _rule_kwargs(rule, m=None, iters=None, nu=1e-6, tau=None, start=None, **kwargs):
    if rule == "cclip":
        return {"m": m, "iters": 3 if iters is None else iters, "tau": tau, "start": "mean" if start is None else start}
    return {"krum": {"m": m}, "geomed": {"iters": 32 if iters is None else iters, "nu": nu}, "average": {}}[rule]


def _make(rule, own_check):
    def aggregate(gradients, f=0, **kwargs):
        return gar.nnm(gradients, f, rule, **_rule_kwargs(rule, **kwargs))

    aggregate.__doc__ = f"{rule} of the gradients mixed over their n - f nearest: Σ_j w_j g_j with the folded weights."

    def check(gradients, f=0, **kwargs):
        msg = own_check(gradients=gradients, f=f, **kwargs)
        if msg:
            return msg
        if rule == "cclip" and (kwargs.get("center") is not None or not isinstance(kwargs.get("start") or "", str)):
            return "Invalid start, expected 'mean' or 'krum' (computed on the mixed gradients) and no center"
        return _check_mix(gradients, f)

    def influence(honests, attacks, f=0, **kwargs):
        """Total weight of the attack gradients (the folded weights are non-zero on nearly every row)."""
        w = gar.nnm_weights(list(honests) + list(attacks), f, rule, **_rule_kwargs(rule, **kwargs))
        return float(w.detach().double().cpu()[len(honests):].sum())

    # no variance-to-norm bound is claimed: upper_bound stays None
    register("nnm-" + rule, aggregate, check, influence=influence)


def _make_coord(rule, own_check):
    """NNM before a coordinate-wise rule: no weights to fold, the rule runs per coordinate over the n
    set means (``gar.nnm_coord``); one ``f`` serves the mixing and the trimming."""
    def aggregate(gradients, f=0, **kwargs):
        return gar.nnm_coord(gradients, f, rule)

    aggregate.__doc__ = f"Coordinate-wise {rule} of the gradients mixed over their n - f nearest."

    def check(gradients, f=0, **kwargs):
        msg = own_check(gradients=gradients, f=f, **kwargs)
        if msg:
            return msg
        return _check_mix(gradients, f)

    # as for the plain coordinate-wise rules there is no weight vector: no influence; no bound is claimed
    register("nnm-" + rule, aggregate, check)


_make("krum", _krum_check)
_make("geomed", _geomed_check)
_make("cclip", _cclip_check)
_make("average", _average_check)
_make_coord("trimmed-mean", _trimmed_mean_check)
_make_coord("median", _median_check)
