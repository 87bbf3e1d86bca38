"""CAF covariance-filter GAR (new, absent from the reference; the covariance-bound agnostic filter of Allouah,
Guerraoui, Gupta, Pinot, Rizk and Voitovych): while more than ``n - 2f`` rows' worth of weight is left, every row
is down-weighted by its squared projection on the top principal direction of the weighted covariance, and the
weighted mean whose covariance had the smallest top eigenvalue is kept. The eigenpairs come from ``iters`` power
rounds per pass on the pairwise distances alone (``docs/GAR_SEMANTICS.md``): all coordinates, no d x d matrix."""
from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import check_gradients, n_of
from garfield_amd.ops import gar


def aggregate(gradients, f=0, iters=16, max_passes=None, **kwargs):
    """Weighted mean of the pass whose weighted covariance had the smallest top eigenvalue."""
    return gar.caf(gradients, f, iters, max_passes)


def check(gradients, f=0, iters=16, max_passes=None, **kwargs):
    msg = check_gradients(gradients)
    if msg:
        return msg
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or f < 0 or 2 * f + 1 > n:
        return f"Invalid number of Byzantine gradients to tolerate, got f = {f!r}, expected 0 <= f <= {(n - 1) // 2}"
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 1:
        return f"Invalid number of power iterations, got iters = {iters!r}, expected an int >= 1"
    if max_passes is not None and (not isinstance(max_passes, int) or isinstance(max_passes, bool) or max_passes < 1):
        return f"Invalid number of filter passes, got max_passes = {max_passes!r}, expected None or an int >= 1"
    return None


def influence(honests, attacks, f=0, iters=16, max_passes=None, **kwargs):
    """The weight that lies on the attack gradients."""
    w = gar.caf_weights(list(honests) + list(attacks), f, iters, max_passes).detach().double().cpu()
    return float(w[len(honests):].sum())


# no variance-to-norm bound is claimed: upper_bound stays None
register("caf", aggregate, check, influence=influence)
