"""SMEA GAR (new, absent from the reference; smallest maximum eigenvalue averaging, Allouah, Guerraoui, Gupta,
Pinot and Stephan, ICML 2023): the average of the (n - f)-subset whose empirical covariance has the smallest
top eigenvalue. The exact counterpart of Brute (smallest diameter) and of the spectral filters ``dnc`` and
``caf``; the subset search runs on the GPU, every subset scored by ``iters`` power rounds on its block of the
pairwise distances alone (``docs/GAR_SEMANTICS.md``)."""
import math

from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import accepted_ratio, check_gradients, n_of
from garfield_amd.ops import gar


def aggregate(gradients, f=0, iters=16, **kwargs):
    """Average of the n - f gradients whose covariance has the smallest top eigenvalue."""
    return gar.smea(gradients, f, iters)


def check(gradients, f=0, iters=16, **kwargs):
    msg = check_gradients(gradients)
    if msg:
        return msg
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or not 0 <= f < n:
        return f"Invalid number of Byzantine gradients to tolerate, got f = {f!r}, expected 0 <= f <= {n - 1}"
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 1:
        return f"Invalid number of power iterations, got iters = {iters!r}, expected an int >= 1"
    if math.comb(n, n - f) > gar.SMEA_MAX_SUBSETS:
        return (f"Too many subsets to enumerate, C({n}, {n - f}) = {math.comb(n, n - f)}, expected at most "
                f"{gar.SMEA_MAX_SUBSETS}")
    return None


def influence(honests, attacks, f=0, iters=16, **kwargs):
    """Ratio of accepted Byzantine gradients among the selected ones."""
    return accepted_ratio(gar.smea_weights(list(honests) + list(attacks), f, iters), len(honests))


# the paper's guarantee is about the honest covariance, not a variance-to-norm ratio: upper_bound stays None
register("smea", aggregate, check, influence=influence)
