"""Geometric-median GAR (new, absent from the reference): the minimiser of the sum of L2
distances to the gradients, by ``iters`` rounds of smoothed Weiszfeld (RFA) iterated on the
pairwise distances alone (``docs/GAR_SEMANTICS.md``). Breakdown point 1/2: ``f`` only enters the
check (``2f + 1 <= n``), not the computation."""
from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import check_gradients, n_of
from garfield_amd.ops import gar


def aggregate(gradients, f=0, iters=32, nu=1e-6, **kwargs):
    """Geometric median: Σ_i a_i g_i with the smoothed-Weiszfeld weights a."""
    return gar.geomed(gradients, f, iters, nu)


def check(gradients, f=0, iters=32, nu=1e-6, **kwargs):
    msg = check_gradients(gradients)
    if msg:
        return msg
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or f < 0 or 2 * f + 1 > n:
        return f"Invalid number of Byzantine gradients to tolerate, got f = {f!r}, expected 0 <= f <= {(n - 1) // 2}"
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 1:
        return f"Invalid number of Weiszfeld iterations, got iters = {iters!r}, expected an int >= 1"
    if isinstance(nu, bool) or not isinstance(nu, (int, float)) or not nu > 0:
        return f"Invalid smoothing floor, got nu = {nu!r}, expected nu > 0"
    return None


def influence(honests, attacks, f=0, iters=32, nu=1e-6, **kwargs):
    """Total weight of the attack gradients (the weights are continuous: every row is 'accepted')."""
    w = gar.geomed_weights(list(honests) + list(attacks), iters, nu).detach().double().cpu()
    return float(w[len(honests):].sum())


# no variance-to-norm bound is claimed: upper_bound stays None
register("geomed", aggregate, check, influence=influence)
