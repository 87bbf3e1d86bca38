"""Centered-clipping GAR (new, absent from the reference; Karimireddy, He, Jaggi, ICML 2021):
``iters`` rounds of v <- v + (1/n) Σ_i (x_i - v) min(1, tau / ||x_i - v||), iterated on the pairwise
distances alone (``docs/GAR_SEMANTICS.md`` "Centered clipping"). ``tau=None`` takes the radius from the
data (the (n - f)-th smallest distance to the centre, every round); ``start="krum"`` starts from the
Multi-Krum average instead of the plain mean, so a large attack is left behind in the first round."""
from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import check_gradients, n_of
from garfield_amd.aggregators.krum import check as _krum_check
from garfield_amd.ops import gar


def aggregate(gradients, f=0, tau=None, iters=3, start=None, center=None, m=None, **kwargs):
    """Centered clipping: Σ_i a_i g_i with the clipped-iteration weights a."""
    return gar.cclip(gradients, f, tau, iters, start, center, m)


def check(gradients, f=0, tau=None, iters=3, start=None, center=None, m=None, **kwargs):
    msg = check_gradients(gradients)
    if msg:
        return msg
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or f < 0 or 2 * f + 1 > n:
        return f"Invalid number of Byzantine gradients to tolerate, got f = {f!r}, expected 0 <= f <= {(n - 1) // 2}"
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 1:
        return f"Invalid number of clipping iterations, got iters = {iters!r}, expected an int >= 1"
    if tau is not None and (isinstance(tau, bool) or not isinstance(tau, (int, float)) or not tau > 0):
        return f"Invalid clipping radius, got tau = {tau!r}, expected None (from the data) or tau > 0"
    if center is not None and start is not None:
        return "Invalid start, got both a center and a start, expected at most one of them"
    if isinstance(start, str):
        if start not in gar.CCLIP_STARTS:
            return f"Invalid start, got start = {start!r}, expected one of {gar.CCLIP_STARTS} or an [n] weight tensor"
        if start == "krum":
            return _krum_check(gradients=gradients, f=f, m=m)
    elif start is not None and (not hasattr(start, "numel") or start.numel() != n):
        return f"Invalid start, expected one of {gar.CCLIP_STARTS} or a weight tensor of {n} entries"
    return None


def influence(honests, attacks, f=0, tau=None, iters=3, start=None, center=None, m=None, **kwargs):
    """Total weight of the attack gradients (the weights are continuous: every row is 'accepted')."""
    w = gar.cclip_weights(list(honests) + list(attacks), f, tau, iters, start, center, m).detach().double().cpu()
    return float(w[len(honests):len(honests) + len(attacks)].sum())


# no variance-to-norm bound is claimed: upper_bound stays None
register("cclip", aggregate, check, influence=influence)
