"""DnC spectral-filtering GAR (new, absent from the reference; Shejwalkar & Houmansadr, NDSS 2021): every
row is scored by its squared projection on the top principal direction of the centred gradients, and the
``m = n - f`` lowest-scoring rows are averaged. The scores come from ``iters`` power rounds on the doubly
centred pairwise distances alone (``docs/GAR_SEMANTICS.md``): all coordinates, no SVD, no sub-sampling."""
from garfield_amd.aggregators import register
from garfield_amd.aggregators._common import check_gradients, n_of
from garfield_amd.ops import gar


def aggregate(gradients, f=0, m=None, iters=16, **kwargs):
    """Average of the m rows (default n - f) of lowest spectral outlier score."""
    return gar.dnc(gradients, f, m, iters)


def check(gradients, f=0, m=None, iters=16, **kwargs):
    msg = check_gradients(gradients)
    if msg:
        return msg
    n = n_of(gradients)
    if not isinstance(f, int) or isinstance(f, bool) or f < 0 or 2 * f + 1 > n:
        return f"Invalid number of Byzantine gradients to tolerate, got f = {f!r}, expected 0 <= f <= {(n - 1) // 2}"
    if m is not None and (not isinstance(m, int) or isinstance(m, bool) or m < 1 or m > n):
        return f"Invalid number of selected gradients, got m = {m!r}, expected 1 <= m <= {n}"
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 1:
        return f"Invalid number of power iterations, got iters = {iters!r}, expected an int >= 1"
    return None


def influence(honests, attacks, f=0, m=None, iters=16, **kwargs):
    """The kept weight that lies on the attack gradients."""
    w = gar.dnc_weights(list(honests) + list(attacks), f, m, iters).detach().double().cpu()
    return float(w[len(honests):].sum())


# no variance-to-norm bound is claimed: upper_bound stays None
register("dnc", aggregate, check, influence=influence)
