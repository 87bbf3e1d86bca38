"""Shared by test_worker_momentum_cpu.py and test_worker_momentum_gpu.py: the case grid of the
worker-momentum operator and the check of one call against the fp64 oracle."""
import torch

from garfield_amd.ops import reference as ref

KS = (1, 3, 8)
DS = (1, 7, 8, 9, 1000, 4099)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
BETAS = (0.5, 0.9, 0.99)
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def ranges(d: int, extra_los=()) -> list:
    """Whole row, (3, d - 2), (0, 1), an empty range, and (lo, d) for every further lo that fits."""
    out = [(0, d), (0, 1), (min(2, d), min(2, d))]
    if d - 2 >= 3:
        out.append((3, d - 2))
    out += [(lo, d) for lo in extra_los if lo < d]
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(_BITS[t.dtype])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def inputs(k: int, ld: int, dtype, seed: int, device="cpu"):
    """Rows (values of both signs and a few magnitudes) and a previous state, generated on the CPU."""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(k, ld, generator=g) * torch.tensor([1e-3, 1.0, 30.0])[torch.randint(0, 3, (k, ld), generator=g)])
    M = torch.randn(k, ld, generator=g)
    return X.to(dtype).to(device), M.to(device)


def check(X0, M0, X1, M1, beta: float, first: bool, lo: int, hi: int) -> None:
    """(X1, M1) = one update of (X0, M0) on [lo, hi) (all [k, ld] views, any device). The state within
    |m - m64| <= 4 * 2^-24 * (beta |m_prev| + (1 - beta) |g|) of the fp64 oracle per element (the
    roundings of omega, of the product and of the fma; exact on the first step), unchanged where g is
    not finite; the row = the state rounded to the row's dtype, the non-finite g kept; both buffers
    bit-unchanged outside [lo, hi)."""
    X0, M0, X1, M1 = (t.detach().cpu() for t in (X0, M0, X1, M1))
    m64, finite = ref.worker_momentum(X0, M0, beta, first, lo, hi)
    g, mp = X0[:, lo:hi].double(), M0[:, lo:hi].double()
    bound = torch.zeros_like(g) if first else 4 * 2.0 ** -24 * (beta * mp.abs() + (1 - beta) * g.abs())
    got = M1[:, lo:hi]
    err = (got.double() - m64).abs()
    assert bool((err[finite] <= bound[finite]).all()), float((err[finite] - bound[finite]).max())
    assert same_bits(got[~finite], M0[:, lo:hi][~finite])                       # the state stays
    assert same_bits(X1[:, lo:hi][finite], got.to(X0.dtype)[finite])            # row = cast(state)
    assert same_bits(X1[:, lo:hi][~finite], X0[:, lo:hi][~finite])              # the row keeps it
    for a, b in ((X0, X1), (M0, M1)):
        assert same_bits(a[:, :lo], b[:, :lo]) and same_bits(a[:, hi:], b[:, hi:])
