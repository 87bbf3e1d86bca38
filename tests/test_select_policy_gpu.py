"""The validity policy of the iterated Gram selections on the GPU (gar_select.hpp: load_valid_distances,
zero_infinite_distances): k_geomed_select, k_cclip_select and k_dnc_select fed the crafted Gram matrices of
_select_policy_common.py directly, against reference.py on the same fp32 distances."""
import pytest
import torch

import _select_policy_common as sp

pytestmark = pytest.mark.gpu


def run(native, cuda, rule, n, cases, nw=None):
    """(weights [B, n], dists or scores [B, n]) of one launch on the batch of crafted Grams `cases`."""
    B, np_ = len(cases), native.gram_padded(n)
    g = torch.zeros(B, np_, np_)
    for b, case in enumerate(cases):
        g[b, :n, :n] = sp.gram(n, case)
    g = g.to(cuda)
    w = torch.full((B, n), -1.0, device=cuda)
    aux = torch.full((B, n), -1.0, device=cuda)
    if rule == "geomed":
        native.gpu_geomed_select(g, n, 32, 1e-6, w, aux, B)
    elif rule == "cclip":
        native.gpu_cclip_select(g, n, nw or sp.nw_of(rule, n, cases[0]), None, 0.0, sp.F, 3, w, aux, B)
    else:
        native.gpu_dnc_select(g, n, n - 3, 16, w, aux, B)
    return w.cpu(), aux.cpu()


@pytest.mark.parametrize("n", sp.SIZES)
@pytest.mark.parametrize("rule,case", sp.CASES)
def test_unusable_pair_and_invalid_row(cuda, native, rule, case, n):
    w, aux = run(native, cuda, rule, n, [case])
    sp.check(rule, n, case, w[0], aux[0])


@pytest.mark.parametrize("rule", sp.RULES)
def test_every_pair_non_finite(cuda, native, rule):
    w, aux = run(native, cuda, rule, 4, ["d"])
    sp.check(rule, 4, "d", w[0], aux[0])


@pytest.mark.parametrize("rule", sp.RULES)
def test_batch_equals_single_launches(cuda, native, rule):
    """(a), (b) and (d) at one n in one launch (centered clipping: with a basis-only last row)."""
    n, cases = 17, ["a", "b", "d"]
    wb, ab = run(native, cuda, rule, n, cases, n - 1)
    for b, case in enumerate(cases):
        w1, a1 = run(native, cuda, rule, n, [case], n - 1)
        assert torch.equal(w1[0], wb[b]) and torch.equal(a1[0], ab[b])
    assert not torch.equal(wb[0], wb[1]) and ab[2].tolist() == [0.0] * n
