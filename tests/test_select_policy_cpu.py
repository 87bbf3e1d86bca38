"""The validity policy of the iterated Gram selections on the CPU (gar_cpu.cpp: valid_rows, Usable):
cpu_geomed_weights, cpu_cclip_weights and cpu_dnc_weights against reference.py on the crafted cases of
_select_policy_common.py."""
import pytest

import _select_policy_common as sp
from garfield_amd.ops.selection import distances_from_gram


def run(native, rule, n, case):
    """(weights, DnC's scores or None) of the native CPU rule on fill_distances' distances of the crafted Gram."""
    D = distances_from_gram(sp.gram(n, case))
    if rule == "geomed":
        return native.cpu_geomed_weights(D, 32, 1e-6), None
    if rule == "cclip":
        return native.cpu_cclip_weights(D, sp.nw_of(rule, n, case), None, 0.0, sp.F, 3), None
    return native.cpu_dnc_weights(D, n - 3, 16)


@pytest.mark.parametrize("n", sp.SIZES)
@pytest.mark.parametrize("rule,case", sp.CASES)
def test_unusable_pair_and_invalid_row(native, rule, case, n):
    sp.check(rule, n, case, *run(native, rule, n, case))


@pytest.mark.parametrize("rule", sp.RULES)
def test_every_pair_non_finite(native, rule):
    sp.check(rule, 4, "d", *run(native, rule, 4, "d"))
