"""The recipe list of a batch that reads the spaced tables: this strand's PAM-pair list without the class "no
substitution in X, all m in O" - and nothing else missing.  The class is enumerated here from its definition; the
trimmed list plus the class must be the whole list as a multiset, so that every site still has exactly one source.
Host only."""
import ctypes as C
from collections import Counter
from importlib import import_module
from itertools import combinations, product

import pytest

api = import_module("guidescan-cli_amd.api")

L, P = 20, 3


def thresholds(m, k, x_len):
    """a*(o) as a batch on PAM-pair + deep tables plans them (gs_enumerate.hip: plan_thresholds)"""
    lib = api.lib()
    lib.gs_debug_choose_thresholds.restype = None
    lib.gs_debug_choose_thresholds.argtypes = [C.c_uint32] * 4 + [C.c_double] * 3 + [C.c_void_p]
    out = (C.c_uint32 * 8)()
    lib.gs_debug_choose_thresholds(m, x_len, k - x_len, L - k, 1.0, 0.4, 1.6, out)
    return [int(x) for x in out]


def substitutions(word):
    """a recipe as the set of its (consumption step, digit) pairs"""
    word = int(word)
    n = word & 7
    return tuple(sorted(((word >> (12 + 7 * i)) & 127) for i in range(n)))


def the_class(m, k, x_len):
    """every way to substitute exactly m of the steps x_len .. k-1, each by one of the three other bases"""
    return [tuple(sorted((s << 2) | d for s, d in zip(steps, digits)))
            for steps in combinations(range(x_len, k), m) for digits in product(range(3), repeat=m)]


@pytest.mark.parametrize("k,x_len", [(14, 8), (13, 9)])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_trimmed_list_plus_the_class_is_the_whole_list(m, k, x_len):
    astar = thresholds(m, k, x_len)
    full = Counter(substitutions(w) for w in api.seed_recipes_a8(k, m, x_len, astar))
    trimmed = Counter(substitutions(w) for w in api.seed_recipes_a8(k, m, x_len, astar, trimmed=True))
    cls = Counter(the_class(m, k, x_len))
    assert max(full.values()) == 1                       # a seed is listed once
    if astar[m] == 0:                                    # the class is the other strand's: nothing to take out
        assert not (set(cls) & set(full))
        cls = Counter()
    assert sum(cls.values()) == (len(list(combinations(range(k - x_len), m))) * 3 ** m if astar[m] else 0)
    assert trimmed + cls == full
    assert not (set(trimmed) & set(cls))


def test_the_class_at_the_headline_shape_has_540_recipes():
    astar = thresholds(3, 14, 8)
    assert astar[3] > 0
    n_full = api.seed_recipes_a8(14, 3, 8, astar).shape[0]
    n_trim = api.seed_recipes_a8(14, 3, 8, astar, trimmed=True).shape[0]
    assert (n_full, n_trim) == (1150, 610)
