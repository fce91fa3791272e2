"""The block planners of the surrogate null tests (`significance.sliding_plan`, `ensemble_plan`, `stack_plan`,
`surrogate_blocks`): pure integer functions, so what a GPU run would only show as a dropped or repeated surrogate is
checked here -- every (surrogate, item) pair in exactly one block, Welford's order, the finalising blocks, the chunk
bound, and literals worked by hand from the rule the planners restate."""
import numpy as np
import pytest

from hyperscanning_signal_analysis_amd import significance as sn


def _check_cover(blocks, S, n_items, item_range):
    """blocks: [(s0, sb, r0, r1, last)], item_range(r0, r1) -> (i0, i1).  Returns the (items, surrogates) sizes."""
    seen = np.zeros((S, n_items), dtype=np.int64)
    done, sizes, prev_s0 = {}, [], 0
    for s0, sb, r0, r1, last in blocks:
        i0, i1 = item_range(r0, r1)
        assert 1 <= sb and 0 <= s0 and s0 + sb <= S and 0 <= i0 <= i1 <= n_items
        assert s0 >= prev_s0                                        # surrogate blocks ascending: Welford's order
        prev_s0 = s0
        assert done.get((r0, r1), 0) == s0                           # ... and without a gap within every row range
        done[(r0, r1)] = s0 + sb
        assert last == (s0 + sb == S)
        seen[s0:s0 + sb, i0:i1] += 1
        sizes.append((i1 - i0, sb))
    assert (seen == 1).all()                                        # every (surrogate, item) pair in exactly one block
    assert all(v == S for v in done.values())                       # one finalising block per row range
    assert sum(last for *_, last in blocks) == len(done)
    return sizes


SLIDING = [(5, 4, 1), (5, 4, 3), (5, 4, 4), (5, 4, 5), (5, 4, 9), (5, 4, 20), (5, 4, 100), (1, 4, 1), (1, 4, 4), (1, 4, 5),
           (1, 1, 1), (7, 1, 3), (3, 10, 7), (3, 10, 29), (3, 10, 30), (3, 10, 31), (8, 3, 8)]


@pytest.mark.parametrize("S,W,chunk", SLIDING)
def test_sliding_blocks(S, W, chunk):
    Sb, Wb = sn.sliding_plan(S, W, chunk)
    assert (Sb, Wb) == (min(S, max(1, chunk // W)) if chunk >= W else 1, min(W, chunk))
    blocks = list(sn.surrogate_blocks(S, Sb, sn.window_ranges(W, Wb)))
    sizes = _check_cover(blocks, S, W, lambda w0, w1: (w0, w1))
    assert all(wb >= 1 and sb * wb <= chunk for wb, sb in sizes)    # a window is one item: no block exceeds the chunk
    assert blocks[0][1] * (blocks[0][3] - blocks[0][2]) == Sb * Wb == max(sb * wb for wb, sb in sizes)
    # the condition contrast: a surrogate is two mix rows of each of wb windows, and only Sb is used
    for wb in range(1, 6):
        assert sn.sliding_plan(S, 2 * wb, chunk)[0] == max(1, min(S, chunk // (2 * wb)))


def test_sliding_literals():
    assert sn.sliding_plan(5, 4, 9) == (2, 4)
    assert sn.sliding_plan(5, 4, 3) == (1, 3)
    assert sn.window_ranges(4, 3) == [(0, 3), (3, 4)]
    assert [b[2:4] for b in sn.surrogate_blocks(5, 1, sn.window_ranges(4, 3))] == [(0, 3), (3, 4)] * 5
    assert sn.sliding_plan(5, 4, 100) == (5, 4)
    assert list(sn.surrogate_blocks(5, 2, [(0, 4)])) == [(0, 2, 0, 4, False), (2, 2, 0, 4, False), (4, 1, 0, 4, True)]


def _inline_ensemble_rule(first, S, chunk):
    """The rule as `ensemble_significance` stated it inline before the planners existed."""
    G, N = len(first) - 1, int(first[-1])
    if N <= chunk:
        return min(S, chunk // N), [(0, G)]
    Sb, blocks, g0 = 1, [], 0
    while g0 < G:
        g1 = g0 + 1
        while g1 < G and first[g1 + 1] - first[g0] <= chunk:
            g1 += 1
        blocks.append((g0, g1))
        g0 = g1
    return Sb, blocks


THREES, GAP, UNEVEN = [0, 3, 6, 9], [0, 3, 3, 6], [0, 1, 6, 8, 8, 12]
ENSEMBLE = [(first, S, chunk) for first in (THREES, GAP, UNEVEN) for S in (1, 5)
            for chunk in sorted({1, 2, 3, 4, 6, first[-1] - 1, first[-1], first[-1] + 1, 2 * first[-1], S * first[-1], 100})]


@pytest.mark.parametrize("first,S,chunk", ENSEMBLE)
def test_ensemble_blocks(first, S, chunk):
    first = np.asarray(first)
    N = int(first[-1])
    Sb, groups = sn.ensemble_plan(first, S, chunk)
    assert (Sb, groups) == _inline_ensemble_rule(first, S, chunk)
    assert groups[0][0] == 0 and groups[-1][1] == len(first) - 1 and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    blocks = list(sn.surrogate_blocks(S, Sb, groups))
    _check_cover(blocks, S, N, lambda g0, g1: (int(first[g0]), int(first[g1])))
    for s0, sb, g0, g1, last in blocks:
        items = int(first[g1] - first[g0])
        if sb * items > chunk:                      # only a single group that is itself larger than the chunk
            assert sb == 1 and g1 == g0 + 1 and items > chunk
    if N <= chunk:
        assert groups == [(0, len(first) - 1)] and Sb == min(S, chunk // N)       # whole surrogates
    else:
        assert Sb == 1                                                            # whole groups of one surrogate


def test_ensemble_literals():
    assert sn.ensemble_plan(THREES, 5, 9) == (1, [(0, 3)])
    assert sn.ensemble_plan(THREES, 5, 20) == (2, [(0, 3)])
    assert sn.ensemble_plan(THREES, 5, 6) == (1, [(0, 2), (2, 3)])
    assert sn.ensemble_plan(THREES, 5, 1) == (1, [(0, 1), (1, 2), (2, 3)])      # a group larger than the chunk goes whole
    # a group without items: it joins a block where it fits and stands alone, as a block the driver skips, where not
    assert sn.ensemble_plan(GAP, 5, 3) == (1, [(0, 2), (2, 3)])
    assert sn.ensemble_plan(GAP, 5, 2) == (1, [(0, 1), (1, 2), (2, 3)])
    assert GAP[1] == GAP[2]


@pytest.mark.parametrize("E,W,per_window,cap", [(4, 10, 100, 4000), (4, 10, 100, 3999), (4, 10, 100, 400), (4, 10, 100, 399),
                                                (4, 10, 100, 0), (1, 1, 8, 8), (7, 5, 4096, 1 << 16), (3, 9, 1 << 20, 12 << 30)])
def test_stack_blocks(E, W, per_window, cap):
    Wb = sn.stack_plan(E, W, per_window, cap)
    assert Wb == (W if E * W * per_window <= cap else max(1, cap // (E * per_window)))
    assert 1 <= Wb <= W and (Wb == 1 or E * Wb * per_window <= cap)
    assert Wb == W or E * (Wb + 1) * per_window > cap                             # as many windows as fit
    r = sn.window_ranges(W, Wb)
    assert r[0][0] == 0 and r[-1][1] == W and all(a[1] == b[0] for a, b in zip(r, r[1:]))
    assert sn.stack_plan(4, 10, 100, 3999) == 9 and sn.stack_plan(4, 10, 100, 0) == 1
