"""CPU checks of the contain model (tests/contain_model.py): the closed form the fast kernel
computes equals the reference's literal walk on strictly ascending lists, is wrong on others,
and the -e threshold is compared as a float."""
import random

import numpy as np

import contain_model as M


def asc(rng, n, universe):
    return sorted(rng.sample(range(universe), n))


def test_closed_form_equals_literal_walk_on_ascending_lists():
    rng = random.Random(11)
    seen = set()
    for _ in range(20000):
        universe = rng.choice((4, 8, 14, 40))          # small: ties are common
        lr, lq = rng.randint(0, min(11, universe)), rng.randint(0, min(11, universe))
        R, Q = asc(rng, lr, universe), asc(rng, lq, universe)
        assert M.closed_form(R, Q) == M.literal(R, Q), (R, Q)
        if lr and lq:
            seen.add(("tie" if R[-1] in Q else "no-tie", (lr > lq) - (lr < lq)))
        else:
            seen.add(("empty", lr == 0, lq == 0))
    # every class the closed form distinguishes was drawn
    assert {("tie", -1), ("tie", 0), ("tie", 1), ("no-tie", -1), ("no-tie", 0), ("no-tie", 1),
            ("empty", True, True), ("empty", True, False), ("empty", False, True)} <= seen


def test_closed_form_named_cases():
    assert M.literal([], [1, 2]) == M.closed_form([], [1, 2]) == (0, 0)
    assert M.literal([1, 2], []) == M.closed_form([1, 2], []) == (0, 0)
    # maxR < Q[0]: R runs out before Q moves
    assert M.literal([1, 2, 3], [5, 6, 7]) == M.closed_form([1, 2, 3], [5, 6, 7]) == (0, 0)
    # a tie with R's maximum is inside the walk
    assert M.literal([2, 9], [1, 9, 12]) == M.closed_form([2, 9], [1, 9, 12]) == (1, 2)
    # maxR above all of Q: j stops at min(lr, lq)
    assert M.literal([1, 5, 99], [1, 2, 3, 4]) == M.closed_form([1, 5, 99], [1, 2, 3, 4]) == (1, 3)
    assert M.literal([1, 2, 3], [1, 2, 3]) == M.closed_form([1, 2, 3], [1, 2, 3]) == (3, 3)
    # Q[j] is never read at or past min(lr, lq)
    assert M.literal([7], [1, 2, 3]) == (0, 1)


def test_closed_form_is_wrong_on_an_unsorted_list():
    assert M.literal([3, 1], [1, 2]) == (0, 2)
    assert M.closed_form([3, 1], [1, 2]) == (1, 1)


def test_grid_ascending_equals_grid():
    rng = np.random.default_rng(5)
    rows = [np.unique(rng.integers(0, 300, n, dtype=np.uint64)) for n in (0, 1, 40, 90, 130)]
    a, b = M.grid(rows, rows), M.grid_ascending(rows, rows)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = M.grid(rows, rows, M.closed_form)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


def test_error_threshold_is_a_float():
    # 1 / sqrt(400) = 0.05 exactly in double, and float(0.05) = 0.0500000007... lets it through;
    # 1 / sqrt(399) = 0.05006...
    assert M.threshold(0.05) > 0.05
    assert M.line(200, 400, "r", "q", 0.05) == "0.5\t0.05\tr\tq"
    assert M.line(200, 399, "r", "q", 0.05) is None
    assert M.line(0, 0, "r", "q", 1.0) is None
    assert M.line(1, 1, "r", "q", 1.0) == "1\t1\tr\tq"
    assert M.line(1, 3, "r", "q", 1.0) == "0.333333\t0.57735\tr\tq"


def test_lines_are_query_major():
    refs, qrys = [[1, 2, 3], [2, 3, 4]], [[1, 2, 3], [3, 4, 5]]
    got = M.lines(refs, qrys, ["r0", "r1"], ["q0", "q1"], e=1)
    assert got == ("1\t0.57735\tr0\tq0\n" "0.666667\t0.57735\tr1\tq0\n"
                   "1\t1\tr0\tq1\n" "1\t0.707107\tr1\tq1\n")
