"""CPU model of the half probe's pair rule (dist_index.hip, probe_rows_kernel<HALF>), no GPU.

One sorted set against itself at sketch size S.  Row r's visited prefix is its positions
[0, H_r), H_r = ceil(S / 2) for a row of at least S entries, else the whole row.  Row q probes
only its visited prefix against the full index; an event pairs two entries of the same coarse
key (bucket + fingerprint, here value >> shift).  Every entry carries the flag "inside its own
row's visited prefix".  Row q keeps seen[r] (some probed hash hit an entry of r) and both[r]
(such an entry was flagged) and takes (seen & M) | (seen & ~both & ~M), M the pair-parity
owner mask of word_mask.

Checked against the literal walk (CommandDistance.cpp:376-400): every pair whose (numer, denom)
differs from the defaults (0, min(S, la + lb)) is taken exactly once, and no pair twice.
"""
import numpy as np
import pytest


def literal(a, b, S):
    """(common, denom) of compareSketches' walk over two ascending distinct lists"""
    i = j = common = denom = 0
    while denom < S and i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif a[i] > b[j]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
        denom += 1
    if denom < S:
        denom += (len(a) - i) + (len(b) - j)
        denom = min(denom, S)
    return common, denom


def owns(q, r):
    """word_mask: the pair {q, r} belongs to the lower row when q + r is odd, to the higher
    row (and the diagonal) when it is even"""
    return r > q if (q + r) & 1 else r <= q


def visited(length, S):
    return (S + 1) // 2 if length >= S else length


def taken_by(rows, S, shift):
    """taken[q] = the refs row q appends as candidates under the half rule"""
    index = {}                                   # coarse key -> [(ref, flag)]
    for r, row in enumerate(rows):
        h = visited(len(row), S)
        for pos, v in enumerate(row):
            index.setdefault(int(v) >> shift, []).append((r, pos < h))
    taken = []
    for q, row in enumerate(rows):
        seen, both = set(), set()
        for v in row[:visited(len(row), S)]:
            for r, flag in index[int(v) >> shift]:
                seen.add(r)
                if flag:
                    both.add(r)
        taken.append({r for r in seen if owns(q, r) or r not in both})
    return taken


def make_rows(rng, S):
    """rows of 0, < S, S, S + 5 and 2 S values from a small range (so that pairs share values
    at every pair of positions, and neighbours collide under a coarse key)"""
    lens = sorted({0, 1, S // 2, S - 1, S, S + 5, 2 * S} - {-1})
    top = 3 * S + 8
    rows = []
    for rep in range(4):
        for n in lens:
            rows.append(np.sort(rng.choice(top, size=min(n, top), replace=False)).astype(np.uint64))
    # the order of the rows decides the owners: not by length
    return [rows[i] for i in rng.permutation(len(rows))]


@pytest.mark.parametrize("shift", [0, 2, 4])
@pytest.mark.parametrize("S", [1, 2, 3, 8, 33])
def test_half_rule_takes_each_pair_once(S, shift):
    rng = np.random.default_rng(100 * S + shift)
    rows = make_rows(rng, S)
    assert {0, S} <= {len(x) for x in rows} and max(len(x) for x in rows) > S
    assert S == 1 or any(0 < len(x) < S for x in rows)
    taken = taken_by(rows, S, shift)
    needed = empty = 0
    for q in range(len(rows)):
        for r in range(q, len(rows)):
            times = (r in taken[q]) + (q != r and q in taken[r])
            assert times <= 1, (q, r, "taken twice")
            la, lb = len(rows[q]), len(rows[r])
            cell = literal(rows[q], rows[r], S)
            assert cell == literal(rows[r], rows[q], S)
            if cell != (0, min(S, la + lb)):
                needed += 1
                assert times == 1, (q, r, la, lb, cell, "not taken")
            else:
                empty += 1
    # the set exercises both kinds of cell
    assert needed > 0 and empty > 0


def test_half_rule_visits_fewer_events():
    """what the rule is for: about half of the full probe's events on rows of S entries"""
    S, shift = 33, 0
    rng = np.random.default_rng(7)
    rows = [np.sort(rng.choice(200, size=S, replace=False)).astype(np.uint64) for _ in range(40)]
    count = {}
    for row in rows:
        for v in row:
            count[int(v)] = count.get(int(v), 0) + 1
    full = sum(count[int(v)] for row in rows for v in row)
    half = sum(count[int(v)] for row in rows for v in row[:visited(S, S)])
    assert half < 0.6 * full
