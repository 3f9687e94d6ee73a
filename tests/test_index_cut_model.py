"""CPU model of the index cut under the half probe (dist_index.hip: idx_kmax_kernel with vcut,
the level-1 kernels' drop, probe_rows_kernel<HALF>), no GPU.

One sorted set against itself at sketch size S.  V* is the largest value any row probes: the
maximum over the non-empty rows of row[H_r - 1], H_r the row's visited prefix (ceil(S / 2) for
a row of at least S entries, else the whole row).  The index holds only the entries whose
value is <= V*; everything else is the half rule of test_probe_half_model.py, whose helpers
are used as they are: row q probes its visited prefix, an event pairs two entries of the same
coarse key (value >> shift: the bucket and an fbits-wide fingerprint), entries carry the flag
"inside its own row's visited prefix", and q takes (seen & M) | (seen & ~both & ~M).

Checked against the literal walk: every pair whose (numer, denom) differs from the defaults
(0, min(S, la + lb)) is taken exactly once, no pair twice, and the cut takes exactly the pairs
of the whole index except pairs seen only through a collision with a dropped entry.
"""
import numpy as np
import pytest

from test_probe_half_model import literal, make_rows, owns, taken_by, visited


def v_star(rows, S):
    """the largest probed value (idx_kmax_kernel with the cut); None when every row is empty"""
    tops = [int(row[visited(len(row), S) - 1]) for row in rows if len(row)]
    return max(tops) if tops else None


def taken_by_cut(rows, S, shift):
    """taken[q] under the half rule over the index of the values <= V*; also (V*, the entries
    indexed, the entries of the rows)"""
    vs = v_star(rows, S)
    index, indexed = {}, 0                       # coarse key -> [(ref, flag)]
    for r, row in enumerate(rows):
        h = visited(len(row), S)
        for pos, v in enumerate(row):
            if int(v) > vs:                      # a key equal to the cut is kept
                assert pos >= h, "an entry inside its row's visited prefix lies above V*"
                continue
            index.setdefault(int(v) >> shift, []).append((r, pos < h))
            indexed += 1
    taken = []
    for q, row in enumerate(rows):
        seen, both = set(), set()
        for v in row[:visited(len(row), S)]:
            # every probed value is <= V*, so at least the row's own entry is there
            post = index[int(v) >> shift]
            assert (q, True) in post
            for r, flag in post:
                seen.add(r)
                if flag:
                    both.add(r)
        taken.append({r for r in seen if owns(q, r) or r not in both})
    return taken, vs, indexed, sum(len(x) for x in rows)


def check(rows, S, shift):
    """each pair at most once, every pair off the defaults exactly once -> (V*, indexed, all,
    pairs off the defaults)"""
    taken, vs, indexed, entries = taken_by_cut(rows, S, shift)
    whole = taken_by(rows, S, shift)
    needed = 0
    for q in range(len(rows)):
        # the cut only removes events: a pair it takes is a pair the whole index shows too
        for r in taken[q]:
            assert r in whole[q] or q in whole[r], (q, r)
        for r in range(q, len(rows)):
            times = (r in taken[q]) + (q != r and q in taken[r])
            assert times <= 1, (q, r, "taken twice")
            la, lb = len(rows[q]), len(rows[r])
            cell = literal(rows[q], rows[r], S)
            if cell != (0, min(S, la + lb)):
                needed += 1
                assert times == 1, (q, r, la, lb, cell, "not taken")
    return vs, indexed, entries, needed


def long_rows(rng, S, n=24):
    """rows of S, S + 5 and 2 S values (none shorter than S: the cut is a real one) from a
    small range, so that pairs share values at every pair of positions.  The values are
    multiples of 8; behind its visited prefix a row holds some of them plus 1, which under a
    coarse key (shift >= 1) collide with the plain value in other rows, below V* and above.
    One row gets V* + 1 behind its prefix: dropped, and colliding with V* itself."""
    top = 3 * S + 8
    H = visited(S, S)
    rows = []
    for i in range(n):
        x = np.sort(rng.choice(top, size=(S, S + 5, 2 * S)[i % 3], replace=False)).astype(np.uint64)
        x = x * np.uint64(8)
        x[H:] += (rng.random(len(x) - H) < 0.3).astype(np.uint64)
        rows.append(x)
    vs = v_star(rows, S)
    assert vs % 8 == 0
    b = next(r for r in range(n) if int(rows[r][H - 1]) < vs
             and not {vs, vs + 1} & {int(v) for v in rows[r]})
    rows[b] = np.sort(np.append(rows[b], np.uint64(vs + 1)))
    assert v_star(rows, S) == vs
    return [rows[i] for i in rng.permutation(n)]


def straddles(rows, vs, shift):
    """dropped values that share their coarse key with an indexed one"""
    vals = {int(v) for row in rows for v in row}
    kept = {v >> shift for v in vals if v <= vs}
    return [v for v in vals if v > vs and (v >> shift) in kept]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 8, 9, 33])
def test_cut_index_takes_each_pair_once(S, shift):
    """rows of at least S values, odd and even S: a real cut (entries dropped) and, with
    fingerprints of 1-3 bits, collisions between an indexed and a dropped value"""
    rng = np.random.default_rng(1000 * S + shift)
    rows = long_rows(rng, S)
    vs, indexed, entries, needed = check(rows, S, shift)
    assert indexed < entries and needed > 0
    assert vs < max(int(row[-1]) for row in rows)
    if shift and S > 1:
        assert straddles(rows, vs, shift), "no collision straddles V*"


@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("S", [2, 3, 8, 33])
def test_rows_shorter_than_S(S, shift):
    """test_probe_half_model's set: rows of 0, 1, S / 2, S - 1 entries beside the long ones.  A
    short row is probed whole, so V* rises to its last value and fewer entries are dropped"""
    rng = np.random.default_rng(100 * S + shift)
    rows = make_rows(rng, S)
    assert any(0 < len(x) < S for x in rows) and any(len(x) == 0 for x in rows)
    vs, indexed, entries, needed = check(rows, S, shift)
    assert needed > 0 and indexed <= entries
    # not below the long rows' own cut, and never above the largest value held
    assert v_star([x for x in rows if len(x) >= S], S) <= vs <= max(int(x[-1]) for x in rows if len(x))


def test_only_short_rows_index_everything():
    S = 8
    rng = np.random.default_rng(5)
    rows = [np.sort(rng.choice(40, size=n, replace=False)).astype(np.uint64)
            for n in (0, 1, 3, 7, 7, 5, 2, 6)]
    vs, indexed, entries, needed = check(rows, S, 0)
    assert indexed == entries and vs == max(int(x[-1]) for x in rows if len(x)) and needed > 0


@pytest.mark.parametrize("shift", [0, 1, 3])
@pytest.mark.parametrize("S", [8, 9])
def test_shared_value_at_the_cut(S, shift):
    """The value V* itself shared with another row, beyond that row's own visited prefix: the
    entry is kept (<= V*), and the row that holds V* at position H - 1 sees the pair.  A value
    just above V* shared by two rows is dropped, and nothing is lost by it."""
    H = (S + 1) // 2
    rng = np.random.default_rng(77 * S + shift)
    # values spaced by 16, so that + 1 .. + 15 are free and collide with their base value
    pool = np.arange(1, 6 * S, dtype=np.uint64) * np.uint64(16)
    rows = [np.sort(rng.choice(pool[:4 * S], size=S, replace=False)) for _ in range(10)]
    vs = v_star(rows, S)
    a = max(range(len(rows)), key=lambda r: int(rows[r][H - 1]))
    assert int(rows[a][H - 1]) == vs
    # b and c: H values below everything else they hold, then V* (b) and V* + 1 (b and c) behind
    low = pool[:4 * S][pool[:4 * S] < np.uint64(vs)]
    assert len(low) >= H
    for _ in range(2):
        head = np.sort(rng.choice(low, size=H, replace=False))
        tail = pool[4 * S:4 * S + S - H]
        rows.append(np.concatenate([head, tail]))
    b, c = len(rows) - 2, len(rows) - 1
    rows[b] = np.sort(np.concatenate([rows[b][:-2], [np.uint64(vs), np.uint64(vs + 1)]]))
    rows[c] = np.sort(np.concatenate([rows[c][:-1], [np.uint64(vs + 1)]]))
    for r in (b, c):
        assert len(rows[r]) == S and len(np.unique(rows[r])) == S
    assert v_star(rows, S) == vs
    pos = int(np.flatnonzero(rows[b] == np.uint64(vs))[0])
    assert pos >= H and int(rows[b][pos + 1]) == vs + 1
    assert np.uint64(vs + 1) in rows[c] and np.uint64(vs) not in rows[c]
    taken, vs2, indexed, entries = taken_by_cut(rows, S, shift)
    assert vs2 == vs and indexed < entries
    # the pair (a, b) is seen through V*: by a, whose prefix ends on it
    assert (b in taken[a]) + (a in taken[b]) == 1
    check(rows, S, shift)
