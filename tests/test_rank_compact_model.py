"""A model of the rank kernel's chunked walk over compacted candidate rows (dist.hip,
rank_rows_kernel with CMP; DESIGN §4, "The compacted candidate rows"), against oracle.compare.

One sorted set against itself.  Row r's compacted copy leaves out the values of its probed
prefix (positions below H = ceil(S / 2), or the whole row when it is shorter than S) that no
other row of the set holds, and keeps each remaining value's position in the row.  Candidate r
is streamed against row q in chunks of 128 kept values: the union rank of a kept value is
pos + j - k (j = #{B < a}, k = shared values below a), and the walk stops after a full chunk
whose last value ranks >= S unless both rows are shorter than S.  The diagonal is answered in
closed form.  numer and denom must equal the reference walk's for every pair, and on a
family-structured set the compacted walk must visit fewer chunks than the plain one.
"""
import numpy as np
import pytest

CHUNK = 128


def _prefix(length, S):
    return (S + 1) // 2 if length >= S else length


def _compact(rows, S):
    """[(kept values, their positions)] per row: the probe's classification, exactly (a value is
    kept iff another row holds it)"""
    allv = np.concatenate([np.asarray(x, np.uint64) for x in rows] + [np.zeros(0, np.uint64)])
    vals, cnt = np.unique(allv, return_counts=True)      # rows hold distinct values
    out = []
    for x in rows:
        x = np.asarray(x, np.uint64)
        H = _prefix(len(x), S)
        multi = cnt[np.searchsorted(vals, x)] >= 2
        keep = multi | (np.arange(len(x)) >= H)
        out.append((x[keep], np.nonzero(keep)[0].astype(np.uint32)))
    return out


def _rank(vals, pos, la, B, S):
    """(numer, denom, chunks visited) of the candidate (vals at positions pos of a row of la
    entries) against the sorted row B"""
    B = np.asarray(B, np.uint64)
    lb = len(B)
    need_all = la < S and lb < S
    shared = cnt = visits = 0
    for c0 in range(0, len(vals), CHUNK):
        a, p = vals[c0:c0 + CHUNK], pos[c0:c0 + CHUNK].astype(np.int64)
        last = c0 + CHUNK >= len(vals)
        j = np.searchsorted(B, a, side="left")
        eq = (j < lb) & (B[np.minimum(j, max(lb - 1, 0))] == a) if lb else np.zeros(len(a), bool)
        k = shared + np.cumsum(eq) - eq
        u = p + j - k
        cnt += int(np.count_nonzero(eq & (u < S)))
        shared += int(np.count_nonzero(eq))
        visits += 1
        if not last and not need_all and u[-1] >= S:
            break
    denom = min(S, la + lb - shared) if need_all else S
    return cnt, denom, visits


def _diagonal(length, S):
    return min(S, length), min(S, length)


def _check_set(oracle, rows, S):
    """every pair of the set, compacted and plain, against the reference walk -> (chunk visits
    compacted, plain) over the off-diagonal pairs"""
    rows = [np.asarray(x, np.uint64) for x in rows]
    comp = _compact(rows, S)
    vc = vp = 0
    for q, B in enumerate(rows):
        for r, A in enumerate(rows):
            exp = oracle.compare(A, B, S)
            if r == q:
                assert _diagonal(len(A), S) == exp, (q, S)
                continue
            nu, de, v = _rank(comp[r][0], comp[r][1], len(A), B, S)
            assert (nu, de) == exp, (r, q, S)
            nu, de, w = _rank(A, np.arange(len(A), dtype=np.uint32), len(A), B, S)
            assert (nu, de) == exp, (r, q, S)
            vc, vp = vc + v, vp + w
    return vc, vp


def _family_rows(rng, n_fam, members, lens, share=0.7):
    """sorted distinct u64 rows in families: a member takes each of its family's base values
    with probability `share` and fills up with values of its own"""
    rows = []
    for f in range(n_fam):
        base = rng.integers(1, 2 ** 63, size=max(lens) * 2, dtype=np.uint64)
        for m in range(members):
            ln = lens[(f * members + m) % len(lens)]
            pick = base[rng.random(len(base)) < share]
            own = rng.integers(1, 2 ** 63, size=ln, dtype=np.uint64)
            rows.append(np.unique(np.concatenate([pick, own]))[:ln])
    return rows


def test_family_sketches_s1000_visit_fewer_chunks(oracle):
    import fpmash.datagen as D
    S = 1000
    seqs = D.family_dna(2, 6, 2000, sub_rate=(0.0, 0.05), seed=1000)
    rows = oracle.sketch_batch(oracle.params(k=21, s=S), seqs)
    assert all(len(x) == S for x in rows)
    vc, vp = _check_set(oracle, rows, S)
    kept = sum(len(v) for v, _ in _compact(rows, S))
    assert kept < len(rows) * S
    assert vc < vp, (vc, vp)


@pytest.mark.parametrize("S", [1000, 64, 9])
def test_row_lengths_around_s(oracle, S):
    """rows shorter than, equal to and longer than S in one set (short rows are classified
    whole, and two short rows need every shared value for their denom)"""
    rng = np.random.default_rng(S)
    lens = [S, S - 1, S + 3, max(S // 3, 1), S, 2 * S, S // 2 + 1, 1]
    rows = _family_rows(rng, 2, 8, lens)
    assert {len(x) < S for x in rows} == {True, False}
    assert any(len(x) > S for x in rows)
    _check_set(oracle, rows + [np.zeros(0, np.uint64)], S)


@pytest.mark.parametrize("S", [1000, 64, 9])
def test_identical_and_disjoint_rows(oracle, S):
    rng = np.random.default_rng(100 + S)
    one = np.unique(rng.integers(1, 2 ** 63, size=S, dtype=np.uint64))
    same = [one.copy() for _ in range(4)]
    comp = _compact(same, S)
    assert all(len(v) == len(one) for v, _ in comp)          # nothing dropped
    _check_set(oracle, same, S)
    pool = np.unique(rng.integers(1, 2 ** 63, size=5 * S, dtype=np.uint64))
    apart = [pool[i::5][:S] for i in range(5)]
    comp = _compact(apart, S)
    H = (S + 1) // 2
    assert all(len(v) == len(x) - _prefix(len(x), S) for (v, _), x in zip(comp, apart))
    assert all(int(p[0]) == H for (_, p), x in zip(comp, apart) if len(x) >= S)
    _check_set(oracle, apart, S)


@pytest.mark.parametrize("S", [1000, 64, 9])
def test_shared_value_behind_one_prefix_inside_the_other(oracle, S):
    """the pair's only shared values sit at positions >= H in row 0 and < H in row 1: row 0
    keeps them in its tail, row 1 keeps exactly them of its prefix"""
    H = (S + 1) // 2
    rng = np.random.default_rng(200 + S)
    lowv = np.unique(rng.integers(1, 2 ** 40, size=H, dtype=np.uint64))
    assert len(lowv) == H
    mid = (np.uint64(1) << np.uint64(41)) + np.arange(2, dtype=np.uint64)
    high0 = np.unique(rng.integers(2 ** 42, 2 ** 62, size=S - H - 2, dtype=np.uint64))
    high1 = np.unique(rng.integers(2 ** 42, 2 ** 62, size=S - 2, dtype=np.uint64))
    rows = [np.concatenate([lowv, mid, high0]), np.concatenate([mid, high1])]
    assert all(np.all(np.diff(x.astype(object)) > 0) for x in rows)
    comp = _compact(rows, S)
    assert comp[0][1][0] == H and np.array_equal(comp[0][0][:2], mid)
    assert np.array_equal(comp[1][0][:2], mid) and list(comp[1][1][:2]) == [0, 1]
    assert len(rows[0]) == len(rows[1]) == S and len(comp[1][0]) == S - H + 2
    assert oracle.compare(rows[0], rows[1], S)[0] == 2      # union ranks H and H + 1, below S
    _check_set(oracle, rows, S)
