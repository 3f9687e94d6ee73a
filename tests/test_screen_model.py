"""tests/screen_model.py against itself: the literal dictionary loops (the reference lines) and
the closed form over sorted arrays (what the GPU path computes) agree on random and adversarial
inputs; the -w rule does not depend on the order a key's holders are visited in, except in full
ties, which go to the lowest index."""
import random

import numpy as np
import pytest

import reads_model as RM
import screen_model as M


def rand_db(rng, n, size, universe):
    return [np.sort(rng.choice(universe, size=int(rng.integers(0, size + 1)), replace=False))
            for _ in range(n)]


def as_matrix(rows, pad, dtype=np.uint64):
    """the rows in a matrix `pad` cells wider than the longest, the cells past each length
    holding the type's largest value (which a row may hold too)"""
    R = np.full((len(rows), max([len(r) for r in rows] + [0]) + pad), np.iinfo(dtype).max, dtype)
    for i, r in enumerate(rows):
        R[i, :len(r)] = r
    return R, np.array([len(r) for r in rows], np.uint32)


def same(rows, keys, **kw):
    a = M.literal(rows, keys, **kw)
    b = M.closed(rows, keys, **{k: v for k, v in kw.items() if k != "visit"})
    assert list(a[0]) == list(b[0])
    assert list(a[1]) == list(b[1])
    # the whole-matrix form (tests/test_gpu_screen_scale.py's reference) against the two
    if "visit" not in kw:
        U, cnt = M.closed_counts(rows, keys)
        for pad in (0, 3):
            R, lens = as_matrix(rows, pad)
            m = M.closed_matrix(R, lens, keys, lengths=kw.get("lengths"))
            assert np.array_equal(m["U"], U) and np.array_equal(m["count"], cnt)
            assert m["count"].dtype == np.uint32
            which = ("wshared", "wmedian") if kw.get("winner") else ("shared", "median")
            assert m[which[0]].tolist() == list(a[0]) and m[which[1]].tolist() == list(a[1])
            if kw.get("winner"):
                plain = M.literal(rows, keys)
                assert m["shared"].tolist() == plain[0] and m["median"].tolist() == plain[1]
    return a


@pytest.mark.parametrize("seed", range(6))
def test_random(seed):
    rng = np.random.default_rng(seed)
    universe = np.unique(rng.integers(1, 2 ** 63, size=400, dtype=np.uint64))
    rows = rand_db(rng, 12, 60, universe)
    pool = np.concatenate([universe, rng.integers(1, 2 ** 63, size=300, dtype=np.uint64)])
    keys = rng.choice(pool, size=3000)
    lengths = [int(x) for x in rng.integers(1, 5, size=len(rows))]
    same(rows, keys)
    same(rows, keys, winner=True, lengths=lengths)


def test_adversarial():
    rows = [np.array([], np.uint64),
            np.array([0], np.uint64),
            np.array([0, 1, 2, 3], np.uint64),
            np.array([2, 3, 2 ** 64 - 1], np.uint64),
            np.array([5, 2 ** 32, 2 ** 32 + 1, 2 ** 33], np.uint64)]
    keys = [0] * 7 + [2] * 3 + [3] + [2 ** 64 - 1] * 2 + [4, 6, 2 ** 32 + 2] + [2 ** 32] * 70000
    sh, me = same(rows, keys)
    assert sh == [0, 1, 3, 3, 1]
    # row 2: depths [7, 3, 1] -> sorted [1, 3, 7], position 3 // 2 = 1
    assert me == [0, 7, 3, 2, 70000]
    same(rows, keys, winner=True, lengths=[1, 1, 1, 1, 1])
    same(rows, [], winner=True, lengths=[1, 1, 1, 1, 1])
    same([], keys)


def test_median_index_and_ties():
    row = np.arange(1, 7, dtype=np.uint64)
    for counts, exp in (([1, 1, 5, 5], 5), ([1, 5, 5], 5), ([2, 2], 2), ([9], 9),
                        ([1, 2, 3, 4, 5, 6], 4), ([1, 65536, 1 << 24], 65536)):
        keys = [int(row[i]) for i, c in enumerate(counts) for _ in range(min(c, 3))]
        U = row.copy()
        cnt = np.zeros(len(U), np.uint32)
        cnt[:len(counts)] = counts
        sh, me = M.closed([row], keys, counts=(U, cnt))
        assert sh == [len(counts)] and me == [exp]


def test_counter_is_u32():
    U, cnt = M.closed_counts([np.array([7], np.uint64)], [7, 7, 8])
    assert list(U) == [7] and list(cnt) == [2] and cnt.dtype == np.uint32
    table, counts = M.literal_counts([[7]], [7, 7, 8])
    assert counts == {7: 2} and table == {7: [0]}


def test_winner_rule_order_independent():
    """Three references share keys; scores differ, or tie with different lengths: any visiting
    order gives the same owner.  A full tie (equal score and length) goes to the first visited
    in the reference; ascending index order makes that the lowest index."""
    a = np.array([1, 2, 3, 10], np.uint64)       # shared 4 of 4
    b = np.array([1, 2, 3, 20, 21], np.uint64)   # shared 3 of 5
    c = np.array([1, 2, 3, 30, 31], np.uint64)   # shared 3 of 5: ties with b
    keys = [1, 2, 2, 3, 3, 3, 10]
    rows = [c, a, b]
    for lengths in ([5, 5, 9], [9, 5, 5]):
        base = M.literal(rows, keys, winner=True, lengths=lengths)
        for seed in range(5):
            rnd = random.Random(seed)

            def visit(ix):
                rnd.shuffle(ix)
                return ix
            assert M.literal(rows, keys, winner=True, lengths=lengths, visit=visit) == base
        assert base == tuple(M.closed(rows, keys, winner=True, lengths=lengths))
        assert base[0] == [0, 4, 0]              # a has the best score: it takes 1, 2, 3
    # without a: b and c tie on score; the longer wins; equal lengths: the lowest index
    rows = [c, b]
    assert M.literal(rows, keys, winner=True, lengths=[5, 9])[0] == [0, 3]
    assert M.closed(rows, keys, winner=True, lengths=[5, 9])[0] == [0, 3]
    assert M.literal(rows, keys, winner=True, lengths=[7, 7])[0] == [3, 0]
    assert M.closed(rows, keys, winner=True, lengths=[7, 7])[0] == [3, 0]
    R, lens = as_matrix(rows, 1)
    assert M.closed_matrix(R, lens, keys, lengths=[5, 9])["wshared"].tolist() == [0, 3]
    assert M.closed_matrix(R, lens, keys, lengths=[7, 7])["wshared"].tolist() == [3, 0]
    # the full tie is the one case the visiting order decides in the reference
    assert M.literal(rows, keys, winner=True, lengths=[7, 7], visit=lambda ix: ix[::-1])[0] == [0, 3]


def test_window_keys_variants(oracle):
    recs = [b"ACGTTGCATGCAACGTNACGTACGATCGATCGTAGC", b"acgtacgtacgaTTTTACGATCAGCTAGCTAGCTAGCAT",
            b"ACGT"]
    k = 11
    assert M.window_keys(oracle, recs, k) == RM.window_hashes(oracle, recs, k)
    # noncanonical keys of a record = canonical-free hashes of its forward windows
    non = M.window_keys(oracle, recs[:1], k, noncanonical=True)
    fwd = recs[0]
    exp = [oracle.get_hash(fwd[i:i + k], 42, RM.use64_of(k)) for i in range(len(fwd) - k + 1)
           if b"N" not in fwd[i:i + k]]
    assert non == exp
    # preserve-case: lower-case bytes are outside the alphabet
    pc = M.window_keys(oracle, recs[1:2], k, preserve_case=True)
    up = recs[1]
    assert len(pc) == sum(1 for i in range(len(up) - k + 1) if up[i:i + k].isupper())
    assert 0 < len(pc) < len(up) - k + 1


def test_set_size_and_lines(oracle):
    keys = [5, 9, 9, 2 ** 40, 7]
    assert list(M.bottom_s(keys, 3)) == [5, 7, 9]
    assert M.set_size(keys, 3) == RM.set_size(np.array([5, 7, 9], np.uint64))
    assert M.set_size([], 3) == 0
    rows = [np.array([5, 9, 11], np.uint64), np.array([1, 2], np.uint64)]
    txt = M.screen_text(oracle, rows, ["a", "b"], ["ca", ""], [1, 1], keys, 3)
    # the set size over 4^21 is far above 1: r is clamped to 1, so Q(1, 1, 3) = 1
    assert txt == "%g\t2/3\t2\t1\ta\tca\n" % ((2.0 / 3.0) ** (1.0 / 21))
    both = M.screen_text(oracle, rows, ["a", "b"], ["ca", ""], [1, 1], keys, 3, identity_min=-1.0)
    assert both == txt + "0\t0/2\t0\t1\tb\t\n"
    assert M.p_value_within(oracle, 0, 10, 100.0, 5) == 1.0
    assert M.p_value_within(oracle, 6, 10, 100.0, 5) == 0.0
    assert abs(M.p_value_within(oracle, 1, 10, 100.0, 5) - (1 - 0.9 ** 5)) < 1e-12
