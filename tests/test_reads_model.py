"""Pins tests/reads_model.py, the reads-mode checker (MinHashHeap::tryInsert with
multiplicityMinimum = m, MinHashHeap.cpp:68-146), on the CPU:
  m = 1   it is the oracle's literal heap (oracle.sketch_batch(counts=True), itself pinned to the
          reference's reads.msh by tests/test_oracle_golden.py);
  m >= 2  its hashes are the first s of the hashes seen >= m times, its counts their full
          counts (an oracle sketch wider than the window count) except the maximum of a full
          sketch, which follows the closed form with T, whatever the record order;
  the set-size formula gives the length stored in reads.msh;
  the inputs of tests/test_gpu_reads_edges.py: each builder's preconditions, closed form ==
          literal heap, and the mutant closed forms each input must tell from the true one.
"""
import numpy as np
import pytest

import mshfmt
import reads_model as RM
from conftest import GOLDEN


def one_group(oracle, recs, k, s):
    h, c = oracle.sketch_batch(oracle.params(k=k, s=s), recs, groups=[0] * len(recs), n_groups=1,
                               counts=True)
    return h[0], c[0]


@pytest.fixture(scope="module")
def base():
    return RM.base_reads()


@pytest.fixture(scope="module")
def streams(oracle, base):
    return {k: RM.window_hashes(oracle, base, k) for k in (21, 12)}


@pytest.mark.parametrize("k,s", [(21, 50), (21, 1), (12, 100), (21, 1000), (21, 100000)])
def test_m1_is_the_oracle_heap(oracle, base, streams, k, s):
    h, c = RM.model_sketch(streams[k], s, 1)
    eh, ec = one_group(oracle, base, k, s)
    assert np.array_equal(h, eh)
    assert np.array_equal(c, ec)


@pytest.mark.parametrize("k,s,m", [(21, 50, 2), (21, 1, 2), (12, 100, 3), (21, 1000, 2),
                                   (21, 50, 4)])
def test_min_copies_hashes_and_counts(oracle, base, streams, k, s, m):
    stream = streams[k]
    ah, ac = one_group(oracle, base, k, len(stream) + 1)     # every distinct hash, full counts
    keep = ac >= m
    fh, fc = ah[keep][:s], ac[keep][:s]
    h, c = RM.model_sketch(stream, s, m)
    assert np.array_equal(h, fh)
    full = len(fh) == s
    n = len(fh) - 1 if full else len(fh)
    assert np.array_equal(c[:n], fc[:n])
    ch, cc = RM.closed_form(stream, s, m)
    assert np.array_equal(h, ch)
    assert np.array_equal(c, cc)
    if full:
        assert m <= c[-1] <= fc[-1]


def test_maximum_count_follows_record_order(oracle):
    """`unit * 30` between / after two copies of a record y: the same hashes, the maximum's
    count differs (s puts a unit hash on top with y hashes below it: with y's second copy last
    the heap settles at the end of the stream, so the maximum counts all 30 of its occurrences;
    with both copies first it settles inside unit's second copy), and both equal the closed
    form."""
    orders, s = RM.order_inputs(oracle)
    got = []
    for order in orders:
        stream = RM.window_hashes(oracle, order, 21)
        for ss, m in ((s, 2), (s, 3), (s + 7, 2), (5, 2)):
            h, c = RM.model_sketch(stream, ss, m)
            ch, cc = RM.closed_form(stream, ss, m)
            assert np.array_equal(h, ch)
            assert np.array_equal(c, cc)
        got.append(RM.model_sketch(stream, s, 2))
    assert np.array_equal(got[0][0], got[1][0])
    assert np.array_equal(got[0][1][:-1], got[1][1][:-1])
    assert got[0][1][-1] == 30 and got[1][1][-1] == 2


def test_set_size_formula_on_fixture():
    ref = mshfmt.read_msh(f"{GOLDEN}/reads.msh")["references"][0]
    assert ref["length"] == 502359
    assert RM.set_size(ref["hashes64"], use64=True) == 502359
    assert RM.set_size([], use64=True) == 0
    assert RM.set_size([1 << 31, 1 << 30], use64=False) == 4


# ---- the additions the edge tests use (tests/test_gpu_reads_edges.py): every builder's
# preconditions run here, with closed_form == the literal heap on each new input, and for each
# input that targets a compare the mutant closed form it must tell from the true one ------------
def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_closed_form_detail(streams):
    stream = streams[21]
    plain = RM.closed_form(stream, 50, 2)
    assert len(plain) == 2                                   # the default return is unchanged
    h, c, T, occ = RM.closed_form(stream, 50, 2, detail=True)
    assert same((h, c), plain)
    assert all(stream[i] == int(h[-1]) for i in occ) and stream.count(int(h[-1])) == len(occ)
    assert occ == sorted(occ) and int(c[-1]) == sum(1 for i in occ if i <= T)
    second = [[i for i, x in enumerate(stream) if x == int(f)][1] for f in h]
    assert T == max(second)
    h, c, T, occ = RM.closed_form(stream, 5000, 2, detail=True)      # not full: no T
    assert 0 < len(h) < 5000 and T is None and len(occ) == int(c[-1])
    assert RM.closed_form([], 5, 2, detail=True)[2:] == (None, [])
    for mutant in RM.MUTANTS:                                # a mutant only moves the cut
        mh, mc = RM.closed_form(stream, 50, 2, mutant=mutant, tile_floor=lambda i: i // 7 * 7)
        assert np.array_equal(mh, plain[0]) and np.array_equal(mc[:-1], plain[1][:-1])


def test_window_positions(oracle):
    recs = [b"ACGTACGTNACGTAC", b"ACG", b"acgtacg", b""]
    k = 4
    pos = RM.window_positions(recs, k)
    #      record 0: windows 0..4 are clean, 5..8 hold the N, 9..11 follow; record 2: 0..3
    assert pos.tolist() == [[0, i] for i in (0, 1, 2, 3, 4, 9, 10, 11)] + [[2, i] for i in range(4)]
    assert len(RM.window_hashes(oracle, recs, k)) == len(pos)
    assert RM.window_positions([b"AC"], 4).shape == (0, 2)
    floor = RM.tile_floor_of(RM.window_positions([b"N" * 3 + b"ACGT" * 4], 4), tile=8)
    # windows 3..15 are emitted: stream 0..4 lie in tile 0, stream 5 (window 8) starts tile 1
    assert [floor(i) for i in (0, 4, 5, 12)] == [0, 0, 5, 5]


@pytest.mark.parametrize("kw", [dict(k=21, noncanonical=True),
                                dict(k=9, alphabet="ACDEFGHIKLMNPQRSTVWY", noncanonical=True)])
def test_noncanonical_and_protein_streams_are_the_oracles(oracle, kw):
    """window_hashes(noncanonical=True) and a non-DNA alphabet, pinned at m = 1 to the oracle's
    literal heap under the same parameters."""
    alphabet = kw.get("alphabet", "ACGT").encode()
    recs, _ = RM.copies_ladder(oracle, kw["k"], alphabet, True, flip_odd=alphabet == b"ACGT")
    stream = RM.window_hashes(oracle, recs, kw["k"], alphabet=alphabet, noncanonical=True)
    for s in (30, 5000):
        eh, ec = oracle.sketch_batch(oracle.params(s=s, **kw), list(recs), groups=[0] * len(recs),
                                     n_groups=1, counts=True)
        assert same(RM.model_sketch(stream, s, 1), (eh[0], ec[0]))
    if alphabet == b"ACGT":
        assert not same(RM.model_sketch(stream, 30, 2),
                        RM.model_sketch(RM.window_hashes(oracle, recs, kw["k"]), 30, 2))


# case -> the mutants its input must tell from the true closed form
PLANTED_MUTANTS = {"a": ("t_minus_1", "tile_skip_ge", "m_minus_1"), "b": ("t_minus_1", "tile_skip_ge"),
                   "c": ("no_cut", "m_plus_1", "t_minus_1"), "d": ("no_cut", "m_plus_1"),
                   "e": ("no_cut", "m_plus_1", "m_minus_1")}


@pytest.mark.parametrize("case", sorted(RM.PLANTED))
def test_planted_record(oracle, case):
    p = RM.planted_record(oracle, *RM.PLANTED[case])         # asserts its own preconditions
    assert len(p.recs) == 1 and len(p.recs[0]) <= 150_000
    assert len(p.recs[0]) - p.k + 1 > RM.TILE                # more than one tile
    exp = RM.model_sketch(p.stream, p.s, p.m)
    assert same(RM.closed_form(p.stream, p.s, p.m), exp)
    assert int(exp[1][-1]) == p.expect and int(exp[0][-1]) == p.M
    floor = RM.tile_floor_of(p.positions)
    for mutant in PLANTED_MUTANTS[case[0]]:
        assert RM.maximum_count(p.stream, p.s, p.m, mutant, floor) != p.expect, mutant


@pytest.mark.parametrize("target", [0, RM.TILE - 1])
def test_mult_record(oracle, target):
    p = RM.mult_record(oracle, target)
    exp = RM.model_sketch(p.stream, p.s, 1)
    assert same(RM.closed_form(p.stream, p.s, 1), exp)
    eh, ec = one_group(oracle, p.recs, p.k, p.s)
    assert same(exp, (eh, ec)) and int(ec[-1]) == 1
    floor = RM.tile_floor_of(p.positions)
    for mutant in ("t_minus_1", "tile_skip_ge", "no_cut", "m_plus_1"):
        assert RM.maximum_count(p.stream, p.s, 1, mutant, floor) != 1, mutant


PERIODIC_M = (2, 3, 5, 8)


def periodic_sizes(unit_len):
    return (1, unit_len // 2, unit_len, unit_len + 1)


@pytest.mark.parametrize("k", [21, 12])
@pytest.mark.parametrize("unit_len,reps", RM.PERIODIC)
def test_periodic_record(oracle, unit_len, reps, k):
    rec = RM.periodic_record(unit_len, reps)
    stream = RM.window_hashes(oracle, [rec], k)
    assert RM.TILE < len(stream) <= 2 * RM.TILE
    h, c = np.unique(np.array(stream, np.uint64), return_counts=True)
    assert len(h) == unit_len and set(c.tolist()) <= {reps - 1, reps}
    floor = RM.tile_floor_of(RM.window_positions([rec], k))
    for m in PERIODIC_M:
        for s in periodic_sizes(unit_len):
            exp = RM.model_sketch(stream, s, m)
            assert same(RM.closed_form(stream, s, m), exp)
            if s > unit_len:
                assert len(exp[0]) == unit_len and set(exp[1].tolist()) <= {reps - 1, reps}
                continue
            assert int(exp[1][-1]) == m
            assert RM.maximum_count(stream, s, m, "m_plus_1") == m + 1
            assert RM.maximum_count(stream, s, m, "m_minus_1") == m - 1
            assert RM.maximum_count(stream, s, m, "no_cut") >= reps - 1
            if s == 1:                                       # the maximum occurs exactly at T
                assert RM.maximum_count(stream, s, m, "t_minus_1") == m - 1
                assert RM.maximum_count(stream, s, m, "tile_skip_ge", floor) == 0
    # -M (m = 1): T_top lies in the first period, so a full sketch's maximum counts once
    for s in periodic_sizes(unit_len):
        exp = RM.model_sketch(stream, s, 1)
        assert same(RM.closed_form(stream, s, 1), exp)
        assert same(exp, one_group(oracle, [rec], k, s))
        if s <= unit_len:
            assert int(exp[1][-1]) == 1
            assert RM.maximum_count(stream, s, 1, "m_plus_1") == 2
            assert RM.maximum_count(stream, s, 1, "no_cut") >= reps - 1


LADDERS = {"dna": (21, b"ACGT", False, False), "u32": (12, b"ACGT", False, False),
           "noncanonical": (21, b"ACGT", True, True), "protein": (9, RM.PROTEIN, True, False)}


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_copies_ladder(oracle, name):
    k, alphabet, noncanonical, flip = LADDERS[name]
    recs, D = RM.copies_ladder(oracle, k, alphabet, noncanonical, flip)
    stream = RM.window_hashes(oracle, recs, k, alphabet=alphabet, noncanonical=noncanonical)
    copies = [stream.count(h) for h in D]
    if not flip:
        assert copies == [1 + i % 9 for i in range(40)]
    cut_shows = 0
    for m in range(2, 10):
        if not flip:                                         # both sides of the threshold
            assert m - 1 in copies and m in copies
        lo, hi = RM.ladder_sizes(stream, m)
        for s in (lo, hi):
            exp = RM.model_sketch(stream, s, m)
            assert same(RM.closed_form(stream, s, m), exp)
            assert len(exp[0]) == (lo if s == lo else hi - 3)
        cut_shows += RM.maximum_count(stream, lo, m, "no_cut") != RM.maximum_count(stream, lo, m)
        if flip:
            break
    assert cut_shows or flip


def test_widening_inputs(oracle):
    """The widths and rounds the GPU tests assert, from the host loop's arithmetic
    (RM.widening_widths restates fpm_sketch_reads_run), and the sample rule at the last width."""
    rec, stream = RM.widening_record(oracle)
    for m, n in ((2, 10), (5, 0)):
        exp = RM.model_sketch(stream, 100, m)
        assert same(RM.closed_form(stream, 100, m), exp) and len(exp[0]) == n
    # one group of 12,288 windows, open until its row holds every hash: round 3
    assert RM.widening_widths(100, 2, [12288], [3]) == [800, 3200, 12289]
    assert RM.widening_widths(100, 2, [300, 12288], [1, 3]) == [800, 3200, 12289]
    # exactly 8 s distinct windows: the full first row is not known to hold every hash
    assert RM.widening_widths(10, 2, [80], [2]) == [80, 81]
    assert RM.widening_widths(10, 2, [79], [1]) == [80]
    assert RM.widening_widths(10, 1, [80], [1]) == [10]
    # the sampled long group of round 2: 66 chunk tiles of the long record + 2 of the packed
    # 21-base records; a 150,000-base record (37 + 2 tiles) is not sampled at width 3,200
    assert RM.widening_widths(100, 2, [280 * 2, RM.SAMPLED_LONG - 20 + 122], [1, 2]) == [800, 3200]
    assert RM.group_is_sampled(66 + 2, 3200) and not RM.group_is_sampled(37 + 2, 3200)
    assert not RM.group_is_sampled(66 + 2, 800)
    x = RM.sampled_round2(oracle)
    assert max(len(r) for r in x.recs) == RM.SAMPLED_LONG
    for g, (s_full, top) in enumerate(((100, 2), (100, 2))):
        exp = RM.model_sketch(x.streams[g], 100, 2)
        assert same(RM.closed_form(x.streams[g], 100, 2), exp)
        assert len(exp[0]) == s_full and int(exp[1][-1]) == top
    # the 100th qualifier of the long group lies beyond the first row and within the second
    D = sorted(set(x.streams[1]))
    assert 800 <= D.index(int(RM.model_sketch(x.streams[1], 100, 2)[0][-1])) < 3200
