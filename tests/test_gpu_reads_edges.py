"""Reads mode (sketch -r / -m N) and the -M counts on the GPU at their position, slot and
widening edges, vs tests/reads_model.py (MinHashHeap::tryInsert restated, MinHashHeap.cpp:68-146)
and, for -M, the oracle's literal heap.  Hashes, counts and estimates are integers: bit-exact.

The inputs come from the builders of tests/reads_model.py.  tests/test_reads_model.py runs their
preconditions on the CPU and shows, with the mutant closed forms, that each input tells a wrong
compare (`<` for `<=` at T, `>=` for `>` in the tile skip, a neighbouring slot of the position
chain, no cut at all) from the right one; here the kernels run over them.

Widths, rounds and routes are asserted through the hooks (reads_rounds, reads_plan): they follow
from the host loop of fpm_sketch_reads_run (RM.widening_widths restates it) and from the sample
rule of csrc/sketch_plan.cpp (RM.group_is_sampled), not from what a run gave.
"""
import numpy as np
import pytest

import reads_model as RM

pytestmark = pytest.mark.gpu


def params(k, s, alphabet=b"ACGT", noncanonical=False):
    import fpmash
    if alphabet == RM.PROTEIN:
        return fpmash.make_params(protein=True, k=k, s=s)
    assert alphabet == b"ACGT"
    return fpmash.make_params(k=k, s=s, noncanonical=noncanonical)


def run(ctx, recs, k, s, m, groups=None, n_groups=1, **kw):
    g = [0] * len(recs) if groups is None else groups
    return ctx.sketch_reads(params(k, s, **kw), list(recs), groups=g, n_groups=n_groups,
                            min_copies=m)


def check(got, g, exp, use64=True):
    eh, ec = exp
    assert np.array_equal(got["hashes"][g], eh), f"group {g}: hashes differ"
    assert np.array_equal(got["counts"][g], ec), \
        f"group {g}: counts differ at {np.nonzero(got['counts'][g] != ec)[0][:10]}: " \
        f"{got['counts'][g][got['counts'][g] != ec][:10]} for {ec[got['counts'][g] != ec][:10]}"
    assert int(got["estimate"][g]) == RM.set_size(eh, use64)


def first_width(s, windows):
    return min(8 * s, windows + 1)


# ---- the position compares ------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(RM.PLANTED))
def test_planted_positions(ctx, oracle, case):
    """T on the first / the last window of a 4,096-window chunk tile, the maximum occurring
    exactly at T (a, b), again after T in the same tile (c) and on the first window of the next
    (d), and on both sides of a T that another hash sets (e); at m = 3 and 4 the chain of
    position slots is that deep."""
    p = RM.planted_record(oracle, *RM.PLANTED[case])
    got = run(ctx, p.recs, p.k, p.s, p.m)
    exp = RM.model_sketch(p.stream, p.s, p.m)
    assert int(exp[1][-1]) == p.expect
    check(got, 0, exp)
    # the planted hashes are among the smallest of the record's: inside the first row of 8 s
    assert sorted(set(p.stream)).index(p.M) < 8 * p.s
    assert got["rounds"] == 1 and got["width"] == 8 * p.s and got["plan"]["n_slots"] == 0


@pytest.mark.parametrize("target", [0, RM.TILE - 1])
def test_mult_planted_positions(ctx, oracle, target):
    """-M: T_top (the last first occurrence among the sketch) is the maximum's own first window,
    on the first / last window of a tile; its later copy is not counted."""
    p = RM.mult_record(oracle, target)
    gh, gc = ctx.sketch(params(p.k, p.s), p.recs, counts=True)
    eh, ec = oracle.sketch_batch(oracle.params(k=p.k, s=p.s), p.recs, counts=True)
    assert np.array_equal(gh[0], eh[0]) and int(ec[0][-1]) == 1
    assert np.array_equal(gc[0], ec[0]), f"-M counts: {gc[0][-3:]} for {ec[0][-3:]}"


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_mult_on_the_planted_records(ctx, oracle, case):
    """-M over the reads-mode records, at sketch sizes around the planted set."""
    p = RM.planted_record(oracle, *RM.PLANTED[case])
    for s in (1, RM.PLANTED_N, 100):
        gh, gc = ctx.sketch(params(p.k, s), p.recs, counts=True)
        eh, ec = oracle.sketch_batch(oracle.params(k=p.k, s=s), p.recs, counts=True)
        assert np.array_equal(gh[0], eh[0])
        assert np.array_equal(gc[0], ec[0]), f"s = {s}"


# ---- the slot chain under contention --------------------------------------------------------
PERIODIC_M = (2, 3, 5, 8)


@pytest.mark.parametrize("k", [21, 12])
@pytest.mark.parametrize("unit_len,reps", RM.PERIODIC)
def test_periodic_contention(ctx, oracle, unit_len, reps, k):
    """unit * reps: every window of a tile pushes its position down one of unit_len chains, ~reps
    windows per chain and up to 8 slots deep; a full sketch's maximum counts m of ~reps.  k = 12:
    u32 hashes.  And -M over the same record."""
    rec = RM.periodic_record(unit_len, reps)
    stream = RM.window_hashes(oracle, [rec], k)
    use64 = RM.use64_of(k)
    windows = len(rec) - k + 1
    for m in PERIODIC_M:
        for s in (1, unit_len // 2, unit_len, unit_len + 1):
            got = run(ctx, [rec], k, s, m)
            exp = RM.model_sketch(stream, s, m)
            if s <= unit_len:
                assert len(exp[0]) == s and int(exp[1][-1]) == m
            check(got, 0, exp, use64)
            # every distinct hash qualifies, so the first row settles it: it holds s
            # qualifiers, or (8 s > unit_len) it is not full
            assert got["rounds"] == 1 and got["width"] == first_width(s, windows)
    for s in (1, unit_len // 2, unit_len, unit_len + 1):
        gh, gc = ctx.sketch(params(k, s), [rec], counts=True)
        eh, ec = oracle.sketch_batch(oracle.params(k=k, s=s), [rec], counts=True)
        assert np.array_equal(gh[0], eh[0])
        assert np.array_equal(gc[0], ec[0]), f"-M, s = {s}"


LADDERS = {"dna": (21, b"ACGT", False, False, range(2, 10)),
           "u32": (12, b"ACGT", False, False, range(2, 10)),
           "noncanonical": (21, b"ACGT", True, True, (2, 3)),
           "protein": (9, RM.PROTEIN, True, False, (2, 3))}


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_copies_ladder(ctx, oracle, name):
    """Hashes with 1..9 copies at every m = 2..9 (some with exactly m - 1, some with exactly m),
    s below and above the number of qualifiers; with u32 hashes, noncanonical (half of the extra
    copies are reverse complements: other hashes) and over the protein alphabet (k = 9)."""
    k, alphabet, noncanonical, flip, ms = LADDERS[name]
    recs, _ = RM.copies_ladder(oracle, k, alphabet, noncanonical, flip)
    stream = RM.window_hashes(oracle, recs, k, alphabet=alphabet, noncanonical=noncanonical)
    for m in ms:
        lo, hi = RM.ladder_sizes(stream, m)
        for s in (lo, hi):
            got = run(ctx, recs, k, s, m, alphabet=alphabet, noncanonical=noncanonical)
            exp = RM.model_sketch(stream, s, m)
            assert len(exp[0]) == (lo if s == lo else hi - 3)
            check(got, 0, exp, RM.use64_of(k, alphabet))


# ---- the widening loop ----------------------------------------------------------------------
def test_widening_to_the_cap(ctx, oracle):
    """One group of 12,288 windows (three tiles), s = 100: 10 qualifiers at m = 2 and none at
    m = 5, so the rows of 800 and 3,200 are full without s of them and the third round has the
    cap, 12,288 + 1: never full, final."""
    rec, stream = RM.widening_record(oracle)
    for m, n in ((2, 10), (5, 0)):
        got = run(ctx, [rec], 21, 100, m)
        exp = RM.model_sketch(stream, 100, m)
        assert len(exp[0]) == n
        check(got, 0, exp)
        assert got["rounds"] == 3 and got["width"] == 12289
        assert list(got["group_round"]) == [3]
        assert got["plan"]["n_slots"] == 0 and sum(got["plan"]["tiles"]) == 3
    assert int(got["estimate"][0]) == 0 and len(got["hashes"][0]) == 0


def test_a_group_closes_two_rounds_early(ctx, oracle):
    """300 windows beside 12,288: rounds 2 and 3 are staged over the second group only."""
    rec, stream = RM.widening_record(oracle)
    short = RM._rand(np.random.default_rng(67), 320)
    got = run(ctx, [short, rec], 21, 100, 2, groups=[0, 1], n_groups=2)
    assert list(got["group_round"]) == [1, 3] and got["rounds"] == 3 and got["width"] == 12289
    check(got, 0, RM.model_sketch(RM.window_hashes(oracle, [short], 21), 100, 2))
    check(got, 1, RM.model_sketch(stream, 100, 2))
    assert len(got["hashes"][0]) == 0 and len(got["hashes"][1]) == 10
    assert sum(got["plan"]["tiles"]) == 3                    # the last round's job: one group


@pytest.mark.parametrize("bases,rounds,width", [(100, 2, 81), (99, 1, 80)])
def test_exactly_eight_s_distinct_windows(ctx, oracle, bases, rounds, width):
    """s = 10 and one read of 80 single-copy windows: the first row (80) is full, so it is not
    known to hold every hash, and a second round of 81 = the cap follows.  79 windows: the cap
    is 80, the row is not full, one round."""
    rec = RM._rand(np.random.default_rng(71), bases)
    stream = RM.window_hashes(oracle, [rec], 21)
    assert len(set(stream)) == len(stream) == bases - 20
    got = run(ctx, [rec], 21, 10, 2)
    check(got, 0, RM.model_sketch(stream, 10, 2))
    assert len(got["hashes"][0]) == 0
    assert got["rounds"] == rounds and got["width"] == width
    # and with a second copy of the read every hash qualifies: one round either way
    got = run(ctx, [rec, rec], 21, 10, 2)
    check(got, 0, RM.model_sketch(stream + stream, 10, 2))
    assert got["rounds"] == 1 and got["width"] == 80


def test_sampled_long_group_in_round_two(ctx, oracle):
    """A group that closes in round 1 beside a long group whose 100th qualifier lies between
    the 800th and the 3,200th of its hashes: round 2 stages a job of width 3,200 over the long
    group alone, and at that width the group is sampled (n_slots = 1): 66 + 2 tiles, every 16th
    sampled, 4 x 4,096 windows >= 4 x 3,200.  (A 150,000-base record has 37 tiles, two of them
    sampled: 8,192 windows < 12,800, not sampled at 3,200; hence 270,000 bases.)  The maximum's
    second copy is at T, its third after it."""
    x = RM.sampled_round2(oracle)
    got = run(ctx, x.recs, 21, 100, 2, groups=x.groups, n_groups=2)
    assert got["rounds"] == 2 and list(got["group_round"]) == [1, 2] and got["width"] == 3200
    assert got["plan"]["n_slots"] >= 1 and got["sampled"] == got["plan"]["n_slots"]
    assert sum(got["plan"]["tiles"]) == 66 + 2               # the long group's tiles only
    for g in (0, 1):
        exp = RM.model_sketch(x.streams[g], 100, 2)
        assert len(exp[0]) == 100 and int(exp[1][-1]) == 2
        check(got, g, exp)


def test_interleaved_groups(ctx, oracle):
    """Records of two groups alternating one by one: each group's result is that of the group
    alone (staging puts a group's records together, in stream order)."""
    a, _ = RM.copies_ladder(oracle)
    b = RM.widening_reads()
    n = min(len(a), len(b))
    a, b = list(a[:n]), list(b[:n])
    assert any(len(r) == 60 for r in b)                      # b keeps its repeated unit
    recs = RM.interleave(a, b)
    groups = [0, 1] * n
    for s, m in ((20, 2), (15, 3), (40, 2)):
        got = run(ctx, recs, 21, s, m, groups=groups, n_groups=2)
        for g, alone in enumerate((a, b)):
            exp = RM.model_sketch(RM.window_hashes(oracle, alone, 21), s, m)
            check(got, g, exp)
            one = run(ctx, alone, 21, s, m)
            assert np.array_equal(got["hashes"][g], one["hashes"][0])
            assert np.array_equal(got["counts"][g], one["counts"][0])
            assert got["group_round"][g] == one["rounds"]


# ---- one job, several runs ------------------------------------------------------------------
def test_job_reuse(ctx, oracle):
    """set_min_copies(3), run; set_min_copies(2), run; run again: each as a fresh job's."""
    import fpmash
    base = RM.base_reads()
    stream = RM.window_hashes(oracle, base, 21)
    P = fpmash.make_params(k=21, s=50)
    job = ctx.sketch_job(P, base, groups=[0] * len(base), n_groups=1)
    try:
        with pytest.raises(fpmash.FpmError) as e:            # no round yet
            job.reads_plan()
        assert e.value.code == fpmash.FPM_EINVAL
        for m, change in ((3, True), (2, True), (2, False)):
            if change:
                job.set_min_copies(m)
            got = ctx._reads_result(job)
            fresh = run(ctx, base, 21, 50, m)
            check(got, 0, RM.model_sketch(stream, 50, m))
            assert np.array_equal(got["hashes"][0], fresh["hashes"][0])
            assert np.array_equal(got["counts"][0], fresh["counts"][0])
            assert (got["rounds"], got["width"], got["plan"]) == \
                (fresh["rounds"], fresh["width"], fresh["plan"])
            assert job.reads_plan() == (got["plan"], got["width"])
    finally:
        job.free()


def test_out_of_memory_is_an_error_code_and_the_job_lives_on(ctx, oracle):
    """min_copies = 2^31 asks for 80 x 2^31 position slots of 8 B (1.4 TB): the host compares
    the bytes with the free device memory and returns FPM_ENOMEM before the counts and slots
    are allocated or any reads kernel is launched.  The same job then runs at min_copies 2."""
    import fpmash
    base = RM.base_reads()[:40]
    stream = RM.window_hashes(oracle, base, 21)
    job = ctx.sketch_job(fpmash.make_params(k=21, s=10), base, groups=[0] * len(base), n_groups=1)
    try:
        job.set_min_copies(2 ** 31)
        with pytest.raises(fpmash.FpmError) as e:
            job.run_reads()
        assert e.value.code == fpmash.FPM_ENOMEM
        assert job.reads_plan()[1] == 80                     # the round that failed
        job.set_min_copies(2)
        got = ctx._reads_result(job)
        exp = RM.model_sketch(stream, 10, 2)
        assert len(exp[0]) == 10
        check(got, 0, exp)
    finally:
        job.free()
