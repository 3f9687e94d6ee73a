"""Reads mode on the GPU (fpm_sketch_reads_run: sketch -r / -m N) vs tests/reads_model.py, the
plain-Python MinHashHeap::tryInsert with multiplicityMinimum = m (MinHashHeap.cpp:68-146; pinned
by tests/test_reads_model.py).  Hashes and counts are integers: bit-exact.  The set-size
estimate is one double expression (MinHashHeap.h:45): equal to Python's.
"""
import numpy as np
import pytest

import reads_model as RM

pytestmark = pytest.mark.gpu


def run(ctx, recs, k, s, m, groups=None, n_groups=1):
    import fpmash
    P = fpmash.make_params(k=k, s=s)
    g = [0] * len(recs) if groups is None else groups
    return ctx.sketch_reads(P, recs, groups=g, n_groups=n_groups, min_copies=m)


def check(got, g, exp, use64=True):
    eh, ec = exp
    assert np.array_equal(got["hashes"][g], eh), f"group {g}: hashes differ"
    assert np.array_equal(got["counts"][g], ec), \
        f"group {g}: counts differ at {np.nonzero(got['counts'][g] != ec)[0][:10]}"
    assert int(got["estimate"][g]) == RM.set_size(eh, use64)


@pytest.fixture(scope="module")
def base():
    return RM.base_reads()


@pytest.fixture(scope="module")
def base_streams(oracle, base):
    return {k: RM.window_hashes(oracle, base, k) for k in (21, 12)}


@pytest.mark.parametrize("k,s,m", [(21, 50, 2), (21, 1, 2), (12, 100, 3), (21, 1000, 2),
                                   (21, 5000, 2), (21, 50, 1)])
def test_base_reads(ctx, base, base_streams, k, s, m):
    """Full sketches (the maximum's exception), s = 1, u32 hashes (k = 12) and, at (21, 5000, 2),
    fewer qualifiers than s: the not-full path, every count is the full one.  (At 8x nearly all
    of the genome's ~2,900 k-mers are seen twice, so s = 1000 is still a full sketch.)"""
    import fpmash
    got = run(ctx, base, k, s, m)
    exp = RM.model_sketch(base_streams[k], s, m)
    if (k, s, m) == (21, 5000, 2):
        assert 0 < len(exp[0]) < s
    else:
        assert len(exp[0]) == s
    check(got, 0, exp, use64=RM.use64_of(k))
    if m == 1:
        assert got["rounds"] == 1
        h, c = ctx.sketch(fpmash.make_params(k=k, s=s), base, groups=[0] * len(base), n_groups=1,
                          counts=True)
        assert np.array_equal(got["hashes"][0], h[0])
        assert np.array_equal(got["counts"][0], c[0])


def test_min_copies_zero_is_rejected(ctx, base):
    import fpmash
    job = ctx.sketch_job(fpmash.make_params(k=21, s=10), base[:3])
    try:
        with pytest.raises(fpmash.FpmError) as e:
            job.set_min_copies(0)
        assert e.value.code == fpmash.FPM_EINVAL
    finally:
        job.free()


def test_widening(ctx, oracle):
    """~1 distinct hash in 500 is seen twice: the first wide row (8 s) cannot hold s of them.
    s = 40 = every qualifier there is: the s-th is the last."""
    recs = RM.widening_reads()
    stream = RM.window_hashes(oracle, recs, 21)
    for s in (30, 40):
        got = run(ctx, recs, 21, s, 2)
        exp = RM.model_sketch(stream, s, 2)
        assert len(exp[0]) == s
        assert got["rounds"] > 1
        check(got, 0, exp)
    got = run(ctx, recs, 21, 41, 2)
    exp = RM.model_sketch(stream, 41, 2)
    assert len(exp[0]) == 40
    check(got, 0, exp)


def test_sth_qualifier_is_the_wide_rows_maximum(ctx, oracle):
    """Single-copy 21-mers, five of them given a second copy as 21-bp records: with s = 5 the
    first wide row holds the 40 smallest distinct hashes (indices 0..39); the fifth repeated one
    sits at index 39, the row's own maximum (one round), or at index 40, just past it (two)."""
    rng = np.random.default_rng(23)
    recs = [RM._rand(rng, 100) for _ in range(60)]
    kmers = {}
    for r in recs:
        for i in range(len(r) - 20):
            kmers[RM.window_hashes(oracle, [r[i:i + 21]], 21)[0]] = r[i:i + 21]
    D = sorted(kmers)
    assert len(D) == 60 * 80
    for last, rounds in ((39, 1), (40, 2)):
        extra = [kmers[D[i]] for i in (3, 10, 17, 30, last)]
        allrecs = recs + extra
        got = run(ctx, allrecs, 21, 5, 2)
        exp = RM.model_sketch(RM.window_hashes(oracle, allrecs, 21), 5, 2)
        assert [int(h) for h in exp[0]] == [D[i] for i in (3, 10, 17, 30, last)]
        check(got, 0, exp)
        assert got["rounds"] == rounds


def test_maximum_count_and_record_order(ctx, oracle):
    """The same records in two orders: the maximum of the full sketch counts 30 occurrences in
    one and 2 in the other (the heap settles at different stream positions)."""
    orders, s = RM.order_inputs(oracle)
    tops = []
    for recs in orders:
        stream = RM.window_hashes(oracle, recs, 21)
        for m in (2, 3):
            check(run(ctx, recs, 21, s, m), 0, RM.model_sketch(stream, s, m))
        tops.append(int(RM.model_sketch(stream, s, 2)[1][-1]))
    assert tops == [30, 2]


def test_exactly_m_and_m_minus_one(ctx, oracle):
    """Neighbours in hash order, one seen exactly m - 1 times and one exactly m times (m = 3):
    only the second enters."""
    rng = np.random.default_rng(29)
    recs = [RM._rand(rng, 100) for _ in range(20)]
    kmers = {}
    for r in recs:
        for i in range(len(r) - 20):
            kmers[RM.window_hashes(oracle, [r[i:i + 21]], 21)[0]] = r[i:i + 21]
    D = sorted(kmers)
    allrecs = recs + [kmers[D[6]]] + [kmers[D[7]]] * 2 + [kmers[D[20]]] * 3 + [kmers[D[21]]]
    got = run(ctx, allrecs, 21, 4, 3)
    exp = RM.model_sketch(RM.window_hashes(oracle, allrecs, 21), 4, 3)
    assert [int(h) for h in exp[0]] == [D[7], D[20]]
    assert list(exp[1]) == [3, 4]
    check(got, 0, exp)


def test_groups(ctx, oracle, base, base_streams):
    """Five groups in one job: empty, shorter than k, no repeated k-mer (nothing qualifies:
    count 0, estimate 0; its 180 windows fit the first wide row of 8 s = 240), and two ordinary
    ones of which the sparse one needs the most widening: a group is final in the round that
    completes it and is not run again."""
    rng = np.random.default_rng(31)
    wide = RM.widening_reads()
    recs = [b"", b"ACGTACGTAC", RM._rand(rng, 200)] + base + wide
    groups = [0, 1, 2] + [3] * len(base) + [4] * len(wide)
    got = run(ctx, recs, 21, 30, 2, groups=groups, n_groups=5)
    for g in (0, 1, 2):
        assert len(got["hashes"][g]) == 0 and len(got["counts"][g]) == 0
        assert int(got["estimate"][g]) == 0
    check(got, 3, RM.model_sketch(base_streams[21], 30, 2))
    check(got, 4, RM.model_sketch(RM.window_hashes(oracle, wide, 21), 30, 2))
    per = [int(r) for r in got["group_round"]]
    assert per[:3] == [1, 1, 1]
    assert 1 <= per[3] < per[4] and got["rounds"] == per[4]


@pytest.mark.parametrize("copies,rate,sampled", [(30, 0.01, 0), (60, 0.002, 1)])
def test_long_group(ctx, oracle, copies, rate, sampled):
    """One long record (4096-window chunk tiles): copies of a 10 kb genome with substitutions,
    m = 2, s = 1000, so the first wide sketch has S' = 8000.
    300,000 bases (74 tiles): the size test_mult_concatenated_and_long_groups uses; at S' = 8000
    its sample (4 tiles, 16,384 windows) is below the 4 S' windows a sample needs, so the wide
    job is not sampled.
    600,000 bases (147 tiles, every 16th sampled: 9 tiles, 36,864 windows >= 4 S'): the wide
    job takes the sampled long-group path (sample pass, bounds, selection) and, with ~1 hash in
    3.5 seen twice, is final in its first round: the reads kernels run over a sampled job's rows.
    Hashes against the oracle's counted sketch of every distinct hash, filtered at 2; counts and
    the maximum's count against the model."""
    rng = np.random.default_rng(37)
    genome = RM._rand(rng, 10_000)
    rec = b"".join(RM.mutate(rng, genome, rate) for _ in range(copies))
    assert len(rec) == copies * 10_000
    s, m = 1000, 2
    got = run(ctx, [rec], 21, s, m)
    ah, ac = oracle.sketch_batch(oracle.params(k=21, s=len(rec)), [rec], counts=True)
    keep = ac[0] >= m
    assert np.array_equal(got["hashes"][0], ah[0][keep][:s])
    assert np.array_equal(got["counts"][0][:-1], ac[0][keep][:s - 1])
    check(got, 0, RM.model_sketch(RM.window_hashes(oracle, [rec], 21), s, m))
    assert got["sampled"] == sampled
    if sampled:
        assert got["rounds"] == 1
