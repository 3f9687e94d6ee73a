"""`screen` on the GPU (fpm_screen_*: table build, pool count pass, per-reference sums, -w,
p-values) against tests/screen_model.py.  Counters, shared counts, medians and set sizes are
integers: bit-exact.  u64 hashes at k = 21, u32 at k = 16.

Staging never makes a class-5 tile (long records are cut into 4,096-start chunks,
tests/test_gpu_sketch_dispatch.py asserts the same), so the pool pass is reached through tile
classes 0..4; its class-5 instance exists only for the launch switch.
"""
import numpy as np
import pytest

import reads_model as RM
import screen_model as M

pytestmark = pytest.mark.gpu

KS = [21, 16]
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def dtype_of(k):
    return np.uint64 if RM.use64_of(k) else np.uint32


def revcomp(s):
    return s.translate(_RC)[::-1]


def make_screen(ctx, lists, k, s=1000, pad=0, poison=None):
    """a Screen over `lists`; pad > 0: rows in a matrix of stride max length + pad whose cells
    past each row's length hold `poison`"""
    import fpmash
    dt = dtype_of(k)
    if not pad:
        return fpmash.Screen.from_lists(ctx, lists, s, use64=dt == np.uint64)
    w = max([len(x) for x in lists] + [1]) + pad
    R = np.full((max(len(lists), 1), w), poison, dtype=dt)
    lens = np.zeros(len(lists), np.uint32)
    for i, l in enumerate(lists):
        R[i, :len(l)] = l
        lens[i] = len(l)
    return fpmash.Screen(ctx, R[:len(lists)], lens, s)


def check_counts_rows(sc, lists, keys, winner_lengths=None, k=21):
    """counters and rows of `sc` equal the model's for the pool keys given so far"""
    U, cnt = sc.counts()
    eU, ecnt = M.closed_counts(lists, keys)
    assert np.array_equal(U, eU)
    assert np.array_equal(cnt, ecnt), f"counters differ at {np.nonzero(cnt != ecnt)[0][:10]}"
    sh, me = sc.rows()
    esh, eme = M.closed(lists, keys, k, counts=(eU, ecnt))
    assert list(sh) == esh
    assert list(me) == eme
    if winner_lengths is not None:
        scores = [M.estimate_identity(a, len(l), k) for a, l in zip(esh, lists)]
        wsh, wme = sc.rows_winner(scores, winner_lengths)
        ewsh, ewme = M.closed(lists, keys, k, winner=True, lengths=winner_lengths,
                              counts=(eU, ecnt))
        assert list(wsh) == ewsh
        assert list(wme) == ewme
    return esh, eme


# ---- conservation ------------------------------------------------------------------------------
def conservation_records(k, seed=5):
    """Records whose tiles take classes 0..4 (long records close the packing of the short ones
    around them), one of them spanning three tiles; lengths k - 1, k, k + 1; N at a tile edge, at
    a record start and at a record end; lower-case stretches; a record and its reverse
    complement; for even k a palindromic k-mer."""
    rng = np.random.default_rng(seed)
    r = lambda n: RM._rand(rng, n)                                     # noqa: E731
    long3 = bytearray(r(9000 + k - 1))      # 4096 + 4096 + 808 starts
    long3[4096 + k - 1] = ord("N")          # the first byte past the first tile's windows
    long3[4095] = ord("N")                  # the last start of the first tile
    long3[0] = ord("N")
    long3[-1] = ord("N")
    low = bytearray(r(400 + k - 1))
    low[50:120] = bytes(low[50:120]).lower()
    x = r(900 + k - 1)
    recs = [r(100 + k - 1), bytes(long3), bytes(low), r(5000 + k - 1), x, r(4200 + k - 1),
            r(1800 + k - 1), r(k - 1), r(k), r(k + 1), revcomp(x)]
    if k % 2 == 0:
        h = r(k // 2)
        recs.append(h + revcomp(h))
    return recs


@pytest.fixture(scope="module")
def conservation(oracle):
    out = {}
    for k in KS:
        recs = conservation_records(k)
        for mode in ("default", "preserve_case", "noncanonical"):
            kw = {} if mode == "default" else {mode: True}
            out[k, mode] = (recs, M.window_keys(oracle, recs, k, **kw), kw)
    return out


@pytest.mark.parametrize("mode", ["default", "preserve_case", "noncanonical"])
@pytest.mark.parametrize("k", KS)
def test_conservation(ctx, oracle, conservation, k, mode):
    """One database row holds every distinct key of the pool: the counters sum to the number of
    valid windows, and each equals the model's."""
    import fpmash
    recs, keys, kw = conservation[k, mode]
    row = np.unique(np.asarray(keys, np.uint64)).astype(dtype_of(k))
    P = fpmash.make_params(k=k, s=1000, **kw)
    sc = make_screen(ctx, [row], k)
    job = ctx.sketch_job(P, recs, groups=[0] * len(recs), n_groups=1)
    try:
        tiles = job.plan()["tiles"]
        assert all(tiles[c] > 0 for c in range(5)) and tiles[5] == 0, tiles
        sc.add_job(job)
        ctx.synchronize()
        U, cnt = sc.counts()
        assert int(cnt.sum(dtype=np.uint64)) == len(keys)
        check_counts_rows(sc, [row], keys, k=k)
        assert sc.set_size() == M.set_size(keys, 1000, RM.use64_of(k))
    finally:
        job.free()
        sc.free()
    if mode == "preserve_case":
        assert len(keys) < len(conservation[k, "default"][1])
    if mode == "default":
        # the record, its reverse complement (and the palindrome) land on the canonical keys
        x = recs[4]
        assert sorted(M.window_keys(oracle, [x], k)) == \
            sorted(M.window_keys(oracle, [revcomp(x)], k))


@pytest.mark.parametrize("k", KS)
def test_contention(ctx, oracle, k):
    """8,192 A: every window is the same k-mer, one counter takes them all"""
    import fpmash
    key = oracle.get_hash(b"A" * k, 42, RM.use64_of(k))
    rows = [np.array([key], dtype_of(k)), np.array(sorted({1, key + 1}), dtype_of(k))]
    sc = make_screen(ctx, rows, k)
    try:
        sc.add_records(fpmash.make_params(k=k, s=1000), [b"A" * 8192])
        U, cnt = sc.counts()
        assert int(cnt[list(U).index(key)]) == 8192 - k + 1
        assert int(cnt.sum()) == 8192 - k + 1
        sh, me = sc.rows()
        assert list(sh) == [1, 0] and list(me) == [8192 - k + 1, 0]
    finally:
        sc.free()


# ---- crafted keys through add_hashes_dev -------------------------------------------------------
def crafted_db(k):
    rng = np.random.default_rng(17)
    if RM.use64_of(k):
        top = 2 ** 63 + 12345
        a = [0, 5, 2 ** 32 + 7, 2 ** 33 + 7, 2 ** 32 + 8, top]      # high / low dword twins
        run = list(range(10 ** 6, 10 ** 6 + 5000))                  # one directory bucket
    else:
        top = 0xFFFFFFFF
        a = [0, 5, 0x80000000, 0x80000001, 0xC0000000, top]         # top bit set
        run = list(range(10 ** 6, 10 ** 6 + 5000))
    shared1, shared2, shared64 = 77, 78, 79
    lists = [sorted(a + [shared1, shared2, shared64]), sorted(run + [shared2, shared64])]
    for i in range(62):
        lists.append(sorted([shared64, 10 ** 7 + 3 * i, 10 ** 7 + 3 * i + 1]))
    lists = [np.array(l, dtype_of(k)) for l in lists]
    U = np.unique(np.concatenate(lists).astype(np.uint64))
    reps = rng.integers(0, 6, size=len(U))
    keys = np.repeat(U, reps)
    miss = np.array([1, 6, 76, 80, 10 ** 6 - 1, 10 ** 6 + 5000, int(U[-1]) - 1,
                     min(int(U[-1]) + 1, 2 ** 64 - 1), 2 ** 40 + 1, 2 ** 62], np.uint64)
    miss = miss[~np.isin(miss, U)]
    keys = np.concatenate([keys, miss, np.array([0, 0, int(U[-1])], np.uint64)])
    rng.shuffle(keys)
    return lists, keys, (shared1, shared2, shared64)


@pytest.mark.parametrize("k", KS)
def test_crafted_keys(ctx, k):
    lists, keys, (s1, s2, s64) = crafted_db(k)
    sc = make_screen(ctx, lists, k)
    try:
        sc.add_hashes(keys)
        check_counts_rows(sc, lists, keys, winner_lengths=list(range(len(lists), 0, -1)), k=k)
        U, cnt = sc.counts()
        # the set-size row is untouched by add_hashes
        assert sc.set_size() == 0
        # every holder of a shared key sees its count: add more of the three and compare again
        more = np.array([s1] * 3 + [s2] * 4 + [s64] * 5, np.uint64)
        sc.add_hashes(more)
        check_counts_rows(sc, lists, np.concatenate([keys, more]), k=k)
    finally:
        sc.free()


# ---- rows --------------------------------------------------------------------------------------
def depth_db(k, lens, seed=3):
    """rows of the given lengths over disjoint keys, and pool keys that give row i a chosen
    number of counted cells with small depths and ties"""
    rng = np.random.default_rng(seed)
    dt = dtype_of(k)
    lists, keys, at = [], [], 1000
    for i, n in enumerate(lens):
        row = np.arange(at, at + 7 * n, 7, dtype=np.uint64)[:n]
        at += 7 * n + 100
        lists.append(row.astype(dt))
        want = [0, 1, 2, 3, n][i % 5] if n else 0
        hit = rng.choice(row, size=min(want, n), replace=False) if n else row
        for h in hit:
            keys += [int(h)] * int(rng.integers(1, 4))
    return lists, np.array(keys, np.uint64)


@pytest.mark.parametrize("k", KS)
def test_rows_lengths_and_shared(ctx, k):
    """row lengths 1 .. 1000 and an empty row; shared of 0, 1, 2, 3 and size; even and odd
    shared; depth ties; padded odd stride with poisoned padding"""
    import fpmash
    lens = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 5, 4, 6, 3, 2, 1000]
    lists, keys = depth_db(k, lens)
    poison = np.iinfo(dtype_of(k)).max
    for pad in (0, 3):
        sc = make_screen(ctx, lists, k, pad=pad, poison=poison)
        try:
            sc.add_hashes(keys)
            esh, _ = check_counts_rows(sc, lists, keys, winner_lengths=[1] * len(lists), k=k)
            assert ctx.last_screen_kernel() == fpmash.SK_ROWS_LDS
            assert {0, 1, 2, 3, 1000} <= set(esh)
        finally:
            sc.free()


def test_rows_large_depths(ctx):
    """counts of 1 beside counts >= 2^16 and >= 2^24: the selection reads all four bytes"""
    row = np.arange(10, 20, dtype=np.uint64)
    big = [(10, 1), (11, 1), (12, 70000), (13, (1 << 24) + 3), (14, 65536), (15, 2)]
    sc = make_screen(ctx, [row, row[:5]], 21)
    try:
        for key, c in big:
            sc.add_hashes(np.full(c, key, np.uint64))
        U, cnt = sc.counts()
        assert list(cnt[:6]) == [c for _, c in big]
        sh, me = sc.rows()
        # row 0: sorted depths [1, 1, 2, 65536, 70000, 2^24 + 3], position 3; row 1: [1, 1,
        # 65536, 70000, 2^24 + 3], position 2
        assert list(sh) == [6, 5] and list(me) == [65536, 65536]
    finally:
        sc.free()


def test_rows_lds_cap(ctx):
    """rows at the LDS cap - 1, at the cap and at the cap + 1: with the longest row at the cap
    the counters are held in LDS; one cell more and every pass gathers from global memory"""
    import fpmash
    cap = ctx.screen_lds_cap()
    rng = np.random.default_rng(9)
    for lens, kern in (([cap - 1, cap, 10], fpmash.SK_ROWS_LDS),
                       ([cap - 1, cap, cap + 1, 10], fpmash.SK_ROWS_GLOBAL)):
        lists = [np.sort(rng.choice(np.arange(1, 4 * cap, dtype=np.uint64), size=n, replace=False))
                 for n in lens]
        U = np.unique(np.concatenate(lists))
        keys = np.repeat(U, rng.integers(0, 4, size=len(U)))
        sc = make_screen(ctx, lists, 21)
        try:
            sc.add_hashes(keys)
            check_counts_rows(sc, lists, keys, winner_lengths=[5, 5, 7, 7][:len(lists)])
            assert ctx.last_screen_kernel() == kern
        finally:
            sc.free()


@pytest.mark.parametrize("n_db", [0, 1, 64, 65])
def test_rows_n_db(ctx, n_db):
    import fpmash
    rng = np.random.default_rng(n_db)
    pool = np.arange(1, 400, dtype=np.uint64) * np.uint64(2 ** 40 + 1)
    lists = [np.sort(rng.choice(pool, size=30, replace=False)) for _ in range(n_db)]
    keys = rng.choice(pool, size=2000)
    sc = make_screen(ctx, lists, 21)
    try:
        sc.add_hashes(keys)
        check_counts_rows(sc, lists, keys, winner_lengths=list(range(n_db)))
        assert ctx.last_screen_kernel() == (fpmash.SK_ROWS_LDS if n_db else fpmash.SK_NONE)
        assert len(sc.pvalues(np.zeros(n_db, np.uint32), 4.0 ** 21)) == n_db
    finally:
        sc.free()


# ---- chunking and set size ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_reads(oracle):
    reads = RM.base_reads()
    return reads, {k: RM.window_hashes(oracle, reads, k) for k in KS}


@pytest.mark.parametrize("k", KS)
def test_chunking(ctx, pool_reads, k):
    """the same pool in one add_job and in three: counters, set size and rows are equal (and the
    model's)"""
    import fpmash
    reads, streams = pool_reads
    keys = streams[k]
    rng = np.random.default_rng(1)
    distinct = np.unique(np.asarray(keys, np.uint64))
    lists = [np.sort(rng.choice(distinct, size=200, replace=False)).astype(dtype_of(k))
             for _ in range(5)]
    P = fpmash.make_params(k=k, s=100)
    got = []
    for cuts in ([0, len(reads)], [0, 7, 150, len(reads)]):
        sc = make_screen(ctx, lists, k, s=100)
        try:
            for a, b in zip(cuts, cuts[1:]):
                sc.add_records(P, reads[a:b])
            check_counts_rows(sc, lists, keys, k=k)
            got.append((sc.counts()[1].tolist(), sc.set_size(), [x.tolist() for x in sc.rows()]))
            assert got[-1][1] == M.set_size(keys, 100, RM.use64_of(k))
        finally:
            sc.free()
    assert got[0] == got[1]


@pytest.mark.parametrize("k", KS)
def test_pool_without_valid_kmer(ctx, k):
    import fpmash
    lists = [np.array([1, 2, 3], dtype_of(k)), np.array([2, 9], dtype_of(k))]
    sc = make_screen(ctx, lists, k, s=10)
    try:
        sc.add_records(fpmash.make_params(k=k, s=10), [b"N" * 100, b"ACGT", b"", b"ACGTN" * 30])
        assert sc.set_size() == 0
        sh, me = sc.rows()
        assert list(sh) == [0, 0] and list(me) == [0, 0]
        assert list(sc.pvalues(sh, 4.0 ** k)) == [1.0, 1.0]
    finally:
        sc.free()


@pytest.mark.parametrize("k", KS)
def test_set_size(ctx, oracle, pool_reads, k):
    """a pool with fewer than s distinct keys and one with more"""
    import fpmash
    reads, streams = pool_reads
    small = [reads[0][:k + 29]]
    small_keys = RM.window_hashes(oracle, small, k)
    for recs, keys, s in ((small, small_keys, 50), (reads, streams[k], 50)):
        exp = M.bottom_s(keys, s)
        assert (len(exp) < s) == (recs is small)
        sc = make_screen(ctx, [np.array([1], dtype_of(k))], k, s=s)
        try:
            sc.add_records(fpmash.make_params(k=k, s=s), recs)
            assert sc.set_size() == RM.set_size(exp, RM.use64_of(k))
        finally:
            sc.free()


# ---- -w ----------------------------------------------------------------------------------------
def test_winner(ctx):
    """a key shared by three references goes to the best score; an equal score is decided by
    length; a full tie goes to the lowest index; a zero-count key goes to nobody; medians come
    from the won depths only"""
    a = np.array([1, 2, 3, 10], np.uint64)        # 4 of 4 counted: score 1
    b = np.array([1, 2, 3, 20, 21], np.uint64)    # 3 of 5
    c = np.array([1, 2, 3, 30, 31], np.uint64)    # 3 of 5: ties with b
    d = np.array([3, 40, 50], np.uint64)          # 2 of 3; 50 is never seen
    keys = np.array([1] * 5 + [2] * 2 + [3] * 9 + [10] + [40] * 4, np.uint64)

    def run(lists, lengths):
        sc = make_screen(ctx, lists, 21)
        try:
            sc.add_hashes(keys)
            sh, _ = sc.rows()
            scores = [M.estimate_identity(int(x), len(l), 21) for x, l in zip(sh, lists)]
            wsh, wme = sc.rows_winner(scores, lengths)
            esh, eme = M.closed(lists, keys, winner=True, lengths=lengths)
            assert (list(wsh), list(wme)) == (esh, eme)
            lsh, lme = M.literal(lists, keys, winner=True, lengths=lengths)
            assert (list(wsh), list(wme)) == (lsh, lme)
            return list(wsh), list(wme)
        finally:
            sc.free()

    # a wins 1, 2, 3 (depths 5, 2, 9 and 10's 1 -> sorted [1, 2, 5, 9], position 2); d keeps 40
    assert run([c, a, b, d], [5, 5, 5, 5]) == ([0, 4, 0, 1], [0, 5, 0, 4])
    # without a: b and c tie at 3 of 5; d's 2 of 3 scores higher than 3 of 5 and takes key 3;
    # the longer of b, c takes 1 and 2
    assert run([c, b, d], [5, 9, 1]) == ([0, 2, 2], [0, 5, 9])
    # full tie: the lowest index
    assert run([c, b, d], [7, 7, 1]) == ([2, 0, 2], [5, 0, 9])
    assert run([b, c, d], [7, 7, 1]) == ([2, 0, 2], [5, 0, 9])


# ---- validation and p-values -------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("bad", [[1, 5, 5, 9], [1, 9, 5, 11]])
def test_rows_must_ascend(ctx, k, bad):
    import fpmash
    good = np.array([1, 2, 3, 4], dtype_of(k))
    with pytest.raises(fpmash.FpmError) as e:
        make_screen(ctx, [good, np.array(bad, dtype_of(k)), good], k)
    assert e.value.code == fpmash.FPM_EINVAL
    # the same values past a row's length are padding, not data
    sc = make_screen(ctx, [good, np.array(bad[:2], dtype_of(k))], k, pad=2, poison=0)
    sc.free()


def test_pvalues(ctx, oracle, pool_reads):
    """pValueWithin against the oracle's gsl_cdf_binomial_Q restatement; r from the screen's own
    set size.  FP64 continued fraction on both sides: 1e-12 relative, as the dist p-values."""
    import fpmash
    reads, streams = pool_reads
    keys = streams[21]
    sizes = [1000, 1000, 500, 10, 1, 1000, 3]
    shared = np.array([0, 1, 2, 10, 1, 1000, 4], np.uint32)
    lists = [np.arange(1, n + 1, dtype=np.uint64) * np.uint64(3) for n in sizes]
    sc = make_screen(ctx, lists, 21, s=1000)
    try:
        sc.add_records(fpmash.make_params(k=21, s=1000), reads)
        ss = sc.set_size()
        assert ss == M.set_size(keys, 1000)
        for space in (4.0 ** 21, float(ss) * 50.0, float(ss) / 2.0):
            got = sc.pvalues(shared, space)
            exp = [M.p_value_within(oracle, int(x), ss, space, n) for x, n in zip(shared, sizes)]
            assert got[0] == 1.0 and got[6] == 0.0
            assert np.allclose(got, exp, rtol=1e-12, atol=0)
    finally:
        sc.free()


def test_context_screen(ctx, oracle, pool_reads):
    """Context.screen end to end (the call __graft_entry__-style users make)"""
    import fpmash
    reads, streams = pool_reads
    keys = streams[21]
    distinct = np.unique(np.asarray(keys, np.uint64))
    db = [distinct[:300], distinct[100:500:2], np.array([5, 6], np.uint64)]
    for winner in (False, True):
        r = ctx.screen(fpmash.make_params(k=21, s=1000), db, reads, lengths=[3, 2, 1],
                       winner=winner, slices=3)
        esh, eme = M.closed(db, keys, winner=winner, lengths=[3, 2, 1])
        assert list(r["shared"]) == esh and list(r["median"]) == eme
        assert r["set_size"] == M.set_size(keys, 1000)
        assert list(r["identity"]) == [M.estimate_identity(a, len(l), 21) for a, l in zip(esh, db)]
