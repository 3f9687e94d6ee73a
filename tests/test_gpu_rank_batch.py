"""GPU parity of the rank kernel's candidate loop at its batch edges (dist.hip: rank_rows_kernel;
DESIGN §4).

A wave of the kernel takes every kRankWaves-th candidate of its query row, in batches of 64: the
cases here put rows with 0, 1, 3, 4, 5, 255, 256, 257, 512 and 513 candidates beside each other
(a wave's first, last and partial batch, the second batch) and run both of the kernel's store
paths.  `list`, `dist16` and `dist` hand it the per-candidate arrays (cnum / cden: the cells and
their mirrors are then written by the finalize kernels, u16 or u32); the counts-only grid
(fpm_compare_grid_dev, `_grid_dev`) hands it none, and its lanes store the u32 cells and their
mirrors themselves.  Both run on the compacted and the plain rows and with a copy of the set as
the query set (no mirror); one set mixes row shapes among the candidates of one wave, one ranks
rows of 2,000 entries.

Every case compares all cells with oracle.dist_grid (numer and denom exact; distance and p-value
to rtol 1e-12 where the entry point computes them) and with the forced dense run of the same
call.
"""
import numpy as np
import pytest

from test_gpu_dist_dispatch import _Rows, _dev_dist
from test_gpu_index_cut import _assert_grid, _oracle_self
from test_rank_compact_model import _compact

K = 21
SPACE = 4.0 ** K
KEYS = ("numer", "denom", "distance", "pvalue", "pass")
WAVES = 4                       # kRankWaves
EDGES = (0, 1, 3, 4, 5, 255, 256, 257, 512, 513)


@pytest.fixture
def cmp_ctx(ctx):
    """forced sparse, every switch on; back to the defaults afterwards"""
    import fpmash

    def defaults():
        ctx.set_rank_compact(True)
        ctx.set_index_cut(True)
        ctx.set_probe_half(True)
    defaults()
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    yield ctx
    defaults()
    ctx.set_dist_mode(fpmash.DIST_AUTO)


def _pool(rng, n, lo=1 << 32):
    """n distinct u64 values in random order, from lo up and below ~0"""
    v = np.unique(rng.integers(lo, 2 ** 64 - 1, size=n + n // 8 + 16, dtype=np.uint64))
    assert len(v) >= n
    return rng.permutation(v)[:n]


def _mutual(sizes, empty, lo, hi, seed):
    """groups of sizes[g] rows, one after the other: every row of group g holds the small hash
    (g + 1) << 56 at position 0 (the groups' hashes differ in their top bits, which the index
    takes its bucket and fingerprint from: no two groups meet in the probe) and lo - 1 .. hi - 1
    hashes of its own, all from 2^60 up, behind it; then `empty` empty rows -> (rows, the group
    of each row, -1 for an empty one)"""
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(lo, hi + 1)) for m in sizes for _ in range(m)]
    own = _pool(rng, sum(lens), lo=1 << 60)
    rows, group, at = [], [], 0
    for g, m in enumerate(sizes):
        for _ in range(m):
            ln = lens[len(rows)]
            rows.append(np.sort(np.concatenate([np.array([(g + 1) << 56], np.uint64),
                                                own[at:at + ln - 1]])))
            group.append(g)
            at += ln - 1
    rows += [np.zeros(0, np.uint64) for _ in range(empty)]
    group += [-1] * empty
    return rows, np.array(group)


def _candidates(group):
    """candidates per row of a set whose rows share a hash exactly within their group: the pair
    (q, r) is ranked once, in the lower row when q + r is odd, in the higher (and the diagonal)
    when it is even"""
    n = len(group)
    idx = np.arange(n)
    out = np.zeros(n, np.int64)
    for q in range(n):
        if group[q] < 0:
            continue
        same = group == group[q]
        odd = ((idx + q) & 1) == 1
        out[q] = np.count_nonzero(same & (((idx > q) & odd) | ((idx <= q) & ~odd)))
    return out


# the two sets of the batch edges: groups of 1,024 (512 / 513 candidates per row), 8 (4 / 5), 5
# (3) and 1 (1) rows with three empty rows (0), and groups of 510 (255 / 256) and 513 (257)
EDGE_SETS = {"a": ((1024, 8, 5, 1), 3, 11), "b": ((510, 513), 1, 12)}


def _edge_rows(name):
    sizes, empty, seed = EDGE_SETS[name]
    return _mutual(sizes, empty, 16, 64, seed)


def _lengths(rows):
    return [3000 + 7 * (i % 89) for i in range(len(rows))]


def _self_runs(ctx, oracle, key, rows, S, apis, stride=None, kernel=None, compact=(True, False),
               candidates=None):
    """the set against itself by `apis`, on the compacted and on the plain rows: each equals the
    oracle and the forced dense run; the candidate total where given"""
    import fpmash
    lengths = _lengths(rows)
    exp = _oracle_self(oracle, key, rows, lengths, S)
    R = _Rows(ctx, rows, lengths, np.uint64, stride=stride, junk=5)
    try:
        for api in apis:
            ctx.set_dist_mode(fpmash.DIST_DENSE)
            dense = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
            assert ctx.last_dist_stats()["sparse"] == 0
            ctx.set_dist_mode(fpmash.DIST_SPARSE)
            _assert_grid(dense, exp)
            for on in compact:
                ctx.set_rank_compact(on)
                got = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
                st = ctx.last_dist_stats()
                assert st["sparse"] == 2 and ctx.last_rank_compact()["compact"] == on
                assert ctx.last_dist_kernel() == (kernel or fpmash.DK_CAND_RANK_1024)
                if candidates is not None:
                    assert st["candidates"] == candidates
                _assert_grid(got, exp)
                for k in KEYS:
                    assert np.array_equal(got[k], dense[k]), (api, on, k)
    finally:
        ctx.set_rank_compact(True)
        ctx.set_dist_mode(fpmash.DIST_SPARSE)
        R.free()
    return exp


def test_edge_sets_hold_every_edge():
    """(no device: runs in the CPU suite) the two sets together hold rows with every candidate count of EDGES"""
    seen = set()
    for name in EDGE_SETS:
        rows, group = _edge_rows(name)
        assert all(len(np.unique(x)) == len(x) for x in rows)
        assert all(16 <= len(x) <= 64 for x, g in zip(rows, group) if g >= 0)
        seen |= set(_candidates(group).tolist())
    assert set(EDGES) <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("name,S", [("a", 16), ("a", 64), ("b", 64), ("b", 16)])
def test_batch_edges(cmp_ctx, oracle, name, S):
    """every pair of a group is a candidate: rows with 0 .. 513 candidates, a wave's batches
    full, partial and empty; S = 16: every row is full (H = 8 probed), S = 64: nearly every row
    is shorter than S (denom from the shared count)"""
    rows, group = _edge_rows(name)
    cand = _candidates(group)
    want = {"a": (0, 1, 3, 4, 5, 512, 513), "b": (0, 255, 256, 257)}[name]
    assert set(want) <= set(cand.tolist())
    exp = _self_runs(cmp_ctx, oracle, ("rb-edge", name, S), rows, S, ("list",),
                     candidates=int(cand.sum()))
    n = len(rows)
    nu = exp[0].reshape(n, n)
    assert np.array_equal(nu > 0, (group[:, None] == group[None, :]) & (group[:, None] >= 0))


def _paths_rows():
    """515 rows that share one hash: 258 candidates per row, 64 or 65 per wave"""
    rows, group = _mutual((515,), 0, 16, 64, 13)
    return rows, _candidates(group)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 16])
def test_entry_points_counts_and_rows(cmp_ctx, oracle, S):
    """the candidate arrays, finalized into the list (`list`) and into u16 and u32 cells
    (`dist16`, `dist`), each on the compacted and on the plain rows"""
    rows, cand = _paths_rows()
    assert cand.min() > 256 and -(-int(cand.max()) // WAVES) > 64
    _self_runs(cmp_ctx, oracle, ("rb-paths", S), rows, S, ("list", "dist16", "dist"),
               candidates=int(cand.sum()))


@pytest.mark.gpu
def test_copy_as_query_set_has_no_mirror(cmp_ctx, oracle):
    """a copy of the rows as the query set: not symmetric, every pair ranked in its own row (515
    candidates per row, three batches per wave), through the candidate arrays"""
    import fpmash
    ctx, S = cmp_ctx, 64
    rows, _ = _paths_rows()
    lengths = _lengths(rows)
    exp = _oracle_self(oracle, ("rb-paths", S), rows, lengths, S)
    R = _Rows(ctx, rows, lengths, np.uint64, junk=5)
    Q = _Rows(ctx, rows, lengths, np.uint64, junk=6)
    try:
        for api in ("list", "dist16", "dist"):
            got = _dev_dist(ctx, R, Q, S, K, SPACE, api=api)
            st = ctx.last_dist_stats()
            assert st["sparse"] == 2 and not ctx.last_rank_compact()["compact"]
            assert ctx.last_dist_kernel() == fpmash.DK_CAND_RANK_1024
            assert st["candidates"] == len(rows) ** 2
            _assert_grid(got, exp)
            ctx.set_dist_mode(fpmash.DIST_DENSE)
            dense = _dev_dist(ctx, R, Q, S, K, SPACE, api=api)
            ctx.set_dist_mode(fpmash.DIST_SPARSE)
            for k in KEYS:
                assert np.array_equal(got[k], dense[k]), (api, k)
    finally:
        ctx.set_dist_mode(fpmash.DIST_SPARSE)
        R.free()
        Q.free()


def _grid_dev(ctx, R, Q, S):
    """fpm_compare_grid_dev on two uploaded row sets: u32 numer / denom of every cell.  The
    counts-only entry point hands the rank kernel no candidate arrays, so the kernel itself
    stores the cells (and, one set against itself, their mirrors); every `_dev_dist` entry
    point goes through the candidate arrays and leaves the cells to the finalize kernels."""
    import fpmash
    n = R.n * Q.n
    bufs = [fpmash.DeviceBuffer(ctx, max(n, 1) * 4) for _ in range(2)]
    try:
        for b in bufs:
            fpmash._check(fpmash.lib().fpm_memset(ctx.h, b.ptr, 0xEE, b.nbytes))
        fpmash._check(fpmash.lib().fpm_compare_grid_dev(
            ctx.h, R.rows, R.len.ptr, R.stride, R.n, Q.rows, Q.len.ptr, Q.stride, Q.n,
            R.dtype.itemsize, S, bufs[0].ptr, bufs[1].ptr, None))
        ctx.synchronize()
        return tuple(b.to_array(np.uint32, max(n, 1))[:n] for b in bufs)
    finally:
        for b in bufs:
            b.free()


def _direct_runs(ctx, exp, R, Q, S, candidates, kernel=None):
    """the rank kernel's own cell stores: the counts-only grid forced sparse, on the compacted
    rows where the call has them and on the plain rows, against the oracle and the dense run"""
    import fpmash
    try:
        ctx.set_dist_mode(fpmash.DIST_DENSE)
        dense = _grid_dev(ctx, R, Q, S)
        assert ctx.last_dist_stats()["sparse"] == 0
        ctx.set_dist_mode(fpmash.DIST_SPARSE)
        seen = set()
        for on in (True, False):
            ctx.set_rank_compact(on)
            nu, de = _grid_dev(ctx, R, Q, S)
            st = ctx.last_dist_stats()
            assert st["sparse"] == 2 and st["candidates"] == candidates
            assert ctx.last_dist_kernel() == (kernel or fpmash.DK_CAND_RANK_1024)
            seen.add(ctx.last_rank_compact()["compact"])
            assert np.array_equal(nu, exp[0]) and np.array_equal(de, exp[1])
            assert np.array_equal(nu, dense[0]) and np.array_equal(de, dense[1])
        return seen
    finally:
        ctx.set_rank_compact(True)
        ctx.set_dist_mode(fpmash.DIST_SPARSE)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 16])
def test_direct_cells_and_mirrors(cmp_ctx, oracle, S):
    """the 515 rows against themselves through the counts-only grid: 258 candidates per row, a
    wave's full and partial batch stored by their owning lanes, cell and mirror cell"""
    rows, cand = _paths_rows()
    lengths = _lengths(rows)
    exp = _oracle_self(oracle, ("rb-paths", S), rows, lengths, S)
    R = _Rows(cmp_ctx, rows, lengths, np.uint64, junk=5)
    try:
        seen = _direct_runs(cmp_ctx, exp, R, R, S, int(cand.sum()))
        assert False in seen
    finally:
        R.free()


@pytest.mark.gpu
def test_direct_cells_copy_as_query_set(cmp_ctx, oracle):
    """a copy of the rows as the query set through the counts-only grid: 515 candidates per row,
    three batches per wave, every cell stored once and no mirror"""
    S = 64
    rows, _ = _paths_rows()
    lengths = _lengths(rows)
    exp = _oracle_self(oracle, ("rb-paths", S), rows, lengths, S)
    R = _Rows(cmp_ctx, rows, lengths, np.uint64, junk=5)
    Q = _Rows(cmp_ctx, rows, lengths, np.uint64, junk=6)
    try:
        assert _direct_runs(cmp_ctx, exp, R, Q, S, len(rows) ** 2) == {False}
    finally:
        R.free()
        Q.free()


def _shape_set(S=300):
    """S = 300.  A family of rows that all hold the hash 7 at position 0 and the x smallest of
    256 family values (two members hold all 256, so a member's x family values are each held by
    another row), the rest of each row its own:
    * short members (below S, probed whole: compacted length x, denom from the shared count) of
      (x, length) with x and length at 1, 64, 65 and 128 past a multiple of 128;
    * full members (S and more: the probed half keeps what it shares, the tail stays);
    * beside the family a short and a full row of values of their own (compacted length 0 and
      S - H: candidates on the diagonal only) and two empty rows.
    The shapes repeat three times, so a wave meets them within one batch."""
    rng = np.random.default_rng(9)
    fam = np.sort(_pool(rng, 255) >> np.uint64(4))
    fam = np.concatenate([np.array([7], np.uint64), fam])
    shapes = [(1, 1), (64, 64), (65, 65), (128, 128), (1, 129), (64, 192), (65, 193), (128, 256),
              (256, 256), (256, 299), (129, 299), (192, 257), (193, 200), (1, 300), (64, 428),
              (65, 512), (128, 1024), (256, 1000)]
    rows = []
    for rep in range(3):
        for x, ln in shapes:
            rows.append(np.sort(np.concatenate([fam[:x], _pool(rng, ln - x)])))
    rows += [np.sort(_pool(rng, 120)), np.sort(_pool(rng, 400)), np.zeros(0, np.uint64),
             np.zeros(0, np.uint64)]
    assert all(len(np.unique(x)) == len(x) for x in rows)
    return rows, shapes


@pytest.mark.gpu
def test_row_shapes_within_a_batch(cmp_ctx, oracle):
    S = 300
    rows, shapes = _shape_set(S)
    n, nf = len(rows), 3 * len(shapes)
    H = (S + 1) // 2
    kept = [len(v) for v, _ in _compact(rows, S)]
    # short members keep their x family values, full members what their probed half shares and
    # their tail; the rows beside the family keep nothing resp. their tail
    for i, (x, ln) in enumerate(shapes * 3):
        if ln < S:
            assert kept[i] == x
        else:
            assert ln - H <= kept[i] <= ln - H + min(x, H)
    assert kept[nf:] == [0, 400 - H, 0, 0]
    # a last chunk of 1, 64, 65 and 128 entries, streamed from the compacted and the plain rows
    for lens in (kept[:nf], [len(x) for x in rows[:nf]]):
        assert {1, 64, 65, 0} <= {ln % 128 for ln in lens if ln}
    group = np.array([0] * nf + [1, 2, -1, -1])
    cand = _candidates(group)
    assert cand[:nf].min() >= nf // 2 and cand[nf:].tolist() == [1, 1, 0, 0]
    exp = _self_runs(cmp_ctx, oracle, ("rb-shapes", S), rows, S, ("list", "dist16"),
                     candidates=int(cand.sum()))
    nu, de = exp[0].reshape(n, n), exp[1].reshape(n, n)
    assert nu[0, 1] == 1 and nu[8, 9] == 256 and nu[3, 7] == 128
    assert de[0, 1] == 64 and de[8, 9] == 299 and (de[15, 16] == S)
    # the same shapes stored by the rank kernel itself (the diagonal's closed form and the denom
    # from the shared count are computed by the storing lanes)
    R = _Rows(cmp_ctx, rows, _lengths(rows), np.uint64, junk=5)
    try:
        _direct_runs(cmp_ctx, exp, R, R, S, int(cand.sum()))
    finally:
        R.free()


@pytest.mark.gpu
def test_rows_of_2000_at_stride_2048(cmp_ctx, oracle):
    """the CAP 2048 instance: 33 rows of 2,000 entries that all share values, 16 or 17
    candidates per row"""
    import fpmash
    S, n = 1000, 33
    rng = np.random.default_rng(6)
    fam = np.sort(_pool(rng, 3000))
    rows = []
    for m in range(n):
        pick = fam[rng.random(len(fam)) < 0.5]
        rows.append(np.sort(np.concatenate([pick, _pool(rng, 2000)]))[:2000])
        assert len(np.unique(rows[-1])) == 2000
    cand = _candidates(np.zeros(n, np.int64))
    assert cand.min() >= 5
    exp = _self_runs(cmp_ctx, oracle, ("rb-2048", S), rows, S, ("list", "dist16"), stride=2048,
                     kernel=fpmash.DK_CAND_RANK_2048, candidates=int(cand.sum()))
    assert (exp[0] > 0).all()
    R = _Rows(cmp_ctx, rows, _lengths(rows), np.uint64, stride=2048, junk=5)
    try:
        _direct_runs(cmp_ctx, exp, R, R, S, int(cand.sum()), kernel=fpmash.DK_CAND_RANK_2048)
    finally:
        R.free()
