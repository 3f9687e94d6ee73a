"""GPU parity of the compacted candidate rows (dist_index.hip: probe_rows_kernel with CMP;
dist.hip: rank_rows_kernel with CMP).

One sorted u64 set against itself through fpm_dist_list_dev and fpm_dist_dev16, the switch on
and off: every cell equals oracle.dist_grid (numer and denom exact, distance and p-value to
rtol 1e-12) and the two runs are equal.  Context.last_rank_compact must say that the candidates
were ranked on compacted rows and how many entries those hold: the rows' entries less the
hashes of each probed prefix that no other row holds (computed here from the rows; a
fingerprint collision may keep one more, which only the near-collision case provokes).
"""
import numpy as np
import pytest

from test_gpu_dist_dispatch import _Rows, _dev_dist
from test_gpu_index_cut import _assert_grid, _oracle_self
from test_gpu_parity import _shared_and_near_lists
from test_rank_compact_model import _compact, _prefix

pytestmark = pytest.mark.gpu

K = 21
SPACE = 4.0 ** K
APIS = ("list", "dist16")
KEYS = ("numer", "denom", "distance", "pvalue", "pass")


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


def _kept(rows, S):
    return sum(len(v) for v, _ in _compact(rows, S))


def _on_off(ctx, oracle, key, rows, S, stride=None, exact=True, kernel=None):
    """the set against itself by both entry points, the switch on and off -> the hook's report
    of the compacted runs"""
    import fpmash
    lengths = [3000 + 7 * i for i in range(len(rows))]
    exp = _oracle_self(oracle, key, rows, lengths, S)
    total, want = sum(len(x) for x in rows), _kept(rows, S)
    R = _Rows(ctx, rows, lengths, np.uint64, stride=stride, junk=5)
    hook = None
    try:
        for api in APIS:
            res = {}
            for on in (True, False):
                ctx.set_rank_compact(on)
                res[on] = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
                assert ctx.last_dist_stats()["sparse"] == 2
                assert ctx.last_dist_probe() == fpmash.PROBE_HALF
                if kernel is not None:
                    assert ctx.last_dist_kernel() == kernel
                h = ctx.last_rank_compact()
                if on:
                    assert h["compact"] and h["entries"] == total
                    assert h["kept"] == want if exact else want <= h["kept"] <= total
                    hook = h
                else:
                    assert h == {"compact": False, "kept": 0, "entries": 0}
                _assert_grid(res[on], exp)
            for k in KEYS:
                assert np.array_equal(res[True][k], res[False][k]), (api, k)
    finally:
        ctx.set_rank_compact(True)
        R.free()
    return hook, exp


def _pool(rng, n):
    """n distinct u64 values in random order, none of them 0 or ~0"""
    v = np.unique(rng.integers(1, 2 ** 64 - 1, size=n + n // 8 + 16, dtype=np.uint64))
    assert len(v) >= n
    return rng.permutation(v)[:n]


@pytest.mark.parametrize("S", [1000, 64])
def test_identical_rows_drop_nothing(cmp_ctx, oracle, S):
    rng = np.random.default_rng(S)
    one = np.sort(_pool(rng, S))
    rows = [one.copy() for _ in range(33)]
    h, exp = _on_off(cmp_ctx, oracle, ("rc-same", S), rows, S)
    assert h["kept"] == h["entries"] == 33 * S
    assert (exp[0] == S).all()


@pytest.mark.parametrize("S", [1000, 9])
def test_disjoint_rows_drop_every_prefix(cmp_ctx, oracle, S):
    """no value in two rows: every probed prefix goes, and the only cells with a shared value,
    hence the only candidates the rank kernel sees, are the diagonal's"""
    rng = np.random.default_rng(10 + S)
    n = 45
    lens = [S, S, max(S // 4, 1), S + 5, 0][:5]
    pool = _pool(rng, n * (S + 5))
    rows = [np.sort(pool[i * (S + 5):i * (S + 5) + lens[i % 5]]) for i in range(n)]
    h, exp = _on_off(cmp_ctx, oracle, ("rc-apart", S), rows, S)
    assert h["kept"] == sum(len(x) - _prefix(len(x), S) for x in rows)
    nu = exp[0].reshape(n, n)
    assert np.array_equal(nu > 0, np.diag([len(x) > 0 for x in rows]))
    assert cmp_ctx.last_dist_stats()["candidates"] == sum(len(x) > 0 for x in rows)


def _spaced(n, member, shared_pos):
    """a row of n values, value i near (i + 1) << 52: the same in every member at the positions
    shared_pos, else moved by the member's own offset (still between its neighbours)"""
    v = (np.arange(1, n + 1, dtype=np.uint64) << np.uint64(52))
    own = np.ones(n, bool)
    own[list(shared_pos)] = False
    v[own] += np.uint64((member + 1) << 38)
    return v


def _edge_set(S=1000):
    """S = 1000, H = 500.
    * a family of 20 full rows sharing the values at chosen positions, on both sides of H and at
      the row's ends;
    * pairs of short rows (400 entries, probed whole) sharing exactly 127 / 128 / 129 / 256
      values: compacted lengths at the rank kernel's chunk edges, no early exit;
    * pairs of full rows sharing 11 / 12 / 13 values of their prefixes: compacted lengths 511 /
      512 / 513;
    * a short row and a full row of values of their own, and two empty rows: compacted length 0
      resp. 500, seen on the diagonal only."""
    rng = np.random.default_rng(4)
    H = (S + 1) // 2
    pos = [0, 1, 2, 63, 64, 127, 128, 300, H - 2, H - 1, H, H + 1, 640, 900, S - 2, S - 1]
    rows = [_spaced(S, m, pos) for m in range(20)]
    want = [(len(pos), S - H + sum(p < H for p in pos))] * 20
    top = np.uint64(1) << np.uint64(63)
    for x in (127, 128, 129, 256):
        both = _pool(rng, x)
        for _ in range(2):
            rows.append(np.sort(np.concatenate([both, _pool(rng, 400 - x)])))
            want.append((x, x))
    for x in (11, 12, 13):
        both = _pool(rng, x) >> np.uint64(1)
        for _ in range(2):
            rows.append(np.sort(np.concatenate([both, _pool(rng, H - x) >> np.uint64(1),
                                                _pool(rng, S - H) | top])))
            want.append((x, S - H + x))
    rows += [np.sort(_pool(rng, 300)), np.sort(_pool(rng, S)), np.zeros(0, np.uint64),
             np.zeros(0, np.uint64)]
    want += [(0, 0), (0, S - H), (0, 0), (0, 0)]
    rows = [np.asarray(x, np.uint64) for x in rows]
    assert all(len(np.unique(x)) == len(x) for x in rows)
    return rows, want


def test_chunk_edges_short_and_empty_rows(cmp_ctx, oracle):
    import fpmash
    S = 1000
    rows, want = _edge_set(S)
    assert len(rows) == 38 and len(rows) % 32
    comp = _compact(rows, S)
    assert [len(v) for v, _ in comp] == [w[1] for w in want]
    assert {0, 127, 128, 129, 256, 511, 512, 513} <= {len(v) for v, _ in comp}
    h, exp = _on_off(cmp_ctx, oracle, ("rc-edges", S), rows, S, kernel=fpmash.DK_CAND_RANK_1024)
    assert h["kept"] == sum(w[1] for w in want) < h["entries"]
    nu = exp[0].reshape(len(rows), len(rows))
    # (of the family's 16 shared positions the 12 up to H + 1 rank below S: 2 p - k < 1000)
    assert nu[0, 1] == 12
    assert nu[20, 21] == 127 and nu[26, 27] == 256 and nu[28, 29] == 11 and nu[32, 33] == 13


def test_rows_of_2000_at_stride_2048(cmp_ctx, oracle):
    """the CAP 2048 instance: rows twice as long as S, their tails copied whole"""
    import fpmash
    S, n = 1000, 33
    rng = np.random.default_rng(6)
    fam = np.sort(_pool(rng, 3000))
    rows = []
    for m in range(n):
        pick = fam[rng.random(len(fam)) < 0.5]
        rows.append(np.sort(np.concatenate([pick, _pool(rng, 2000)]))[:2000])
        assert len(np.unique(rows[-1])) == 2000
    h, exp = _on_off(cmp_ctx, oracle, ("rc-2048", S), rows, S, stride=2048,
                     kernel=fpmash.DK_CAND_RANK_2048)
    assert n * 1500 < h["kept"] < h["entries"] == n * 2000
    assert (exp[0] > 0).all()


@pytest.mark.parametrize("S", [9, 64])
def test_small_sketch_sizes(cmp_ctx, oracle, S):
    """odd S (H = 5) and S = 64: families of full rows, a short row in each"""
    rng = np.random.default_rng(20 + S)
    rows = []
    for f in range(5):
        base = np.sort(_pool(rng, 2 * S))
        for m in range(8):
            pick = base[rng.random(len(base)) < 0.6]
            ln = S if m else S // 2
            rows.append(np.sort(np.concatenate([pick, _pool(rng, S)]))[:ln])
    assert len(rows) == 40
    h, exp = _on_off(cmp_ctx, oracle, ("rc-small", S), rows, S)
    assert 0 < h["kept"] < h["entries"]
    assert (exp[0] > 0).sum() > len(rows)


def test_near_collision_rows(cmp_ctx, oracle):
    """_shared_and_near_lists: rows of the same base values offset by 0 / 1 / 2 share bucket and
    fingerprint but no value (an event on another row's entry keeps a value no row shares), and
    rows up to 1,100 entries, longer than S"""
    rng = np.random.default_rng(77)
    rows = _shared_and_near_lists(rng)
    assert len(rows) == 192
    for S in (1000, 300):
        h, _ = _on_off(cmp_ctx, oracle, ("rc-near", S), rows, S, exact=False)
        assert h["kept"] < h["entries"]


def test_speculated_probe_hit_and_capacity_miss(cmp_ctx, oracle):
    """the second call of a shape enqueues its probe, compacted rows included, before the index
    build's counters are read; a set of the same shape with far more candidates than the
    profile's capacity drops that probe and runs a second one"""
    ctx = cmp_ctx
    # (S = 9: the disjoint set's posting events, hence the profile's capacity, stay well below
    # the 1,600 pairs that the identical rows then need)
    S, n = 9, 40
    rng = np.random.default_rng(31)
    pool = _pool(rng, n * S)
    apart = [np.sort(pool[i * S:(i + 1) * S]) for i in range(n)]
    same = [apart[0].copy() for _ in range(n)]
    lengths = [3000 + 7 * i for i in range(n)]
    exp_a = _oracle_self(oracle, ("rc-spec-apart", S), apart, lengths, S)
    exp_s = _oracle_self(oracle, ("rc-spec-same", S), same, lengths, S)
    Ra = _Rows(ctx, apart, lengths, np.uint64)
    Rs = _Rows(ctx, same, lengths, np.uint64)
    try:
        first = _dev_dist(ctx, Ra, Ra, S, K, SPACE, api="list")
        h0, m0 = ctx.spec_stats()
        again = _dev_dist(ctx, Ra, Ra, S, K, SPACE, api="list")
        assert ctx.spec_stats() == (h0 + 1, m0)
        assert ctx.last_rank_compact() == {"compact": True, "kept": n * (S - (S + 1) // 2),
                                           "entries": n * S}
        _assert_grid(first, exp_a)
        _assert_grid(again, exp_a)
        dense = _dev_dist(ctx, Rs, Rs, S, K, SPACE, api="list")
        assert ctx.spec_stats() == (h0 + 1, m0 + 1)
        assert ctx.last_rank_compact() == {"compact": True, "kept": n * S, "entries": n * S}
        _assert_grid(dense, exp_s)
    finally:
        Ra.free()
        Rs.free()


def test_other_paths_are_not_compacted(cmp_ctx, oracle):
    """another ref set (a copy of the rows), the full probe form and the dense walk: the hook
    says so, the results are the oracle's"""
    import fpmash
    ctx = cmp_ctx
    S = 64
    rng = np.random.default_rng(20 + S)
    rows = []
    for f in range(5):
        base = np.sort(_pool(rng, 2 * S))
        for m in range(8):
            pick = base[rng.random(len(base)) < 0.6]
            rows.append(np.sort(np.concatenate([pick, _pool(rng, S)]))[:S if m else S // 2])
    lengths = [3000 + 7 * i for i in range(len(rows))]
    exp = _oracle_self(oracle, ("rc-small", S), rows, lengths, S)
    none = {"compact": False, "kept": 0, "entries": 0}
    R = _Rows(ctx, rows, lengths, np.uint64)
    Q = _Rows(ctx, rows, lengths, np.uint64)
    try:
        for api in APIS:
            got = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
            assert ctx.last_rank_compact()["compact"]
            _assert_grid(got, exp)
            got = _dev_dist(ctx, R, Q, S, K, SPACE, api=api)
            assert ctx.last_dist_stats()["sparse"] == 2 and ctx.last_rank_compact() == none
            _assert_grid(got, exp)
            ctx.set_probe_half(False)
            got = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
            assert ctx.last_dist_probe() == fpmash.PROBE_FULL and ctx.last_rank_compact() == none
            _assert_grid(got, exp)
            ctx.set_probe_half(True)
            ctx.set_dist_mode(fpmash.DIST_DENSE)
            got = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
            assert ctx.last_dist_stats()["sparse"] == 0 and ctx.last_rank_compact() == none
            _assert_grid(got, exp)
            ctx.set_dist_mode(fpmash.DIST_SPARSE)
    finally:
        R.free()
        Q.free()
