"""The screen table build (fpm_screen_create) where its job size changes what it launches,
against tests/screen_model.py's whole-matrix reference (closed_matrix, pinned to the list-by-list
model in tests/test_screen_model.py), exact.  Each table is built once and every check reads it.

B and F are the scan's block and the most blocks its two-launch form takes (fpm_scan_limits);
SBITS_MAX and DBITS_MAX are the clamps include/fpmash.h states for fpm_screen_table_info.

  fold-edge    the fewest rows of 1,000 u64 cells with more than F * B cells: the scan of the run
               heads over the cells takes three launches, the sort has 2^22 buckets without being
               clamped, and their scan is exactly F blocks, the most the two-launch form takes
  clamped      the fewest rows with more than 2^23 cells and more than 2^23 distinct values: the
               sort is clamped at 2^22 buckets of more than two cells, the directory at 2^24
               entries for more than 2^23 keys
  u32          fold-edge in u32 rows, three cells of padding that hold 0xFFFFFFFF
  heavy-tail   fold-edge where 0.1 % of the keys are held by 2,000 rows each: runs of 2,000 equal
               keys in the sort's buckets and posting lists as long for -w
"""
import numpy as np
import pytest

import fpmash
import screen_model as M

pytestmark = pytest.mark.gpu

B, F = fpmash.scan_limits()
SBITS_MAX, DBITS_MAX = 22, 24
WIDTH = 1000
DRAWS = 2_000_000
FOLD_ROWS = F * B // WIDTH + 1
# every cell but the ones scale_db gives to a shared key holds a value of its own
CLAMP_ROWS = ((1 << (SBITS_MAX + 1)) + M.scale_holders()) // WIDTH + 1
HEAVY_ROWS = 2000
# heavy keys h, each in HEAVY_ROWS cells, among u distinct: h = u / 1000 and
# u = cells - h * (HEAVY_ROWS - 1)
HEAVY = FOLD_ROWS * WIDTH // (1000 + HEAVY_ROWS - 1)

CASES = {
    "fold-edge": dict(n=FOLD_ROWS, dtype=np.uint64, pad=0),
    "clamped": dict(n=CLAMP_ROWS, dtype=np.uint64, pad=0),
    "u32": dict(n=FOLD_ROWS, dtype=np.uint32, pad=3),
    "heavy-tail": dict(n=FOLD_ROWS, dtype=np.uint64, pad=0, heavy=HEAVY),
}


class Built:
    pass


@pytest.fixture(scope="module", params=list(CASES))
def built(ctx, request):
    """the case's database, its table on the device with the pool's keys counted, the rows and
    -w read back, and the reference"""
    case = CASES[request.param]
    n, dtype, pad = case["n"], case["dtype"], case["pad"]
    heavy = case.get("heavy", 0)
    R, hot = M.scale_db(len(request.param), n, WIDTH, dtype, heavy, HEAVY_ROWS if heavy else 0)
    if pad:
        R = np.concatenate([R, np.full((n, pad), np.iinfo(dtype).max, dtype)], axis=1)
    lens = np.full(n, WIDTH, np.uint32)
    U = np.unique(R[:, :WIDTH]).astype(np.uint64)
    keys, miss = M.scale_pool(7, U, DRAWS, hot)
    b = Built()
    b.name, b.n, b.heavy, b.miss = request.param, n, heavy, miss
    b.lengths = np.random.default_rng(3).integers(1, 4, size=n).astype(np.uint64)
    b.ref = M.closed_matrix(R, lens, keys, lengths=b.lengths)
    sc = fpmash.Screen(ctx, R, lens, WIDTH)
    try:
        b.info = sc.table_info()
        sc.add_hashes(keys)
        b.U_dev, b.count = sc.counts()
        b.shared, b.median = sc.rows()
        b.rows_kernel = ctx.last_screen_kernel()
        b.wshared, b.wmedian = sc.rows_winner(b.ref["scores"], b.lengths)
        b.winner_kernel = ctx.last_screen_kernel()
    finally:
        sc.free()
    return b


def test_the_case_sits_where_it_is_named_for(built):
    info, E = built.info, built.n * WIDTH
    assert info["cells"] == E and E > F * B                 # the heads scan: three launches
    assert info["n_distinct"] == len(built.ref["U"])
    if built.name == "clamped":
        assert info["sbits"] == SBITS_MAX and 2 << SBITS_MAX < E
        assert info["dbits"] == DBITS_MAX and 1 << DBITS_MAX < 2 * info["n_distinct"]
        assert (built.n - 1) * WIDTH - M.scale_holders() <= 1 << (SBITS_MAX + 1)   # the fewest rows
    else:
        # 2^22 buckets because two cells per bucket ask for them, not because of the clamp; their
        # scan is the two-launch form at its most blocks
        assert (built.n - 1) * WIDTH <= F * B
        assert 2 << (info["sbits"] - 1) < E <= 2 << info["sbits"]
        assert 1 << info["sbits"] == F * B
        assert 1 << info["dbits"] >= 2 * info["n_distinct"] and info["dbits"] < DBITS_MAX
    if built.heavy:
        # a thousandth of the keys, each HEAVY_ROWS times in the sort and in its posting list
        assert 0.0009 < built.heavy / info["n_distinct"] < 0.0011
        assert int((built.ref["holders"] == HEAVY_ROWS).sum()) == built.heavy
    assert int(built.ref["holders"].max()) == (HEAVY_ROWS if built.heavy else M.SCALE_SHARED_ROWS)


def test_the_pool_holds_what_it_should(built):
    U, cnt, miss = built.ref["U"], built.ref["count"], built.miss
    assert len(miss) > 3000 and miss.min() < U[0] and miss.max() > U[-1]
    assert 1 < int(cnt.max()) < 2 ** 31 and (cnt == 0).sum() > len(U) // 2
    # medians that are not all alike, and -w moves entries between rows
    assert len(np.unique(built.ref["median"])) > 1
    assert not np.array_equal(built.ref["wshared"], built.ref["shared"])


def test_table_and_counters(built):
    assert np.array_equal(built.U_dev, built.ref["U"])
    bad = np.nonzero(built.count != built.ref["count"])[0]
    assert len(bad) == 0, f"{len(bad)} counters differ, the first at {bad[:10]}"


def test_rows(built):
    assert built.rows_kernel == fpmash.SK_ROWS_LDS
    assert np.array_equal(built.shared, built.ref["shared"])
    assert np.array_equal(built.median, built.ref["median"])


def test_rows_winner(built):
    assert built.winner_kernel == fpmash.SK_ROWS_LDS
    assert np.array_equal(built.wshared, built.ref["wshared"])
    assert np.array_equal(built.wmedian, built.ref["wmedian"])
    # every counted entry went to exactly one of its holders
    assert int(built.wshared.sum()) == int((built.ref["count"] > 0).sum())
