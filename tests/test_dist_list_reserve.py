"""GPU parity of the compact-list finalize (dist_cand_list_kernel and its block-wide slot
reservation): fpm_dist_list_dev must list exactly the cells that fpm_dist_dev16 marks with
numer > 0, with distance and p-value bit-equal between the two calls (the same device code on
the same inputs) and the count word equal to their number; counts exact and values to rtol
1e-12 against oracle.dist_grid.

The sets are small sorted u64 rows built on the host with the candidate count driven across
the kernel's boundaries: 256 candidates per workgroup pass, 4,096 workgroups at most (one more
candidate than 4,096 x 256 makes the grid-stride loop's second pass: the launcher sizes the
grid from the candidate capacity, which is never below the count, so no smaller set reaches
it).  A candidate is a pair that shares a value anywhere in its rows; one that shares a value
only beyond the union's S-th has numer 0 and stays out of the list.
"""
import numpy as np
import pytest

from test_gpu_dist_dispatch import RTOL, _Rows, _dev_dist, _dev_mirror

pytestmark = pytest.mark.gpu

S, KMER, SPACE = 16, 21, 4.0 ** 21
N_REF = 16
CHUNK, MAX_BLOCKS = 256, 4096
RANK_PATH = 2                         # last_dist_stats()["sparse"]: index + bucketed rank (C2's path)

# The index finds candidates by bucket and fingerprint (the top ~38 bits of a value), so the
# values are spread: two of them never share their top 28 bits unless they are equal.
G = 1 << 43                           # shared by all references and the full query rows


def _u(r):
    """shared by one pair (small: inside the union's first S)"""
    return (1 << 44) + (r << 40)


def _z(r):
    """shared by one pair, past the union's S-th"""
    return (1 << 63) + (r << 40)


class _Private:
    """distinct values between the _u and the _z, 2^36 apart, in random order"""

    def __init__(self, rng, n):
        self.pool = ((1 << 50) + (rng.permutation(n).astype(np.uint64) << np.uint64(36)))
        self.at = 0

    def __call__(self, n):
        out = self.pool[self.at:self.at + n]
        assert len(out) == n
        self.at += n
        return out


def _row(*parts):
    return np.sort(np.concatenate([np.asarray(p, np.uint64) for p in parts]))


def _sets(n_listed, n_zero, seed):
    """16 references and the queries that make candidates p = 0 .. n_listed - 1 the pairs
    (p // 16, p % 16), each sharing one small value, n_zero pairs sharing only a value past the
    union's S-th, and three queries sharing nothing -> (refs, ref lengths, qrys, qry lengths)"""
    rng = np.random.default_rng(seed)
    full, m = divmod(n_listed, N_REF)
    priv = _Private(rng, 8 * (N_REF + full + 1) + 9 * (n_zero + 3))
    refs = [_row([G, _u(r), _z(r)], priv(8)) for r in range(N_REF)]
    block = priv(8 * full).reshape(full, 8)
    qrys = [_row([G], block[q]) for q in range(full)]
    if m:
        qrys.append(_row([_u(r) for r in range(m)], priv(min(8, S - m))))
    for j in range(n_zero):
        qrys.append(_row([_z(j)], priv(9)))
    for _ in range(3):
        qrys.append(_row(priv(9)))
    rl = rng.integers(1000, 5000, size=len(refs)).astype(np.uint64)
    ql = rng.integers(1000, 5000, size=len(qrys)).astype(np.uint64)
    return refs, rl, qrys, ql


def _sparse(ctx):
    import fpmash
    ctx.set_dist_mode(fpmash.DIST_SPARSE)


def _auto(ctx):
    import fpmash
    ctx.set_dist_mode(fpmash.DIST_AUTO)


def _assert_same_cells(lst, full):
    """the expanded compact output against the five-array output of the same inputs: counts
    equal, and distance / p-value / pass of the listed cells bit-equal (expand_compact has
    checked that the list is exactly the cells with numer > 0, each once, and fetch that the
    count word is its length)"""
    assert np.array_equal(lst["numer"], full["numer"])
    assert np.array_equal(lst["denom"], full["denom"])
    on = full["numer"] > 0
    for key in ("distance", "pvalue"):
        assert np.array_equal(lst[key][on].view(np.uint64), full[key][on].view(np.uint64)), key
    assert np.array_equal(lst["pass"][on], full["pass"][on])


def _assert_oracle(got, exp):
    nu, de, di, pv = exp
    assert np.array_equal(got["numer"], nu) and np.array_equal(got["denom"], de)
    np.testing.assert_allclose(got["distance"], di, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["pvalue"], pv, rtol=RTOL, atol=0)


_CASES = [(0, 0), (1, 0), (255, 0), (256, 0), (257, 0), (254, 2), (255, 2),
          (MAX_BLOCKS * CHUNK + 1, 0)]


@pytest.mark.parametrize("n_listed,n_zero", _CASES)
def test_candidate_count_boundaries(ctx, oracle, n_listed, n_zero):
    refs, rl, qrys, ql = _sets(n_listed, n_zero, 8100 + n_listed % 1000 + n_zero)
    exp = oracle.dist_grid(refs, list(rl), qrys, list(ql), S, KMER, SPACE, threads=8)
    assert int((exp[0] > 0).sum()) == n_listed
    R, Q = _Rows(ctx, refs, rl, np.uint64), _Rows(ctx, qrys, ql, np.uint64)
    _sparse(ctx)
    try:
        lst = _dev_dist(ctx, R, Q, S, KMER, SPACE, api="list")
        st = ctx.last_dist_stats()
        full = _dev_dist(ctx, R, Q, S, KMER, SPACE, api="dist16")
    finally:
        _auto(ctx)
        R.free()
        Q.free()
    if n_listed + n_zero:
        assert st["sparse"] == RANK_PATH and st["candidates"] == n_listed + n_zero
    _assert_same_cells(lst, full)
    _assert_oracle(lst, exp)


def test_symmetric_self_set_mixes_one_and_two_entries(ctx, oracle):
    """One set against itself: a diagonal cell lists one entry, a pair off it two (the cell and
    its mirror), neighbours in one wave."""
    rng = np.random.default_rng(8201)
    n = 40
    priv = _Private(rng, 6 * n)
    rows = [_row([_u(i), _u(i + 1)], priv(6)) for i in range(n)]
    lens = rng.integers(1000, 5000, size=n).astype(np.uint64)
    exp = oracle.dist_grid(rows, list(lens), rows, list(lens), S, KMER, SPACE, threads=8)
    assert int((exp[0] > 0).sum()) == n + 2 * (n - 1)
    R = _Rows(ctx, rows, lens, np.uint64)
    _sparse(ctx)
    try:
        lst = _dev_dist(ctx, R, R, S, KMER, SPACE, api="list")
        assert ctx.last_dist_stats()["sparse"] == RANK_PATH
        full = _dev_dist(ctx, R, R, S, KMER, SPACE, api="dist16")
    finally:
        _auto(ctx)
        R.free()
    _assert_same_cells(lst, full)
    _assert_oracle(lst, exp)


def test_list_smaller_than_count(ctx, oracle):
    """cap < count: the count is exact, the first cap entries are listed cells (each once), and
    nothing is written past cap."""
    import fpmash
    n_listed, cap, room = 257, 100, 300
    refs, rl, qrys, ql = _sets(n_listed, 2, 8301)
    exp = oracle.dist_grid(refs, list(rl), qrys, list(ql), S, KMER, SPACE, threads=8)
    R, Q = _Rows(ctx, refs, rl, np.uint64), _Rows(ctx, qrys, ql, np.uint64)
    n = R.n * Q.n
    L = fpmash.lib()
    bufs = [fpmash.DeviceBuffer(ctx, n * 2) for _ in range(2)]
    lst = fpmash.CellList(ctx, room)
    for b in lst.bufs[:5]:
        fpmash._check(L.fpm_memset(ctx.h, b.ptr, 0xEE, b.nbytes))
    lst.struct.cap = cap
    _sparse(ctx)
    try:
        fpmash._check(L.fpm_dist_list_dev(ctx.h, R.rows, R.len.ptr, R.length.ptr, R.stride, R.n,
                                          Q.rows, Q.len.ptr, Q.length.ptr, Q.stride, Q.n, 8, S,
                                          KMER, SPACE, -1.0, -1.0, bufs[0].ptr, bufs[1].ptr,
                                          lst.ref, None))
        ctx.synchronize()
        assert lst.count() == n_listed
        q, r, di, pv, pa = (b.to_array(t, room) for b, t in zip(
            lst.bufs[:5], (np.uint32, np.uint32, np.float64, np.float64, np.uint8)))
    finally:
        _auto(ctx)
        for b in bufs + [R, Q, lst]:
            b.free()
    for a in (q, r, di, pv, pa):
        assert (a[cap:].view(np.uint8) == 0xEE).all()
    cell = q[:cap].astype(np.int64) * N_REF + r[:cap]
    assert len(np.unique(cell)) == cap and (exp[0][cell] > 0).all()
    np.testing.assert_allclose(di[:cap], exp[2][cell], rtol=RTOL, atol=0)
    np.testing.assert_allclose(pv[:cap], exp[3][cell], rtol=RTOL, atol=0)
    assert (pa[:cap] == 1).all()


@pytest.mark.parametrize("n_listed,n_zero", [(257, 2), (700, 0)])
def test_resident_set_mirror_lists(ctx, oracle, n_listed, n_zero):
    """fpm_refset_dist_mirror_list_dev: the grid's list and the transposed grid's, each against
    the five-array output of the same pairs."""
    refs, rl, qrys, ql = _sets(n_listed, n_zero, 8400 + n_listed)
    exp = oracle.dist_grid(refs, list(rl), qrys, list(ql), S, KMER, SPACE, threads=8)
    exp_t = oracle.dist_grid(qrys, list(ql), refs, list(rl), S, KMER, SPACE, threads=8)
    assert int((exp[0] > 0).sum()) == n_listed == int((exp_t[0] > 0).sum())
    R, Q = _Rows(ctx, refs, rl, np.uint64), _Rows(ctx, qrys, ql, np.uint64)
    _sparse(ctx)
    try:
        prim, mirr = _dev_mirror(ctx, R, Q, S, KMER, SPACE, compact=True)
        assert ctx.last_dist_stats()["sparse"] == RANK_PATH
        full = _dev_dist(ctx, R, Q, S, KMER, SPACE, api="dist16")
    finally:
        _auto(ctx)
        R.free()
        Q.free()
    _assert_same_cells(prim, full)
    full_t = {k: np.ascontiguousarray(v.reshape(Q.n, R.n).T).reshape(-1) for k, v in full.items()}
    _assert_same_cells(mirr, full_t)
    _assert_oracle(prim, exp)
    _assert_oracle(mirr, exp_t)
