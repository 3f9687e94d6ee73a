"""GPU parity of the half probe (dist_index.hip, probe_rows_kernel<HALF>): one sorted set
against itself on the forced index path, where each row probes only its visited prefix and a
pair is taken by its parity owner when that row sees it, else by the other row.

Every case compares the result with oracle.dist_grid: numer and denom exact, distance and
p-value to RTOL, and no (qry, ref) repeated in the compact list.  Where the path allows it the
call must report the HALF form (Context.last_dist_probe), and the arrays must be bit-identical
with the switch off (Context.set_probe_half(False)), which must report FULL.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-12
K = 21
SPACE = 4.0 ** K

_EXP = {}


def _oracle_self(oracle, key, lists, lengths, S):
    """the oracle's grid of one set against itself (computed once per key, never modified)"""
    if key not in _EXP:
        res = oracle.dist_grid(list(lists), list(lengths), list(lists), list(lengths), S, K, SPACE,
                               threads=8)
        for a in res:
            a.setflags(write=False)
        _EXP[key] = res
    return _EXP[key]


def _assert_grid(got, exp):
    nu, de, di, pv = exp
    assert np.array_equal(np.asarray(got["numer"]).astype(np.uint32), nu)
    assert np.array_equal(np.asarray(got["denom"]).astype(np.uint32), de)
    np.testing.assert_allclose(got["distance"], di, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got["pvalue"], pv, rtol=RTOL, atol=0)


def _assert_same(a, b):
    for key in ("numer", "denom", "distance", "pvalue", "pass"):
        assert np.array_equal(a[key], b[key]), key


def _no_repeats(listed, n):
    idx = listed["qry"].astype(np.int64) * n + listed["ref"].astype(np.int64)
    assert len(np.unique(idx)) == len(idx), "a (qry, ref) is listed twice"


@pytest.fixture
def sparse(ctx):
    """the forced index path, and the half switch back on afterwards"""
    import fpmash
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    ctx.set_probe_half(True)
    yield ctx
    ctx.set_probe_half(True)
    ctx.set_dist_mode(fpmash.DIST_AUTO)


def _self_both_forms(ctx, lists, lengths, S, exp, half_form=None):
    """the set against itself through ctx.dist and ctx.dist_list, with the switch on (the
    form `half_form`, HALF unless given) and off (FULL): each equals the oracle, the two are
    bit-identical"""
    import fpmash
    want = fpmash.PROBE_HALF if half_form is None else half_form
    n = len(lists)
    kw = dict(use64=True, k=K, ref_lengths=lengths, qry_lengths=lengths)
    res = {}
    for on in (True, False):
        ctx.set_probe_half(on)
        full = ctx.dist(lists, lists, S, **kw)
        assert ctx.last_dist_stats()["sparse"] == 2
        assert ctx.last_dist_probe() == (want if on else fpmash.PROBE_FULL)
        _assert_grid(full, exp)
        nu, de, listed = ctx.dist_list(lists, lists, S, expand=False, **kw)
        assert ctx.last_dist_stats()["sparse"] == 2
        assert ctx.last_dist_probe() == (want if on else fpmash.PROBE_FULL)
        _no_repeats(listed, n)
        comp = fpmash.expand_compact(nu, de, listed, n)
        _assert_grid(comp, exp)
        res[on] = (full, comp)
    _assert_same(res[True][0], res[False][0])
    _assert_same(res[True][1], res[False][1])


# ---- 1. boundary grid ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _boundary_rows(S):
    """for every (i, p) in [0, S)^2 a pair of rows of S values whose only shared value sits at
    position i of one and p of the other; every other value a private random u64"""
    rng = np.random.default_rng(900 + S)
    rows = []

    def row(v, at):
        lo = rng.integers(1, int(v), size=at, dtype=np.uint64)
        hi = rng.integers(int(v) + 1, 2 ** 64, size=S - 1 - at, dtype=np.uint64)
        x = np.sort(np.concatenate([lo, [np.uint64(v)], hi]).astype(np.uint64))
        assert len(np.unique(x)) == S and x[at] == v
        return x
    for i in range(S):
        for p in range(S):
            v = rng.integers(2 ** 62, 2 ** 63, dtype=np.uint64)
            rows += [row(v, i), row(v, p)]
    assert len(np.unique(np.concatenate(rows))) == len(rows) * S - S * S
    return rows, [1000 + 13 * j for j in range(len(rows))]


@pytest.mark.parametrize("S", [8, 9])
def test_boundary_grid(sparse, oracle, S):
    """The shared value at every pair of positions: i + p = S - 1 counts (numer 1) and i + p =
    S does not; i < H <= p, p < H <= i, and both sides at H - 1 and at H (H = ceil(S / 2):
    even and odd S)."""
    rows, lengths = _boundary_rows(S)
    n = len(rows)
    assert n == 2 * S * S <= 162
    exp = _oracle_self(oracle, ("boundary", S), rows, lengths, S)
    nu = exp[0].reshape(n, n)
    for i in range(S):
        for p in range(S):
            a = 2 * (i * S + p)
            assert nu[a, a + 1] == nu[a + 1, a] == (1 if i + p < S else 0), (i, p)
    _self_both_forms(sparse, rows, lengths, S, exp)


# ---- 2. mixed lengths ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mixed_rows(oracle):
    """8 x 12 family sketches of 1000 hashes, an empty row, rows shorter than S and a prefix of
    another row, spread over the set"""
    import fpmash.datagen as D
    seqs = D.family_dna(8, 12, 2000, sub_rate=(0.0, 0.08), seed=23)
    sk = oracle.sketch_batch(oracle.params(k=K, s=1000), seqs)
    assert all(len(x) == 1000 for x in sk)
    rows = list(sk)
    extra = [(5, sk[0][:10]), (17, np.zeros(0, np.uint64)), (40, sk[30][:700]),
             (41, sk[9][:300]), (66, sk[50][:999]), (90, sk[77][:500]), (3, sk[20][:1])]
    for at, x in extra:
        rows.insert(at, x)
    return rows, [2000 + 7 * j for j in range(len(rows))]


@pytest.mark.parametrize("S", [1000, 301, 2, 1])
def test_mixed_lengths(sparse, oracle, S):
    """Rows of S hashes, shorter rows (visited whole: their denom may differ from the default),
    an empty row and a prefix row; at S = 301 the 1000-long rows are longer than S, at S = 2
    and 1 the visited prefix is one hash."""
    rows, lengths = _mixed_rows(oracle)
    exp = _oracle_self(oracle, ("mixed", S), rows, lengths, S)
    assert (exp[0] > 0).any() and (exp[0] == 0).any()
    assert any(0 < len(x) < S for x in rows) or S == 1
    _self_both_forms(sparse, rows, lengths, S, exp)


# ---- 3. collisions across the cut ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _collision_rows():
    """Rows of 100-150 low values (some shared by many rows, the rest private) below a stretch
    of 300-340 values drawn from the same 400 base values offset by 0, 1 or 2: rows of different
    offsets share none of those but every one's bucket and fingerprint.  A few values inside
    the stretch are truly shared.  S = 400: the cut H = 200 falls inside the stretch."""
    rng = np.random.default_rng(303)
    top = np.uint64(1) << np.uint64(63)
    base = np.unique((rng.integers(0, 2 ** 61, size=400, dtype=np.uint64) << np.uint64(2)) | top)
    shared_lo = np.unique(rng.integers(1, 2 ** 62, size=60, dtype=np.uint64))
    shared_hi = np.unique(((rng.integers(0, 2 ** 61, size=12, dtype=np.uint64) << np.uint64(2))
                           | top) + np.uint64(3))
    rows = []
    for i in range(36):
        # every fourth row holds no shared low value, every eighth no shared value at all
        low = [rng.choice(shared_lo, size=0 if i % 4 == 3 else int(rng.integers(10, 50)),
                          replace=False),
               rng.integers(1, 2 ** 62, size=100, dtype=np.uint64)]
        pick = rng.choice(base, size=int(rng.integers(300, 341)), replace=False) + np.uint64(i % 3)
        hi = rng.choice(shared_hi, size=0 if i % 8 == 7 else int(rng.integers(0, 6)),
                        replace=False)
        rows.append(np.unique(np.concatenate(low + [pick, hi])))
    return rows, [5000 + 11 * j for j in range(len(rows))]


def test_collisions_across_the_cut(sparse, oracle):
    """Events between entries that share no value (same bucket and fingerprint) on both sides
    of the cut, mixed with truly shared values: the seen / both rule must take each pair once
    whichever kind of event shows it."""
    rows, lengths = _collision_rows()
    S = 400
    H = (S + 1) // 2
    top = np.uint64(1) << np.uint64(63)
    for x in rows:
        assert len(x) >= S
        stretch = np.flatnonzero(x >= top)
        assert stretch[0] < H - 20 and H + 20 < stretch[-1]
    exp = _oracle_self(oracle, ("collide", S), rows, lengths, S)
    n = len(rows)
    nu = exp[0].reshape(n, n)
    # rows of different offsets that share nothing at all, and pairs with shared values
    assert (nu == 0).any() and (nu[~np.eye(n, dtype=bool)] > 0).any()
    _self_both_forms(sparse, rows, lengths, S, exp)


# ---- 4. a resident set as its own query ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _resident_rows(oracle):
    import fpmash.datagen as D
    seqs = D.family_dna(20, 10, 2000, sub_rate=(0.0, 0.08), seed=29)
    sk = oracle.sketch_batch(oracle.params(k=K, s=1000), seqs)
    sk[7] = sk[7][:400]
    sk[150] = sk[150][:0]
    return sk, [2000] * len(sk)


def test_resident_set_as_itself(sparse, oracle):
    """fpm_refset_create_dev over device rows, then fpm_refset_dist_list_dev with the set's own
    pointers as the query block (the self job of a sharded all-vs-all): HALF at the set's
    sketch size, FULL at another (its flags were cut at the set's), both equal the oracle."""
    import fpmash
    ctx = sparse
    L = fpmash.lib()
    rows, lengths = _resident_rows(oracle)
    n, stride, S0 = len(rows), 1000, 1000
    host = np.zeros((n, stride), np.uint64)
    lens = np.zeros(n, np.uint32)
    for i, x in enumerate(rows):
        host[i, :len(x)] = x
        lens[i] = len(x)
    bufs = [fpmash.DeviceBuffer.from_array(ctx, a)
            for a in (host, lens, np.asarray(lengths, np.uint64))]
    outs = [fpmash.DeviceBuffer(ctx, n * n * 2) for _ in range(2)]
    lst = fpmash.CellList(ctx, n * n)
    h = C.c_void_p()
    try:
        d_rows, d_len, d_length = (b.ptr for b in bufs)
        fpmash._check(L.fpm_refset_create_dev(ctx.h, d_rows, d_len, d_length, stride, n, 8, S0,
                                              C.byref(h)))
        for S, form in ((S0, fpmash.PROBE_HALF), (500, fpmash.PROBE_FULL)):
            exp = _oracle_self(oracle, ("resident", S), rows, lengths, S)
            res = {}
            for on in (True, False):
                ctx.set_probe_half(on)
                for o in outs:
                    fpmash._check(L.fpm_memset(ctx.h, o.ptr, 0xEE, o.nbytes))
                fpmash._check(L.fpm_refset_dist_list_dev(
                    h, d_rows, d_len, d_length, stride, n, S, K, SPACE, -1.0, -1.0, outs[0].ptr,
                    outs[1].ptr, lst.ref, None))
                ctx.synchronize()
                assert ctx.last_dist_stats()["sparse"] == 2
                assert ctx.last_dist_probe() == (form if on else fpmash.PROBE_FULL)
                listed = lst.fetch()
                _no_repeats(listed, n)
                res[on] = fpmash.expand_compact(outs[0].to_array(np.uint16, n * n),
                                                outs[1].to_array(np.uint16, n * n), listed, n)
                _assert_grid(res[on], exp)
            _assert_same(res[True], res[False])
    finally:
        if h:
            L.fpm_refset_free(h)
        for b in bufs + outs:
            b.free()
        lst.free()


# ---- 5. the speculated probe ---------------------------------------------------------------------

@pytest.mark.parametrize("on", [True, False])
def test_speculated_probe_takes_the_same_form(sparse, oracle, on):
    """Two self calls of one shape: the second one's probe is enqueued behind the index build
    before the counters are read (spec_stats shows a hit) and takes the form the confirmed call
    would; the result equals the oracle."""
    import fpmash
    ctx = sparse
    rows, lengths = _mixed_rows(oracle)
    S = 1000
    exp = _oracle_self(oracle, ("mixed", S), rows, lengths, S)
    form = fpmash.PROBE_HALF if on else fpmash.PROBE_FULL
    ctx.set_probe_half(on)
    kw = dict(use64=True, k=K, ref_lengths=lengths, qry_lengths=lengths)
    first = ctx.dist(rows, rows, S, **kw)            # sets (or keeps) the shape's profile
    assert ctx.last_dist_probe() == form
    h0, m0 = ctx.spec_stats()
    got = ctx.dist(rows, rows, S, **kw)
    h1, m1 = ctx.spec_stats()
    assert (h1, m1) == (h0 + 1, m0), (h0, m0, h1, m1)
    assert ctx.last_dist_probe() == form
    assert ctx.last_dist_stats()["sparse"] == 2
    _assert_grid(first, exp)
    _assert_grid(got, exp)
    _assert_same(first, got)
