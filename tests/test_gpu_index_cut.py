"""GPU parity of the index cut (dist_index.hip: idx_kmax_kernel with vcut, the level-1 kernels'
drop): the index a compare builds for one sorted u64 set against itself leaves out every hash
above V*, the largest value any row's probed half holds.

Every case runs with the cut on and off and compares each result with oracle.dist_grid: numer
and denom exact, distance and p-value to rtol 1e-12; the compact lists of the two runs must be
equal as sets.  Context.last_index_cut must report what the case expects, and with a cut
exactly the entries whose value is <= V* (computed here from the rows).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_dist_dispatch import _Rows, _dev_dist

pytestmark = pytest.mark.gpu

RTOL = 1e-12
K = 21
SPACE = 4.0 ** K

_EXP = {}


def _oracle_self(oracle, key, lists, lengths, S, use64=True):
    """the oracle's grid of one set against itself (computed once per key, never modified)"""
    if key not in _EXP:
        res = oracle.dist_grid(list(lists), list(lengths), list(lists), list(lengths), S, K, SPACE,
                               use64=use64, threads=8)
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


def _as_set(listed):
    return set(zip(listed["qry"].tolist(), listed["ref"].tolist(), listed["distance"].tolist(),
                   listed["pvalue"].tolist(), listed["pass"].tolist()))


def _expected_index(rows, S):
    """(entries <= V*, all entries) of sorted rows: what a cut index holds"""
    H = (S + 1) // 2
    tops = [int(x[(H if len(x) >= S else len(x)) - 1]) for x in rows if len(x)]
    vs = max(tops)
    return sum(int(np.count_nonzero(np.asarray(x, np.uint64) <= np.uint64(vs))) for x in rows), \
        sum(len(x) for x in rows)


@pytest.fixture
def cut_ctx(ctx):
    """the switches back to their defaults afterwards"""
    import fpmash
    ctx.set_index_cut(True)
    ctx.set_probe_half(True)
    yield ctx
    ctx.set_index_cut(True)
    ctx.set_probe_half(True)
    ctx.set_dist_mode(fpmash.DIST_AUTO)


def _both(ctx, rows, lengths, S, exp, cut, sparse=2, use64=True):
    """the set against itself through ctx.dist and ctx.dist_list with the cut on and off: each
    equals the oracle, the lists are equal as sets; on: the hook reports `cut` (None: a cut
    index of exactly the entries <= V*; "all": a cut that drops nothing; False: no cut), off:
    never a cut -> the hook's report with the switch on"""
    import fpmash
    n = len(rows)
    kw = dict(use64=use64, k=K, ref_lengths=lengths, qry_lengths=lengths)
    lists, hook = {}, None
    for on in (True, False):
        ctx.set_index_cut(on)
        for api in ("dist", "list"):
            if api == "dist":
                got = ctx.dist(rows, rows, S, **kw)
            else:
                nu, de, listed = ctx.dist_list(rows, rows, S, expand=False, **kw)
                got = fpmash.expand_compact(nu, de, listed, n)
                lists[on] = _as_set(listed)
            st, h = ctx.last_dist_stats(), ctx.last_index_cut()
            assert st["sparse"] == sparse
            if sparse == 2:
                assert ctx.last_dist_probe() == fpmash.PROBE_HALF
            _assert_grid(got, exp)
            total = sum(len(x) for x in rows)
            if not on or cut is False:
                assert not h["cut"]
                if sparse == 2:
                    assert h["indexed"] == h["entries"] == total
            else:
                want, all_ = _expected_index(rows, S)
                assert h["cut"] and h["entries"] == all_ == total
                assert h["indexed"] == want
                assert (want == all_) if cut == "all" else (want < all_)
                hook = h
    assert lists[True] == lists[False]
    return hook


@functools.lru_cache(maxsize=None)
def _family_sketches(oracle, S, short=False):
    """3 families x 20 members x 600 bp sketched at S; short: one 150 bp row among them"""
    import fpmash.datagen as D
    seqs = D.family_dna(3, 20, 600, sub_rate=(0.0, 0.08), seed=41)
    if short:
        seqs[27] = seqs[27][:150]
    sk = oracle.sketch_batch(oracle.params(k=K, s=S), seqs)
    return sk, [len(s) for s in seqs]


@pytest.mark.parametrize("S", [200, 9])
def test_families(cut_ctx, oracle, S):
    """every row holds S hashes (even and odd S): a cut, fewer indexed entries than cells"""
    import fpmash
    cut_ctx.set_dist_mode(fpmash.DIST_SPARSE)
    rows, lengths = _family_sketches(oracle, S)
    assert all(len(x) == S for x in rows)
    exp = _oracle_self(oracle, ("fam", S), rows, lengths, S)
    assert (exp[0] > 0).any() and (exp[0] == 0).any()
    h = _both(cut_ctx, rows, lengths, S, exp, None)
    assert h["indexed"] < len(rows) * S
    # the full probe reads every entry: no cut without the half form
    cut_ctx.set_index_cut(True)
    cut_ctx.set_probe_half(False)
    got = cut_ctx.dist(rows, rows, S, use64=True, k=K, ref_lengths=lengths, qry_lengths=lengths)
    assert cut_ctx.last_dist_probe() == fpmash.PROBE_FULL
    assert cut_ctx.last_index_cut() == {"cut": False, "indexed": len(rows) * S,
                                        "entries": len(rows) * S}
    _assert_grid(got, exp)


def test_one_short_row(cut_ctx, oracle):
    """a 150 bp row holds every one of its 130 hashes, fewer than S: it is probed whole, V* is
    its last value, above every bottom-200 row's maximum: indexed == all"""
    import fpmash
    cut_ctx.set_dist_mode(fpmash.DIST_SPARSE)
    S = 200
    rows, lengths = _family_sketches(oracle, S, True)
    assert len(rows[27]) == 130 and all(len(x) == S for i, x in enumerate(rows) if i != 27)
    assert int(rows[27][-1]) > max(int(x[-1]) for i, x in enumerate(rows) if i != 27)
    exp = _oracle_self(oracle, ("fam-short", S), rows, lengths, S)
    h = _both(cut_ctx, rows, lengths, S, exp, "all")
    assert h["indexed"] == h["entries"]


@functools.lru_cache(maxsize=None)
def _mixed_sketches(oracle):
    """400 bp and 5,000 bp rows at S = 100, 240 rows in families of two.  The long rows' values
    crowd into the lowest ~7 % of the bucket scale, so the library's event count (bucket sizes)
    is several times the entries; the set is large enough for AUTO's rule (4 x events <= pairs
    x S, the pairs growing with the square of the rows) to keep the index all the same"""
    import fpmash.datagen as D
    a = D.family_dna(60, 2, 400, sub_rate=(0.0, 0.08), seed=43)
    b = D.family_dna(60, 2, 5000, sub_rate=(0.0, 0.08), seed=44)
    seqs = [x for pair in zip(a, b) for x in pair]
    return oracle.sketch_batch(oracle.params(k=K, s=100), seqs), [len(s) for s in seqs]


@pytest.mark.parametrize("mode", ["auto", "sparse"])
def test_mixed_lengths(cut_ctx, oracle, mode):
    """rows whose bottom-100 maxima differ by an order of magnitude: V* comes from the 400 bp
    rows, and most of their upper halves still lie below it"""
    import fpmash
    cut_ctx.set_dist_mode(fpmash.DIST_SPARSE if mode == "sparse" else fpmash.DIST_AUTO)
    S = 100
    rows, lengths = _mixed_sketches(oracle)
    assert len(rows) ** 2 >= 4096 and all(len(x) == S for x in rows)
    exp = _oracle_self(oracle, ("mixed", S), rows, lengths, S)
    _both(cut_ctx, rows, lengths, S, exp, None)


def _handmade(S=8):
    """V* = 2^62 at position H - 1 of row 0; row 1 holds it behind its visited prefix, followed
    by V* + 1, which row 2 holds too (behind its prefix: the one entry pair above the cut that
    shares a value).  Filler rows share a few low values."""
    H = (S + 1) // 2
    V = 1 << 62
    rng = np.random.default_rng(8)

    def low(n):
        return rng.integers(1, V - 1, size=n, dtype=np.uint64)

    def high(n):
        return rng.integers(V + 16, 2 ** 64 - 1, size=n, dtype=np.uint64)
    def u64(*v):
        return np.array(v, np.uint64)
    shared = low(3)
    rows = [np.concatenate([low(H - 1), u64(V), high(S - H)]),
            np.concatenate([low(H), u64(V, V + 1), high(S - H - 2)]),
            np.concatenate([low(H), u64(V + 1), high(S - H - 1)])]
    for i in range(13):
        rows.append(np.concatenate([shared[:1 + i % 3], low(H - 1 - i % 3), high(S - H)]))
    rows = [np.sort(np.asarray(x, np.uint64)) for x in rows]
    assert all(len(np.unique(x)) == S for x in rows)
    assert int(rows[0][H - 1]) == V and int(rows[1][H]) == V and int(rows[1][H + 1]) == V + 1
    assert int(rows[2][H]) == V + 1 and all(int(x[H - 1]) < V for x in rows[1:])
    return rows, [1500 + 9 * i for i in range(len(rows))]


@pytest.mark.parametrize("api", ["dist", "dist16", "list"])
def test_shared_value_at_the_cut(cut_ctx, oracle, api):
    """rows uploaded directly: the entry equal to V* is kept (the pair (0, 1) counts it: 3 + 4
    < S), the shared V* + 1 is dropped (5 + 4 >= S: the walk never counts it)"""
    import fpmash
    ctx = cut_ctx
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    S = 8
    rows, lengths = _handmade(S)
    n = len(rows)
    exp = _oracle_self(oracle, ("hand", S), rows, lengths, S)
    nu = exp[0].reshape(n, n)
    assert nu[0, 1] == nu[1, 0] == 1 and nu[1, 2] == nu[2, 1] == 0
    want, all_ = _expected_index(rows, S)
    assert want == sum(int(np.count_nonzero(x <= np.uint64(1 << 62))) for x in rows) < all_
    R = _Rows(ctx, rows, lengths, np.uint64)
    try:
        res = {}
        for on in (True, False):
            ctx.set_index_cut(on)
            res[on] = _dev_dist(ctx, R, R, S, K, SPACE, api=api)
            h = ctx.last_index_cut()
            assert ctx.last_dist_stats()["sparse"] == 2
            assert h == {"cut": on, "indexed": want if on else all_, "entries": all_}
            _assert_grid(res[on], exp)
        for key in ("numer", "denom", "distance", "pvalue", "pass"):
            assert np.array_equal(res[True][key], res[False][key]), key
    finally:
        R.free()


def test_speculated_probe_then_larger_cut(cut_ctx, oracle):
    """two identical calls (the second one's probe is enqueued behind the build of its cut
    index, before the host knows V* or the counters), then a set of the same shape whose V* is
    far larger: every index is cut at its own call's V*"""
    import fpmash
    ctx = cut_ctx
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    S = 200
    rows, lengths = _family_sketches(oracle, S)
    exp = _oracle_self(oracle, ("fam", S), rows, lengths, S)
    kw = dict(use64=True, k=K, ref_lengths=lengths, qry_lengths=lengths)
    want, all_ = _expected_index(rows, S)
    first = ctx.dist(rows, rows, S, **kw)
    h0, m0 = ctx.spec_stats()
    got = ctx.dist(rows, rows, S, **kw)
    assert ctx.spec_stats() == (h0 + 1, m0)
    assert ctx.last_index_cut() == {"cut": True, "indexed": want, "entries": all_}
    assert ctx.last_dist_probe() == fpmash.PROBE_HALF
    _assert_grid(first, exp)
    _assert_grid(got, exp)
    # the same shape, every value doubled or so: stretched over the whole u64 range
    top = max(int(x[-1]) for x in rows)
    f = (2 ** 64 - 1) // top
    assert f >= 2
    big = [x * np.uint64(f) for x in rows]
    exp2 = _oracle_self(oracle, ("fam-stretched", S), big, lengths, S)
    assert np.array_equal(exp2[0], exp[0]) and np.array_equal(exp2[1], exp[1])
    want2, all2 = _expected_index(big, S)
    assert (want2, all2) == (want, all_)
    got2 = ctx.dist(big, big, S, **kw)
    assert ctx.last_index_cut() == {"cut": True, "indexed": want2, "entries": all2}
    _assert_grid(got2, exp2)


def test_unsorted_row_is_rebuilt_over_records(cut_ctx, oracle):
    """one row out of order: the raw (cut) index only reports it, the records are indexed
    whole and the candidates walked literally; the hook reports no cut"""
    import fpmash
    cut_ctx.set_dist_mode(fpmash.DIST_SPARSE)
    S = 200
    rows, lengths = _family_sketches(oracle, S)
    rows = [x.copy() for x in rows]
    rows[11][[3, 150]] = rows[11][[150, 3]]
    exp = _oracle_self(oracle, ("fam-unsorted", S), rows, lengths, S)
    assert (exp[0] > 0).any()
    _both(cut_ctx, rows, lengths, S, exp, False, sparse=1)
    assert cut_ctx.last_dist_kernel() == fpmash.DK_CAND_WALK


def test_u32_set_is_not_cut(cut_ctx, oracle):
    import fpmash
    cut_ctx.set_dist_mode(fpmash.DIST_SPARSE)
    import fpmash.datagen as D
    S, k = 200, 14
    seqs = D.family_dna(3, 20, 600, sub_rate=(0.0, 0.08), seed=47)
    rows = oracle.sketch_batch(oracle.params(k=k, s=S), seqs)
    rows = [np.asarray(x).astype(np.uint32) for x in rows]
    lengths = [len(s) for s in seqs]
    key = ("fam-u32", S)
    if key not in _EXP:
        _EXP[key] = oracle.dist_grid(rows, lengths, rows, lengths, S, k, 4.0 ** k, use64=False,
                                     threads=8)
    exp = _EXP[key]
    kw = dict(use64=False, k=k, ref_lengths=lengths, qry_lengths=lengths)
    for on in (True, False):
        cut_ctx.set_index_cut(on)
        got = cut_ctx.dist(rows, rows, S, **kw)
        h = cut_ctx.last_index_cut()
        assert cut_ctx.last_dist_stats()["sparse"] >= 1 and not h["cut"]
        assert h["indexed"] == h["entries"]
        _assert_grid(got, exp)


def test_resident_set_self_job_is_not_cut(cut_ctx, oracle):
    """a resident set as its own query block takes the half probe over the set's whole index"""
    import fpmash
    ctx = cut_ctx
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    L = fpmash.lib()
    S = 200
    rows, lengths = _family_sketches(oracle, S)
    exp = _oracle_self(oracle, ("fam", S), rows, lengths, S)
    n = len(rows)
    R = _Rows(ctx, rows, lengths, np.uint64)
    outs = [fpmash.DeviceBuffer(ctx, n * n * 2) for _ in range(2)]
    lst = fpmash.CellList(ctx, n * n)
    h = C.c_void_p()
    try:
        fpmash._check(L.fpm_refset_create_dev(ctx.h, R.rows, R.len.ptr, R.length.ptr, R.stride, n,
                                              8, S, C.byref(h)))
        fpmash._check(L.fpm_refset_dist_list_dev(h, R.rows, R.len.ptr, R.length.ptr, R.stride, n,
                                                 S, K, SPACE, -1.0, -1.0, outs[0].ptr,
                                                 outs[1].ptr, lst.ref, None))
        ctx.synchronize()
        assert ctx.last_dist_probe() == fpmash.PROBE_HALF
        assert ctx.last_index_cut() == {"cut": False, "indexed": n * S, "entries": n * S}
        got = fpmash.expand_compact(outs[0].to_array(np.uint16, n * n),
                                    outs[1].to_array(np.uint16, n * n), lst.fetch(), n)
        _assert_grid(got, exp)
    finally:
        if h:
            L.fpm_refset_free(h)
        for b in outs:
            b.free()
        lst.free()
        R.free()


def test_forced_sparse_on_a_dense_set(cut_ctx, oracle):
    """near-identical rows: AUTO's rule (on the events of the whole index, which the cut index's
    count is scaled to) takes the dense walk; DIST_SPARSE forced runs the cut index"""
    import fpmash
    import fpmash.datagen as D
    ctx = cut_ctx
    S = 100
    seqs = D.family_dna(1, 70, 600, sub_rate=(0.0, 0.004), seed=53)
    rows = oracle.sketch_batch(oracle.params(k=K, s=S), seqs)
    lengths = [len(s) for s in seqs]
    exp = _oracle_self(oracle, ("dense-fam", S), rows, lengths, S)
    kw = dict(use64=True, k=K, ref_lengths=lengths, qry_lengths=lengths)
    ev = {}
    for on in (True, False):
        ctx.set_index_cut(on)
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        got = ctx.dist(rows, rows, S, **kw)
        st = ctx.last_dist_stats()
        assert st["sparse"] == 0, "AUTO was expected to take the dense walk"
        ev[on] = st["events"]
        _assert_grid(got, exp)
    # the scaled count stands for the whole index's: same side of the rule, same magnitude
    assert 4 * min(ev.values()) > len(rows) ** 2 * S
    assert 0.5 * ev[False] <= ev[True] <= 2.0 * ev[False]
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    h = _both(ctx, rows, lengths, S, exp, None)
    assert h["cut"]
