"""GPU parity of dist at its kernel dispatch edges: sorted u32 sketches, u64 rows wider than the
rank kernel's cap, the thresholds between the compare kernels, the image kernel's tile map,
unequal strides / padding / alignment through the C ABI, and the zero-extended k <= 16 rows a
sketch job leaves on the device.

Every grid is compared with oracle.dist_grid (the CPU restatement of the literal walk): numer
and denom bit-exact, distance and p-value to rtol 1e-12.  Every test also asserts the compare
kernel the call launched (Context.last_dist_kernel) and, where the index path is possible,
last_dist_stats()["sparse"], so a moved threshold fails here instead of moving the coverage.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _mode(name):
    import fpmash
    return {"auto": fpmash.DIST_AUTO, "dense": fpmash.DIST_DENSE,
            "sparse": fpmash.DIST_SPARSE}[name]


# ---- the oracle's grids (computed once per key, shared, never modified) ----------------------

_EXP = {}


def _oracle_grid(oracle, key, refs, rl, qrys, ql, S, k, space, use64):
    if key not in _EXP:
        res = oracle.dist_grid(list(refs), list(rl), list(qrys), list(ql), S, k, space,
                               use64=use64, threads=8)
        for a in res:
            a.setflags(write=False)
        _EXP[key] = res
    return _EXP[key]


def _check_data(exp, lists, S, sorted_=True):
    """what the grid must contain to mean anything: cells with and without shared hashes and
    (sorted sets) lists shorter than S"""
    nu = exp[0]
    assert (nu > 0).any() and (nu == 0).any()
    if sorted_:
        assert any(0 < len(x) < S for x in lists)


def _assert_grid(got, exp, max_dist=-1.0, max_pvalue=-1.0):
    nu, de, di, pv = exp
    assert np.array_equal(got["numer"], nu)
    assert np.array_equal(got["denom"], de)
    np.testing.assert_allclose(got["distance"], di, rtol=RTOL, atol=0)
    # compareSketches returns before pValue for a pair past -d (CommandDistance.cpp:416-423):
    # the p-value is compared where the distance passes
    near = np.ones(len(di), bool) if max_dist < 0 else di <= max_dist
    np.testing.assert_allclose(got["pvalue"][near], pv[near], rtol=RTOL, atol=0)
    ok = near & (np.ones(len(pv), bool) if max_pvalue < 0 else pv <= max_pvalue)
    assert np.array_equal(np.asarray(got["pass"]).astype(bool), ok)


def _assert_kernel(ctx, kernel, sparse=None):
    import fpmash
    got = ctx.last_dist_kernel()
    assert got == kernel, f"{fpmash.DIST_KERNELS[got]} ran, {fpmash.DIST_KERNELS[kernel]} expected"
    if sparse is not None:
        assert ctx.last_dist_stats()["sparse"] == sparse


def _dense_kernel(use64, S, ref_stride, qry_stride):
    """the dense walk's kernel as compare_impl documents it: W = min(S, max stride); u32 with
    64 <= W <= 1023 and S <= W on the rank images; else in LDS while 32 lists of W (+ a
    window of 4, rounded to 4) entries fit in 156 KB; else from global memory"""
    import fpmash
    W = min(S, max(ref_stride, qry_stride))
    if not use64 and 64 <= W <= 1023 and S <= W:
        return fpmash.DK_GRID_IMG
    if W > 0 and 32 * ((W + 7) & ~3) * (8 if use64 else 4) <= 156 * 1024:
        return fpmash.DK_GRID_LDS
    return fpmash.DK_GRID_GLOBAL


# ---- a helper that uploads rows itself and calls the *_dev entry points ----------------------

class _Rows:
    """n lists as rows of `stride` entries, starting `off` elements into a DeviceBuffer that
    holds `tail` more elements after the last row; what is not a list entry (row padding, the
    offset, the tail) holds `junk` values when given, else zeros."""

    def __init__(self, ctx, lists, lengths, dtype, stride=None, off=0, tail=0, junk=None):
        import fpmash
        self.n, self.dtype = len(lists), np.dtype(dtype)
        self.stride = int(stride if stride is not None else max([len(x) for x in lists] + [1]))
        assert all(len(x) <= self.stride for x in lists)
        total = off + max(self.n, 1) * self.stride + tail
        if junk is None:
            host = np.zeros(total, self.dtype)
        else:
            host = np.random.default_rng(junk).integers(
                0, np.iinfo(self.dtype).max, size=total, dtype=self.dtype, endpoint=True)
        lens = np.zeros(max(self.n, 1), np.uint32)
        for i, x in enumerate(lists):
            at = off + i * self.stride
            host[at:at + len(x)] = x
            lens[i] = len(x)
        self.buf = fpmash.DeviceBuffer.from_array(ctx, host)
        self.rows = self.buf.ptr + off * self.dtype.itemsize
        self.len = fpmash.DeviceBuffer.from_array(ctx, lens)
        L = np.zeros(max(self.n, 1), np.uint64)
        L[:self.n] = lengths
        self.length = fpmash.DeviceBuffer.from_array(ctx, L)

    def free(self):
        for b in (self.buf, self.len, self.length):
            b.free()


_FULL = (np.float64, np.float64, np.uint8)


def _outputs(ctx, n, count_bytes, full=True):
    """device outputs of one grid, set to 0xEE first (a cell the call does not write shows)"""
    import fpmash
    sizes = (count_bytes, count_bytes) + ((8, 8, 1) if full else ())
    bufs = [fpmash.DeviceBuffer(ctx, max(n, 1) * b) for b in sizes]
    for b in bufs:
        fpmash._check(fpmash.lib().fpm_memset(ctx.h, b.ptr, 0xEE, b.nbytes))
    return bufs


def _fetch_full(bufs, n, count_bytes):
    ct = np.uint16 if count_bytes == 2 else np.uint32
    nu, de, di, pv, pa = (b.to_array(t, max(n, 1))[:n] for b, t in zip(bufs, (ct, ct) + _FULL))
    return {"numer": nu, "denom": de, "distance": di, "pvalue": pv, "pass": pa.astype(bool)}


def _dev_dist(ctx, R, Q, S, k, space, api="dist", max_dist=-1.0, max_pvalue=-1.0):
    """fpm_dist_dev ("dist"), fpm_dist_dev16 ("dist16") or fpm_dist_list_dev ("list") on two
    uploaded row sets (Q is R: one set against itself, same buffers) -> the five per-cell
    arrays"""
    import fpmash
    L = fpmash.lib()
    hb = R.dtype.itemsize
    n = R.n * Q.n
    args = (ctx.h, R.rows, R.len.ptr, R.length.ptr, R.stride, R.n, Q.rows, Q.len.ptr,
            Q.length.ptr, Q.stride, Q.n, hb, S, k, space, max_dist, max_pvalue)
    bufs, lst = [], None
    try:
        if api == "list":
            bufs = _outputs(ctx, n, 2, full=False)
            lst = fpmash.CellList(ctx, max(n, 1))
            fpmash._check(L.fpm_dist_list_dev(*args, bufs[0].ptr, bufs[1].ptr, lst.ref, None))
            ctx.synchronize()
            nu, de = (b.to_array(np.uint16, max(n, 1))[:n] for b in bufs)
            return fpmash.expand_compact(nu, de, lst.fetch(), R.n, max_dist, max_pvalue)
        cb = 2 if api == "dist16" else 4
        bufs = _outputs(ctx, n, cb)
        fn = L.fpm_dist_dev16 if api == "dist16" else L.fpm_dist_dev
        fpmash._check(fn(*args, *[b.ptr for b in bufs], None))
        ctx.synchronize()
        return _fetch_full(bufs, n, cb)
    finally:
        for b in bufs:
            b.free()
        if lst is not None:
            lst.free()


def _dev_mirror(ctx, R, Q, S, k, space, compact, max_dist=-1.0, max_pvalue=-1.0):
    """fpm_refset_create_dev over R, then fpm_refset_dist_mirror_dev (or _list_dev, compact)
    with the query rows Q -> (the grid, its transposed grid), five arrays each"""
    import fpmash
    L = fpmash.lib()
    hb = R.dtype.itemsize
    n = R.n * Q.n
    cb = 2 if compact else 4
    prim = _outputs(ctx, n, cb, full=not compact)
    mirr = _outputs(ctx, n, cb, full=not compact)
    lsts = [fpmash.CellList(ctx, max(n, 1)) for _ in range(2)] if compact else []
    h = C.c_void_p()
    try:
        fpmash._check(L.fpm_refset_create_dev(ctx.h, R.rows, R.len.ptr, R.length.ptr, R.stride,
                                              R.n, hb, S, C.byref(h)))
        if compact:
            fpmash._check(L.fpm_refset_dist_mirror_list_dev(
                h, Q.rows, Q.len.ptr, Q.length.ptr, Q.stride, Q.n, S, k, space, max_dist,
                max_pvalue, prim[0].ptr, prim[1].ptr, lsts[0].ref, mirr[0].ptr, mirr[1].ptr,
                lsts[1].ref, None))
            ctx.synchronize()
            return tuple(
                fpmash.expand_compact(bb[0].to_array(np.uint16, max(n, 1))[:n],
                                      bb[1].to_array(np.uint16, max(n, 1))[:n], ls.fetch(), nr,
                                      max_dist, max_pvalue)
                for bb, ls, nr in ((prim, lsts[0], R.n), (mirr, lsts[1], Q.n)))
        fpmash._check(L.fpm_refset_dist_mirror_dev(
            h, Q.rows, Q.len.ptr, Q.length.ptr, Q.stride, Q.n, S, 4, k, space, max_dist,
            max_pvalue, *[b.ptr for b in prim], *[b.ptr for b in mirr], None))
        ctx.synchronize()
        return _fetch_full(prim, n, 4), _fetch_full(mirr, n, 4)
    finally:
        if h:
            L.fpm_refset_free(h)
        for b in prim + mirr:
            b.free()
        for ls in lsts:
            ls.free()


# ---- list sets -----------------------------------------------------------------------------

def _family_lists(rng, dtype, n_fam, members, max_len, lens, p_new=0.15, interleave=False):
    """sorted distinct lists in families: a member keeps each of its family's max_len values
    with probability 1 - p_new and draws the rest anew; the prefix of lens(i) entries (a
    bottom-s sketch of fewer hashes).  Values over the whole range of dtype.  Family by
    family, or (interleave) the families' first members, then their second ones, ..."""
    top = np.iinfo(dtype).max
    out = []
    for f in range(n_fam):
        base = np.unique(rng.integers(1, top, size=max_len, dtype=dtype))
        for m in range(members):
            keep = base[rng.random(len(base)) >= p_new]
            new = rng.integers(1, top, size=max_len - len(keep) + 8, dtype=dtype)
            x = np.unique(np.concatenate([keep, new]))
            out.append(x[:min(len(x), lens(len(out)))].astype(dtype))
    if interleave:
        out = [out[f * members + m] for m in range(members) for f in range(n_fam)]
    return out


def _fp_lists(rng, n, lo, hi, vocab, alien=2):
    """-fp style u32 lists: file-order draws (with repeats) from a vocabulary that holds 0 and
    0xFFFFFFFF; the last `alien` lists draw from a vocabulary of their own (no shared value
    with the others)"""
    base = rng.integers(0, 2 ** 32, size=vocab, dtype=np.uint64).astype(np.uint32)
    base[0], base[1] = 0, 0xFFFFFFFF
    other = np.setdiff1d(rng.integers(0, 2 ** 32, size=vocab, dtype=np.uint64).astype(np.uint32),
                         base)
    out = []
    for i in range(n):
        src = other if i >= n - alien else base
        out.append(src[rng.integers(0, len(src), size=int(rng.integers(lo, hi + 1)))])
    return out


def _lengths(lists):
    return [7 * len(x) + 1000 for x in lists]


# ---- 1. sorted u32 sketches (k <= 16) --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _u32_sketches(oracle, k, s):
    """oracle sketches at k <= 16 (u32 hashes, ascending) of 8 x 8 family sequences, with an
    empty list, a 10-entry prefix, a list of s - 1 entries and lists holding 0 and 0xFFFFFFFF
    at either end of the set"""
    import fpmash.datagen as D
    seqs = D.family_dna(8, 8, 2000, sub_rate=(0.0, 0.08), seed=31 + k)
    P = oracle.params(k=k, s=s)
    assert not P.use64
    sk = [x.astype(np.uint32) for x in oracle.sketch_batch(P, seqs)]
    assert all(len(x) == s and np.all(x[1:] > x[:-1]) for x in sk)
    assert all(0 < x[0] and x[-1] < 0xFFFFFFFF for x in sk)
    u = np.uint32
    ends = lambda x: np.concatenate([[u(0)], x, [u(0xFFFFFFFF)]]).astype(u)
    head = [sk[0][:0], sk[0][:10], sk[3][:s - 1], ends(sk[1][:s - 2]), ends(sk[9][:50])]
    tail = [ends(sk[20][:40]), ends(sk[33][1:s - 1]), sk[25][:s - 1], sk[40][:10], sk[5][:0]]
    lists = head + sk + tail
    lengths = [2000] * len(lists)
    for i in (0, len(lists) - 1):
        lengths[i] = 100
    return lists, lengths


def _u32_case(oracle, k, s, which):
    lists, lengths = _u32_sketches(oracle, k, s)
    if which == "self":
        qrys, ql = lists, lengths
    elif which == "copy":
        qrys, ql = [x.copy() for x in lists], list(lengths)
    else:
        qrys, ql = lists[-25:], lengths[-25:]
    exp = _oracle_grid(oracle, ("u32", k, s, which != "short"), lists, lengths, qrys, ql, s, k,
                       4.0 ** k, False)
    _check_data(exp, lists, s)
    return lists, lengths, qrys, ql, exp


def _events(refs, qrys):
    """posting events: for every query hash, the reference lists that hold it"""
    val, cnt = np.unique(np.concatenate(refs), return_counts=True)
    q = np.concatenate(qrys)
    at = np.searchsorted(val, q)
    at[at == len(val)] = 0
    return int(cnt[at][val[at] == q].sum())


@pytest.mark.parametrize("which", ["self", "copy", "short"])
@pytest.mark.parametrize("mode", ["dense", "sparse", "auto"])
@pytest.mark.parametrize("k,s", [(16, 1000), (12, 300)])
def test_sorted_u32_sketches(ctx, oracle, k, s, mode, which):
    """Sorted u32 rows (every sketch made at k <= 16): the index path learns their order from
    the records, builds the raw index and walks the candidates (walk_cand_kernel<u32>, with
    its self-pair shortcut for one set against itself); the dense path takes the image
    kernel.  One set against itself (same lists), against a copy and against a shorter query
    set, through dist, dist16 and dist_list, with and without the -d / -v filters."""
    import fpmash
    refs, rl, qrys, ql, exp = _u32_case(oracle, k, s, which)
    n_pairs = len(refs) * len(qrys)
    # AUTO tries the index from 4096 pairs on (the short query set stays below) and keeps it
    # while 4 x events <= pairs x S.  The events are the library's own count (bucket sizes, at
    # least the exact posting events: the lists' 0xFFFFFFFF stretches the bucket scale, so the
    # bottom-300 rows at k = 12 crowd into a few buckets and AUTO walks them densely); the
    # rule is applied to that count, and the k = 16 set must take the index.
    assert (n_pairs < 4096) == (which == "short")
    kw = dict(use64=False, k=k, kmer_space=4.0 ** k, ref_lengths=rl, qry_lengths=ql)
    ctx.set_dist_mode(_mode(mode))
    try:
        for api in (ctx.dist, ctx.dist16, ctx.dist_list):
            for flt in ({}, dict(max_dist=0.1, max_pvalue=1e-8)):
                got = api(refs, qrys, s, **kw, **flt)
                index = mode == "sparse"
                if mode == "auto" and which != "short":
                    ev = ctx.last_dist_stats()["events"]
                    assert ev >= _events(refs, qrys)
                    index = 4 * ev <= n_pairs * s
                    assert index or k == 12
                _assert_kernel(ctx, fpmash.DK_CAND_WALK if index else fpmash.DK_GRID_IMG,
                               1 if index else 0)
                _assert_grid(got, exp, **flt)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)


@pytest.mark.parametrize("mode", ["dense", "sparse", "auto"])
@pytest.mark.parametrize("k,s", [(16, 1000), (12, 300)])
def test_sorted_u32_refset_and_mirror(ctx, oracle, k, s, mode):
    """The same rows through a resident set: host query blocks of 13, and both mirror entry
    points.  A transposed grid of u32 rows cannot be scattered (no rank kernel), so it comes
    from the swapped call, whose kernel the hook then reports; both orientations equal the
    oracle's."""
    import fpmash
    lists, lengths = _u32_sketches(oracle, k, s)
    refs, rl, qrys, ql = lists[:40], lengths[:40], lists[40:], lengths[40:]
    space = 4.0 ** k
    exp = _oracle_grid(oracle, ("u32rs", k, s), refs, rl, qrys, ql, s, k, space, False)
    exp_t = _oracle_grid(oracle, ("u32rs-t", k, s), qrys, ql, refs, rl, s, k, space, False)
    _check_data(exp, lists, s)
    assert any(0 in x and 0xFFFFFFFF in x for x in refs if len(x))
    assert any(0 in x and 0xFFFFFFFF in x for x in qrys if len(x))
    # every call here has fewer than 4096 pairs: AUTO walks densely
    assert len(refs) * len(qrys) < 4096
    index = mode == "sparse"
    kernel = fpmash.DK_CAND_WALK if index else fpmash.DK_GRID_IMG
    w = max(len(x) for x in lists)
    ctx.set_dist_mode(_mode(mode))
    R = Q = None
    try:
        rs = ctx.refset(refs, s, use64=False, ref_lengths=rl, width=w)
        try:
            got = []
            for i in range(0, len(qrys), 13):
                got.append(rs.dist(qrys[i:i + 13], k=k, kmer_space=space,
                                   qry_lengths=ql[i:i + 13], max_dist=-1.0, max_pvalue=0.5))
                _assert_kernel(ctx, kernel, 1 if index else 0)
        finally:
            rs.free()
        _assert_grid({key: np.concatenate([g[key] for g in got]) for key in got[0]}, exp,
                     max_pvalue=0.5)
        R = _Rows(ctx, refs, rl, np.uint32, stride=w)
        Q = _Rows(ctx, qrys, ql, np.uint32, stride=w)
        for compact in (False, True):
            p, m = _dev_mirror(ctx, R, Q, s, k, space, compact, max_dist=0.9, max_pvalue=0.5)
            _assert_kernel(ctx, kernel, 1 if index else 0)
            _assert_grid(p, exp, max_dist=0.9, max_pvalue=0.5)
            _assert_grid(m, exp_t, max_dist=0.9, max_pvalue=0.5)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        for x in (R, Q):
            if x is not None:
                x.free()


# ---- 2. u64 rows wider than the rank kernel's 2048 --------------------------------------------

@functools.lru_cache(maxsize=None)
def _wide_u64():
    rng = np.random.default_rng(41)
    cut = {0: 0, 3: 2048, 7: 2049, 11: 9999, 13: 500, 17: 5000, 22: 2050, 30: 1}

    def lens(i):
        return cut.get(i, 10000 if i % 3 else int(rng.integers(6000, 10001)))
    lists = _family_lists(rng, np.uint64, 5, 8, 10000, lens)
    assert max(len(x) for x in lists) == 10000 and min(len(x) for x in lists) == 0
    return lists, _lengths(lists)


@pytest.mark.parametrize("which", ["self", "other"])
@pytest.mark.parametrize("mode", ["sparse", "dense"])
@pytest.mark.parametrize("S", [10000, 2049])
def test_wide_u64_rows(ctx, oracle, S, mode, which):
    """u64 sketches of 10,000 hashes (stride past the rank kernel's 2048): the index path
    walks the candidates (walk_cand_kernel<u64>, the compact list then built from the cells
    written in place, the transposed grid by the swapped call), the dense path walks from
    global memory.  S = 10,000 and S = 2,049 (the walk stops inside the rows)."""
    import fpmash
    lists, lengths = _wide_u64()
    if which == "self":
        refs, rl, qrys, ql = lists, lengths, lists, lengths
    else:
        # three of every five on the reference side: each family is on both sides
        ri = [i for i in range(len(lists)) if i % 5 < 3]
        qi = [i for i in range(len(lists)) if i % 5 >= 3]
        refs, rl = [lists[i] for i in ri], [lengths[i] for i in ri]
        qrys, ql = [lists[i] for i in qi], [lengths[i] for i in qi]
    space = 4.0 ** 21
    exp = _oracle_grid(oracle, ("wide", S, which), refs, rl, qrys, ql, S, 21, space, True)
    _check_data(exp, refs + qrys, S)
    index = mode == "sparse"
    kernel = fpmash.DK_CAND_WALK if index else fpmash.DK_GRID_GLOBAL
    assert _dense_kernel(True, S, 10000, 10000) == fpmash.DK_GRID_GLOBAL
    kw = dict(use64=True, k=21, ref_lengths=rl, qry_lengths=ql)
    ctx.set_dist_mode(_mode(mode))
    R = Q = None
    try:
        for api, flt in ((ctx.dist, {}), (ctx.dist_list, {}),
                         (ctx.dist_list, dict(max_dist=0.2, max_pvalue=1e-3))):
            got = api(refs, qrys, S, **kw, **flt)
            _assert_kernel(ctx, kernel, 1 if index else 0)
            _assert_grid(got, exp, **flt)
        if which == "other":
            exp_t = _oracle_grid(oracle, ("wide-t", S), qrys, ql, refs, rl, S, 21, space, True)
            R = _Rows(ctx, refs, rl, np.uint64, stride=10000)
            Q = _Rows(ctx, qrys, ql, np.uint64, stride=10000)
            for compact in (False, True):
                p, m = _dev_mirror(ctx, R, Q, S, 21, space, compact)
                _assert_kernel(ctx, kernel, 1 if index else 0)
                _assert_grid(p, exp)
                _assert_grid(m, exp_t)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        for x in (R, Q):
            if x is not None:
                x.free()


# ---- 3. the thresholds between the kernels ----------------------------------------------------

_N_REF, _N_QRY = 40, 24


@functools.lru_cache(maxsize=None)
def _straddle_set(kind):
    """40 + 24 lists, most of them longer than the largest S of their straddles (so the
    S-th step decides the counts), a few short or empty.  kind: "u64" (sorted, up to 2049
    entries), "u32" (sorted, up to 1400) or "fp" (unsorted u32 with repeats, up to 1400)."""
    rng = np.random.default_rng({"u64": 51, "u32": 52, "fp": 53}[kind])
    n = _N_REF + _N_QRY
    if kind == "fp":
        lists = _fp_lists(rng, n, 1300, 1400, 400)
        for i, m in ((2, 0), (5, 63), (9, 64), (30, 700), (45, 0), (50, 1023), (55, 1244),
                     (20, 40), (33, 10)):
            lists[i] = lists[i][:m]
        return lists
    top = 2049 if kind == "u64" else 1400
    cut = {2: 0, 5: 63, 9: 64, 30: 700, 45: 0, 50: 1023, 55: 1244, 12: 621, 47: 620, 20: 40,
           33: 10}
    lists = _family_lists(rng, np.uint64 if kind == "u64" else np.uint32, 8, 8, top,
                          lambda i: cut.get(i, top if i % 2 else top - int(rng.integers(0, 60))),
                          interleave=True)
    assert max(len(x) for x in lists) == top
    return lists


def _straddle_rows(ctx, kind, cap=None):
    """(refs, qrys) of the set as uploaded rows, the lists cut to `cap` entries"""
    lists = _straddle_set(kind)
    if cap is not None:
        lists = [x[:cap] for x in lists]
    refs, qrys = lists[:_N_REF], lists[_N_REF:]
    dt = np.uint64 if kind == "u64" else np.uint32
    stride = cap if cap is not None else max(len(x) for x in lists)
    return (refs, qrys, _Rows(ctx, refs, _lengths(refs), dt, stride=stride),
            _Rows(ctx, qrys, _lengths(qrys), dt, stride=stride))


_DENSE_STRADDLES = [("u64", 620, "lds"), ("u64", 621, "global")] + [
    (kind, S, kern) for kind in ("u32", "fp")
    for S, kern in ((63, "lds"), (64, "img"), (1023, "img"), (1024, "lds"), (1244, "lds"),
                    (1245, "global"))]


@pytest.mark.parametrize("kind,S,kern", _DENSE_STRADDLES)
def test_dense_kernel_thresholds(ctx, oracle, kind, S, kern):
    """The dense walk on either side of each kernel threshold, W = S (strides >= S): u64 in
    LDS up to W = 620 and from global memory from 621; u32 (sorted, and unsorted -fp lists)
    in LDS below 64, on the rank images for 64..1023, in LDS for 1024..1244, from global
    memory from 1245."""
    import fpmash
    kernel = {"lds": fpmash.DK_GRID_LDS, "img": fpmash.DK_GRID_IMG,
              "global": fpmash.DK_GRID_GLOBAL}[kern]
    use64 = kind == "u64"
    k, space = (21, 4.0 ** 21) if kind != "fp" else (1, 10.0)
    refs, qrys, R, Q = _straddle_rows(ctx, kind)
    ctx.set_dist_mode(fpmash.DIST_DENSE)
    try:
        assert R.stride >= S and _dense_kernel(use64, S, R.stride, Q.stride) == kernel
        exp = _oracle_grid(oracle, ("straddle", kind, S), refs, _lengths(refs), qrys,
                           _lengths(qrys), S, k, space, use64)
        _check_data(exp, refs + qrys, S, sorted_=kind != "fp")
        # longer lists than S on both sides: the S-th step, not the lists' ends, stops the walk
        assert sum(len(x) > S for x in refs) > 20 and sum(len(x) > S for x in qrys) > 12
        for api in ("dist", "dist16", "list"):
            got = _dev_dist(ctx, R, Q, S, k, space, api)
            _assert_kernel(ctx, kernel, 0)
            _assert_grid(got, exp)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        R.free()
        Q.free()


@pytest.mark.parametrize("sorted_", [True, False])
def test_dense_u32_sketch_size_above_stride(ctx, oracle, sorted_):
    """u32 rows of stride 900 at S = 1000: W = 900 is inside the image kernel's range but
    S > W (its padded walk would leave the rows), so the LDS walk runs."""
    import fpmash
    kind = "u32" if sorted_ else "fp"
    k, space = (21, 4.0 ** 21) if sorted_ else (1, 10.0)
    refs, qrys, R, Q = _straddle_rows(ctx, kind, cap=900)
    ctx.set_dist_mode(fpmash.DIST_DENSE)
    try:
        assert _dense_kernel(False, 1000, 900, 900) == fpmash.DK_GRID_LDS
        exp = _oracle_grid(oracle, ("s>w", kind), refs, _lengths(refs), qrys, _lengths(qrys),
                           1000, k, space, False)
        _check_data(exp, refs + qrys, 1000, sorted_)
        for api in ("dist", "list"):
            got = _dev_dist(ctx, R, Q, 1000, k, space, api)
            _assert_kernel(ctx, fpmash.DK_GRID_LDS, 0)
            _assert_grid(got, exp)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        R.free()
        Q.free()


@pytest.mark.parametrize("below", [0, 300])
@pytest.mark.parametrize("stride,kern", [(1024, "rank1024"), (1025, "rank2048"),
                                         (2048, "rank2048"), (2049, "walk")])
def test_rank_kernel_cap_thresholds(ctx, oracle, stride, kern, below):
    """Sorted u64 rows on the index path at the rank kernel's caps: stride 1024 takes CAP
    1024, 1025 and 2048 take CAP 2048, 2049 the literal walk.  Rows as long as the stride on
    both sides (a query row of CAP entries fills every staging slot and puts its 8 sentinels
    at the end of the LDS arrays), S equal to that length and 300 below it; the set against
    another and against itself (the symmetric pair rule)."""
    import fpmash
    kernel, path = {"rank1024": (fpmash.DK_CAND_RANK_1024, 2),
                    "rank2048": (fpmash.DK_CAND_RANK_2048, 2),
                    "walk": (fpmash.DK_CAND_WALK, 1)}[kern]
    S = stride - below
    space = 4.0 ** 21
    refs, qrys, R, Q = _straddle_rows(ctx, "u64", cap=stride)
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    try:
        assert sum(len(x) == stride for x in refs) >= 3
        assert sum(len(x) == stride for x in qrys) >= 3
        rl, ql = _lengths(refs), _lengths(qrys)
        exp = _oracle_grid(oracle, ("cap", stride, S), refs, rl, qrys, ql, S, 21, space, True)
        exp_s = _oracle_grid(oracle, ("cap-self", stride, S), refs, rl, refs, rl, S, 21, space,
                             True)
        _check_data(exp, refs + qrys, S)
        for api in ("dist", "dist16", "list"):
            got = _dev_dist(ctx, R, Q, S, 21, space, api)
            _assert_kernel(ctx, kernel, path)
            _assert_grid(got, exp)
            got = _dev_dist(ctx, R, R, S, 21, space, api)
            _assert_kernel(ctx, kernel, path)
            _assert_grid(got, exp_s)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        R.free()
        Q.free()


# ---- 4. the image kernel's XCD tile map -------------------------------------------------------

@pytest.mark.parametrize("n_ref,n_qry", [(330, 40), (256, 33), (520, 70)])
def test_image_kernel_tile_map(ctx, oracle, n_ref, n_qry):
    """compare_grid_img_kernel deals the tiles to the 8 XCDs: per = (ref blocks of 32) / 8
    blocks owned by each XCD, the rest dealt tile by tile.  11, 8 and 17 ref blocks: per = 1
    with 3 left over, per = 1 with none, per = 2 with 1; 2 and 3 query blocks; row counts
    that are no multiples of 32.  Every cell against the oracle."""
    import fpmash
    nrb, nqb = (n_ref + 31) // 32, (n_qry + 31) // 32
    assert nrb // 8 >= 1 and (nrb % 8, nqb) in ((3, 2), (0, 2), (1, 3))
    rng = np.random.default_rng(n_ref)
    lists = _fp_lists(rng, n_ref + n_qry, 64, 100, 150, alien=0)
    refs, qrys = lists[:n_ref], lists[n_ref:]
    refs[7] = refs[7][:0]
    qrys[3] = qrys[3][:0]
    rl, ql = _lengths(refs), _lengths(qrys)
    exp = oracle.dist_grid(refs, rl, qrys, ql, 64, 1, 10.0, use64=False, threads=8)
    _check_data(exp, lists, 64, sorted_=False)
    R = _Rows(ctx, refs, rl, np.uint32, stride=100)
    Q = _Rows(ctx, qrys, ql, np.uint32, stride=100)
    ctx.set_dist_mode(fpmash.DIST_DENSE)
    try:
        for api in ("dist", "dist16"):
            got = _dev_dist(ctx, R, Q, 64, 1, 10.0, api)
            _assert_kernel(ctx, fpmash.DK_GRID_IMG, 0)
            _assert_grid(got, exp)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        R.free()
        Q.free()


# ---- 5. unequal strides, padding, alignment ---------------------------------------------------

# (ref stride, qry stride, ref offset, qry offset, ref lists cut to, qry lists cut to): the
# equal-stride base; one side narrower than S and the other past 1024, both ways; strides
# past every length; odd strides; row bases one element off a 16-byte boundary
_LAYOUTS = {
    "base": (1000, 1000, 0, 0, 1000, 1000),
    "narrow-ref": (700, 1100, 0, 0, 700, 1000),
    "narrow-qry": (1100, 700, 0, 0, 1000, 700),
    "wide": (1500, 1500, 0, 0, 1000, 1000),
    "odd": (1001, 1003, 0, 0, 1000, 1000),
    "offset": (1000, 1000, 1, 1, 1000, 1000),
    "offset-ref": (1004, 1000, 1, 0, 1000, 1000),
}


@functools.lru_cache(maxsize=None)
def _layout_set(kind):
    """33 + 21 lists of up to 1000 entries (row counts that are no multiples of a tile)"""
    rng = np.random.default_rng({"u64": 61, "u32": 62, "fp": 63}[kind])
    if kind == "fp":
        lists = _fp_lists(rng, 54, 900, 1000, 400)
        for i, m in ((4, 0), (20, 300), (40, 0), (50, 650)):
            lists[i] = lists[i][:m]
        return lists
    cut = {4: 0, 20: 300, 40: 0, 50: 650, 8: 999}
    return _family_lists(rng, np.uint64 if kind == "u64" else np.uint32, 6, 9, 1000,
                         lambda i: cut.get(i, 1000 if i % 2 else 1000 - int(rng.integers(0, 90))),
                         interleave=True)


def _layout_kernel(kind, mode, S, rs, qs):
    import fpmash
    if mode == "dense":
        return _dense_kernel(kind == "u64", S, rs, qs), 0
    if kind != "u64":
        return fpmash.DK_CAND_WALK, 1
    return (fpmash.DK_CAND_RANK_1024 if max(rs, qs) <= 1024 else fpmash.DK_CAND_RANK_2048), 2


@pytest.mark.parametrize("layout", [x for x in _LAYOUTS if x != "base"])
@pytest.mark.parametrize("kind,mode,S,kern", [
    ("u64", "sparse", 1000, "rank"), ("u64", "dense", 600, "lds"),
    ("u32", "dense", 1000, "img"), ("fp", "dense", 1000, "img"),
    ("u32", "dense", 1100, "lds"), ("fp", "dense", 1100, "lds"),
    ("u32", "sparse", 1000, "walk"), ("fp", "sparse", 1000, "walk")])
def test_strides_padding_alignment(ctx, oracle, kind, mode, S, kern, layout):
    """ref_stride != qry_stride (the kernels mix max(strides) with min(stride, CAP)), rows
    padded past every length with values that are no list entries, odd strides and row
    bases 4 / 8 bytes off a 16-byte boundary (the LDS walk's element-loop staging): the
    results equal those of the same lists in equal 16-byte-aligned strides, and the
    oracle's."""
    import fpmash
    rs, qs, r_off, q_off, r_cut, q_cut = _LAYOUTS[layout]
    lists = _layout_set(kind)
    refs, qrys = [x[:r_cut] for x in lists[:33]], [x[:q_cut] for x in lists[33:]]
    rl, ql = _lengths(refs), _lengths(qrys)
    dt = np.uint64 if kind == "u64" else np.uint32
    k, space = (21, 4.0 ** 21) if kind != "fp" else (1, 10.0)
    exp = _oracle_grid(oracle, ("layout", kind, S, r_cut, q_cut), refs, rl, qrys, ql, S, k,
                       space, kind == "u64")
    _check_data(exp, refs + qrys, S, sorted_=kind != "fp")
    kernel, path = _layout_kernel(kind, mode, S, rs, qs)
    names = {"rank": (fpmash.DK_CAND_RANK_1024, fpmash.DK_CAND_RANK_2048),
             "lds": (fpmash.DK_GRID_LDS,), "img": (fpmash.DK_GRID_IMG,),
             "walk": (fpmash.DK_CAND_WALK,)}
    assert kernel in names[kern]
    eq = max(rs, qs) + (-max(rs, qs)) % 4
    rows = []
    ctx.set_dist_mode(_mode(mode))
    try:
        R = _Rows(ctx, refs, rl, dt, stride=rs, off=r_off, tail=5, junk=71)
        rows.append(R)
        Q = _Rows(ctx, qrys, ql, dt, stride=qs, off=q_off, tail=3, junk=72)
        rows.append(Q)
        R0 = _Rows(ctx, refs, rl, dt, stride=eq)
        rows.append(R0)
        Q0 = _Rows(ctx, qrys, ql, dt, stride=eq)
        rows.append(Q0)
        assert R0.rows % 16 == 0 and Q0.rows % 16 == 0
        assert (R.rows % 16 != 0) == (r_off != 0) and (Q.rows % 16 != 0) == (q_off != 0)
        for api in ("dist", "list"):
            got = _dev_dist(ctx, R, Q, S, k, space, api)
            _assert_kernel(ctx, kernel, path)
            base = _dev_dist(ctx, R0, Q0, S, k, space, api)
            _assert_kernel(ctx, _layout_kernel(kind, mode, S, eq, eq)[0], path)
            _assert_grid(got, exp)
            _assert_grid(base, exp)
            for key in got:
                assert np.array_equal(got[key], base[key]), key
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        for x in rows:
            x.free()


# ---- 6. zero-extended k <= 16 rows from the sketch job ----------------------------------------

def test_sketch_job_k16_rows_rank_kernel(ctx, oracle):
    """A device pipeline at k = 16: the sketch job leaves u32 hashes as zero-extended u64
    rows, handed to fpm_dist_list_dev with hash_bytes = 8.  In the rank kernel these are full
    rows of at most 32 bits (no high-dword keys, key shift 0).  The grid equals the oracle's
    for the oracle's own k = 16 sketches."""
    import fpmash
    import fpmash.datagen as D
    L = fpmash.lib()
    k, s = 16, 1000
    seqs = D.family_dna(6, 10, 2000, sub_rate=(0.0, 0.08), seed=77)
    n = len(seqs)
    sk = oracle.sketch_batch(oracle.params(k=k, s=s), seqs)
    assert all(len(x) == s and int(x[-1]) < 2 ** 32 for x in sk)
    exp = _oracle_grid(oracle, ("job16",), sk, [2000] * n, sk, [2000] * n, s, k, 4.0 ** k, True)
    assert (exp[0] > 0).any() and (exp[0] == 0).any()
    P = fpmash.make_params(k=k, s=s)
    assert not P.use64
    job = ctx.sketch_job(P, seqs)
    lens = fpmash.DeviceBuffer.from_array(ctx, np.full(n, 2000, np.uint64))
    bufs = _outputs(ctx, n * n, 2, full=False)
    lst = fpmash.CellList(ctx, n * n)
    ctx.set_dist_mode(fpmash.DIST_SPARSE)
    try:
        job.run()
        rows, cnt, ng, stride = job.device_output()
        assert (ng, stride) == (n, s)
        fpmash._check(L.fpm_dist_list_dev(ctx.h, rows, cnt, lens.ptr, stride, n, rows, cnt,
                                          lens.ptr, stride, n, 8, s, k, 4.0 ** k, -1.0, -1.0,
                                          bufs[0].ptr, bufs[1].ptr, lst.ref, None))
        ctx.synchronize()
        _assert_kernel(ctx, fpmash.DK_CAND_RANK_1024, 2)
        got = fpmash.expand_compact(bufs[0].to_array(np.uint16, n * n),
                                    bufs[1].to_array(np.uint16, n * n), lst.fetch(), n)
        _assert_grid(got, exp)
    finally:
        ctx.set_dist_mode(fpmash.DIST_AUTO)
        for b in bufs + [lens]:
            b.free()
        lst.free()
        job.free()


def test_no_pairs_reports_no_kernel(ctx):
    """a device grid without pairs launches no compare kernel (after a call that did)"""
    import fpmash
    lists = [np.arange(1, 50, dtype=np.uint64), np.arange(20, 90, dtype=np.uint64)]
    R = _Rows(ctx, lists, [1000, 1000], np.uint64)
    Q = _Rows(ctx, [], [], np.uint64, stride=R.stride)
    try:
        got = _dev_dist(ctx, R, R, 100, 21, 4.0 ** 21, "dist")
        assert got["numer"].tolist() == [49, 30, 30, 70]
        _assert_kernel(ctx, fpmash.DK_GRID_LDS, 0)
        for api in ("dist", "list"):
            got = _dev_dist(ctx, R, Q, 100, 21, 4.0 ** 21, api)
            assert len(got["numer"]) == 0
            _assert_kernel(ctx, fpmash.DK_NONE, 0)
    finally:
        R.free()
        Q.free()
