"""GPU parity of contain (fpm_contain / fpm_contain_dev) with the model of the reference's walk
(tests/contain_model.py), for u64 and u32 rows.

Every case runs in AUTO mode and in forced LITERAL mode; both must equal the model cell for
cell, hence each other.  The cases sit where the kernels can go wrong: lengths at the wave (64)
and 16-byte chunk edges, the order and value edges of the closed form, padded and odd strides
with poisoned padding, the workgroup's ref-row count, the LDS cap of the query row, and rows
that are not strictly ascending.  Every test asserts the kernel that ran
(Context.last_contain_kernel), so a moved threshold fails here instead of moving the coverage.
"""
import numpy as np
import pytest

import contain_model as M

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)


def _dt(use64):
    return np.uint64 if use64 else np.uint32


def _pool(rng, n, use64):
    """n distinct ascending values over the whole unsigned range (about half with the top bit
    set: a signed compare would misorder them)"""
    bits = 64 if use64 else 32
    v = np.unique(rng.integers(0, 2 ** bits, 2 * n, dtype=np.uint64, endpoint=False))
    v = v[rng.permutation(len(v))[:n]]
    v.sort()
    assert (v >> np.uint64(bits - 1)).any() and not (v >> np.uint64(bits - 1)).all()
    return v.astype(_dt(use64))


def _sample(rng, pool, n):
    return np.sort(pool[rng.permutation(len(pool))[:n]])


def _matrix(lists, stride, poison, dt):
    m = np.full((max(len(lists), 1), stride), poison, dtype=dt)
    for i, l in enumerate(lists):
        m[i, : len(l)] = l
    return m[: len(lists)], np.array([len(l) for l in lists], np.uint32)


def _run(ctx, refs, qrys, use64, expected, auto_kernel, ref_stride=None, qry_stride=None,
         poison=0):
    """both modes against `expected` = (common, steps); the AUTO call must launch auto_kernel"""
    import fpmash
    dt = _dt(use64)
    rs = ref_stride or max([len(x) for x in refs] + [1])
    qs = qry_stride or max([len(x) for x in qrys] + [1])
    R, rl = _matrix(refs, rs, poison, dt)
    Q, ql = _matrix(qrys, qs, poison, dt)
    out = {}
    try:
        for mode, want in ((fpmash.CONTAIN_AUTO, auto_kernel),
                           (fpmash.CONTAIN_LITERAL, fpmash.CK_LITERAL)):
            ctx.set_contain_mode(mode)
            got = ctx.contain_rows(R, rl, Q, ql)
            k = ctx.last_contain_kernel()
            assert k == want, f"{fpmash.CONTAIN_KERNELS[k]} ran, {fpmash.CONTAIN_KERNELS[want]} expected"
            assert np.array_equal(got["steps"], expected[1]), mode
            assert np.array_equal(got["common"], expected[0]), mode
            out[mode] = got
    finally:
        ctx.set_contain_mode(fpmash.CONTAIN_AUTO)
    a, b = out[fpmash.CONTAIN_AUTO], out[fpmash.CONTAIN_LITERAL]
    assert np.array_equal(a["common"], b["common"]) and np.array_equal(a["steps"], b["steps"])
    return a


def _length_rows(use64, seed):
    rng = np.random.default_rng(seed)
    pool = _pool(rng, 260, use64)
    refs = [_sample(rng, pool, n) for n in LENGTHS]
    qrys = [_sample(rng, pool, n) for n in LENGTHS]
    return refs, qrys


@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
def test_lengths_at_wave_and_chunk_edges(ctx, use64):
    import fpmash
    refs, qrys = _length_rows(use64, 3)
    exp = M.grid(refs, qrys)
    # the grid means something: full, partial and empty intersections, walks cut by either list
    assert (exp[0] > 0).any() and (exp[0] == 0).any() and (exp[1] == 0).any()
    assert (exp[0] < exp[1]).any()
    _run(ctx, refs, qrys, use64, exp, fpmash.CK_ROWS_LDS)


@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
def test_order_edges(ctx, use64):
    import fpmash
    rng = np.random.default_rng(17)
    P = _pool(rng, 240, use64)
    one = P.dtype.type(1)
    Q0 = P[50:150]
    between = np.append(P[20:99], P[99] + one)        # maxR strictly between two Q entries
    assert between[-1] < P[100]
    refs = [P[0:50],            # 0: maxR < Q[0]
            P[20:100],          # 1: maxR equal to an element of Q
            between,            # 2
            P[60:240],          # 3: maxR > max Q
            Q0,                 # 4: identical rows
            P[60:140:2],        # 5: R a strict subset of Q
            P[30:170]]          # 6: Q a strict subset of R
    qrys = [Q0, P[30:170], P[149:150]]
    exp = M.grid(refs, qrys)
    co, st = (a.reshape(len(qrys), len(refs)) for a in exp)
    assert (co[0, 0], st[0, 0]) == (0, 0)
    assert (co[0, 1], st[0, 1]) == (50, 50)            # Q0[49] = P[99] = maxR is counted
    assert (co[0, 2], st[0, 2]) == (49, 50)            # ... the value above it is passed, not matched
    assert (co[0, 3], st[0, 3]) == (90, 100)
    assert (co[0, 4], st[0, 4]) == (100, 100)
    # 40 ref entries let the walk pass Q0[0..40) = P[50:90], which holds P[60], P[62] .. P[88]
    assert (co[0, 5], st[0, 5]) == (15, 40)
    assert (co[0, 6], st[0, 6]) == (100, 100)
    _run(ctx, refs, qrys, use64, exp, fpmash.CK_ROWS_LDS)


def test_value_edges_u64_dwords(ctx):
    """values built from a few high and low dwords: many pairs equal in one dword only"""
    import fpmash
    rng = np.random.default_rng(23)
    hi = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], np.uint64)
    lo = np.array([0, 1, 5, 2 ** 31, 2 ** 32 - 1], np.uint64)
    pool = np.sort((hi[:, None] << np.uint64(32) | lo[None, :]).ravel())
    refs = [_sample(rng, pool, n) for n in (20, 7, 12, 3, 20)]
    qrys = [_sample(rng, pool, n) for n in (20, 9, 14, 1)]
    refs[0] = pool.copy()
    exp = M.grid(refs, qrys)
    assert (exp[0] > 0).any() and (exp[0] < exp[1]).any()
    _run(ctx, refs, qrys, True, exp, fpmash.CK_ROWS_LDS)


def test_value_edges_u32_top_bit(ctx):
    import fpmash
    rng = np.random.default_rng(29)
    pool = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1], np.uint32)
    refs = [_sample(rng, pool, n) for n in (7, 3, 4, 5, 2)]
    qrys = [_sample(rng, pool, n) for n in (7, 4, 5, 1)]
    exp = M.grid(refs, qrys)
    _run(ctx, refs, qrys, False, exp, fpmash.CK_ROWS_LDS)


@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
def test_clustered_values_share_a_bucket(ctx, use64):
    """runs of consecutive values: hundreds of entries in one bucket of the staged row's
    directory (searched by bisection) beside empty buckets; and the rows [0] and [max]"""
    import fpmash
    dt = _dt(use64)
    rng = np.random.default_rng(33)
    top = np.iinfo(dt).max
    base = [0, 1000, int(top) // 2 - 150, int(top) - 299]
    pool = np.concatenate([np.arange(b, b + 300, dtype=np.uint64) for b in base]).astype(dt)
    refs = [_sample(rng, pool, n) for n in (700, 300, 64, 1200)] + [pool[:1], pool[-1:]]
    qrys = [_sample(rng, pool, n) for n in (650, 129, 1200)] + [pool[:1], pool[-1:],
                                                              pool[300:600], pool[100:250]]
    exp = M.grid_ascending(refs, qrys)
    lit = M.grid(refs[1:3], qrys[1:2])
    assert lit[0].tolist() == [exp[0][len(refs) + 1], exp[0][len(refs) + 2]]
    assert (exp[0] > 4).any() and (exp[0] < exp[1]).any()
    _run(ctx, refs, qrys, use64, exp, fpmash.CK_ROWS_LDS)


@pytest.mark.parametrize("poison", [0, -1], ids=["zeros", "ones"])
@pytest.mark.parametrize("use64,ref_stride,qry_stride",
                         [(True, 131, 133), (True, 140, 130), (False, 133, 131),
                          (False, 130, 135), (False, 132, 134)])
def test_padded_and_odd_strides(ctx, use64, ref_stride, qry_stride, poison):
    """rows start at every 16-byte residue (odd strides) and the cells past each length hold
    one shared value on both sides: a read past a length would count or stop wrongly"""
    import fpmash
    refs, qrys = _length_rows(use64, 5)
    poison = np.iinfo(_dt(use64)).max if poison else 0
    # the shared value is also a real entry of some rows (the smallest / largest possible hash)
    edge = _dt(use64)(poison)
    for rows in (refs, qrys):
        rows[3] = np.unique(np.append(rows[3][:-1], edge))
        rows[5] = np.unique(np.append(rows[5][1:], edge))
    exp = M.grid(refs, qrys)
    _run(ctx, refs, qrys, use64, exp, fpmash.CK_ROWS_LDS, ref_stride, qry_stride, poison)


@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
@pytest.mark.parametrize("n_qry", [1, 3])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_ref_rows_around_a_workgroup(ctx, use64, n_qry, d):
    import fpmash
    n_ref = fpmash.CONTAIN_BLOCK_REFS + d
    rng = np.random.default_rng(40 + d)
    pool = _pool(rng, 120, use64)
    refs = [_sample(rng, pool, int(rng.integers(0, 100))) for _ in range(n_ref)]
    qrys = [_sample(rng, pool, 70 + 5 * i) for i in range(n_qry)]
    exp = M.grid(refs, qrys)
    _run(ctx, refs, qrys, use64, exp, fpmash.CK_ROWS_LDS, 101, 99)


def test_more_query_rows_than_a_grid_dimension(ctx):
    """70,000 one-entry query rows: the launch cannot put the query index in gridDim.y"""
    import fpmash
    rng = np.random.default_rng(51)
    pool = _pool(rng, 64, True)
    refs = [pool[:40:2], pool[10:50]]
    qv = pool[rng.integers(0, 64, 70000)]
    exp_c = np.stack([np.isin(qv, r) for r in refs], 1).astype(np.uint32).ravel()
    exp_s = np.stack([qv <= r[-1] for r in refs], 1).astype(np.uint32).ravel()
    assert M.grid(refs, [qv[:1], qv[1:2]])[0].tolist() == exp_c[:4].tolist()
    R, rl = _matrix(refs, 40, 0, np.uint64)
    got = ctx.contain_rows(R, rl, qv.reshape(-1, 1), np.ones(len(qv), np.uint32))
    assert ctx.last_contain_kernel() == fpmash.CK_ROWS_LDS
    assert np.array_equal(got["common"], exp_c) and np.array_equal(got["steps"], exp_s)


@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_query_row_at_the_lds_cap(ctx, use64, d):
    import fpmash
    cap = ctx.contain_lds_cap(use64)
    # 156 KB of dynamic LDS (63 KB where the limit stays) less 32 bytes of alignment padding
    # and spare entries and the largest bucket directory (4,097 u32, rounded to 16 bytes)
    assert cap in [(b * 1024 - 32 - 16400) // (8 if use64 else 4) for b in (156, 63)]
    L = cap + d
    rng = np.random.default_rng(61)
    pool = _pool(rng, L + L // 2, use64)
    Q = _sample(rng, pool, L)
    # a superset and the row itself read Q's last entry; a short ref stops the walk early
    refs = [pool, Q, _sample(rng, pool, 5000), pool[:0], pool[-1:], Q[: L // 2]]
    qrys = [Q, _sample(rng, pool, 100)]
    exp = M.grid_ascending(refs, qrys)
    assert exp[1][0] == L and exp[0][0] == L and exp[0][1] == L and exp[1][3] == 0
    want = fpmash.CK_ROWS_LDS if d <= 0 else fpmash.CK_ROWS_GLOBAL
    _run(ctx, refs, qrys, use64, exp, want)


def _ascending(use64, seed, n_rows=3):
    rng = np.random.default_rng(seed)
    pool = _pool(rng, 150, use64)
    return [_sample(rng, pool, n) for n in (129, 64, 100)[:n_rows]]


@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
@pytest.mark.parametrize("case", ["descending", "repeat", "last-two-qry", "last-two-ref"])
def test_rows_not_strictly_ascending_take_the_literal_walk(ctx, use64, case):
    import fpmash
    refs, qrys = _ascending(use64, 71), _ascending(use64, 72)
    if case == "descending":
        qrys[1] = qrys[1][::-1].copy()
        refs[2] = refs[2][::-1].copy()
    elif case == "repeat":
        refs[0] = refs[0].copy()
        refs[0][40] = refs[0][39]
    else:
        rows, other = (qrys, refs) if case == "last-two-qry" else (refs, qrys)
        other[0] = rows[-1].copy()      # the same row, in order, on the other side: that walk
        r = rows[-1].copy()             # reaches the inversion
        r[-2], r[-1] = r[-1], r[-2]
        rows[-1] = r
    exp = M.grid(refs, qrys)
    if case != "repeat":
        # the closed form would be wrong here: the dispatch matters
        cf = M.grid(refs, qrys, M.closed_form)
        assert not (np.array_equal(exp[0], cf[0]) and np.array_equal(exp[1], cf[1]))
    _run(ctx, refs, qrys, use64, exp, fpmash.CK_LITERAL, 131, 135, 0)


def test_fp_style_lists_with_repeats_everywhere(ctx):
    """the shape of `sketch -fp` rows: u32, any order, many repeats"""
    import fpmash
    rng = np.random.default_rng(81)
    refs = [rng.integers(0, 40, n).astype(np.uint32) for n in (129, 65, 1, 0, 200)]
    qrys = [rng.integers(0, 40, n).astype(np.uint32) for n in (128, 63, 7, 0)]
    exp = M.grid(refs, qrys)
    assert (exp[0] > 0).any()
    _run(ctx, refs, qrys, False, exp, fpmash.CK_LITERAL)


def test_empty_grid(ctx):
    import fpmash
    refs, qrys = _ascending(True, 91), _ascending(True, 92)
    got = ctx.contain(refs, qrys)
    assert ctx.last_contain_kernel() == fpmash.CK_ROWS_LDS and len(got["common"]) == 9
    for r, q in ((refs, []), ([], qrys), ([], [])):
        got = ctx.contain(r, q)
        assert ctx.last_contain_kernel() == fpmash.CK_NONE
        assert len(got["common"]) == 0 and len(got["steps"]) == 0


def test_device_entry_on_a_query_sub_block(ctx):
    """fpm_contain_dev on rows of a larger device matrix, the way the CLI walks query blocks:
    the query pointer starts mid-buffer at an odd row"""
    import fpmash
    refs, qrys = _length_rows(True, 7)
    R, rl = _matrix(refs, 131, 0, np.uint64)
    Q, ql = _matrix(qrys, 133, 0, np.uint64)
    exp = M.grid(refs, qrys[3:])
    nr, nq = len(refs), len(qrys) - 3
    bufs = [fpmash.DeviceBuffer.from_array(ctx, a) for a in (R, rl, Q, ql)]
    outs = [fpmash.DeviceBuffer(ctx, nr * nq * 4) for _ in range(2)]
    try:
        ctx.contain_dev(bufs[0].ptr, bufs[1].ptr, 131, nr, bufs[2].ptr + 3 * 133 * 8,
                        bufs[3].ptr + 3 * 4, 133, nq, True, outs[0].ptr, outs[1].ptr)
        ctx.synchronize()
        assert ctx.last_contain_kernel() == fpmash.CK_ROWS_LDS
        got = [o.to_array(np.uint32, nr * nq) for o in outs]
    finally:
        for b in bufs + outs:
            b.free()
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
