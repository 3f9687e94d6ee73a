"""Every path of the library over poisoned device memory (Context.set_poison / poison_now).

The library reads device memory from its pool of released buffers, its grow-only scratch slots,
plain allocations and fpm_malloc.  A fresh allocation is usually zero and the session context's
slots hold what the previous test wrote, so a kernel that needs a 0 or a ~0 nobody wrote passes
the other modules by luck.  Here a module-scoped context of its own fills every buffer it hands
out with one byte (0xFF, 0xA5 and 0x00 in turn: a missing 0xff memset only shows under 0x00, a
missing zero under the other two), and every test has one shape: case A, poison_now, a smaller
or differently shaped case B, poison_now, A again.  poison_now overwrites every scratch slot
and every free pooled buffer, so each case runs over memory that holds neither zeros nor its own
earlier results.

Results are compared exactly as in the modules the builders are imported from: integers and
hashes bit-exact, distance and p-value to RTOL = 1e-12, every cell of every full-form output.
The route (plan(), last_dist_kernel, last_dist_probe, the hooks) is asserted where those modules
assert it, so a moved threshold fails here instead of taking the path out of the test."""
import functools

import numpy as np
import pytest

import contain_model as CM
import kfinger_fact_model as KF
import reads_model as RM
import screen_model as SM
import seqio
import test_gpu_contain as TC
import test_gpu_dist_dispatch as TD
import test_gpu_fptext_edges as TF
import test_gpu_kfinger as TK
import test_gpu_kfinger_fact as TKF
import test_gpu_parity as TP
import test_gpu_screen as TS
import test_gpu_sketch_dispatch as SD
import test_gpu_taxscreen as TT

pytestmark = pytest.mark.gpu

RTOL = TP.RTOL
BYTES = (0xFF, 0xA5, 0x00)


@pytest.fixture(scope="module", params=BYTES, ids=["0xFF", "0xA5", "0x00"])
def pctx(request):
    """a context of this module's own with poison on (the shared `ctx` is left alone)"""
    import fpmash
    c = fpmash.Context(0)
    c.set_poison(request.param)
    yield c
    c.close()


def aba(pctx, case_a, case_b):
    """A, poison, B, poison, A"""
    case_a()
    pctx.poison_now()
    case_b()
    pctx.poison_now()
    case_a()


def test_hook_switch(pctx):
    """poison_now needs poison on; set_poison refuses bytes outside -1 .. 255"""
    import fpmash
    L = fpmash.lib()
    assert L.fpm_ctx_set_poison(pctx.h, 256) == fpmash.FPM_EINVAL
    assert L.fpm_ctx_set_poison(pctx.h, -2) == fpmash.FPM_EINVAL
    with fpmash.Context(0) as c:
        c.set_poison(None)                              # (FPM_POISON may have started it on)
        assert L.fpm_ctx_poison_now(c.h) == fpmash.FPM_EINVAL
        c.set_poison(0x5A)
        c.poison_now()                                  # nothing allocated yet
        b = fpmash.DeviceBuffer(c, 4096)
        assert (b.to_array(np.uint8, 4096) == 0x5A).all()     # fpm_malloc
        b.free()
        c.set_poison(None)
        assert L.fpm_ctx_poison_now(c.h) == fpmash.FPM_EINVAL
    pctx.poison_now()


# ---- sketch, host-staged ------------------------------------------------------------------------

def test_sketch_tile_classes(pctx, oracle):
    """-i records whose tiles take classes 0-4 and records without a k-mer: rows, counts, -M"""
    k = 21
    recs = list(SD.straddle_records(k)) + [b"N" * 300, b"ACG", b""]
    want = np.sum([SD.straddle_classes(n) for n in SD.STRADDLE_STARTS], axis=0)
    want[SD.tile_class(300 - k + 1)] += 1               # the N record: a tile without a valid window

    def a():
        plan, _ = SD.run_parity(pctx, oracle, dict(k=k, s=1000), recs, what="A")
        assert plan["tiles"] == list(want) and all(plan["tiles"][c] > 0 for c in range(5))

    def b():
        plan, _ = SD.run_parity(pctx, oracle, dict(k=16, s=64), list(SD.straddle_records(16))[:5],
                                what="B")
        assert plan["tiles"][5] == 0
    aba(pctx, a, b)


def test_sketch_survivors_group(pctx, oracle):
    """one group of 32 chunks: sample bound, selection, merge rounds, the survivors kernel and
    its redo list"""
    k, s, ntile = SD.SURVIVOR_CASES[0]
    rec, _bound, _keys = SD.survivors_group(k, s, ntile)
    rng = np.random.default_rng(71)
    small = [SD.rand_acgt(rng, n) for n in (5000, 300, 4200)]

    def a():
        plan, hooks = SD.run_parity(pctx, oracle, dict(k=k, s=s), [rec], [0], 1, what="A")
        assert plan["tiles"] == [0, 0, 0, 0, ntile, 0] and plan["thr4"] == 1
        assert plan["sample_tiles"] == [0, 0, 0, 0, 2, 0] and plan["tight"] == 1
        assert plan["n_slots"] == 1 and plan["n_sel"] > 0
        assert hooks["short"] == 0 and hooks["redo"] == len(SD.THR_OVER) > 0

    def b():
        plan, _ = SD.run_parity(pctx, oracle, dict(k=k, s=500), small, [0] * 3, 1, what="B")
        assert plan["rounds"] >= 1 and plan["n_slots"] == 0
    aba(pctx, a, b)


def test_sketch_reads_mode(pctx, oracle):
    """reads mode at min_copies = 2: records doubled across tile classes, and a set that needs a
    second widening round"""
    k, s = 21, 1000
    rng = np.random.default_rng(6700)
    recs, groups = [], []
    for g, rec in enumerate(SD.straddle_records(k)[2::3]):
        recs += SD.doubled(rec, k, rng)
        groups += [g] * 3
    wide = RM.widening_reads()
    stream = RM.window_hashes(oracle, wide, 21)
    exp_wide = RM.model_sketch(stream, 30, 2)
    assert len(exp_wide[0]) == 30

    def a():
        SD.run_reads(pctx, oracle, k, s, recs, groups, groups[-1] + 1, what="A")

    def b():
        import fpmash
        got = pctx.sketch_reads(fpmash.make_params(k=21, s=30), wide, groups=[0] * len(wide),
                                n_groups=1, min_copies=2)
        assert got["rounds"] > 1
        assert np.array_equal(got["hashes"][0], exp_wide[0])
        assert np.array_equal(got["counts"][0], exp_wide[1])
        assert int(got["estimate"][0]) == RM.set_size(exp_wide[0], True)
    aba(pctx, a, b)


# ---- sketch, device-parsed ----------------------------------------------------------------------

def _fastq_of(recs):
    return b"".join(b"@q%d c\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(recs))


def _parsed_case(pctx, oracle, text, k, s):
    """fpm_seq_parse -> fpm_seq_packed -> fpm_sketch_stage_seq over one file image, -i"""
    import fpmash
    want = [sq for _n, _c, sq in seqio.parse(text)]
    job, rec, quality = pctx.seq_parse([text])
    try:
        assert not quality
        assert [int(x) for x in rec["seq_len"]] == [len(x) for x in want]
        packed, off = pctx.seq_packed(job, n_rec=len(want))
        assert packed == b"".join(x + b"\0" for x in want)
        assert [int(x) for x in off] == list(np.cumsum([0] + [len(x) + 1 for x in want[:-1]]))
        keep = [x for x in want if len(x) >= k]
        groups, g = np.full(len(want), fpmash.NO_GROUP, np.uint32), 0
        for i, x in enumerate(want):
            if len(x) >= k:
                groups[i], g = g, g + 1
        got, mult = pctx.sketch_seq(fpmash.make_params(k=k, s=s), job, groups, g, counts=True)
    finally:
        pctx.seq_free(job)
    exp, exp_m = oracle.sketch_batch(oracle.params(k=k, s=s), keep, counts=True)
    SD.assert_same(got, exp, "parsed sketch")
    SD.assert_same(mult, exp_m, "parsed multiplicities")


def test_sketch_device_parsed(pctx, oracle):
    rng = np.random.default_rng(72)
    fa = SD.fasta_of([SD.rand_acgt(rng, n, p_lower=0.1) for n in
                      (30, 5, 9000, 20, 21, 2048 + 20, 700, 4096 + 21)])
    fq = _fastq_of([SD.rand_acgt(rng, n) for n in (150, 10, 2600, 21)])
    assert fq.startswith(b"@q0")
    aba(pctx, lambda: _parsed_case(pctx, oracle, fa, 21, 1000),
        lambda: _parsed_case(pctx, oracle, fq, 21, 100))


# ---- -fp text and refs --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _big_text():
    rng = np.random.default_rng(73)
    lines = []
    for i in range(2500):
        idv = b"T%05d" % (i // int(rng.integers(1, 30)))
        vals = rng.integers(0, 200, size=int(rng.integers(0, 16)))
        sep = [b" ", b"\t", b"  "][int(rng.integers(0, 3))]
        lines.append(idv + sep + sep.join(str(v).encode() for v in vals))
    return b"\n".join(lines)


@TF.WIDTHS
def test_fp_text_and_refs(pctx, oracle, use64):
    """a large text, then texts ending 1 .. 15 bytes into the last 16-byte load of the pooled
    buffer (the bytes past the text are the poison, or the large text's)"""
    big = _big_text()

    def b():
        for r in range(1, 16):
            for n in (r, 16 + r, 4096 + r):
                ids, _ = TF.check_text(None, oracle, b"x" * n, use64, c=pctx)
                assert ids == [b"x" * n]
            t = b"A 1 2\nB 3\nB 4 5 6\n" + b"C " + b"7" * r
            TF.check_text(None, oracle, t, use64, c=pctx)
    aba(pctx, lambda: TF.check_text(None, oracle, big, use64, c=pctx), b)


# ---- dist -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _families():
    """A: 96 sorted u64 rows at S = 1000 (two cut short, one empty); B: 7 rows at S = 64"""
    from oracle import oracle as O
    import fpmash.datagen as D
    seqs = D.family_dna(8, 12, 2000, sub_rate=(0.0, 0.08), seed=74)
    A = O.sketch_batch(O.params(k=21, s=1000), seqs)
    A[17], A[40], A[95] = A[17][:10], A[40][:0], A[95][:700]
    la = [len(x) for x in seqs]
    B = O.sketch_batch(O.params(k=21, s=64), seqs[:7])
    B[3] = B[3][:20]
    for x in A + B:
        x.setflags(write=False)
    return A, la, B, la[:7]


@functools.lru_cache(maxsize=None)
def _fp_rows():
    """unsorted u32 -fp rows with repeats: A 40 rows, B 7 rows"""
    rng = np.random.default_rng(75)
    base = rng.integers(0, 2 ** 32, size=3000, dtype=np.uint64).astype(np.uint32)
    A = [base[rng.integers(0, 3000 if i % 2 else 200, size=int(rng.integers(0, 1500)))]
         for i in range(40)]
    B = [base[rng.integers(0, 100, size=n)] for n in (0, 5, 64, 65, 200, 1, 90)]
    return A, [int(rng.integers(1, 20000)) for _ in A], B, [int(rng.integers(1, 900)) for _ in B]


def _grid(pctx, oracle, key, refs, rl, qrys, ql, S, use64=True, api="dist", maxd=-1.0, maxp=-1.0):
    """one grid through Context.dist / dist16 / dist_list against the oracle's, every cell"""
    k, space = (21, 4.0 ** 21) if use64 else (1, 10.0)
    exp = TD._oracle_grid(oracle, ("poison", key, S), refs, rl, qrys, ql, S, k, space, use64)
    fn = {"dist": pctx.dist, "dist16": pctx.dist16, "list": pctx.dist_list}[api]
    got = fn(refs, qrys, S, use64=use64, k=k, kmer_space=space, ref_lengths=rl, qry_lengths=ql,
             max_dist=maxd, max_pvalue=maxp)
    TD._assert_grid(got, exp, maxd, maxp)
    return exp


@pytest.fixture
def mode(request, pctx):
    pctx.set_dist_mode(TD._mode(request.param))
    yield request.param
    pctx.set_dist_mode(TD._mode("auto"))


@pytest.mark.parametrize("mode", ["dense", "sparse"], indirect=True)
def test_dist_sorted_u64(pctx, oracle, mode):
    import fpmash
    A, la, B, lb = _families()
    qa, qla = [x.copy() for x in A[5:25]], la[5:25]
    qb = [x.copy() for x in B]

    def route(S, stride):
        if mode == "dense":
            TD._assert_kernel(pctx, TD._dense_kernel(True, S, stride, stride), sparse=0)
            assert pctx.last_dist_probe() == fpmash.PROBE_NONE
        else:
            TD._assert_kernel(pctx, fpmash.DK_CAND_RANK_1024, sparse=2)
            assert pctx.last_dist_probe() == fpmash.PROBE_FULL

    def a():
        exp = _grid(pctx, oracle, "A", A, la, qa, qla, 1000)
        TD._check_data(exp, A, 1000)
        route(1000, 1000)

    def b():
        _grid(pctx, oracle, "B", B, lb, qb, lb, 64)
        route(64, 64)
    aba(pctx, a, b)


@pytest.mark.parametrize("mode", ["dense", "sparse"], indirect=True)
def test_dist_unsorted_u32_fp(pctx, oracle, mode):
    """unsorted -fp rows: the record index and walk_cand (sparse), the literal dense walk"""
    import fpmash
    A, la, B, lb = _fp_rows()

    def case(key, rows, lens, S):
        exp = _grid(pctx, oracle, key, rows, lens, rows, lens, S, use64=False)
        if mode == "sparse":
            TD._assert_kernel(pctx, fpmash.DK_CAND_WALK, sparse=1)
            assert pctx.last_dist_stats()["candidates"] <= len(rows) ** 2
        else:
            assert pctx.last_dist_stats()["sparse"] == 0
        return exp

    def a():
        exp = case("fpA", A, la, 1000)
        assert (exp[0] > 0).any()
    aba(pctx, a, lambda: case("fpB", B, lb, 64))


def test_dist_self_symmetric(pctx, oracle):
    """a set against itself: symmetric path, half probe, cut index, compacted rank rows, fill"""
    import fpmash
    A, la, B, lb = _families()
    pctx.set_dist_mode(fpmash.DIST_SPARSE)
    try:
        def case(key, rows, lens, S, filt=False):
            _grid(pctx, oracle, key, rows, lens, rows, lens, S,
                  **(dict(maxd=0.1, maxp=1e-10) if filt else {}))
            TD._assert_kernel(pctx, fpmash.DK_CAND_RANK_1024, sparse=2)
            assert pctx.last_dist_probe() == fpmash.PROBE_HALF
            cut, rc = pctx.last_index_cut(), pctx.last_rank_compact()
            assert cut["cut"] and 0 < cut["indexed"] <= cut["entries"]
            assert rc["compact"] and 0 < rc["kept"] <= rc["entries"]
            assert rc["entries"] == sum(len(x) for x in rows)
            return rc

        def a():
            r1 = case("selfA", A, la, 1000)
            pctx.poison_now()
            # the lengths were read before the slots were overwritten: the same answer again
            assert pctx.last_rank_compact() == r1
            st = pctx.last_dist_stats()
            assert st["sparse"] == 2 and 0 < st["candidates"] <= len(A) ** 2
            case("selfA", A, la, 1000, filt=True)
        aba(pctx, a, lambda: case("selfB", B, lb, 64))
    finally:
        pctx.set_dist_mode(fpmash.DIST_AUTO)


@pytest.mark.parametrize("mode", ["dense", "sparse"], indirect=True)
def test_dist_forms(pctx, oracle, mode):
    """the full form, u16 counts and the compact list (a capacity miss included), one set against
    itself and against another"""
    import fpmash
    A, la, B, lb = _families()
    A, la = A[:60], la[:60]
    qa, qla = [x.copy() for x in A[10:40]], la[10:40]

    def a():
        for api in ("dist", "dist16", "list"):
            exp = _grid(pctx, oracle, "formsS", A, la, A, la, 500, api=api)
            _grid(pctx, oracle, "formsO", A, la, qa, qla, 500, api=api, maxd=0.5, maxp=1.0)
        n = int((exp[0] > 0).sum())
        assert n > 17
        # a list too small for the cells with numer > 0: the count still reports every cell
        with pytest.raises(fpmash.FpmError):
            pctx.dist_list(A, A, 500, ref_lengths=la, qry_lengths=la, cap=17)
        nu, de, listed = pctx.dist_list(A, A, 500, ref_lengths=la, qry_lengths=la, cap=n,
                                        expand=False)
        assert len(listed["qry"]) == n and np.array_equal(nu, exp[0]) and np.array_equal(de, exp[1])

    def b():
        for api in ("list", "dist16", "dist"):
            _grid(pctx, oracle, "formsB", B, lb, B, lb, 64, api=api)
    aba(pctx, a, b)


def test_dist_speculated_probe(pctx, oracle):
    """the same shape twice with poison_now between: the second call enqueues its probe over
    poisoned candidate, segment and compacted-row slots before the host knows the path"""
    import fpmash.datagen as D
    S = 37
    rand = oracle.sketch_batch(oracle.params(k=21, s=S), D.family_dna(300, 1, 1500, seed=3))
    fam = oracle.sketch_batch(oracle.params(k=21, s=S),
                              D.family_dna(30, 10, 1500, sub_rate=(0.0, 0.03), seed=4))
    L = [1500] * 300
    _A, _la, B, lb = _families()
    grown = []

    def a():
        _grid(pctx, oracle, "specR", rand, L, rand, L, S)         # sets the profile
        h0, m0 = pctx.spec_stats()
        pctx.poison_now()
        _grid(pctx, oracle, "specR", rand, L, rand, L, S)         # speculated, kept
        assert pctx.spec_stats() == (h0 + 1, m0)
        pctx.poison_now()
        # speculated too: past the profile's capacity and redone the first time, kept once the
        # profile has grown
        exp = _grid(pctx, oracle, "specF", fam, L, fam, L, S)
        h1, m1 = pctx.spec_stats()
        assert h1 + m1 == h0 + m0 + 2 and m1 == m0 + (0 if grown else 1)
        grown.append(1)
        assert (exp[0] > 0).sum() >= 3000
    aba(pctx, a, lambda: _grid(pctx, oracle, "selfB", B, lb, B, lb, 64))


def test_dist_index_overflow_rebuild(pctx, oracle):
    """skewed values: the one-pass index overflows a partition slot and the exact build replaces
    it; then skewed unsorted -fp values, whose overflowed raw index gives way to the record
    index"""
    import fpmash
    rng = np.random.default_rng(77)
    common = np.unique(rng.integers(1, 1 << 52, size=400, dtype=np.uint64))
    lists = [np.unique(np.concatenate([common, rng.integers(1 << 52, 1 << 62, dtype=np.uint64,
                                                            size=int(rng.integers(50, 200)))]))
             for _ in range(600)]
    L = [len(x) * 3 for x in lists]
    rows = list(range(0, 600, 37))
    exp = TD._oracle_grid(oracle, ("poison", "overflow"), lists, L, [lists[r] for r in rows],
                          [L[r] for r in rows], 500, 21, 4.0 ** 21, True)
    base = rng.integers(0, 2 ** 32, size=20000, dtype=np.uint64).astype(np.uint32)
    fp = TP._skewed_fp_lists(rng, base, 60)
    fl = [int(rng.integers(1, 20000)) for _ in fp]
    pctx.set_dist_mode(fpmash.DIST_SPARSE)
    try:
        def a():
            before = pctx.index_rebuilds()
            d = pctx.dist(lists, lists, 500, ref_lengths=L, qry_lengths=L)
            assert pctx.index_rebuilds() > before
            n = len(lists)
            for key, e in (("numer", exp[0]), ("denom", exp[1]), ("distance", exp[2]),
                           ("pvalue", exp[3])):
                got = np.concatenate([d[key][r * n:(r + 1) * n] for r in rows])
                if key in ("numer", "denom"):
                    assert np.array_equal(got, e), key
                else:
                    np.testing.assert_allclose(got, e, rtol=RTOL, atol=0)

        def b():
            e = _grid(pctx, oracle, "skewfp", fp, fl, fp, fl, 1000, use64=False)
            assert pctx.last_dist_stats()["sparse"] == 1
            assert (e[0] > 0).any() and (e[0] == 0).any()
        aba(pctx, a, b)
    finally:
        pctx.set_dist_mode(fpmash.DIST_AUTO)


@pytest.mark.parametrize("kind", ["sorted", "fp"])
def test_dist_resident_refset(pctx, oracle, kind):
    """a resident set: created over poisoned slots, two query blocks with poison_now between and
    the first block again; then the mirror list call on device rows"""
    import fpmash
    if kind == "sorted":
        A, la, _B, _lb = _families()
        refs, rl, qrys, ql, S, use64 = A[:45], la[:45], A[30:70], la[30:70], 1000, True
    else:
        A, la, _B, _lb = _fp_rows()
        refs, rl, qrys, ql, S, use64 = A[:25], la[:25], A[15:], la[15:], 1000, False
    k, space = (21, 4.0 ** 21) if use64 else (1, 10.0)
    blocks = [(0, 13), (13, len(qrys))]
    exp = [TD._oracle_grid(oracle, ("poison", "rs", kind, i), refs, rl, qrys[a:b], ql[a:b], S, k,
                           space, use64) for i, (a, b) in enumerate(blocks)]
    mexp = TD._oracle_grid(oracle, ("poison", "rsm", kind), qrys, ql, refs, rl, S, k, space, use64)
    pexp = TD._oracle_grid(oracle, ("poison", "rsp", kind), refs, rl, qrys, ql, S, k, space, use64)
    dt = np.uint64 if use64 else np.uint32
    pctx.set_dist_mode(fpmash.DIST_SPARSE)
    try:
        rs = pctx.refset(refs, S, use64=use64, ref_lengths=rl,
                         width=max(len(x) for x in refs + qrys))
        try:
            for i in (0, 1, 0):
                a, b = blocks[i]
                got = rs.dist(qrys[a:b], k=k, kmer_space=space, qry_lengths=ql[a:b])
                TD._assert_grid(got, exp[i])
                assert pctx.last_dist_stats()["sparse"] == (2 if use64 else 1)
                pctx.poison_now()
        finally:
            rs.free()
        w = max(len(x) for x in refs + qrys)
        R = TD._Rows(pctx, refs, rl, dt, stride=w, junk=5)
        Q = TD._Rows(pctx, qrys, ql, dt, stride=w, junk=6)
        try:
            for compact in (True, False):
                prim, mirr = TD._dev_mirror(pctx, R, Q, S, k, space, compact)
                TD._assert_grid(prim, pexp)
                TD._assert_grid(mirr, mexp)
                pctx.poison_now()
        finally:
            R.free()
            Q.free()
    finally:
        pctx.set_dist_mode(fpmash.DIST_AUTO)


@pytest.mark.parametrize("mode", ["dense", "sparse"], indirect=True)
def test_dist_list_prefill(pctx, oracle, mode):
    """a prefill the dist call takes over, and one it does not (it waits for it)"""
    import fpmash
    A, la, B, lb = _families()
    A, la = A[:50], la[:50]
    L = fpmash.lib()

    def taken(key, rows, lens, S):
        exp = TD._oracle_grid(oracle, ("poison", key, S), rows, lens, rows, lens, S, 21,
                              4.0 ** 21, True)
        got = pctx.dist_list(rows, rows, S, ref_lengths=lens, qry_lengths=lens, prefill=True)
        TD._assert_grid(got, exp)

    def not_taken():
        spare = [fpmash.DeviceBuffer(pctx, 64 * 64 * 2) for _ in range(4)]
        try:
            for i, S in ((0, 300), (2, 400)):
                fpmash._check(L.fpm_dist_list_prefill(pctx.h, spare[i].ptr, spare[i + 1].ptr, 64,
                                                      64, S, None))
            pctx.poison_now()            # a pending prefill is caller memory: left alone
            exp = TD._oracle_grid(oracle, ("poison", "pfB", 64), B, lb, B, lb, 64, 21, 4.0 ** 21,
                                  True)
            TD._assert_grid(pctx.dist_list(B, B, 64, ref_lengths=lb, qry_lengths=lb), exp)
            pctx.synchronize()
            for i, S in ((0, 300), (2, 400)):
                assert not spare[i].to_array(np.uint16, 64 * 64).any()
                assert (spare[i + 1].to_array(np.uint16, 64 * 64) == S).all()
        finally:
            for b in spare:
                b.free()
    aba(pctx, lambda: taken("pfA", A, la, 500), not_taken)


# ---- the slot the index build and the device merge share -------------------------------------

def test_merge_dev_and_index_share_a_slot(pctx, oracle):
    """fpm_sketch_merge_dev with 5 parts, a sparse dist (whose one-pass index build keeps its
    partition fills in the same slot), then a merge of 2 parts"""
    import fpmash
    from fpmash.shard import kmer_shard
    s = 1000
    rng = np.random.default_rng(78)
    unit = TP.rand_seq(rng, 3000)
    genome = TP.rand_seq(rng, 60_000) + unit * 4 + TP.rand_seq(rng, 30_000)
    exp = oracle.sketch_batch(oracle.params(k=21, s=s), [genome])[0]
    P = fpmash.make_params(k=21, s=s)
    A, la, _B, _lb = _families()

    def merge(parts):
        segs = [genome[a:b] for a, b in (kmer_shard(len(genome), 21, parts, r)
                                         for r in range(parts))]
        sk = pctx.sketch(P, segs)
        m = np.zeros((parts, s), np.uint64)
        for i, x in enumerate(sk):
            m[i, :len(x)] = x
        bufs = [fpmash.DeviceBuffer.from_array(pctx, m),
                fpmash.DeviceBuffer.from_array(pctx, np.array([len(x) for x in sk], np.uint32)),
                fpmash.DeviceBuffer(pctx, s * 8), fpmash.DeviceBuffer(pctx, 4)]
        try:
            fpmash._check(fpmash.lib().fpm_sketch_merge_dev(pctx.h, bufs[0].ptr, bufs[1].ptr, parts,
                                                            s, bufs[2].ptr, bufs[3].ptr, None))
            pctx.synchronize()
            n = int(bufs[3].to_array(np.uint32, 1)[0])
            assert n == len(exp)
            assert np.array_equal(bufs[2].to_array(np.uint64, s)[:n], exp)
        finally:
            for b in bufs:
                b.free()

    def dist():
        pctx.set_dist_mode(fpmash.DIST_SPARSE)
        try:
            _grid(pctx, oracle, "selfA", A, la, A, la, 1000)
            assert pctx.last_dist_stats()["sparse"] == 2
        finally:
            pctx.set_dist_mode(fpmash.DIST_AUTO)
    merge(5)
    dist()                   # no poison between: the fills land on the merge's rows
    merge(2)
    pctx.poison_now()
    dist()
    merge(5)


# ---- contain, screen, taxscreen ---------------------------------------------------------------

@pytest.mark.parametrize("use64", [True, False], ids=["u64", "u32"])
def test_contain(pctx, use64):
    """LDS rows and the literal walk (TC._run runs both modes); then rows that are not strictly
    ascending, which AUTO hands to the literal walk by the flag in the counter block"""
    import fpmash
    refs, qrys = TC._length_rows(use64, 3)
    exp = CM.grid(refs, qrys)
    rng = np.random.default_rng(79)
    pool = TC._pool(rng, 60, use64)
    r2 = [TC._sample(rng, pool, n) for n in (5, 0, 33)]
    q2 = [TC._sample(rng, pool, 20), np.array([pool[3], pool[3], pool[9]], pool.dtype)]
    exp2 = CM.grid(r2, q2)
    aba(pctx, lambda: TC._run(pctx, refs, qrys, use64, exp, fpmash.CK_ROWS_LDS),
        lambda: TC._run(pctx, r2, q2, use64, exp2, fpmash.CK_LITERAL))


@pytest.mark.parametrize("k", TS.KS)
def test_screen(pctx, oracle, k):
    """table build, pool pass in three chunks, rows and -w; then a tiny table"""
    import fpmash
    reads = RM.base_reads()
    keys = RM.window_hashes(oracle, reads, k)
    rng = np.random.default_rng(80)
    distinct = np.unique(np.asarray(keys, np.uint64))
    lists = [np.sort(rng.choice(distinct, size=n, replace=False)).astype(TS.dtype_of(k))
             for n in (200, 1, 150, 64)]
    small = [np.array([1, 2, 3, 10], TS.dtype_of(k)), np.array([3, 40, 50], TS.dtype_of(k))]
    skeys = np.array([1] * 5 + [3] * 9 + [40] * 4 + [77], np.uint64)

    def a():
        sc = TS.make_screen(pctx, lists, k, s=100, pad=3, poison=TS.dtype_of(k)(0x5A5A5A5A))
        try:
            for lo, hi in ((0, 7), (7, 150), (150, len(reads))):
                sc.add_records(fpmash.make_params(k=k, s=100), reads[lo:hi])
            TS.check_counts_rows(sc, lists, keys, winner_lengths=[5, 4, 3, 2], k=k)
            assert sc.set_size() == SM.set_size(keys, 100, RM.use64_of(k))
        finally:
            sc.free()

    def b():
        sc = TS.make_screen(pctx, small, k)
        try:
            sc.add_hashes(skeys)
            TS.check_counts_rows(sc, small, skeys, winner_lengths=[4, 4], k=k)
        finally:
            sc.free()
    aba(pctx, a, b)


def test_taxscreen(pctx):
    """the LCA fold by a wave (a list at the cut) and by one lane, tallies and clade sums"""
    import fpmash
    cut = pctx.tax_wave_cut()
    rng = np.random.default_rng(cut)
    nodes = TT.tree_forest()
    genus = [1002, 1503, 1504, 1505]
    pick = [int(x) for x in rng.choice(genus, size=cut + 8)] + \
        [int(x) for x in rng.choice(list(nodes), size=len(TT.REAL) - cut - 8)]
    ref_taxids = TT.ref_taxids_over(nodes, rng, pick)
    under_one = TT.REAL[:cut + 8]
    short = [[int(x) for x in rng.choice(TT.REAL, size=n, replace=False)]
             for n in (1, 2, cut - 2, cut - 1)] + [under_one[:cut - 1]]
    counts = TT.counts_for(rng, len(short))
    long_ = short + [under_one[:cut], under_one[:cut + 1]]
    aba(pctx, lambda: TT.run_case(pctx, nodes, ref_taxids, long_, counts + [2, 0],
                                  kernel=fpmash.TK_WAVE),
        lambda: TT.run_case(pctx, nodes, ref_taxids, short, counts, kernel=fpmash.TK_THREAD))


# ---- kfinger, positional grid, p-values --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _kf_models():
    """(sequences, window, model) of the four k-finger cases, built once"""
    seqs = [TK.rand(81 + i, n) for i, n in enumerate(TK.length_pattern(100))]
    small = [TK.rand(91, 30), b"acgtn", TK.rand(92, 101)]
    wide, narrow = TKF.LDSW + 1, 100
    sw, sn = KF.window_seqs(wide, TKF.R), KF.window_seqs(narrow, TKF.R)
    return {"cflA": (seqs, 100, TK.M.Model(seqs, TK.default_ids(len(seqs)), 100, None)),
            "cflB": (small, 17, TK.M.Model(small, TK.default_ids(len(small)), 17, None)),
            "icflA": (sw, wide, KF.Model(sw, KF.default_ids(len(sw)), wide, "ICFL", None)),
            "icflB": (sn, narrow, KF.Model(sn, KF.default_ids(len(sn)), narrow, "ICFL", None))}


def test_kfinger_cfl(pctx, oracle):
    def case(name):
        seqs, w, m = _kf_models()[name]
        return lambda: TK.check(pctx, oracle, seqs, w, model=m)
    aba(pctx, case("cflA"), case("cflB"))


def test_kfinger_icfl(pctx, oracle):
    """ICFL at a window whose working memory is a pooled device buffer, then one inside LDS"""
    def case(name):
        seqs, w, m = _kf_models()[name]
        assert (w > TKF.LDSW) == (name == "icflA")
        return lambda: TKF.check(pctx, oracle, seqs, w, "ICFL", model=m)
    aba(pctx, case("icflA"), case("icflB"))


def test_positional_grid(pctx, oracle):
    rng = np.random.default_rng(82)

    def case(n_lists, hi):
        lists = [rng.integers(0, 20, size=int(rng.integers(0, hi))).astype(np.uint32)
                 for _ in range(n_lists)]

        def run():
            got = pctx.positional(lists, lists, max_dist=0.9, max_pvalue=0.5)
            for q, b in enumerate(lists):
                for r, a in enumerate(lists):
                    m, mn, dv, pv = oracle.positional(a, b)
                    c = q * len(lists) + r
                    assert got["numer"][c] == m and got["denom"][c] == mn
                    if mn:
                        assert got["distance"][c] == pytest.approx(dv, rel=RTOL, abs=0)
                    else:
                        assert np.isnan(got["distance"][c])
                    assert got["pvalue"][c] == pytest.approx(pv, rel=RTOL, abs=0)
                    assert got["pass"][c] == (dv <= 0.9 and pv <= 0.5)
        return run
    aba(pctx, case(9, 60), case(3, 5))


def test_pvalue_batch(pctx, oracle):
    rng = np.random.default_rng(83)

    def case(n, dt, k, space):
        denom = rng.integers(1, 2000, size=n).astype(np.uint32)
        numer = np.minimum(rng.integers(0, 2000, size=n), denom).astype(np.uint32)
        numer[:5] = 0
        numer[5:10] = denom[5:10]
        lr = rng.integers(1, 10 ** 9, size=n, dtype=np.uint64)
        lq = rng.integers(1, 10 ** 9, size=n, dtype=np.uint64)
        lr[10:15] = 21
        want_d = [oracle.distance(int(a), int(b), k) for a, b in zip(numer, denom)]
        want_p = [oracle.pvalue(int(a), int(x), int(y), space, int(b))
                  for a, b, x, y in zip(numer, denom, lr, lq)]

        def run():
            d, p = pctx.pvalue_batch(numer.astype(dt), denom.astype(dt), lr, lq, k=k,
                                     kmer_space=space)
            np.testing.assert_allclose(d, want_d, rtol=RTOL, atol=0)
            np.testing.assert_allclose(p, want_p, rtol=RTOL, atol=0)
        return run
    aba(pctx, case(700, np.uint32, 21, 4.0 ** 21), case(33, np.uint16, 1, 10.0))
