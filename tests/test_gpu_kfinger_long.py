"""fpm_kfinger_stage_split / _stage_split_seq, fpm_kfinger_text of a split job and
fpm_kfinger_fact_text against tests/kfinger_long_model.py, exact: the two texts, the values per
piece, the piece hashes and the record -> first piece map.  Inputs are a few KB and are built in
kfinger_long_model, where tests/test_kfinger_long_model.py shows that the pack inputs sit on the
edges they are named for.  R is the run length (pieces per workgroup at most) and KMAX the widest
window and split, from fpm_kfinger_limits; STAGE = R + KMAX - 1 the bytes one descriptor packs."""
import ctypes as C

import numpy as np
import pytest

import fpmash
import kfinger_comb_model as K
import kfinger_fact_model as F
import kfinger_long_model as L
import kfinger_model as M

pytestmark = pytest.mark.gpu

KMAX, R = fpmash.kfinger_limits()
STAGE = R + KMAX - 1


def check(ctx, oracle, seqs, N, fact, ids=None, model=None):
    ids = L.long_ids(len(seqs)) if ids is None else ids
    m = model or L.Model(seqs, ids, N, fact)
    r = ctx.kfinger(seqs, split=N, ids=ids, values=True, text=True, fact_text=True,
                    factorization=fact)
    assert r["n_lines"] == len(m.vals)
    assert np.array_equal(r["rec_first_line"], m.rec_first_line)
    assert np.array_equal(r["n_vals"], m.n_vals)
    assert np.array_equal(r["val_off"], m.val_off)
    assert np.array_equal(r["vals"], m.flat)
    assert r["text"] == m.text
    assert r["fact_text"] == m.fact_text
    assert np.array_equal(r["hash"], m.hashes(oracle, 42, False))
    return m, r


@pytest.mark.parametrize("fact", ["CFL_ICFL-30", "ICFL_COMB"])
@pytest.mark.parametrize("empty_at", ["first", "middle", "last"])
@pytest.mark.parametrize("N", [1, 2, 150, 300])
def test_record_lengths_around_the_split(ctx, oracle, N, empty_at, fact):
    """records of 0, 1, N - 1, N, N + 1, 2N and 2N + 1 bytes in one job: one piece below the
    split, no empty trailing piece where N divides n, no line for the empty record"""
    seqs = L.edge_seqs(N, empty_at)
    m, r = check(ctx, oracle, seqs, N, fact)
    assert m.text.count(b"\n") == len(seqs) - 1
    e = [len(s) for s in seqs].index(0)
    assert r["rec_first_line"][e] == r["rec_first_line"][e + 1]


@pytest.mark.parametrize("fact", ["CFL", "ICFL"])
@pytest.mark.parametrize("N", [1, 7])
def test_pack_boundary(ctx, oracle, N, fact):
    """R + 1 pieces in one record, and a record whose pieces begin in one descriptor and end in
    the next"""
    check(ctx, oracle, L.pack_seqs(N, R, STAGE), N, fact)


@pytest.mark.parametrize("fact", ["CFL", "ICFL_COMB"])
@pytest.mark.parametrize("N", [150, 300])
def test_pieces_fill_and_overflow_one_stage(ctx, oracle, N, fact):
    check(ctx, oracle, L.stage_fill_seqs(N, STAGE), N, fact)


@pytest.mark.parametrize("fact", ["ICFL", "ICFL_COMB"])
@pytest.mark.parametrize("past", [0, 1])
def test_split_where_the_working_memory_leaves_lds(ctx, oracle, fact, past):
    N = K.lds_window(fact) + past
    seqs = [F.rand(81, 2 * N + 1), F.rand(82, 2 * N + 1)]
    _m, r = check(ctx, oracle, seqs, N, fact)
    assert (r["wide_groups"] > 0) == bool(past)


@pytest.mark.parametrize("fact", ["CFL", "CFL_ICFL-30", "ICFL_COMB"])
def test_widest_split(ctx, oracle, fact):
    m, _r = check(ctx, oracle, [F.rand(83, KMAX + 1)], KMAX, fact)
    assert [int(v.sum()) for v in m.vals] == [KMAX, 1]


@pytest.mark.parametrize("fact", L.FACTS)
@pytest.mark.parametrize("N", [7, 100])
def test_byte_rules(ctx, oracle, N, fact):
    """lower case, N, an IUPAC code, 0x24 and bytes >= 0x80: a-z fold, every other byte stays,
    and the factor text carries the folded bytes"""
    seqs = K.byte_rule_seqs()
    assert seqs[0] == K.BYTE_RULES
    m, _r = check(ctx, oracle, seqs, N, fact)
    assert b"\x80" in m.fact_text and b"$" in m.fact_text
    assert not any(0x61 <= c <= 0x7A for c in m.fact_text)


@pytest.fixture(scope="module")
def words():
    return L.long_words()


@pytest.mark.parametrize("fact", L.FACTS)
def test_words_are_lyn2vecs(ctx, words, fact):
    """the 200 words of long_words.json.gz as one job at N = 7: lyn2vec's own two lines each"""
    at = 1 + 2 * (words["splits"].index(7) * len(words["facts"]) + words["facts"].index(fact))
    seqs = [row[0].encode() for row in words["rows"]]
    r = ctx.kfinger(seqs, split=7, ids=[b"w"] * len(seqs), text=True, fact_text=True,
                    factorization=fact)
    assert r["text"] == "".join(row[at] for row in words["rows"]).encode()
    assert r["fact_text"] == "".join(row[at + 1] for row in words["rows"]).encode()


# ---- the factor text of window jobs ----------------------------------------------------------

def check_window(ctx, seqs, w, fact, model=None):
    ids = F.default_ids(len(seqs))
    r = ctx.kfinger(seqs, window=w, ids=ids, text=True, fact_text=True, factorization=fact)
    assert r["fact_text"] == L.fact_text(seqs, ids, w, fact)
    assert r["text"] == (model or F.Model(seqs, ids, w, fact)).text
    return r


@pytest.mark.parametrize("fact", ["CFL", "ICFL", "CFL_ICFL_COMB-10"])
def test_window_fact_text(ctx, fact):
    """a record shorter than the window, one of exactly the window, one spanning two runs, an
    empty one, and short records sharing a pack"""
    w = 100
    seqs = [F.rand(91, w - 1), F.rand(92, w), b"", F.rand(93, R + 40), F.rand(94, 3), F.rand(95, 1)]
    r = check_window(ctx, seqs, w, fact)
    assert r["n_lines"] == 1 + w + R + 40 + 2


@pytest.mark.parametrize("fact", ["CFL", "ICFL_COMB"])
def test_window_fact_text_at_window_1(ctx, fact):
    seqs = [F.rand(96, R + 3), b"a"]
    r = check_window(ctx, seqs, 1, fact)
    assert r["fact_text"].startswith(b"G00000_0 " + seqs[0][:1] + b"\n")


@pytest.mark.parametrize("fact", ["ICFL", "ICFL_COMB"])
@pytest.mark.parametrize("past", [0, 1])
def test_window_fact_text_at_the_lds_edge(ctx, fact, past):
    w = K.lds_window(fact) + past
    seqs = [F.rand(97, w + 5), F.rand(98, w - 1)]
    r = check_window(ctx, seqs, w, fact)
    assert (r["wide_groups"] > 0) == bool(past)


def test_window_fact_text_with_folded_bytes(ctx):
    check_window(ctx, K.byte_rule_seqs(), 100, "CFL_COMB")


# ---- the device parse ------------------------------------------------------------------------

@pytest.mark.parametrize("fact", ["CFL", "ICFL_COMB"])
def test_stage_split_seq_equals_the_host_path(ctx, oracle, fact):
    """a FASTA image parsed on the device, with a take mask: the ID is the record's name"""
    N = 150
    recs = [(b"T%d G%d rest" % (i, i), F.rand(30 + i, n)) for i, n in enumerate([2 * N + 1, 7, N, 99])]
    take = [1, 0, 1, 1]
    image = b"".join(b">" + h + b"\n" + b"".join(s[o:o + 60] + b"\n" for o in range(0, len(s), 60))
                     for h, s in recs)
    ids = [h.split()[0] for h, _ in recs]
    kept = [s if t else b"" for (_, s), t in zip(recs, take)]
    m = L.Model(kept, ids, N, fact)
    d = ctx.kfinger_fasta([image], take=take, split=N, values=True, text=True, fact_text=True,
                          factorization=fact)
    h = ctx.kfinger(kept, split=N, ids=ids, values=True, text=True, fact_text=True,
                    factorization=fact)
    for r in (d, h):
        assert r["text"] == m.text and r["fact_text"] == m.fact_text
        assert np.array_equal(r["vals"], m.flat)
        assert np.array_equal(r["rec_first_line"], m.rec_first_line)
        assert np.array_equal(r["hash"], m.hashes(oracle, 42, False))
    assert m.text.startswith(b"T0  ") and b"G0" not in m.text


def test_jobs_without_pieces(ctx):
    for seqs in ([], [b"", b""]):
        r = ctx.kfinger(seqs, split=5, ids=L.long_ids(len(seqs)), values=True, text=True,
                        fact_text=True, factorization="ICFL_COMB")
        assert r["n_lines"] == 0 and r["text"] == b"" and r["fact_text"] == b""
        assert r["rec_first_line"].tolist() == [0] * (len(seqs) + 1)
    d = ctx.kfinger_fasta([b">a b\nACGTACGT\n>c d\nTTGA\n"], take=[0, 0], split=3, text=True,
                          fact_text=True)
    assert d["n_lines"] == 0 and d["text"] == b"" and d["fact_text"] == b""


# ---- the C ABI calls themselves --------------------------------------------------------------

def test_error_codes(ctx):
    lib = fpmash.lib()
    OK, EINVAL = fpmash.FPM_OK, fpmash.FPM_EINVAL
    seqs = [b"ACGTTGCAACG", b"", b"ACGTTGCAAC"]
    data, off = fpmash.pack_records(seqs)
    job, n = C.c_void_p(), C.c_uint64()
    for bad in (0, KMAX + 1, 0xFFFFFFFF):
        assert lib.fpm_kfinger_stage_split(ctx.h, data, fpmash._p(off, fpmash.u64p), 3, bad,
                                           C.byref(job), C.byref(n)) == EINVAL
        assert not job.value
    image = b">a\nACGT\n"
    seq_job, _recs, _q = ctx.seq_parse([image])
    try:
        for bad in (0, KMAX + 1):
            assert lib.fpm_kfinger_stage_split_seq(ctx.h, seq_job, None, bad, C.byref(job),
                                                   C.byref(n)) == EINVAL
            assert not job.value
    finally:
        lib.fpm_seq_free(seq_job)
    ids, id_off = fpmash.pack_records([b"r3", b"r2", b"r1"])
    idp = fpmash._p(id_off, fpmash.u64p)
    nb = C.c_uint64()
    for split, window in ((5, None), (None, 100)):
        if split:
            fpmash._check(lib.fpm_kfinger_stage_split(ctx.h, data, fpmash._p(off, fpmash.u64p), 3,
                                                      split, C.byref(job), C.byref(n)))
            assert n.value == 5
            want = L.long_fact_line(seqs[0], b"r3", 5, "CFL") + L.long_fact_line(seqs[2], b"r1", 5, "CFL")
            text = L.long_line(seqs[0], b"r3", 5, "CFL") + L.long_line(seqs[2], b"r1", 5, "CFL")
            assert want.startswith(b"r3  ACGTT | G C AAC | G | \n")
            assert text.startswith(b"r3  5 | 1 1 3 | 1 | \n")
        else:
            fpmash._check(lib.fpm_kfinger_stage(ctx.h, data, fpmash._p(off, fpmash.u64p), 3, window,
                                                0xFFFFFFFFFFFFFFFF, C.byref(job), C.byref(n)))
            want = L.fact_text(seqs, [b"r3", b"r2", b"r1"], window, "CFL")
            text = F.Model(seqs, [b"r3_0", b"r2_0", b"r1_0"], window, "CFL").text.replace(b"_0", b"")
        try:
            assert lib.fpm_kfinger_fact_text(job, ids, idp, None, 0, C.byref(nb)) == EINVAL
            fpmash._check(lib.fpm_kfinger_run(job, 42, 0, None))
            assert lib.fpm_kfinger_fact_text(job, ids, idp, None, 0, None) == EINVAL
            assert lib.fpm_kfinger_fact_text(job, None, idp, None, 0, C.byref(nb)) == EINVAL
            assert lib.fpm_kfinger_fact_text(job, ids, idp, None, 0, C.byref(nb)) == OK
            assert nb.value == len(want)
            out = np.full(len(want) + 1, 0x2A, np.uint8)
            nb.value = 0
            assert lib.fpm_kfinger_fact_text(job, ids, idp, out.ctypes.data, len(want) - 1,
                                             C.byref(nb)) == EINVAL
            assert nb.value == len(want) and out.tobytes() == b"*" * (len(want) + 1)
            # the k-finger text between the two factor-text calls takes the size pass over
            tb = C.c_uint64()
            assert lib.fpm_kfinger_text(job, ids, idp, None, 0, C.byref(tb)) == OK
            assert lib.fpm_kfinger_fact_text(job, ids, idp, out.ctypes.data, len(want),
                                             C.byref(nb)) == OK
            assert out.tobytes() == want + b"*"
            txt = np.zeros(tb.value, np.uint8)
            assert lib.fpm_kfinger_text(job, ids, idp, txt.ctypes.data, tb.value, C.byref(tb)) == OK
            assert txt.tobytes() == text
        finally:
            lib.fpm_kfinger_free(job)
    assert lib.fpm_kfinger_fact_text(None, ids, idp, None, 0, C.byref(nb)) == EINVAL


def test_binding_refuses_max_lines_with_split(ctx):
    with pytest.raises(ValueError):
        ctx.kfinger([b"ACGT"], split=2, max_lines=1)


# ---- over stale memory -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def pctx():
    """a context of this module's own with poison on (the shared `ctx` is left alone)"""
    c = fpmash.Context(0)
    c.set_poison(0x5A)
    yield c
    c.close()


def test_over_poisoned_memory(pctx, oracle):
    """a split job, poison, a differently shaped window job with its factor text, poison, the
    split job again: no output byte comes from stale memory"""
    N = K.lds_window("ICFL_COMB") + 1
    a = [F.rand(85, 2 * N + 1), b"", F.rand(86, N - 1), F.rand(87, 3 * N)]
    ma = L.Model(a, L.long_ids(len(a)), N, "ICFL_COMB")
    b = [F.rand(88, 130), F.rand(89, 7)]
    check(pctx, oracle, a, N, "ICFL_COMB", model=ma)
    pctx.poison_now()
    check_window(pctx, b, 61, "CFL_ICFL-10")
    pctx.poison_now()
    check(pctx, oracle, a, N, "ICFL_COMB", model=ma)
    check(pctx, oracle, L.edge_seqs(2, "middle"), 2, "CFL")
