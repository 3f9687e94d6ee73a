"""Device buffers change hands between the handles of the C ABI (a parse's packed records go to
the sketch or k-finger job staged over them, a reads-mode job lends its records to its wide
jobs, a host-built RefSet / Screen takes its uploads, released -fp text buffers come back from
the context's pool).  Every sequence here is valid use per fpmash.h; each is run in both legal
free orders, or twice, and the results compared: who frees a buffer must not show in them."""
import ctypes as C

import numpy as np
import pytest

import fpmash

pytestmark = pytest.mark.gpu

S = 32
N_REC = 5


@pytest.fixture(scope="module")
def records():
    rng = np.random.default_rng(20)
    seqs = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n)))
            for n in rng.integers(200, 400, N_REC)]
    fasta = b"".join(b">r%d some text\n" % i + b"\n".join(s[o:o + 60] for o in range(0, len(s), 60))
                     + b"\n" for i, s in enumerate(seqs))
    return seqs, fasta


@pytest.fixture(scope="module")
def host_sketch(ctx, records):
    P = fpmash.make_params(k=15, s=S)
    return P, ctx.sketch(P, records[0])


@pytest.mark.parametrize("parse_first", [True, False])
def test_parse_then_sketch_free_orders(ctx, records, host_sketch, parse_first):
    P, want = host_sketch
    seq_job, recs, quality = ctx.seq_parse([records[1]])
    assert not quality and len(recs["seg"]) == N_REC
    job = ctx.sketch_seq_job(P, seq_job, np.arange(N_REC), N_REC)
    if parse_first:
        ctx.seq_free(seq_job)   # the job took over the packed records
    job.run()
    rows, cnt = job.fetch()
    job.free()
    if not parse_first:
        ctx.seq_free(seq_job)
    assert len(cnt) == N_REC
    for i in range(N_REC):
        assert np.array_equal(rows[i, :cnt[i]], want[i])


@pytest.fixture(scope="module")
def host_kfinger(ctx, records):
    ids = [fpmash.kfinger_id(b"r%d some text" % i) for i in range(N_REC)]
    return ids, ctx.kfinger(records[0], window=50, ids=ids, values=True, text=True)


def _same_kfinger(got, want):
    assert got["n_lines"] == want["n_lines"] and got["text"] == want["text"]
    for key in ("rec_first_line", "hash", "n_vals", "val_off", "vals"):
        assert np.array_equal(got[key], want[key]), key


def test_parse_then_kfinger_parse_freed_first(ctx, records, host_kfinger):
    # kfinger_fasta frees the parse handle once the job is staged, before the job runs
    _same_kfinger(ctx.kfinger_fasta([records[1]], window=50, values=True, text=True), host_kfinger[1])


def test_parse_then_kfinger_job_freed_first(ctx, records, host_kfinger):
    ids, want = host_kfinger
    seq_job, recs, _ = ctx.seq_parse([records[1]])
    try:
        job, n = C.c_void_p(), C.c_uint64()
        fpmash._check(fpmash.lib().fpm_kfinger_stage_seq(ctx.h, seq_job, None, 50, 2 ** 64 - 1,
                                                         C.byref(job), C.byref(n)))
        # runs, fetches and frees the job
        got = ctx._kfinger_out(job, n.value, N_REC, 42, False, ids, True, True)
    finally:
        ctx.seq_free(seq_job)
    _same_kfinger(got, want)


def test_reads_mode_twice(ctx, records):
    # every k-mer of a record twice: min_copies 2 keeps them, and the windows of a record
    # outnumber s, so each run stages wide jobs over the staged job's records
    seqs = [s + s for s in records[0]]
    P = fpmash.make_params(k=15, s=S)
    runs = []
    for _ in range(2):
        job = ctx.sketch_job(P, seqs, min_copies=2)
        try:
            job.run_reads()
            runs.append(job.fetch_reads() + (job.reads_rounds()[0],))
        finally:
            job.free()
    assert runs[0][4] >= 1 and int(runs[0][1].min()) > 0
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)


def test_refset_from_host_rows_twice(ctx, host_sketch):
    rows = host_sketch[1]
    lengths = [1000] * N_REC
    out = []
    for _ in range(2):
        rs = ctx.refset(rows, S, ref_lengths=lengths)
        try:
            out.append(rs.dist(rows, k=15, qry_lengths=lengths))
        finally:
            rs.free()
    assert int(out[0]["numer"].max()) == S
    for key in out[0]:
        assert np.array_equal(out[0][key], out[1][key]), key


@pytest.mark.parametrize("n_db", [0, 1])
def test_screen_without_cells_twice(ctx, n_db):
    # no row, and one empty row: the table build's minimum sizes
    out = []
    for _ in range(2):
        sc = fpmash.Screen(ctx, np.zeros((n_db, 4), np.uint64), np.zeros(n_db, np.uint32), S)
        try:
            out.append(sc.rows() + sc.counts())
        finally:
            sc.free()
    assert all(len(a) == n for a, n in zip(out[0], (n_db, n_db, 0, 0)))
    assert not out[0][0].any()   # nothing is shared with an empty row
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_fp_text_pooled_reuse(ctx, oracle):
    text = b"T1 8 34 57 1\nT1 5 2 34 59\n\nT2\t1 1 1 1 2 34 60\r\nT2 +3 -4 x 9"
    first, second = ctx.fp_text(text), ctx.fp_text(text)   # the second gets the first's buffers
    _ids, vals, _used = oracle.fp_parse(text)
    assert [int(x) for x in first["hash"]] == [oracle.get_hash_fp(v, 42, False) for v in vals]
    for key in first:
        assert np.array_equal(first[key], second[key]), key
