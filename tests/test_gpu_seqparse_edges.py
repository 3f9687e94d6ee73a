"""The device FASTA / FASTQ parser (csrc/seqparse.hip, fpm_seq_parse) at its chunk, scan and
window edges.  Every comparison is exact and per record: file, name, comment, sequence length,
the packed bytes themselves (fpm_seq_packed) and the 0x00 behind them, against kseq_read over
each file (the reference's kseq.h compiled into oracle/_ref, else tests/seqio.py).  The inputs
come from tests/seqparse_model.py, whose CPU tests (tests/test_seqparse_model.py) show that
they sit on the edges named here; each test asserts the counts that put it there again."""
import functools

import numpy as np
import pytest

import seqparse_model as M
from test_gpu_seqparse import kseq_records

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def expected_records(data):
    """[(name, comment, sequence)] of kseq_read over one file, by content"""
    recs = kseq_records(data)
    assert recs is not None
    return recs


def parse_all(ctx, files):
    """One fpm_seq_parse over `files` -> (records table, packed bytes, seq_off, quality flag),
    with the layout checked: n_bytes = the lengths' sum + the record count, record r at the
    lengths before it + r, one 0x00 behind every record."""
    job, rec, quality = ctx.seq_parse(files)
    try:
        n = len(rec["seq_len"])
        packed, off = ctx.seq_packed(job, n)
    finally:
        ctx.seq_free(job)
    lens = rec["seq_len"].astype(np.int64)
    assert len(packed) == int(lens.sum()) + n
    want_off = np.cumsum(lens) - lens + np.arange(n)
    assert np.array_equal(off.astype(np.int64), want_off)
    buf = np.frombuffer(packed, np.uint8)
    assert not buf[want_off + lens].any() if n else len(packed) == 0
    return rec, packed, off, quality


def records_by_file(files, rec, packed, off):
    """per file [(name, comment, packed sequence bytes)], dropping a marker that is a file's last
    byte (kseq_read's name read meets the end of the stream there; it has no sequence)"""
    out = [[] for _ in files]
    for r in range(len(rec["seq_len"])):
        f = int(rec["seg"][r])
        o, hl, n = int(rec["hdr_off"][r]), int(rec["hdr_len"][r]), int(rec["seq_len"][r])
        assert o + hl <= len(files[f])
        if o + 1 >= len(files[f]):
            assert n == 0
            continue
        a = int(off[r])
        out[f].append(M.split_header(files[f][o + 1:o + hl]) + (packed[a:a + n],))
    return out


def check_parse(ctx, files, expect=None):
    """the whole comparison of one parse; expect: per file records (default: kseq_read's)"""
    rec, packed, off, quality = parse_all(ctx, files)
    assert not quality
    got = records_by_file(files, rec, packed, off)
    for f, data in enumerate(files):
        want = expected_records(data) if expect is None else expect[f]
        assert got[f] == want, (f, data[:80])
    return rec, packed, off


def test_event_at_boundaries(ctx):
    """every (prior state, event) pair with the event's first byte at offsets 15..8192 of its
    file: thread (16 B), wave (1024 B) and chunk (4096 B) edges, one file per case in one
    parse; the files whose stream ended (0xff from S0) give no record and do not leak into the
    file behind them"""
    cases = M.event_files()
    assert len(cases) == 4 * 6 * 10
    files = [c[3] for c in cases]
    assert {(o % 16, o % 1024, o % 4096) for _p, _e, o, _d in cases} >= \
        {(15, 15, 15), (0, 16, 16), (15, 1023, 1023), (0, 0, 1024), (15, 1023, 4095), (0, 0, 0)}
    rec, _packed, _off = check_parse(ctx, files)
    n_by_file = np.bincount(rec["seg"], minlength=len(files))
    for i, (prior, ev, _off, _data) in enumerate(cases):
        assert (n_by_file[i] == 0) == (prior == "S0" and ev == b"\xff")


def test_runs_longer_than_a_chunk(ctx):
    runs = M.long_run_files()
    names, files = list(runs), list(runs.values())
    rec, _packed, _off = check_parse(ctx, files)
    n_by_file = dict(zip(names, np.bincount(rec["seg"], minlength=len(files))))
    assert n_by_file["stream ended"] == 0 and n_by_file["empty"] == 0
    assert n_by_file["after stream ended"] == 4
    assert n_by_file["long header"] == 2 and n_by_file["long record"] == 1
    # the header the file ends in is clamped to the file, not run into the padding
    f = names.index("ends in header")
    r = int(np.flatnonzero(rec["seg"] == f)[-1])
    assert int(rec["hdr_off"][r]) + int(rec["hdr_len"][r]) == len(files[f])
    assert files[f][int(rec["hdr_off"][r]):] == b">tail no newline"
    for n in (4095, 4096, 4097):
        assert n_by_file["ends in sequence %d" % n] == 1
        assert n_by_file["after ends in sequence %d" % n] == 1


@pytest.mark.parametrize("n,per", [(1024, 1), (1025, 2), (2047, 2), (2048, 2), (2049, 3), (3073, 4)])
def test_chunk_scan_partitions(ctx, n, per):
    """the chunk-level scan with 1..4 chunks per thread: multi-chunk files carrying S1, S2 and
    S3 across a thread's range edge, trailing threads with empty ranges (1025 chunks: threads
    513..1023), and the totals read from the last thread"""
    files, spans = M.partition_files(n)
    assert sum((len(f) + 1 + 4095) // 4096 for f in files) == n
    assert (n + 1023) // 1024 == per
    for start, chunks in spans:
        assert start // per != (start + chunks - 1) // per        # crosses a range edge
    assert [s % per for s, _c in spans] == [per - 1, 1 % per, per - 1]
    empty_threads = 1024 - (n + per - 1) // per
    assert empty_threads == {1024: 0, 1025: 511, 2047: 0, 2048: 0, 2049: 341, 3073: 255}[n]
    rec, _packed, _off = check_parse(ctx, files)
    assert int(rec["seg"][-1]) == len(files) - 1                  # the last file's records
    assert len(rec["seg"]) == sum(len(expected_records(f)) + (f == b">") for f in files)


def test_fastq_emit_windows(ctx):
    """sequence lines of 0..129 bytes, bare, with a trailing '\\r', with spaces and tabs at the
    64-byte window's edges, a non-base every third byte, 0x7f (a quality byte, not a base);
    '@', '>' and 0x7f among the counted quality bytes; one file CRLF throughout"""
    files = M.window_files()
    rec, _packed, _off = check_parse(ctx, files)
    lens = {int(x) for x in rec["seq_len"]}
    assert lens >= {0, 1, 63, 64, 65, 127, 128, 129}
    assert len(rec["seq_len"]) == 2 * (3 * len(M.WINDOW_LENGTHS) + 2)


def scans_block_edges(ctx):
    """FASTQ files of 1023, 1, 0, 1025, 2048 and 0 records in one parse: the 1024-record blocks
    of the record scan end inside files, and the record -> file search meets an empty file in
    the middle and at the end"""
    files, recs = M.scan_files()
    assert tuple(len(r) for r in recs) == (1023, 1, 0, 1025, 2048, 0)
    rec, _packed, _off = check_parse(ctx, files, expect=recs)
    assert np.array_equal(np.bincount(rec["seg"], minlength=6), [1023, 1, 0, 1025, 2048, 0])
    assert len({int(x) for x in rec["seq_len"]}) > 30             # irregular kept_at


def scans_two_carry_rounds(ctx):
    """one file of 263,145 minimal records: 257 block totals, so the carry loop of the totals'
    scan runs a second round.  The expectation is the generator's own (pinned by the model's CPU
    test); lengths, offsets and packed bytes are compared whole, names on a sample."""
    data, names, seqs = M.big_fastq()
    n = len(names)
    assert n == 263145 and (n + 1023) // 1024 == 257 > 256
    rec, packed, off, quality = parse_all(ctx, [data])
    assert not quality and len(rec["seq_len"]) == n
    assert np.array_equal(rec["seq_len"], [len(s) for s in seqs])
    assert packed == b"".join(s + b"\x00" for s in seqs)
    assert not rec["seg"].any()
    edge = 1024 * 256
    sample = sorted({0, 1, 1023, 1024, edge - 1, edge, edge + 1, n - 2, n - 1} |
                    {int(x) for x in np.random.default_rng(1).integers(0, n, 2000)})
    for r in sample:
        o, hl, a = int(rec["hdr_off"][r]), int(rec["hdr_len"][r]), int(off[r])
        assert data[o:o + 1] == b"@" and data[o + 1:o + hl] == names[r]
        assert packed[a:a + len(seqs[r]) + 1] == seqs[r] + b"\x00"


@pytest.mark.parametrize("part", [scans_block_edges, scans_two_carry_rounds],
                         ids=["block_edges", "two_carry_rounds"])
def test_fastq_record_scans(ctx, part):
    part(ctx)


def test_packed_accessor(ctx, oracle):
    import fpmash
    seq = M.bases(np.random.default_rng(2), 800)
    files = [b">a one\nAC GT\n>b\n\n>c\n" + seq + b"\n"]
    job, rec, quality = ctx.seq_parse(files)
    try:
        assert not quality and list(rec["seq_len"]) == [4, 0, len(seq)]
        want = b"ACGT\x00\x00" + seq + b"\x00"
        L = fpmash.lib()
        nb = fpmash.C.c_uint64()
        assert L.fpm_seq_packed(job, None, None, 0, fpmash.C.byref(nb)) == fpmash.FPM_OK
        assert nb.value == len(want)                              # the size query
        with pytest.raises(fpmash.FpmError) as e:
            ctx.seq_packed(job, 3, cap=len(want) - 1)             # one byte short
        assert e.value.code == fpmash.FPM_EINVAL
        first = ctx.seq_packed(job, 3)
        assert first[0] == want and list(first[1]) == [0, 5, 6]
        again = ctx.seq_packed(job)                               # the record count from the 0x00s
        assert again[0] == want and list(again[1]) == [0, 5, 6]
        groups = np.array([fpmash.NO_GROUP, fpmash.NO_GROUP, 0], np.uint32)
        got = ctx.sketch_seq(fpmash.make_params(k=21, s=100), job, groups, 1)
        exp = oracle.sketch_batch(oracle.params(k=21, s=100), [seq])
        assert len(got) == 1 and np.array_equal(got[0], exp[0])
        with pytest.raises(fpmash.FpmError) as e:                 # the sketch job took the records
            ctx.seq_packed(job, 3)
        assert e.value.code == fpmash.FPM_EINVAL
    finally:
        ctx.seq_free(job)
