"""CPU checks of the device parser's model (tests/seqparse_model.py): the four-state machine and
the 4-line FASTQ rules read every input as kseq_read does (tests/seqio.py, and the reference's
compiled kseq.h where oracle/_ref is built), the range summaries the kernels fold compose
associatively over any split, and the inputs the GPU edge tests are built from hit the edges
they are named for."""
import os
import random

import numpy as np
import pytest

import seqio
import seqparse_model as M
from test_gpu_seqparse import EDGE, FASTQ_HOST, FASTQ_OK


def seqio_parse(data):
    try:
        return seqio.parse(data)
    except ValueError:
        return None


def test_machine_equals_seqio_on_random_strings():
    n = 0
    seen = set()
    for data in M.random_strings(1, 60000):
        recs = M.records(data)
        assert M.named(data, recs) == seqio.parse(data), data
        n += 1
        st = M.run(data)[0]
        seen.add(("end", st))
        if any(data[p] == 0xFF for p, _e, _s in recs):
            seen.add("0xff starts a record")
        if recs and recs[-1][0] == len(data) - 1:
            seen.add("marker is the last byte")
        if recs and recs[-1][1] is None:
            seen.add("ends inside a header")
    assert n >= 50000
    assert {("end", 0), ("end", 1), ("end", 2), ("end", 3), "0xff starts a record",
            "marker is the last byte", "ends inside a header"} <= seen


def test_model_on_the_named_cases():
    """EDGE / FASTQ_OK / FASTQ_HOST of test_gpu_seqparse.py: what the model says the device
    reports is kseq_read's records; the FASTQ_HOST cases (and only they) go to the host"""
    for data in EDGE + FASTQ_OK:
        assert M.device_parse(data) == (seqio.parse(data), False), data
    for data in EDGE:
        assert not M.run(data)[3]
    for data in FASTQ_OK + FASTQ_HOST:
        assert M.run(data)[3]
    for data in FASTQ_HOST:
        assert M.device_parse(data) == (None, True), data


def test_machine_equals_compiled_kseq(tmp_path):
    from oracle import oracle as O
    if O.ref() is None:
        pytest.skip("oracle/_ref (the reference's kseq.h) is not built")
    cases = list(M.random_strings(2, 300)) + EDGE
    for i, data in enumerate(cases):
        path = tmp_path / ("x%d.fa" % i)
        path.write_bytes(data)
        recs, st = O.ref_kseq_records(str(path))
        assert st == -1
        assert M.named(data, M.records(data)) == [(n, c, s) for n, c, s, _q in recs], data


def random_split(rng, data):
    """pieces of `data`: 16-byte and 4096-byte pieces among random ones (empty ones too)"""
    out, at = [], 0
    while at < len(data):
        n = rng.choice((0, 1, 2, 5, 16, 16, 16, 17, 64, 256, 1000, 4096, 4096, 4097))
        out.append(data[at:at + n])
        at += n
    return out


def long_strings(seed, count, lo, hi):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(M.ALPHABET + b"+ACGTACGTACGTACGTACGT\n", np.uint8)
    for _ in range(count):
        yield alpha[rng.integers(0, len(alpha), int(rng.integers(lo, hi)))].tobytes()


def test_summaries_fold_over_any_split():
    rng = random.Random(3)
    cases = list(M.random_strings(4, 3000, 80)) + list(long_strings(5, 12, 4096, 3 * 4096))
    sizes = set()
    for data in cases:
        whole = M.summary(data)
        assert whole == tuple(M.run(data, s) for s in range(4))
        for _ in range(2):
            pieces = random_split(rng, data)
            sizes |= {len(p) for p in pieces}
            assert M.fold(pieces) == whole, (data, pieces)
        # fixed pieces, as the kernels cut them: threads, then chunks
        assert M.fold([data[i:i + M.THREAD_BYTES] for i in range(0, len(data), M.THREAD_BYTES)]) \
            == whole
        assert M.fold([data[i:i + M.CHUNK] for i in range(0, len(data), M.CHUNK)]) == whole
        recs = M.records(data)
        assert whole[0][1:3] == (len(recs), sum(len(s) for _p, _e, s in recs))
    assert {0, 16, 4096} <= sizes


def test_compose_is_associative():
    xs = [M.summary(d) for d in M.random_strings(6, 400, 12)]
    rng = random.Random(7)
    for _ in range(3000):
        f, g, h = rng.choice(xs), rng.choice(xs), rng.choice(xs)
        assert M.compose(M.compose(f, g), h) == M.compose(f, M.compose(g, h))
        assert M.compose(M.identity(), f) == f == M.compose(f, M.identity())


def test_first_chunk_resets_every_state():
    rng = random.Random(8)
    for data in list(M.random_strings(9, 2000, 60)):
        cut = rng.randint(0, len(data))
        x = M.compose(M.reset(M.summary(data[:cut])), M.summary(data[cut:]))
        assert x == (M.run(data, M.S0),) * 4, data
    # a file behind one whose stream ended (S3), or that ended inside a header (S2)
    before = M.summary(b"\xff>a\nAC\n")
    assert before[0][0] == M.S3
    nxt = M.summary(b">b\nGG\n")
    assert M.compose(before, nxt)[0][1] == 0                    # without the reset: no record
    assert M.compose(before, M.reset(nxt))[0][1:3] == (1, 2)


def mutate(rng, text):
    b = bytearray(text)
    for _ in range(rng.randint(1, 3)):
        op = rng.randint(0, 2)
        i = rng.randint(0, len(b))
        c = rng.choice(b"@>+\n\n\r \xff\x7fAI")
        if op == 0:
            b.insert(i, c)
        elif op == 1 and i < len(b):
            b[i] = c
        elif i < len(b):
            del b[i]
    return bytes(b)


def test_fastq_four_line_rules():
    for data in FASTQ_OK:
        assert M.fastq_four_line(data) == seqio.parse(data)
    for data in FASTQ_HOST:
        assert M.fastq_four_line(data) is None
    rng = random.Random(10)
    base = [b"@r1 x\nACGT\n+\nII@I\n@r2\nGG\n+r2\n>I\n", b"@a\r\nAC\r\n+\r\nI\x7f\r\n@b\r\n\r\n+\r\n\r\n",
            b"@e\n\n+\n\n@f\nA C\n+\nI I"]
    accepted = rejected = 0
    for _ in range(6000):
        data = mutate(rng, rng.choice(base))
        got = M.fastq_four_line(data)
        if got is None:
            rejected += 1
            continue
        accepted += 1
        assert got == seqio_parse(data), data
    assert accepted > 500 and rejected > 500


def test_generated_fasta_inputs():
    """the FASTA inputs of the GPU edge tests: '+'-free, the model reads them as seqio does, and
    the events sit where their names say, in the state their names say"""
    cases = M.event_files()
    assert len(cases) == len(M.PRIORS) * len(M.EVENTS) * len(M.EVENT_OFFSETS)
    want = {"S0": M.S0, "S1": M.S1, "S2": M.S2, "S2ff": M.S2}
    for prior, ev, off, data in cases:
        assert data[off:off + len(ev)] == ev and data[off + len(ev):] == M.EVENT_TAIL
        assert M.run(data[:off])[0] == want[prior]
        got, quality = M.device_parse(data)
        assert not quality and got == seqio.parse(data)
        # a complete record behind the event, unless the event ended the stream
        ended = prior == "S0" and ev == b"\xff"
        assert (M.run(data)[0] == M.S3) == ended
        assert (got[-1:] == [(b"t2", b"", b"GG")]) != ended
    assert {d[15] for p, e, o, d in cases if o == 15} >= {62, 64, 10, 13, 0xFF, 32}
    for data in list(M.long_run_files().values()) + M.tiny_pool():
        assert M.device_parse(data) == (seqio.parse(data), False)
    runs = M.long_run_files()
    assert M.run(runs["stream ended"])[:2] == (M.S3, 0) and len(runs["stream ended"]) > 4.5 * M.CHUNK
    assert M.run(runs["long header"][:3 * M.CHUNK])[:2] == (M.S2, 1)
    assert M.run(runs["long preamble"][:2 * M.CHUNK])[:2] == (M.S0, 0)
    assert M.records(runs["ends in header"])[-1][1] is None
    assert [len(runs["ends in sequence %d" % n]) for n in (4095, 4096, 4097)] == [4095, 4096, 4097]


@pytest.mark.parametrize("n,per", [(1024, 1), (1025, 2), (2047, 2), (2048, 2), (2049, 3), (3073, 4)])
def test_partition_inputs_sit_on_the_scan_edges(n, per):
    files, spans = M.partition_files(n)
    assert M.n_chunks(files) == n and (n + M.SCAN_THREADS - 1) // M.SCAN_THREADS == per
    assert [c for _s, c in spans] == [5, 6, 7]
    states = []
    at = 0
    for f in files:
        c = M.n_chunks([f])
        if c > 1:
            assert (at, c) == spans[len(states)]
            # the file crosses a thread's range edge away from its first chunk: the state it
            # carries there is S1, S2 and S3 in turn
            edge = (at // per + 1) * per
            assert at < edge < at + c or per == 1
            states.append(M.run(f[:(edge - at) * M.CHUNK])[0])
        at += c
    assert states == [M.S1, M.S2, M.S3]
    assert [s % per for s, _c in spans] == [per - 1, 1 % per, per - 1]
    assert M.records(files[-1])
    for f in set(files):
        assert M.device_parse(f) == (seqio.parse(f), False)


def test_generated_fastq_inputs():
    lf, crlf = M.window_files()
    for data in (lf, crlf):
        got, quality = M.device_parse(data)
        assert not quality and got == seqio.parse(data)
        assert {len(s) for _n, _c, s in got} >= {0, 1, 63, 64, 65, 127, 128, 129}
    assert b"\n" not in crlf.replace(b"\r\n", b"")
    files, recs = M.scan_files()
    assert tuple(len(r) for r in recs) == M.SCAN_FILE_RECORDS
    for f, r in zip(files, recs):
        assert M.device_parse(f) == (r, False) and seqio.parse(f) == r
    # the large file's records are the generator's own: pinned on both of its ends
    data, names, seqs = M.big_fastq()
    n = M.BIG_FASTQ_RECORDS
    assert len(names) == n and (n + M.SCAN_BLOCK - 1) // M.SCAN_BLOCK > M.SUMS_ROUND
    lines = data.split(b"\n")
    assert len(lines) == 4 * n + 1
    head = b"\n".join(lines[:4 * 3000]) + b"\n"
    tail = b"\n".join(lines[4 * (n - 2000):])
    want = [(nm, b"", s) for nm, s in zip(names, seqs)]
    assert M.device_parse(head) == (want[:3000], False) and seqio.parse(head) == want[:3000]
    assert M.device_parse(tail) == (want[n - 2000:], False) and seqio.parse(tail) == want[n - 2000:]
    assert all(ln[:1] == b"@" and ln[1:] == nm for ln, nm in zip(lines[0::4], names))
    assert lines[1:4 * n:4] == seqs
