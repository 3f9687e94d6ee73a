"""The kseq record rules: tests/seqio.py (the Python restatement the device parser was first
pinned to) against the reference's own kseq.h (kseq_read over gzopen, as Sketch.cpp:478-522
reads a file), on FASTA / FASTQ edge cases, random files and the fork's FASTQ fixtures.
kseq_read's results are recorded in tests/golden/kseq_records.json (written by
tests/golden/make_golden.py --kseq from kseq.h compiled into oracle/_ref), so the tests run
without oracle/_ref; where it is built, kseq_read runs too and must reproduce the recording.
CPU only."""
import functools
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import seqio
from conftest import GOLDEN

O = pytest.importorskip("oracle.oracle")

FASTA_EDGE = [
    b"",
    b">",
    b"\n\n>a\nACGT",
    b"preamble text\nmore ACGT\n>x desc\nACGT\nAC GT\n\nTTT>y\nGGG>z inline > marker\nCC",
    b">a\tcomment with tab\nACGT\r\nACGT\r\n>b\r\nAAAA",
    b">a b>c @d\nAC>GT\n@q hdr\nTTTT\n>\n>empty\n>last",
    b">only header",
    b">n\x00ul\nAC\x00GT\x80\xffAC\n",
]
FASTQ_EDGE = [
    b"@r1 x\nACGT\n+\nIIII\n@r2\nGGGG\n+r2\nII@I\n",           # '@' inside a quality line
    b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+\r\nII\r\n",  # CRLF
    b"@r1\nAC\nGT\n+\nII\nII\n@r2\nA\n+\nI\n",                 # multi-line records
    b"@r1\nACGT\n+\nII",                                       # truncated quality
    b"@r1\nACGT\n+",                                           # '+' line at EOF
    b"@e\n\n+\n\n@f\nA\n+\nI",                                 # empty sequence, no final '\n'
    b"@r1\nACGT\n+\nIIII@x\n>y\nAC\n",                         # quality longer than the bases
    b"@r1\nAC GT\n+\nI I I I\n",                               # spaces in both lines
]
FIXTURES = ["reads1.fastq.gz", "reads2.fastq.gz"]


def random_files():
    """30 seeded files, FASTA and FASTQ in turn, 1-29 records of 0-199 bases"""
    rng = np.random.default_rng(3)
    for t in range(30):
        out = bytearray()
        for i in range(int(rng.integers(1, 30))):
            L = int(rng.integers(0, 200))
            seq = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)].tobytes()
            if t % 2:
                q = bytes(rng.integers(33, 75, L).astype(np.uint8))
                out += b"@r%d c%d\n%s\n+\n%s\n" % (i, i, seq, q)
            else:
                out += b">r%d c%d\n" % (i, i)
                for j in range(0, len(seq), 60):
                    out += seq[j:j + 60] + b"\n"
        yield bytes(out)


def digest(recs):
    """SHA-256 of the records' (name, comment, sequence), each as 8-byte length + bytes: equal
    digests = equal record lists"""
    h = hashlib.sha256()
    for r in recs:
        for f in r[:3]:
            h.update(len(f).to_bytes(8, "little") + f)
    return h.hexdigest()


def record(recs, st, keep):
    """One entry of kseq_records.json from kseq_read's records and last return value; keep:
    store the records themselves (hex) beside their count and digest."""
    e = {"status": st, "n": len(recs), "digest": digest(recs),
         "qual_len_is_seq_len": all(len(q) == len(s) for _n, _c, s, q in recs)}
    if keep:
        e["records"] = [[f.hex() for f in r] for r in recs]
    return e


@functools.lru_cache(maxsize=None)
def _golden():
    return json.load(open(os.path.join(GOLDEN, "kseq_records.json")))


def _kseq(path, data):
    """The recording of kseq_read over the file image `data` (keyed by its SHA-256).  Where
    oracle/_ref is built, kseq_read runs over `path` (written from `data` when absent) and must
    reproduce the recording."""
    g = _golden()[hashlib.sha256(data).hexdigest()]
    if O.ref() is not None:
        if not os.path.exists(path):
            with open(path, "wb") as f:
                f.write(data)
        recs, st = O.ref_kseq_records(str(path))
        assert record(recs, st, "records" in g) == g
    return g


def _seqio(data):
    try:
        return [(n, c, s) for n, c, s in seqio.parse(data)], -1
    except ValueError:
        return None, -2


@pytest.mark.parametrize("data", FASTA_EDGE + FASTQ_EDGE)
def test_seqio_equals_compiled_kseq(tmp_path, data):
    g = _kseq(tmp_path / "x.fq", data)
    recs, st = [tuple(bytes.fromhex(f) for f in r) for r in g["records"]], g["status"]
    got, gst = _seqio(data)
    if st == -2:
        # truncated quality: kseq_read returns -2 (the records before it are read)
        assert gst == -2
        return
    assert got == [(n, c, s) for n, c, s, _q in recs]


def test_seqio_equals_compiled_kseq_random(tmp_path):
    for t, data in enumerate(random_files()):
        g = _kseq(tmp_path / f"x{t}.fq", data)
        assert g["status"] == -1
        got = _seqio(data)[0]
        assert got is not None and (len(got), digest(got)) == (g["n"], g["digest"])


@pytest.mark.parametrize("name", FIXTURES)
def test_fastq_fixtures_compiled_kseq(name):
    path = os.path.join(GOLDEN, name)
    g = _kseq(path, open(path, "rb").read())
    assert g["status"] == -1 and g["n"] == 1000
    got = seqio.read_records(path)
    assert (len(got), digest(got)) == (g["n"], g["digest"])
    assert g["qual_len_is_seq_len"]
    assert gzip.open(path).read().count(b"\n+") >= 1000
