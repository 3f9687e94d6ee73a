"""Reads mode of the host CLI (`fpmash sketch -r / -m / -g`, `fpmash dist -m`) against the
reference's own read-set sketch (tests/golden/reads.msh = `mash sketch -r -I reads reads1.fastq
reads2.fastq`), the oracle's counted sketches and tests/reads_model.py.
"""
import gzip
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN
import mshfmt
import reads_model as RM
import seqio
from test_cli import run

pytestmark = pytest.mark.gpu

FQ = ("reads1.fastq", "reads2.fastq")


@pytest.fixture(scope="module")
def reads_dir(tmp_path_factory):
    """The two read files, gzipped as shipped and inflated."""
    d = tmp_path_factory.mktemp("reads")
    for f in FQ:
        shutil.copy(os.path.join(GOLDEN, f + ".gz"), d / (f + ".gz"))
        (d / f).write_bytes(gzip.open(os.path.join(GOLDEN, f + ".gz")).read())
    return d


@pytest.fixture(scope="module")
def records():
    return [[r[2] for r in seqio.read_records(os.path.join(GOLDEN, f + ".gz"))] for f in FQ]


@pytest.fixture(scope="module")
def wide_counted(oracle, records):
    """Every distinct hash of the two files' records with its full count (an oracle sketch wider
    than the window count), computed once."""
    recs = RM.interleave(*records)
    n = sum(len(r) for r in recs)
    h, c = oracle.sketch_batch(oracle.params(k=21, s=n), recs, groups=[0] * len(recs), n_groups=1,
                               counts=True)
    return h[0], c[0]


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_sketch_reads_fixture_parity(reads_dir, suffix):
    exp_h = mshfmt.read_msh(os.path.join(GOLDEN, "reads.msh"))
    exp = exp_h["references"][0]
    out = f"out{len(suffix)}"
    p = run(["sketch", "-r", "-I", "reads", FQ[0] + suffix, FQ[1] + suffix, "-o", out],
            cwd=reads_dir)
    got_h = mshfmt.read_msh(str(reads_dir / (out + ".msh")))
    got = got_h["references"][0]
    assert len(got_h["references"]) == 1
    for key in ("kmer", "windowSize", "sketchSize", "concatenated", "noncanonical",
                "preserveCase", "error", "seed", "alphabet"):
        assert got_h[key] == exp_h[key], key
    assert np.array_equal(got["hashes64"], exp["hashes64"])
    assert np.array_equal(got["counts"], exp["counts"])
    assert got["length"] == exp["length"] == 502359
    assert got["name"] == exp["name"] == b"reads"
    # (reads.msh was made from CRLF files, whose '\r' kseq keeps in the comment; the shipped
    # .gz files have LF ends, as in test_cli.test_sketch_fastq_gz_hashes)
    assert got["comment"] == exp["comment"].replace(b"\r", b"")
    assert got["comment"].startswith(b"[2000 seqs] SRR7885321.1 1 length=302")
    err = p.stderr.decode()
    assert "Estimated genome size: 502359\n" in err
    cov = float(np.sum(exp["counts"], dtype=np.uint64)) / len(exp["counts"])
    assert f"Estimated coverage:    {cov:g}\n" in err


def test_sketch_min_copies_2(reads_dir, wide_counted):
    ah, ac = wide_counted
    keep = ac >= 2
    fh, fc = ah[keep][:1000], ac[keep][:1000]
    assert len(fh) == 1000
    run(["sketch", "-m", "2", "-o", "m2", FQ[0], FQ[1]], cwd=reads_dir)
    got = mshfmt.read_msh(str(reads_dir / "m2.msh"))["references"][0]
    assert np.array_equal(got["hashes64"], fh)
    assert np.array_equal(got["counts"][:-1], fc[:-1])
    assert 2 <= got["counts"][-1] <= fc[-1]
    assert got["length"] == RM.set_size(fh, use64=True)
    assert got["name"] == FQ[0].encode()


def test_sketch_fasta_reads(tmp_path, oracle):
    """FASTA read sets: two files of unequal length taken round-robin into one sketch (the
    longer file's tail follows once the shorter has ended), and one file alone (its records
    parsed and packed on the device)."""
    from fpmash import datagen
    reads = RM.base_reads()
    a, b = reads[:150], reads[150:]
    for name, part in (("a.fa", a), ("b.fa", b)):
        (tmp_path / name).write_bytes(datagen.fasta_bytes(part, [f"{name}{i}" for i in range(len(part))]))
    for files, recs, m, s in ((["a.fa", "b.fa"], RM.interleave(a, b), 2, 50),
                              (["b.fa", "a.fa"], RM.interleave(b, a), 3, 40),
                              (["a.fa"], a, 2, 50), (["a.fa"], a, 1, 50)):
        run(["sketch", "-r", "-m", str(m), "-s", str(s), "-o", "o"] + files, cwd=tmp_path)
        got = mshfmt.read_msh(str(tmp_path / "o.msh"))["references"][0]
        eh, ec = RM.model_sketch(RM.window_hashes(oracle, recs, 21), s, m)
        assert np.array_equal(got["hashes64"], eh)
        assert np.array_equal(got["counts"], ec)
        assert got["length"] == RM.set_size(eh)
        assert got["name"] == files[0].encode()
        assert got["comment"] == \
            f"[{len(recs)} seqs] T00000{files[0]}0 G00000{files[0]}0 [...]".encode()


def test_sketch_genome_size(reads_dir):
    p = run(["sketch", "-g", "5000000", "-o", "g5", FQ[0] + ".gz"], cwd=reads_dir)
    h = mshfmt.read_msh(str(reads_dir / "g5.msh"))
    assert h["references"][0]["length"] == 5000000
    assert h["references"][0]["counts"] is not None and len(h["references"][0]["counts"]) == 1000
    assert b"Estimated genome size: " in p.stderr


@pytest.mark.parametrize("args,msg", [
    (["-b", "1M"], b"-b (Bloom filter) and -c (target coverage) are not supported"),
    (["-c", "10"], b"-b (Bloom filter) and -c (target coverage) are not supported"),
    (["-r", "-i"], b"The option i cannot be used with r."),
    (["-m", "2", "-b", "1M"], b"The option m cannot be used with b."),
])
def test_rejected_combinations(reads_dir, args, msg):
    out = "rej" + "".join(a.strip("-") for a in args)
    p = run(["sketch"] + args + ["-o", out, FQ[0]], cwd=reads_dir, check=False)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not (reads_dir / (out + ".msh")).exists()


def test_dist_min_copies_query(reads_dir, oracle, records):
    """`dist -m 2 genome1.fna.msh reads1.fastq.gz`: the read file is sketched on its own with
    the min-copies heap; its length in the p-value is the set-size estimate."""
    ref = mshfmt.read_msh(os.path.join(GOLDEN, "genome1.fna.msh"))["references"][0]
    qh, _ = RM.model_sketch(RM.window_hashes(oracle, records[0], 21), 1000, 2)
    nu, de = oracle.compare(ref["hashes64"], qh, 1000, use64=True)
    d = oracle.distance(nu, de, 21)
    pv = oracle.pvalue(nu, ref["length"], RM.set_size(qh), 4.0 ** 21, de)
    out = run(["dist", "-m", "2", os.path.join(GOLDEN, "genome1.fna.msh"), FQ[0] + ".gz"],
              cwd=reads_dir).stdout.decode().splitlines()
    assert out == [f"{ref['name'].decode()}\t{FQ[0]}.gz\t{d:g}\t{pv:g}\t{nu}/{de}"]
