"""`fpmash screen` against tests/screen_model.py: stdout byte for byte the model's lines.

Fixture A is generated here from fixed seeds: six 20 kb genomes sketched and pasted with fpmash
into one .msh, and 100-base reads at about 5x from three of them in two FASTA files.  Fixture B
is the golden genome sketches against the golden gzipped FASTQ reads.  The model reads the .msh
with mshfmt, takes the pool's distinct keys and their counts from the oracle's counted sketch
(wider than the pool has windows, so never full and every count complete) and the thresholds as
the floats the option parser makes of them (stof, Command.cpp:73)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import mshfmt
import reads_model as RM
import screen_model as M
import seqio

FPMASH = os.path.join(ROOT, "fp-mash_amd", "bin", "fpmash")
SEED = 11


def run(args, cwd=None, check=True, env=None, stdin=None):
    p = subprocess.run([FPMASH, "screen"] + args, cwd=cwd, capture_output=True, input=stdin,
                       env=None if env is None else {**os.environ, **env})
    if check and p.returncode != 0:
        raise AssertionError(f"fpmash screen {args} failed: {p.stderr.decode()}")
    return p


def fasta(recs, prefix):
    return b"".join(b">%s%d read %d\n%s\n" % (prefix, i, i, r) for i, r in enumerate(recs))


def fixture_a(seed=SEED):
    """-> (genomes, read files).  g1 and g2 share half their sequence, g4 carries 90 bases of
    g0, g5 is unrelated; the reads come from g0, g1 and g3 with 1 % substitutions."""
    rng = np.random.default_rng(seed)
    g = [RM._rand(rng, 20000) for _ in range(6)]
    g[2] = g[1][:10000] + g[2][10000:]
    g[4] = g[4][:5000] + g[0][7000:7090] + g[4][5090:]
    files = [[], []]
    for n, src in enumerate((0, 1, 3)):
        for i in range(1000):
            at = int(rng.integers(0, 20000 - 100))
            files[(n + i) % 2].append(RM.mutate(rng, g[src][at:at + 100], 0.01))
    return g, files


def pool_counts(oracle, recs, k):
    """every distinct window key of the records, ascending, with its number of windows"""
    n = max(1, sum(len(r) for r in recs))
    h, c = oracle.sketch_batch(oracle.params(k=k, s=n), recs, groups=[0] * len(recs), n_groups=1,
                               counts=True)
    return h[0], c[0]


def load_db(path):
    h = mshfmt.read_msh(path)
    s = h["sketchSize"]
    refs = h["references"]
    use64 = refs[0]["hashes64"] is not None
    rows = [(r["hashes64"] if use64 else r["hashes32"])[:s].astype(np.uint64) for r in refs]
    return dict(rows=rows, names=[r["name"].decode() for r in refs],
                comments=[r["comment"].decode() for r in refs],
                lengths=[int(r["length"]) for r in refs], k=h["kmer"], s=s, use64=use64)


def model(oracle, db, recs, winner=False, identity_min=0.0, pvalue_max=1.0):
    keys, kc = pool_counts(oracle, recs, db["k"])
    U = np.unique(np.concatenate(db["rows"]))
    cnt = np.zeros(len(U), np.uint32)
    at = np.searchsorted(keys, U)
    hit = at < len(keys)
    hit[hit] = keys[at[hit]] == U[hit]
    cnt[hit] = kc[at[hit]]
    shared, median = M.closed(db["rows"], None, db["k"], winner, db["lengths"], counts=(U, cnt))
    setsize = RM.set_size(keys[:db["s"]], db["use64"])
    text = M.lines(oracle, db["rows"], db["names"], db["comments"], shared, median, setsize,
                   db["k"], 4.0 ** db["k"], float(np.float32(identity_min)),
                   float(np.float32(pvalue_max)))
    return text, shared, median


def between_pvalues(text):
    """a threshold, as the text given to -v, strictly between two printed p-values"""
    ps = sorted({float(l.split("\t")[3]) for l in text.splitlines()})
    assert len(ps) >= 2, ps
    lo, hi = ps[-2], ps[-1]
    v = (lo * hi) ** 0.5 if lo > 0 else hi / 10
    arg = "%.3g" % v
    assert lo < float(np.float32(float(arg))) < hi and float(np.float32(float(arg))) > 0
    return arg


@pytest.fixture(scope="module")
def fix_a(tmp_path_factory):
    from test_cli import run as fpmash
    d = tmp_path_factory.mktemp("screen_a")
    g, files = fixture_a()
    for i, s in enumerate(g):
        (d / f"g{i}.fa").write_bytes(b">g%d genome %d\n%s\n" % (i, i, s))
    fpmash(["sketch", "-o", "a", "g0.fa", "g1.fa", "g2.fa"], cwd=d)
    fpmash(["sketch", "-o", "b", "g3.fa", "g4.fa", "g5.fa"], cwd=d)
    fpmash(["paste", "db", "a.msh", "b.msh"], cwd=d)
    (d / "r1.fa").write_bytes(fasta(files[0], b"x"))
    (d / "r2.fa").write_bytes(fasta(files[1], b"y"))
    (d / "r12.fa").write_bytes(fasta(files[0], b"x") + fasta(files[1], b"y"))
    return d, load_db(str(d / "db.msh")), files[0] + files[1]


@pytest.mark.gpu
def test_fixture_a_is_not_vacuous(oracle, fix_a):
    d, db, recs = fix_a
    assert [len(r) for r in db["rows"]] == [1000] * 6
    text, shared, median = model(oracle, db, recs)
    assert text.count("\n") >= 3
    assert any(int(l.split("\t")[2]) >= 2 for l in text.splitlines())
    every, _, _ = model(oracle, db, recs, identity_min=-1.0)
    assert 0 in shared and every.count("\n") == 6 > text.count("\n")
    _, wshared, _ = model(oracle, db, recs, winner=True)
    assert wshared != shared


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default", "all", "i0.9", "v", "w", "w_all"])
def test_fixture_a(oracle, fix_a, case):
    d, db, recs = fix_a
    if case == "v":
        v = between_pvalues(model(oracle, db, recs)[0])
        args, kw = ["-v", v], dict(pvalue_max=float(v))
    else:
        args, kw = {"default": ([], {}), "all": (["-i", "-1"], dict(identity_min=-1.0)),
                    "i0.9": (["-i", "0.9"], dict(identity_min=0.9)),
                    "w": (["-w"], dict(winner=True)),
                    "w_all": (["-w", "-i", "-1"], dict(winner=True, identity_min=-1.0))}[case]
    exp = model(oracle, db, recs, **kw)[0]
    p = run(args + ["db.msh", "r1.fa", "r2.fa"], cwd=d)
    assert p.stdout.decode() == exp
    if case in ("v", "i0.9"):
        assert 0 < exp.count("\n") < model(oracle, db, recs)[0].count("\n")
    if case == "default":
        err = p.stderr.decode()
        assert "Loading db.msh...\n" in err and "Streaming from 2 inputs...\n" in err
        assert "   Estimated distinct k-mers in pool: " in err and "Writing output...\n" in err


@pytest.mark.gpu
def test_pool_files_concatenation_stdin_and_slices(oracle, fix_a):
    d, db, recs = fix_a
    exp = model(oracle, db, recs, identity_min=-1.0)[0]
    a = ["-i", "-1", "db.msh"]
    assert run(a + ["r1.fa", "r2.fa"], cwd=d).stdout.decode() == exp
    assert run(a + ["r12.fa"], cwd=d).stdout.decode() == exp
    assert run(a + ["r2.fa", "r1.fa"], cwd=d).stdout.decode() == exp
    assert run(a + ["-"], cwd=d, stdin=(d / "r12.fa").read_bytes()).stdout.decode() == exp
    assert run(a + ["-", "r2.fa"], cwd=d, stdin=(d / "r1.fa").read_bytes()).stdout.decode() == exp
    # slices of 20,000 bytes: the pool goes to the device in about ten parts
    p = run(a + ["r1.fa", "r2.fa"], cwd=d, env={"FPMASH_SCREEN_SLICE": "20000"})
    assert p.stdout.decode() == exp


@pytest.mark.gpu
@pytest.mark.parametrize("winner", [False, True])
def test_fixture_b_golden_fastq_gz(oracle, tmp_path, winner):
    from test_cli import run as fpmash
    msh = [os.path.join(GOLDEN, f"genome{i}.fna.msh") for i in (1, 2, 3)]
    fpmash(["paste", "db"] + msh, cwd=tmp_path)
    fq = [os.path.join(GOLDEN, f"reads{i}.fastq.gz") for i in (1, 2)]
    recs = [r[2] for f in fq for r in seqio.read_records(f)]
    db = load_db(str(tmp_path / "db.msh"))
    exp = model(oracle, db, recs, winner=winner, identity_min=-1.0)[0]
    assert exp.count("\n") == 3
    p = run((["-w"] if winner else []) + ["-i", "-1", "db.msh"] + fq, cwd=tmp_path)
    assert p.stdout.decode() == exp
    # the inflated text through the same path
    (tmp_path / "r.fq").write_bytes(b"".join(gzip.open(f).read() for f in fq))
    p = run((["-w"] if winner else []) + ["-i", "-1", "db.msh", "r.fq"], cwd=tmp_path)
    assert p.stdout.decode() == exp


# ---- refusals: one ERROR: line, exit 1, empty stdout -------------------------------------------
def refused(p, msg):
    assert p.returncode == 1 and p.stdout == b""
    lines = [l for l in p.stderr.decode().splitlines() if l.startswith("ERROR:")]
    assert lines == [msg], p.stderr.decode()


def test_first_argument_must_be_a_sketch():
    p = run(["genome1.fna", "reads1.fastq.gz"], cwd=GOLDEN, check=False)
    refused(p, "ERROR: genome1.fna does not look like a sketch (.msh)")


def test_protein_database(tmp_path):
    hdr = dict(kmer=9, windowSize=0, sketchSize=10, concatenated=False, noncanonical=True,
               preserveCase=False, error=0.0, seed=42, alphabet=b"ACDEFGHIKLMNPQRSTVWY")
    (tmp_path / "p.msh").write_bytes(mshfmt.write_msh(
        hdr, [dict(name=b"p", comment=b"", length=100, hashes=np.arange(1, 11, dtype=np.uint64))]))
    (tmp_path / "r.fa").write_bytes(b">r\nACGTACGTACGTACGTACGTACGT\n")
    p = run(["p.msh", "r.fa"], cwd=tmp_path, check=False)
    refused(p, "ERROR: p.msh is an amino acid sketch; translated screening is not supported")


def test_stdin_must_be_first():
    p = run(["genome1.fna.msh", "reads1.fastq.gz", "-"], cwd=GOLDEN, check=False)
    refused(p, "ERROR: '-' for stdin must be first query")


def test_unreadable_pool_file():
    p = run(["genome1.fna.msh", "reads1.fastq.gz", "no_such_file.fq"], cwd=GOLDEN, check=False)
    refused(p, "ERROR: could not open no_such_file.fq")


@pytest.mark.gpu
def test_database_rows_must_ascend():
    """DNA1-sketch.msh was made with -fp: unsorted lists with repeats"""
    p = run(["DNA1-sketch.msh", "test_sequence.fasta"], cwd=GOLDEN, check=False)
    assert p.returncode == 1 and p.stdout == b""
    lines = [l for l in p.stderr.decode().splitlines() if l.startswith("ERROR:")]
    assert len(lines) == 1 and lines[0].startswith(
        "ERROR: DNA1-sketch.msh: screen needs sketches whose hashes are in strictly ascending order")


@pytest.mark.gpu
def test_pool_without_records(tmp_path):
    (tmp_path / "empty.fa").write_bytes(b"\n\n")
    p = run([os.path.join(GOLDEN, "genome1.fna.msh"), "empty.fa"], cwd=tmp_path, check=False)
    refused(p, "ERROR: Did not find sequence records in inputs")
