"""`fpmash taxscreen` against tests/taxscreen_model.py: stdout byte for byte the model's report.

The genomes and reads are fixture A of tests/test_cli_screen.py (six 20 kb genomes, reads from
g0, g1 and g3; g1 and g2 share half their sequence, g4 carries 90 bases of g0).  The taxonomy,
written here in the NCBI dump format: species 30 and 31 in genus 20 and species 32 in genus 21,
both genera in family 10; species 40 in another family; g0 -> 30, g1 -> 31, g2 and g4 -> 32 by the
mapping file, g3 -> 40 only by its comment, g5 without a taxID.  So hashes g1 and g2 share land on
the family, g3's stand apart, and g5's only count in the denominator's database side.

The refusals need no device: they run on any host."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import mshfmt
import taxscreen_model as T
from test_cli_screen import fasta, fixture_a, load_db, pool_counts, refused

FPMASH = os.path.join(ROOT, "fp-mash_amd", "bin", "fpmash")

NODES = [(1, 1, "no rank"), (2, 1, "superkingdom"), (10, 2, "family"), (11, 2, "family"),
         (20, 10, "genus"), (21, 10, "genus"), (30, 20, "species"), (31, 20, "species"),
         (32, 21, "species"), (40, 11, "species")]
NAMES = [(1, "root", "", "scientific name"), (1, "all", "", "synonym"),
         (2, "Bacteria", "Bacteria <bacteria>", "scientific name"),
         (10, "Alphaceae", "", "scientific name"), (11, "Betaceae", "", "scientific name"),
         (20, "Alpha", "", "scientific name"), (21, "Gamma", "", "scientific name"),
         (30, "Alpha one", "", "scientific name"), (31, "Alpha two", "", "scientific name"),
         (32, "Gamma one", "", "scientific name"), (32, "G. one", "", "common name"),
         (40, "Beta lone", "", "scientific name")]
MAPPING = b"30\tg0.fa\n31\tg1.fa\n32 g2.fa\n32\tg4.fa\n77\tnot in the database\n"
# FASTA comments: g3's taxID is only here; g0's and g1's are overridden by the mapping file
COMMENTS = [b"taxid 30", b"strain x taxid 31 y", b"", b"isolate taxid 40", b"", b"no taxonomy"]


def nodes_dmp(rows):
    return "".join("%d\t|\t%d\t|\t%s\t|\tXX\t|\t0\t|\n" % r for r in rows).encode()


def names_dmp(rows):
    return "".join("%d\t|\t%s\t|\t%s\t|\t%s\t|\n" % r for r in rows).encode()


def write_taxonomy(d, nodes=NODES, names=NAMES):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "nodes.dmp"), "wb") as f:
        f.write(nodes_dmp(nodes))
    with open(os.path.join(d, "names.dmp"), "wb") as f:
        f.write(names_dmp(names))


def run(args, cwd=None, check=True, env=None, stdin=None):
    p = subprocess.run([FPMASH, "taxscreen"] + args, cwd=cwd, capture_output=True, input=stdin,
                       env=None if env is None else {**os.environ, **env})
    if check and p.returncode != 0:
        raise AssertionError(f"fpmash taxscreen {args} failed: {p.stderr.decode()}")
    return p


@pytest.fixture(scope="module")
def fix(tmp_path_factory):
    from test_cli import run as fpmash
    d = tmp_path_factory.mktemp("taxscreen")
    g, files = fixture_a()
    for i, s in enumerate(g):
        (d / f"g{i}.fa").write_bytes(b">g%d %s\n%s\n" % (i, COMMENTS[i], s))
    fpmash(["sketch", "-o", "a", "g0.fa", "g1.fa", "g2.fa"], cwd=d)
    fpmash(["sketch", "-o", "b", "g3.fa", "g4.fa", "g5.fa"], cwd=d)
    fpmash(["paste", "db", "a.msh", "b.msh"], cwd=d)
    (d / "r1.fa").write_bytes(fasta(files[0], b"x"))
    (d / "r2.fa").write_bytes(fasta(files[1], b"y"))
    (d / "r12.fa").write_bytes(fasta(files[0], b"x") + fasta(files[1], b"y"))
    write_taxonomy(str(d / "tax"))
    (d / "map.tsv").write_bytes(MAPPING)
    return d, load_db(str(d / "db.msh")), files[0] + files[1]


_MODEL = {}


def model(oracle, db, recs, mapping):
    """-> (report text, closed's arrays, taxIDs per reference); computed once per mapping"""
    key = mapping is not None
    if key not in _MODEL:
        nodes = T.parse_nodes(nodes_dmp(NODES))
        tax = T.Tax(nodes, T.parse_names(names_dmp(NAMES), nodes))
        keys, kc = pool_counts(oracle, recs, db["k"])
        U, holders = T.holders_of(db["rows"])
        cnt = np.zeros(len(U), np.uint32)
        at = np.searchsorted(keys, U)
        hit = at < len(keys)
        hit[hit] = keys[at[hit]] == U[hit]
        cnt[hit] = kc[at[hit]]
        ids = T.reference_taxids(db["names"], db["comments"],
                                 T.parse_mapping(mapping) if mapping is not None else None)
        r = T.closed(tax, [tax.node_of(t) for t in ids], holders, cnt)
        _MODEL[key] = (T.report(tax, r), r, ids)
    return _MODEL[key]


@pytest.mark.gpu
def test_fixture_is_not_vacuous(oracle, fix):
    d, db, recs = fix
    text, r, ids = model(oracle, db, recs, MAPPING)
    assert ids == [30, 31, 32, 40, 32, 0]
    assert model(oracle, db, recs, None)[2] == [30, 31, 0, 40, 0, 0]
    lines = text.splitlines()[1:]
    assert len(lines) >= 5
    indents = {len(l.split("\t")[7]) - len(l.split("\t")[7].lstrip(" ")) for l in lines}
    assert len(indents) > 2
    assert any(l.split("\t")[1] != l.split("\t")[2] for l in lines)
    # hashes on an inner node (the family, from g1 and g2's shared half) and hashes of no taxon
    assert any(l.split("\t")[5] == "family" and int(l.split("\t")[2]) > 0 for l in lines)
    assert r["total_hashes"] > int(r["clade_hashes"][0]) and text != model(oracle, db, recs, None)[0]


@pytest.mark.gpu
def test_report_with_mapping_file(oracle, fix):
    d, db, recs = fix
    exp = model(oracle, db, recs, MAPPING)[0]
    p = run(["-m", "map.tsv", "-t", "tax", "db.msh", "r1.fa", "r2.fa"], cwd=d)
    assert p.stdout.decode() == exp
    err = p.stderr.decode()
    want = ["Loading taxonomy files ...\n", "   10 distinct taxa\n", "Reading mapping file ...\n",
            "Could not find taxID for reference g5.fa in comment field or mapping file!\n",
            "Loading db.msh...\n", " distinct hashes.\n", "Streaming from 2 inputs...\n",
            "   Estimated distinct k-mers in pool: ", "Assigning LCA taxIDs to hashes ...\n",
            "Writing output...\n"]
    at = 0
    for w in want:
        at = err.find(w, at)
        assert at >= 0, (w, err)
    assert err.count("Could not find taxID") == 1
    # -i and -v are accepted and change nothing
    p = run(["-i", "0.9", "-v", "0.01", "-m", "map.tsv", "-t", "tax", "db.msh", "r12.fa"], cwd=d)
    assert p.stdout.decode() == exp


@pytest.mark.gpu
def test_report_with_comment_only_taxids(oracle, fix):
    d, db, recs = fix
    exp = model(oracle, db, recs, None)[0]
    p = run(["-t", "tax", "db.msh", "r1.fa", "r2.fa"], cwd=d)
    assert p.stdout.decode() == exp
    assert p.stderr.decode().count("Could not find taxID") == 3
    # -t defaults to the working directory
    assert run([str(d / "db.msh"), str(d / "r12.fa")], cwd=d / "tax").stdout.decode() == exp


@pytest.mark.gpu
def test_pool_order_stdin_and_slices(oracle, fix):
    d, db, recs = fix
    exp = model(oracle, db, recs, MAPPING)[0]
    a = ["-m", "map.tsv", "-t", "tax", "db.msh"]
    assert run(a + ["r2.fa", "r1.fa"], cwd=d).stdout.decode() == exp
    assert run(a + ["-"], cwd=d, stdin=(d / "r12.fa").read_bytes()).stdout.decode() == exp
    p = run(a + ["r1.fa", "r2.fa"], cwd=d, env={"FPMASH_SCREEN_SLICE": "20000"})
    assert p.stdout.decode() == exp


@pytest.mark.gpu
def test_pool_without_records(tmp_path):
    write_taxonomy(str(tmp_path))
    (tmp_path / "empty.fa").write_bytes(b"\n\n")
    p = run([os.path.join(GOLDEN, "genome1.fna.msh"), "empty.fa"], cwd=tmp_path, check=False)
    refused(p, "ERROR: Did not find sequence records in inputs")


# ---- refusals before any device work: one ERROR: line, exit 1, empty stdout ---------------------
MSH = os.path.join(GOLDEN, "genome1.fna.msh")
READS = os.path.join(GOLDEN, "reads1.fastq.gz")


def test_first_argument_must_be_a_sketch(tmp_path):
    write_taxonomy(str(tmp_path))
    p = run(["-t", str(tmp_path), "genome1.fna", "reads1.fastq.gz"], cwd=GOLDEN, check=False)
    refused(p, "ERROR: genome1.fna does not look like a sketch (.msh)")


@pytest.mark.parametrize("missing", ["names.dmp", "nodes.dmp", "both"])
def test_missing_dump_files(tmp_path, missing):
    write_taxonomy(str(tmp_path))
    for f in ("names.dmp", "nodes.dmp"):
        if missing in (f, "both"):
            os.remove(tmp_path / f)
    p = run(["-t", str(tmp_path), MSH, READS], cwd=tmp_path, check=False)
    refused(p, f"ERROR: Could not find a file names.dmp or nodes.dmp in directory {tmp_path}")
    if missing == "both":                         # the default directory is the working one
        p = run([MSH, READS], cwd=tmp_path, check=False)
        refused(p, "ERROR: Could not find a file names.dmp or nodes.dmp in directory .")


def test_unreadable_mapping_file(tmp_path):
    write_taxonomy(str(tmp_path))
    p = run(["-m", "no_such_map.tsv", MSH, READS], cwd=tmp_path, check=False)
    refused(p, "ERROR: unable to open mapping file no_such_map.tsv")


def test_protein_database(tmp_path):
    write_taxonomy(str(tmp_path))
    hdr = dict(kmer=9, windowSize=0, sketchSize=10, concatenated=False, noncanonical=True,
               preserveCase=False, error=0.0, seed=42, alphabet=b"ACDEFGHIKLMNPQRSTVWY")
    (tmp_path / "p.msh").write_bytes(mshfmt.write_msh(
        hdr, [dict(name=b"p", comment=b"", length=100, hashes=np.arange(1, 11, dtype=np.uint64))]))
    (tmp_path / "r.fa").write_bytes(b">r\nACGTACGTACGTACGTACGTACGT\n")
    p = run(["p.msh", "r.fa"], cwd=tmp_path, check=False)
    refused(p, "ERROR: p.msh is an amino acid sketch; translated screening is not supported")


def test_stdin_must_be_first(tmp_path):
    write_taxonomy(str(tmp_path))
    p = run([MSH, READS, "-"], cwd=tmp_path, check=False)
    refused(p, "ERROR: '-' for stdin must be first query")


def test_unreadable_pool_file(tmp_path):
    write_taxonomy(str(tmp_path))
    p = run([MSH, READS, "no_such_file.fq"], cwd=tmp_path, check=False)
    refused(p, "ERROR: could not open no_such_file.fq")


@pytest.mark.parametrize("nodes,who", [
    ([(1, 1, "no rank"), (5, 6, "genus"), (6, 5, "species")], 5),
    ([(1, 1, "no rank"), (4, 1, "family"), (5, 6, "genus"), (6, 7, "species"), (7, 5, "x"),
      (8, 7, "y")], 5)])
def test_parent_chain_without_a_root(tmp_path, nodes, who):
    write_taxonomy(str(tmp_path), nodes=nodes, names=[])
    p = run([MSH, READS], cwd=tmp_path, check=False)
    refused(p, f"ERROR: ./nodes.dmp: the parent chain of tax ID {who} never reaches a root")
    with pytest.raises(ValueError):
        T.Tax(T.parse_nodes(nodes_dmp(nodes)))
