"""`fpmash kfinger -F` against lyn2vec's own lines for the first three records of DNA1.fasta
(tests/golden/DNA1-ICFL.txt.gz, DNA1-CFL_ICFL-10.txt.gz), against tests/kfinger_fact_model.py
for the whole file, and with -S against the .msh `sketch -fp` writes for the text."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
import kfinger_fact_model as F
import kfinger_model as M
import seqio

pytestmark = pytest.mark.gpu

FPMASH = os.path.join(ROOT, "fp-mash_amd", "bin", "fpmash")
DNA1 = os.path.join(GOLDEN, "DNA1.fasta")


def run(args, cwd=None, check=True):
    p = subprocess.run([FPMASH] + args, cwd=cwd, capture_output=True)
    if check and p.returncode != 0:
        raise AssertionError(f"fpmash {args} failed: {p.stderr.decode()}")
    return p


@pytest.mark.parametrize("fact, name", [("ICFL", "DNA1-ICFL.txt"),
                                        ("CFL_ICFL-10", "DNA1-CFL_ICFL-10.txt")])
def test_text_is_lyn2vecs_and_the_models(tmp_path, fact, name):
    p = run(["kfinger", "-F", fact, "-o", "out", DNA1], cwd=tmp_path)
    assert p.stdout == b""
    text = (tmp_path / "out.txt").read_bytes()
    golden = F.golden(name)
    assert golden and text[:len(golden)] == golden
    recs = seqio.read_records(DNA1)
    # the golden text ends where the fourth record's lines begin
    assert golden.count(b"\n") == sum(len(s) for _, _, s in recs[:3])
    m = F.Model([s for _, _, s in recs], [M.line_id(n + b" " + c) for n, c, _ in recs], 100, fact,
                fast=True)
    assert text == m.text
    assert sorted(os.listdir(tmp_path)) == ["out.txt"]


@pytest.mark.parametrize("fact", ["ICFL", "CFL_ICFL-10"])
def test_sketch_is_sketch_fp_of_the_text(tmp_path, fact):
    run(["kfinger", "-F", fact, "-o", "out", DNA1], cwd=tmp_path)
    p = run(["kfinger", "-S", "-F", fact, "-o", "a", DNA1], cwd=tmp_path)
    assert p.stdout == b""
    run(["sketch", "-fp", "-o", "b", "out.txt"], cwd=tmp_path)
    assert (tmp_path / "a.msh").read_bytes() == (tmp_path / "b.msh").read_bytes()
    assert not (tmp_path / "a.txt").exists()
    # the sketch options reach the .msh as they do through sketch -fp
    run(["kfinger", "-S", "-F", fact, "-s", "50", "-seed", "7", "-o", "c", DNA1], cwd=tmp_path)
    run(["sketch", "-fp", "-s", "50", "-S", "7", "-o", "d", "out.txt"], cwd=tmp_path)
    assert (tmp_path / "c.msh").read_bytes() == (tmp_path / "d.msh").read_bytes()


def test_cfl_is_the_default(tmp_path):
    run(["kfinger", "-o", "plain", DNA1], cwd=tmp_path)
    run(["kfinger", "-F", "CFL", "-o", "named", DNA1], cwd=tmp_path)
    plain = (tmp_path / "plain.txt").read_bytes()
    assert plain == (tmp_path / "named.txt").read_bytes()
    assert plain == open(os.path.join(GOLDEN, "DNA1-CFL.txt"), "rb").read()
    run(["kfinger", "-S", "-o", "plain", DNA1], cwd=tmp_path)
    run(["kfinger", "-S", "-F", "CFL", "-o", "named", DNA1], cwd=tmp_path)
    assert (tmp_path / "plain.msh").read_bytes() == (tmp_path / "named.msh").read_bytes()


def test_window_and_threshold_off_the_defaults(tmp_path):
    """-w with -F, a threshold that is none of lyn2vec's three, a window past the LDS bound, and
    the host walk in small slices"""
    recs = [(b"T%d G%d" % (i, i), F.rand(40 + i, n)) for i, n in enumerate([300, 16, 17, 260])]
    fa = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    (tmp_path / "a.fa").write_bytes(fa)
    ids = [M.line_id(h) for h, _ in recs]
    for w, fact in ((17, "CFL_ICFL-7"), (200, "ICFL")):
        run(["kfinger", "-w", str(w), "-F", fact, "-o", "o", "a.fa"], cwd=tmp_path)
        assert (tmp_path / "o.txt").read_bytes() == F.Model([s for _, s in recs], ids, w, fact).text
    p = subprocess.run([FPMASH, "kfinger", "-w", "17", "-F", "CFL_ICFL-7", "-o", "sl", "a.fa"],
                       cwd=tmp_path, capture_output=True,
                       env={**os.environ, "FPMASH_KFINGER_SLICE": "150"})
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "sl.txt").read_bytes() == \
        F.Model([s for _, s in recs], ids, 17, "CFL_ICFL-7").text


@pytest.mark.parametrize("w", ["100", "200"])
def test_records_without_a_base(tmp_path, w):
    """records with empty sequences make a job without lines: an empty text, as under CFL, also
    past the window where a job with lines takes a working buffer"""
    (tmp_path / "e.fa").write_bytes(b">a b\n\n>c d\n\n")
    for fact in ("CFL", "ICFL", "CFL_ICFL-10"):
        run(["kfinger", "-w", w, "-F", fact, "-o", "out", "e.fa"], cwd=tmp_path)
        assert (tmp_path / "out.txt").read_bytes() == b""


@pytest.mark.parametrize("fact", ["FOO", "CFL_ICFL-0", "CFL_ICFL-"])
def test_unknown_factorization(tmp_path, fact):
    p = run(["kfinger", "-F", fact, "-o", "out", DNA1], cwd=tmp_path, check=False)
    assert p.returncode == 1 and p.stdout == b""
    err = p.stderr.decode().strip().split("\n")
    assert len(err) == 1 and err[0].startswith("ERROR:")
    assert os.listdir(tmp_path) == []
