"""`fpmash kfinger -F` with the combined factorizations against lyn2vec's own text: the fork's
training fingerprint of dna2.fasta under ICFL_COMB (tests/golden/dna2-ICFL_COMB.txt) and
lyn2vec's lines for the first three records of DNA1.fasta under CFL_COMB and CFL_ICFL_COMB-10
(tests/golden/KFINGER_COMB.md); with -S against the .msh `sketch -fp` writes for the text."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
import kfinger_fact_model as F
import seqio

pytestmark = pytest.mark.gpu

FPMASH = os.path.join(ROOT, "fp-mash_amd", "bin", "fpmash")
DNA1 = os.path.join(GOLDEN, "DNA1.fasta")
DNA2 = os.path.join(GOLDEN, "dna2.fasta")


def run(args, cwd=None, check=True):
    p = subprocess.run([FPMASH] + args, cwd=cwd, capture_output=True)
    if check and p.returncode != 0:
        raise AssertionError(f"fpmash {args} failed: {p.stderr.decode()}")
    return p


def test_icfl_comb_text_is_the_forks_training_fingerprint(tmp_path):
    p = run(["kfinger", "-F", "ICFL_COMB", "-o", "out", DNA2], cwd=tmp_path)
    assert p.stdout == b""
    with open(os.path.join(GOLDEN, "dna2-ICFL_COMB.txt"), "rb") as f:
        golden = f.read()
    assert len(golden) == 28943
    assert (tmp_path / "out.txt").read_bytes() == golden
    assert sorted(os.listdir(tmp_path)) == ["out.txt"]


@pytest.mark.parametrize("fact, name", [("CFL_COMB", "DNA1-CFL_COMB.txt"),
                                        ("CFL_ICFL_COMB-10", "DNA1-CFL_ICFL_COMB-10.txt")])
def test_text_is_lyn2vecs_on_dna1(tmp_path, fact, name):
    recs = seqio.read_records(DNA1)[:3]
    (tmp_path / "three.fa").write_bytes(
        b"".join(b">" + n + b" " + c + b"\n" + s + b"\n" for n, c, s in recs))
    run(["kfinger", "-F", fact, "-o", "out", "three.fa"], cwd=tmp_path)
    golden = F.golden(name)
    assert golden.count(b"\n") == sum(len(s) for _, _, s in recs)
    assert (tmp_path / "out.txt").read_bytes() == golden


def test_sketch_is_sketch_fp_of_the_text(tmp_path):
    run(["kfinger", "-F", "ICFL_COMB", "-o", "out", DNA2], cwd=tmp_path)
    p = run(["kfinger", "-S", "-F", "ICFL_COMB", "-o", "a", DNA2], cwd=tmp_path)
    assert p.stdout == b""
    run(["sketch", "-fp", "-o", "b", "out.txt"], cwd=tmp_path)
    assert (tmp_path / "a.msh").read_bytes() == (tmp_path / "b.msh").read_bytes()
    assert not (tmp_path / "a.txt").exists()


def test_window_and_slices(tmp_path):
    """-w with a combined form on either side of its LDS window, and the host walk in slices"""
    import fpmash
    import kfinger_comb_model as K
    import kfinger_model as M
    recs = [(b"T%d G%d" % (i, i), F.rand(40 + i, n)) for i, n in enumerate([300, 16, 17, 260])]
    (tmp_path / "a.fa").write_bytes(b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs))
    ids = [M.line_id(h) for h, _ in recs]
    lds = fpmash.kfinger_lds_window("ICFL_COMB")
    for w, fact in ((17, "CFL_ICFL_COMB-7"), (lds, "ICFL_COMB"), (lds + 1, "ICFL_COMB")):
        run(["kfinger", "-w", str(w), "-F", fact, "-o", "o", "a.fa"], cwd=tmp_path)
        assert (tmp_path / "o.txt").read_bytes() == K.Model([s for _, s in recs], ids, w, fact).text
    p = subprocess.run([FPMASH, "kfinger", "-w", "17", "-F", "CFL_ICFL_COMB-7", "-o", "sl", "a.fa"],
                       cwd=tmp_path, capture_output=True,
                       env={**os.environ, "FPMASH_KFINGER_SLICE": "150"})
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "sl.txt").read_bytes() == \
        K.Model([s for _, s in recs], ids, 17, "CFL_ICFL_COMB-7").text


@pytest.mark.parametrize("fact", ["FOO", "CFL_COMB-10", "ICFL_COMB-3", "CFL_ICFL_COMB-0",
                                  "CFL_ICFL_COMB-", "CFL_ICFL_COMB-4097", "COMB"])
def test_unknown_factorization(tmp_path, fact):
    p = run(["kfinger", "-F", fact, "-o", "out", DNA2], cwd=tmp_path, check=False)
    assert p.returncode == 1 and p.stdout == b""
    err = p.stderr.decode().strip().split("\n")
    assert len(err) == 1 and err[0].startswith("ERROR: unknown factorization " + fact)
    assert "CFL_COMB, ICFL_COMB or CFL_ICFL_COMB-<T>" in err[0]
    assert os.listdir(tmp_path) == []
