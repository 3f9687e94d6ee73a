"""`fpmash kfinger` against the golden chain DNA1.fasta -> DNA1-CFL.txt -> DNA1-sketch.msh and
against tests/kfinger_model.py: the text byte for byte, and with -S the .msh that `sketch -fp`
writes for that text."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import kfinger_model as M
import mshfmt

pytestmark = pytest.mark.gpu

FPMASH = os.path.join(ROOT, "fp-mash_amd", "bin", "fpmash")
DNA1 = os.path.join(GOLDEN, "DNA1.fasta")


def run(args, cwd=None, check=True, env=None):
    p = subprocess.run([FPMASH] + args, cwd=cwd, capture_output=True,
                       env=None if env is None else {**os.environ, **env})
    if check and p.returncode != 0:
        raise AssertionError(f"fpmash {args} failed: {p.stderr.decode()}")
    return p


def rand(seed, n):
    rng = np.random.default_rng(seed)
    return bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))


def fasta(recs, width=60):
    return b"".join(b">" + h + b"\n" + b"".join(s[o:o + width] + b"\n" for o in range(0, len(s), width))
                    for h, s in recs)


def fastq(recs):
    return b"".join(b"@" + h + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for h, s in recs)


def model_text(recs, w):
    return M.Model([s for _, s in recs], [M.line_id(h) for h, _ in recs], w).text


def test_text_is_the_golden_cfl(tmp_path):
    p = run(["kfinger", "-o", "out", DNA1], cwd=tmp_path)
    assert p.stdout == b""
    assert (tmp_path / "out.txt").read_bytes() == open(os.path.join(GOLDEN, "DNA1-CFL.txt"), "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["out.txt"]


def test_sketch_is_sketch_fp_of_the_text(tmp_path, oracle):
    run(["kfinger", "-o", "out", DNA1], cwd=tmp_path)
    p = run(["kfinger", "-S", "-o", "a", DNA1], cwd=tmp_path)
    assert p.stdout == b""
    run(["sketch", "-fp", "-o", "b", "out.txt"], cwd=tmp_path)
    a = (tmp_path / "a.msh").read_bytes()
    assert a == (tmp_path / "b.msh").read_bytes()
    assert not (tmp_path / "a.txt").exists()
    got = mshfmt.read_msh(a)
    want = mshfmt.read_msh(os.path.join(GOLDEN, "DNA1-sketch.msh"))
    assert len(got["references"]) == len(want["references"])
    for g, w in zip(got["references"], want["references"]):
        assert (g["name"], g["comment"], g["length"]) == (w["name"], w["comment"], w["length"])
        assert np.array_equal(g["hashes32"], w["hashes32"])
    # and the model's References of the model's text
    refs = M.references(oracle, (tmp_path / "out.txt").read_bytes())
    assert [(r[0], r[1]) for r in refs] == [(g["name"], g["length"]) for g in got["references"]]
    # the sketch options reach the .msh as they do through sketch -fp
    run(["kfinger", "-S", "-s", "50", "-seed", "7", "-o", "c", DNA1], cwd=tmp_path)
    run(["sketch", "-fp", "-s", "50", "-S", "7", "-o", "d", "out.txt"], cwd=tmp_path)
    assert (tmp_path / "c.msh").read_bytes() == (tmp_path / "d.msh").read_bytes()


def test_window_files_fastq_and_headers(tmp_path):
    recs_a = [(b"T%d G%d x y" % (i, i), rand(40 + i, n)) for i, n in enumerate([300, 16, 17, 18])]
    recs_b = [(b"OnlyName", rand(50, 120)), (b"T9\tG9", rand(51, 40)), (b"T9 G9 again", rand(52, 33)),
              (b"Empty G10", b"")]
    recs_q = [(b"R%d Q%d" % (i, i), rand(60 + i, 90 + i)) for i in range(4)]
    (tmp_path / "a.fa").write_bytes(fasta(recs_a))
    (tmp_path / "b.fa").write_bytes(fasta(recs_b))
    with gzip.open(tmp_path / "q.fastq.gz", "wb") as f:
        f.write(fastq(recs_q))
    # -w 17, default prefix = the first input
    run(["kfinger", "-w", "17", "a.fa"], cwd=tmp_path)
    assert (tmp_path / "a.fa.txt").read_bytes() == model_text(recs_a, 17)
    # several inputs, in input order, in one text; a header without a comment; gzipped FASTQ
    run(["kfinger", "-o", "all", "b.fa", "q.fastq.gz", "a.fa"], cwd=tmp_path)
    assert (tmp_path / "all.txt").read_bytes() == model_text(recs_b + recs_q + recs_a, 100)
    # the same through small slices (the host walk, several jobs per file)
    run(["kfinger", "-o", "sl", "b.fa", "q.fastq.gz", "a.fa"], cwd=tmp_path,
        env={"FPMASH_KFINGER_SLICE": "150"})
    assert (tmp_path / "sl.txt").read_bytes() == (tmp_path / "all.txt").read_bytes()
    # -S over them: consecutive records of one ID (T9's) share a Reference
    run(["kfinger", "-S", "-o", "all", "b.fa", "q.fastq.gz", "a.fa"], cwd=tmp_path)
    run(["sketch", "-fp", "-o", "ref", "all.txt"], cwd=tmp_path)
    assert (tmp_path / "all.msh").read_bytes() == (tmp_path / "ref.msh").read_bytes()
    names = [r["name"] for r in mshfmt.read_msh(str(tmp_path / "all.msh"))["references"]]
    assert names[:3] == [b"OnlyName_0", b"G9_0", b"Q0_0"]


def test_no_sequence_record(tmp_path):
    (tmp_path / "none.fa").write_bytes(b"no record here\n")
    for extra in ([], ["-S"]):
        p = run(["kfinger"] + extra + ["-o", "out", "none.fa"], cwd=tmp_path, check=False)
        assert p.returncode == 1 and p.stdout == b""
        err = p.stderr.decode().strip().split("\n")
        assert len(err) == 1 and err[0].startswith("ERROR:")
    assert sorted(os.listdir(tmp_path)) == ["none.fa"]


def test_line_cap(tmp_path):
    """21 records of 50,000 bases: 1.05 M windows, of which `sketch -fp` and `kfinger -S` use the
    first 1,000,000; the last Reference is cut there"""
    rng = np.random.default_rng(99)
    recs = [(b"T%d G%d" % (i, i), bytes(rng.choice(list(b"ACGT"), 50000).astype(np.uint8)))
            for i in range(21)]
    (tmp_path / "big.fa").write_bytes(fasta(recs, 80))
    run(["kfinger", "-o", "big", "big.fa"], cwd=tmp_path)
    text = (tmp_path / "big.txt").read_bytes()
    assert text.count(b"\n") == 21 * 50000
    run(["kfinger", "-S", "-o", "big", "big.fa"], cwd=tmp_path)
    run(["sketch", "-fp", "-o", "ref", "big.txt"], cwd=tmp_path)
    got = (tmp_path / "big.msh").read_bytes()
    assert got == (tmp_path / "ref.msh").read_bytes()
    refs = mshfmt.read_msh(got)["references"]
    assert len(refs) == 20 and refs[-1]["name"] == b"G19_0"
    assert sum(len(r["hashes32"]) for r in refs) == 1000000
    assert len(refs[-1]["hashes32"]) == 50000
