"""CPU tests of the k-finger generator's rules (tests/kfinger_model.py), of fpm_kfinger_limits
and of the `fpmash kfinger` refusals that are decided before any device work."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import kfinger_model as M
import seqio

FPMASH = os.path.join(ROOT, "fp-mash_amd", "bin", "fpmash")


@pytest.mark.parametrize("header, want", [
    (b"T1", b"T1_0"),                           # one token: no comment, the name
    (b"T1 G1", b"G1_0"),                        # two: the comment's first token
    (b"T1 G1 rest of it", b"G1_0"),             # three and more
    (b"T1\tG1\tx", b"G1_0"),                    # tab-separated
    (b"T1 \t G1", b"G1_0"),                     # a run of separators
    (b"T1 ", b"T1_0"),                          # a comment of whitespace only
    (b"T1 G1\r", b"G1_0"),                      # the '\r' kseq keeps in the comment is whitespace
    (b" G1 x", b"G1_0"),                        # an empty name
    (b"", b"_0"),
])
def test_id_rule(header, want):
    import fpmash
    assert M.line_id(header) == want
    assert fpmash.kfinger_id(header) == want
    # the same through kseq's own header split
    (name, comment, _seq), = seqio.parse(b">" + header + b"\nACGT\n")
    tok = comment.split()
    assert (tok[0] if tok else name) + b"_0" == want


def test_id_rule_on_the_golden_fasta():
    recs = seqio.read_records(os.path.join(GOLDEN, "DNA1.fasta"))
    ids = {M.line_id(n + b" " + c) for n, c, _ in recs}
    golden = {l.split()[0] for l in open(os.path.join(GOLDEN, "DNA1-CFL.txt"), "rb")}
    assert ids == golden


@pytest.mark.parametrize("w", [1, 2, 5, 100])
def test_line_count_rule(w):
    rng = np.random.default_rng(w)
    for n in sorted({0, 1, w - 1, w, w + 1}):
        seq = bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8))
        lines = M.record_lines(seq, b"g_0", w)
        assert len(lines) == M.n_lines(n, w)
        if n:
            assert len(lines) == (1 if n < w else n)
            # every line factorizes a whole window
            assert all(sum(int(x) for x in l.split()[1:]) == min(n, w) for l in lines)
        else:
            assert lines == []


def test_fast_lines_equal_cfl_lines():
    """the model's two sources of lines agree (cflgen is test tooling pinned to cfl_lines)"""
    rng = np.random.default_rng(3)
    for n, w in [(1, 100), (99, 100), (100, 100), (257, 100), (40, 17), (300, 256)]:
        seq = bytes(rng.choice(list(b"ACGTacgtN"), n).astype(np.uint8))
        assert M.record_lines(seq, b"id_0", w, fast=True) == M.record_lines(seq, b"id_0", w, fast=False)


def test_model_reproduces_the_golden_text():
    recs = seqio.read_records(os.path.join(GOLDEN, "DNA1.fasta"))
    m = M.Model([s for _, _, s in recs], [M.line_id(n + b" " + c) for n, c, _ in recs], 100)
    assert m.text == open(os.path.join(GOLDEN, "DNA1-CFL.txt"), "rb").read()
    assert m.rec_first_line[-1] == len(m.lines) == sum(len(s) for _, _, s in recs)


def test_limits():
    import fpmash
    max_window, run = fpmash.kfinger_limits()
    assert 1024 <= max_window <= 4096
    assert max_window <= 65535                      # lengths fit u16
    assert run >= 64 and run % 64 == 0              # whole waves
    # NULL outputs are allowed
    fpmash.lib().fpm_kfinger_limits(None, None)


def run(args, cwd=None):
    return subprocess.run([FPMASH, "kfinger"] + args, cwd=cwd, capture_output=True)


def one_error(p):
    assert p.returncode == 1
    assert p.stdout == b""
    err = p.stderr.decode().strip().split("\n")
    assert len(err) == 1 and err[0].startswith("ERROR:"), p.stderr


@pytest.mark.parametrize("sketch", [False, True])
def test_cli_refusals_before_device_work(tmp_path, sketch):
    import fpmash
    max_window, _ = fpmash.kfinger_limits()
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">a b\nACGT\n")
    extra = ["-S"] if sketch else []
    for w in ("0", str(max_window + 1), "x", "1.5"):
        one_error(run(extra + ["-w", w, "-o", "out", "in.fa"], cwd=tmp_path))
    one_error(run(extra + ["-o", "out", "in.fa", "missing.fa"], cwd=tmp_path))
    one_error(run(extra + ["-o", "out", "missing.fa"], cwd=tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["in.fa"]


def test_window2_closed_form():
    """the closed form tests/test_gpu_kfinger_scale.py checks four million lines with, against
    the model, on a record with lower case, equal neighbours and a wrap"""
    rng = np.random.default_rng(12)
    seq = bytes(rng.choice(list(b"ACGTacgt"), 300).astype(np.uint8))
    for s in (seq, b"AC", b"CA", b"AA", b"aC" + seq + b"T"):
        m = M.Model([s], [b"g_0"], 2)
        c = M.window2(s, b"g_0")
        assert len(m.lines) == len(s) == len(c["rising"])
        assert c["text"] == m.text
        assert np.array_equal(c["n_vals"], m.n_vals) and np.array_equal(c["val_off"], m.val_off)
        assert np.array_equal(c["vals"], m.flat) and c["vals"].dtype == m.flat.dtype
        assert [v.tolist() for v in m.vals] == [[2] if r else [1, 1] for r in c["rising"]]
    assert M.window2(b"AC", b"x")["text"] == b"x 2\nx 1 1\n"
