"""tests/kfinger_long_model.py against lyn2vec's own lines (tests/golden/KFINGER_LONG.md): the
long-read fingerprint and factor lines of DNA1.fasta's first three records, the window-mode factor
lines of its first record, and both lines of 200 short words at five splits under six
factorizations, byte for byte; and the piece rule at its edges.  No GPU."""
import os

import pytest

from conftest import GOLDEN
import kfinger_long_model as L
import kfinger_model as M
import seqio

DNA1 = os.path.join(GOLDEN, "DNA1.fasta")


@pytest.fixture(scope="module")
def dna1():
    return seqio.read_records(DNA1)


@pytest.mark.parametrize("split, fact", [(300, "CFL_ICFL-30"), (150, "ICFL_COMB")])
def test_long_lines_are_lyn2vecs_on_dna1(dna1, split, fact):
    recs = dna1[:3]
    text = b"".join(L.long_line(s, n, split, fact) for n, _c, s in recs)
    facts = b"".join(L.long_fact_line(s, n, split, fact) for n, _c, s in recs)
    assert text == L.golden("DNA1-long%d-%s.txt" % (split, fact))
    assert facts == L.golden("DNA1-long%d-%s.fact.txt" % (split, fact))
    assert text.count(b"\n") == 3 and text.count(b"|") == sum(-(-len(s) // split) for _, _, s in recs)


@pytest.mark.parametrize("fact", ["CFL", "ICFL_COMB"])
def test_window_fact_lines_are_lyn2vecs_on_dna1(dna1, fact):
    n, c, s = dna1[0]
    got = L.fact_text([s], [M.line_id(n + b" " + c)], 100, fact)
    assert got == L.golden("DNA1-%s.fact.txt" % fact)
    assert got.count(b"\n") == len(s)


def test_words():
    d = L.long_words()
    assert tuple(d["facts"]) == L.FACTS and d["splits"] == [1, 2, 3, 7, 40]
    assert len(d["rows"]) == 200
    lengths = set()
    for row in d["rows"]:
        word = row[0].encode()
        lengths.add(len(word))
        at = 1
        for split in d["splits"]:
            for fact in d["facts"]:
                assert L.long_line(word, b"w", split, fact) == row[at].encode(), (word, split, fact)
                assert L.long_fact_line(word, b"w", split, fact) == row[at + 1].encode()
                at += 2
        assert at == len(row)
    assert lengths == set(range(1, 41))


def test_issue_examples():
    assert L.long_line(b"ACGTTGCAACG", b"r3", 5, "CFL") == b"r3  5 | 1 1 3 | 1 | \n"
    assert L.long_fact_line(b"ACGTTGCAACG", b"r3", 5, "CFL") == b"r3  ACGTT | G C AAC | G | \n"
    assert L.long_line(b"ACGTTGCAAC", b"r1", 5, "ICFL") == b"r1  1 1 1 2 | 5 | \n"
    assert L.long_fact_line(b"ACGTTGCAAC", b"r1", 5, "ICFL") == b"r1  A C G TT | GCAAC | \n"
    assert L.fact_line(b"ACGTTG", b"g_0", "CFL_ICFL-2") == b"g_0 A C G TTG\n"
    assert L.long_line(b"acgtn", b"x", 9, "CFL") == L.long_line(b"ACGTN", b"x", 9, "CFL")
    assert L.long_fact_line(b"acgtn", b"x", 9, "CFL") == b"x  ACGTN | \n"


@pytest.mark.parametrize("N", [1, 2, 3, 7, 150])
def test_pieces(N):
    assert L.pieces(b"", N) == []
    for n in L.edge_lengths(N):
        s = L.rand(n, n)
        p = L.pieces(s, N)
        assert b"".join(p) == s and all(p)
        if n < N:
            assert p == [s]
        else:
            assert [len(x) for x in p] == [N] * (n // N) + ([n % N] if n % N else [])
    assert sorted(L.edge_lengths(N)) == sorted({n for n in (1, N - 1, N, N + 1, 2 * N, 2 * N + 1) if n})


def test_gpu_inputs_sit_on_their_edges():
    import fpmash
    KMAX, R = fpmash.kfinger_limits()
    stage = R + KMAX - 1
    for N in (1, 7):
        seqs = L.pack_seqs(N, R, stage)
        lens = [len(p) for s in seqs for p in L.pieces(s, N)]
        d = L.descs(lens, R, stage)
        # R pieces fill the first descriptor; the first record's last piece opens the second,
        # which the third record's pieces leave for a third
        assert d[0] == (0, R) and d[1][0] == R and len(d) == 3
        assert d[1] == (R, R) and d[2] == (2 * R, 4)
    for N in (150, 300):
        a, b = L.stage_fill_seqs(N, stage)
        la = [len(p) for p in L.pieces(a, N)]
        assert sum(la) == stage and L.descs(la, R, stage) == [(0, len(la))]
        lb = [len(p) for p in L.pieces(b, N)]
        assert L.descs(lb, R, stage) == [(0, len(lb) - 1), (len(lb) - 1, 1)]
