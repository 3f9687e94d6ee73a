"""CPU tests of the combined-factorization restatement (fpmash.datagen.comb_lengths behind
factor_lengths / cfl_lines, bin/cflgen's third argument) against lyn2vec's own results in
tests/golden/ (KFINGER_COMB.md), of the names the binding takes, and of the inputs
tests/test_gpu_kfinger_comb.py runs: each sits on the edge it is named for."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN
import kfinger_comb_model as K
import kfinger_fact_model as F
import kfinger_model as M
import seqio
import fpmash
from fpmash import datagen

THRESHOLDS = [1, 3, 10, 20, 29, 30, 31, 40]


@pytest.fixture(scope="module")
def words():
    g = json.loads(F.golden("comb_words.json"))
    assert g["thresholds"] == THRESHOLDS and len(g["rows"]) == 2000
    return g["rows"]


def ints(s):
    return [int(x) for x in s.split()]


def records(name, n=None):
    recs = seqio.read_records(os.path.join(GOLDEN, name))[:n]
    return [s for _, _, s in recs], [M.line_id(h + b" " + c) for h, c, _ in recs]


def test_restatement_equals_lyn2vec_on_the_golden_words(words):
    for word, cfl, icfl, *by_t in words:
        w = word.encode("latin-1")
        assert set(w) <= set(b"ACGTN") and 1 <= len(w) <= 300
        assert datagen.factor_lengths(w, "CFL_COMB") == ints(cfl), word
        assert datagen.factor_lengths(w, "ICFL_COMB") == ints(icfl), word
        for T, want in zip(THRESHOLDS, by_t):
            assert datagen.factor_lengths(w, "CFL_ICFL_COMB-%d" % T) == ints(want), (word, T)
    assert sum(len(r[0]) >= 100 for r in words) == 100


def test_golden_words_sit_on_their_edges(words):
    """the reverse side runs at 30 whatever T is, and the words show it: for every T but 30 some
    word's lengths would differ with the reverse side at T; some words have a cut both sides
    share (one boundary, never a zero length); some equal their own reverse complement"""
    differ = {T: 0 for T in THRESHOLDS}
    shared = own = 0
    for word, _cfl, _icfl, *by_t in words:
        w = word.encode("latin-1")
        for T, want in zip(THRESHOLDS, by_t):
            assert K.lengths_with_reverse_at(w, T, 30) == ints(want)
            differ[T] += K.lengths_with_reverse_at(w, T, T) != ints(want)
            assert 0 not in ints(want) and sum(ints(want)) == len(w)
        fwd, back = K.side_cuts(w, "ICFL_COMB")
        shared += bool(fwd & back)
        own += K.is_own_reverse_complement(w)
    assert differ[30] == 0
    assert all(differ[T] >= 1 for T in (1, 29, 31, 40)), differ
    assert shared >= 100 and own >= 64


@pytest.mark.parametrize("fact, name", [("CFL_COMB", "DNA1-CFL_COMB.txt"),
                                        ("CFL_ICFL_COMB-10", "DNA1-CFL_ICFL_COMB-10.txt")])
def test_cfl_lines_and_cflgen_reproduce_the_dna1_texts(fact, name):
    seqs, ids = records("DNA1.fasta", 3)
    golden = F.golden(name)
    assert golden.count(b"\n") == sum(len(s) for s in seqs)
    assert K.Model(seqs, ids, 100, fact, fast=False).text == golden
    assert K.Model(seqs, ids, 100, fact, fast=True).text == golden


def test_cfl_lines_and_cflgen_reproduce_the_forks_training_text():
    seqs, ids = records("dna2.fasta")
    assert [len(s) for s in seqs] == [200] * 4
    with open(os.path.join(GOLDEN, "dna2-ICFL_COMB.txt"), "rb") as f:
        golden = f.read()
    assert len(golden) == 28943 and golden.count(b"\n") == 800
    assert K.Model(seqs, ids, 100, "ICFL_COMB", fast=False).text == golden
    assert K.Model(seqs, ids, 100, "ICFL_COMB", fast=True).text == golden


def test_cflgen_equals_the_restatement_on_the_golden_words(words):
    """one record per word, each shorter than the window: one line each"""
    seqs = [r[0].encode("latin-1") for r in words]
    ids = K.default_ids(len(seqs))
    col = {"CFL_COMB": 1, "ICFL_COMB": 2, "CFL_ICFL_COMB-10": 3 + THRESHOLDS.index(10),
           "CFL_ICFL_COMB-40": 3 + THRESHOLDS.index(40), "CFL_ICFL_COMB-29": 3 + THRESHOLDS.index(29)}
    for fact, c in col.items():
        m = K.Model(seqs, ids, 301, fact, fast=True)
        assert [v.tolist() for v in m.vals] == [ints(r[c]) for r in words], fact


@pytest.mark.parametrize("w", [1, 2, 3, 17, 100, 256])
def test_cflgen_equals_the_restatement_on_the_gpu_inputs(w):
    seqs = [F.rand(w + i, n, a) for i, (n, a) in enumerate(
        [(1, b"AC"), (w + 1, b"AC"), (w + 40, b"ACGT"), (max(w - 1, 1), b"ACGTacgtN"),
         (w + 7, b"AC")])] + K.byte_rule_seqs() + K.own_reverse_complements()
    ids = K.default_ids(len(seqs))
    for fact in K.FACTS:
        assert K.Model(seqs, ids, w, fact, fast=True).text == \
            K.Model(seqs, ids, w, fact, fast=False).text, fact


def test_constructed_inputs_sit_on_their_edges():
    for s in K.own_reverse_complements():
        assert K.is_own_reverse_complement(s) and len(s) >= 100
        fwd, back = K.side_cuts(s, "CFL_COMB")
        assert {len(s) - c for c in fwd} - {0} == back - {len(s)}
    # the byte rules: every class of byte in one record, and the complement leaves all but
    # ACGT alone
    up = K.BYTE_RULES.upper()
    assert {ord("N"), ord("R"), ord("Y"), 0x24, 0x80, 0xFF} <= set(up)
    assert any(0x61 <= c <= 0x7A for c in K.BYTE_RULES)
    assert datagen.reverse_complement(b"ACGTNRY$\x80\xff") == b"\xff\x80$YRNACGT"
    # a short record's mirror runs over its own length, not the window's
    # (AGTCA: AGTC A forwards; its reverse complement TGACT gives T G ACT, cuts 1 and 2, which
    # mirror to 4 and 3)
    assert datagen.cfl_lines(b"agtca", "g", 100, "CFL_COMB") == ["g_0 3 1 1\n"]
    assert datagen.factor_lengths(b"AGTCA", "CFL") == [4, 1]
    assert datagen.factor_lengths(b"A", "ICFL_COMB") == [1]
    # the reverse side of CFL_ICFL_COMB-T at 30, on the records the GPU tests run
    R = fpmash.kfinger_limits()[1]
    for T in (10, 40):
        wins = [w for s in F.window_seqs(100, R) for w in F.windows(s, 100)]
        assert any(K.lengths_with_reverse_at(w, T, T) !=
                   datagen.factor_lengths(w, "CFL_ICFL_COMB-%d" % T) for w in wins[::7]), T


def test_binding_names():
    max_window, _ = fpmash.kfinger_limits()
    assert fpmash.parse_factorization("CFL_COMB") == ("CFL_COMB", 0)
    assert fpmash.parse_factorization("ICFL_COMB") == ("ICFL_COMB", 0)
    assert fpmash.parse_factorization("CFL_ICFL_COMB-10") == ("CFL_ICFL_COMB", 10)
    assert fpmash.kfinger_factorization("CFL_COMB") == (fpmash.KF_CFL, 0, 1)
    assert fpmash.kfinger_factorization("ICFL_COMB") == (fpmash.KF_ICFL, 0, 1)
    assert fpmash.kfinger_factorization("CFL_ICFL_COMB-%d" % max_window) == \
        (fpmash.KF_CFL_ICFL, max_window, 1)
    # what today's names give has not changed
    assert fpmash.parse_factorization("CFL") == ("CFL", 0)
    assert fpmash.parse_factorization("ICFL") == ("ICFL", 0)
    assert fpmash.parse_factorization("CFL_ICFL-20") == ("CFL_ICFL", 20)
    assert fpmash.kfinger_factorization("CFL_ICFL-20") == (fpmash.KF_CFL_ICFL, 20)
    for bad in ("CFL_COMB-10", "ICFL_COMB-3", "CFL_ICFL_COMB-0", "CFL_ICFL_COMB-",
                "CFL_ICFL_COMB-%d" % (max_window + 1), "CFL_ICFL_COMB", "COMB", "FOO"):
        with pytest.raises(ValueError):
            fpmash.kfinger_factorization(bad)
        if bad.endswith(str(max_window + 1)):
            continue                                   # (cflgen knows no widest window)
        p = subprocess.run([M.CFLGEN, "100", "1", bad], input=b"a\tACGT\n", capture_output=True)
        assert p.returncode == 1 and p.stdout == b""


def test_lds_windows():
    """the query needs no device; the non-combined kinds keep the window the existing tests
    hard-code, and a combined form's is no wider than its plain form's"""
    max_window, _ = fpmash.kfinger_limits()
    assert fpmash.kfinger_lds_window("CFL") == max_window
    assert fpmash.kfinger_lds_window("ICFL") == fpmash.kfinger_lds_window("CFL_ICFL-10") == 192
    for fact in K.FACTS:
        assert 100 <= K.lds_window(fact) < max_window
        assert K.lds_window(fact) <= fpmash.kfinger_lds_window(K.PLAIN[fact])
    assert K.lds_window("ICFL_COMB") == K.lds_window("CFL_ICFL_COMB-10") < 192
    import ctypes as C
    w = C.c_uint32()
    L = fpmash.lib()
    assert L.fpm_kfinger_lds_window(3, 0, C.byref(w)) == fpmash.FPM_EINVAL
    assert L.fpm_kfinger_lds_window(0, 2, C.byref(w)) == fpmash.FPM_EINVAL
    assert L.fpm_kfinger_lds_window(0, 1, None) == fpmash.FPM_EINVAL
