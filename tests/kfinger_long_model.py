"""The model of `fpmash kfinger -L N` / `-f` and of fpm_kfinger_stage_split and
fpm_kfinger_fact_text, for the tests: lyn2vec's long-read ("generalized") fingerprints
(`--type generalized --split N`: factors_string, fingerprint_utils.py:114-130, and
compute_long_fingerprint_by_list, :480-518) and its factor file (`--fact create`: :471-474 in
window mode, :509-511 in long-read mode), restated.

The factorizations come from fpmash.datagen.factor_lengths, which the earlier model tests pin to
lyn2vec; the piece rule and the line layouts are restated here and pinned to lyn2vec's own lines
(tests/golden/KFINGER_LONG.md) by tests/test_kfinger_long_model.py.

Where the product departs from lyn2vec, the model is the product's:
  - records are found by kseq's rules; lyn2vec's reader takes a header line and one sequence
    line in turn;
  - a header of two tokens makes lyn2vec factorize the second token as if it were the read
    (fingerprint_utils.py:421-430); here the long-read ID is the record's name, the first token of
    its header, with no "_0" (lyn2vec appends it only under --rev_comb true), and the read is the
    sequence;
  - a record with an empty sequence makes no line, where lyn2vec raises IndexError;
  - every byte is taken: a-z fold to A-Z, every other byte stays, bytes compare unsigned, and
    in the combined forms a byte outside ACGT is its own complement (kfinger_comb_model).
"""
import json

import numpy as np

import kfinger_fact_model as F
from fpmash import datagen

golden = F.golden
rand = F.rand

FACTS = ("CFL", "ICFL", "CFL_ICFL-3", "CFL_COMB", "ICFL_COMB", "CFL_ICFL_COMB-3")


def upper(seq: bytes) -> bytes:
    """ASCII a-z upper-cased, every other byte (those >= 0x80 too) as it is"""
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in seq)


def pieces(seq: bytes, split: int):
    """factors_string (fingerprint_utils.py:114-130): the whole record when it is shorter than
    the split, else consecutive pieces of `split` bytes, the last one of n mod split bytes when
    that is not 0.  An empty record has no piece (lyn2vec never gets that far with one)."""
    n = len(seq)
    if n == 0:
        return []
    if n < split:
        return [seq]
    return [seq[i:i + split] for i in range(0, n, split)]


def factors(word: bytes, fact: str):
    """the factors of an upper-cased word, as bytes"""
    out, at = [], 0
    for ln in datagen.factor_lengths(word, fact):
        out.append(word[at:at + ln])
        at += ln
    assert at == len(word)
    return out


def long_line(seq: bytes, rid: bytes, split: int, fact: str) -> bytes:
    """the fingerprint line of one record (:494-495, :507-508, :513): "<id>" + two spaces, per
    piece its lengths joined by single spaces and " | ", then a newline; b"" for an empty record"""
    if not seq:
        return b""
    return rid + b"  " + b"".join(
        b" ".join(b"%d" % len(f) for f in factors(p, fact)) + b" | "
        for p in pieces(upper(seq), split)) + b"\n"


def long_fact_line(seq: bytes, rid: bytes, split: int, fact: str) -> bytes:
    """the factor line of one record (:496, :510-511, :514): long_line with each factor's bytes
    in place of its length"""
    if not seq:
        return b""
    return rid + b"  " + b"".join(b" ".join(factors(p, fact)) + b" | "
                                  for p in pieces(upper(seq), split)) + b"\n"


def fact_line(window: bytes, full_id: bytes, fact: str) -> bytes:
    """the factor line of one upper-cased window of a window job (:471-474): "<id>" + one space,
    the factors joined by single spaces, a newline; full_id carries its "_0\""""
    return full_id + b" " + b" ".join(factors(window, fact)) + b"\n"


def fact_text(seqs, ids, w: int, fact: str) -> bytes:
    """the factor text of a window job: fact_line of every window of every record, in line order"""
    return b"".join(fact_line(win, i, fact) for s, i in zip(seqs, ids)
                    for win in F.windows(bytes(s), w))


def long_ids(n):
    return [b"R%04d" % i for i in range(n)]


class Model:
    """what a split job over records `seqs` with IDs `ids` gives: the two texts, and per piece
    (the job's "line") its values; rec_first_line[r] is record r's first piece"""

    def __init__(self, seqs, ids, split, fact):
        self.text = b"".join(long_line(bytes(s), i, split, fact) for s, i in zip(seqs, ids))
        self.fact_text = b"".join(long_fact_line(bytes(s), i, split, fact)
                                  for s, i in zip(seqs, ids))
        self.vals = []
        self.rec_first_line = [0]
        for s in seqs:
            for p in pieces(upper(bytes(s)), split):
                self.vals.append(np.array(datagen.factor_lengths(p, fact), np.uint64))
            self.rec_first_line.append(len(self.vals))
        self.rec_first_line = np.array(self.rec_first_line, np.uint64)
        self.n_vals = np.array([len(v) for v in self.vals], np.uint32)
        self.val_off = np.zeros(len(self.vals) + 1, np.uint64)
        self.val_off[1:] = np.cumsum(self.n_vals)
        self.flat = (np.concatenate(self.vals) if self.vals
                     else np.zeros(0, np.uint64)).astype(np.uint16)
        self._hash = {}

    hashes = F.Model.hashes


def long_words():
    """tests/golden/long_words.json.gz: {"splits", "facts", "rows": [word, then per split and
    per factorization the two lines of lyn2vec for the read line "w <word>"]}"""
    return json.loads(golden("long_words.json"))


# ---- the inputs of tests/test_gpu_kfinger_long.py --------------------------------------------

def edge_lengths(N):
    """record lengths around the split: 1, N - 1, N, N + 1, 2N, 2N + 1 (those above 0, once)"""
    out = []
    for n in (1, N - 1, N, N + 1, 2 * N, 2 * N + 1):
        if n > 0 and n not in out:
            out.append(n)
    return out


def edge_seqs(N, empty_at):
    """records of the edge lengths with an empty one first, in the middle or last"""
    seqs = [rand(5000 + 7 * N + i, n) for i, n in enumerate(edge_lengths(N))]
    at = {"first": 0, "middle": len(seqs) // 2, "last": len(seqs)}[empty_at]
    return seqs[:at] + [b""] + seqs[at:]


def pack_seqs(N, R, stage):
    """one record of R + 1 pieces (a pack of R pieces, then one more, at N = 1 .. stage // R);
    then two records of which the second begins in the first one's last descriptor and ends in
    the next: 3 pieces, then R pieces"""
    assert N * R <= stage
    return [rand(61, N * (R + 1)), rand(62, 3 * N), rand(63, R * N)]


def stage_fill_seqs(N, stage):
    """pieces of N bytes whose bytes just fill one LDS stage (stage // N pieces and one of
    stage mod N bytes, in one record), then a record of the same pieces and one byte more, whose
    last piece goes to the next descriptor"""
    assert N < stage and stage % N
    return [rand(64, stage), rand(65, stage + 1)]


def descs(piece_lens, R, stage):
    """the descriptors fpm_kfinger_stage_split makes: consecutive pieces share one while they
    number at most R and fill at most `stage` bytes -> [(first piece, pieces)]"""
    out, first, n, b = [], 0, 0, 0
    for i, ln in enumerate(piece_lens):
        if n == R or b + ln > stage:
            out.append((first, n))
            n = b = 0
        if n == 0:
            first = i
        n += 1
        b += ln
    if n:
        out.append((first, n))
    return out
