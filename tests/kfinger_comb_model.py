"""tests/kfinger_fact_model.py for the combined factorizations: the model of `fpmash kfinger -F
CFL_COMB / ICFL_COMB / CFL_ICFL_COMB-<T>` and of fpm_kfinger_set_comb, for the tests.

Lines come from fpmash.datagen.cfl_lines(..., factorization=...), whose combined forms are
pinned to lyn2vec's own results (tests/golden/comb_words.json.gz, DNA1-CFL_COMB.txt.gz,
DNA1-CFL_ICFL_COMB-10.txt.gz, dna2-ICFL_COMB.txt; tests/golden/KFINGER_COMB.md) by
tests/test_kfinger_comb_model.py; wide-window cases take them from bin/cflgen, which the same
file pins to the Python restatement.  kfinger_fact_model.Model passes the name through to both,
so it is the model here too.

The inputs the GPU tests run are built here, so that the CPU tests can show that each one sits
on the edge it is named for.
"""
import fpmash
import kfinger_fact_model as F
from fpmash import datagen

# the two forms without a threshold, lyn2vec's own CFL_ICFL_COMB-10, and a threshold above the
# reverse side's 30
FACTS = ("CFL_COMB", "ICFL_COMB", "CFL_ICFL_COMB-10", "CFL_ICFL_COMB-40")
# each form beside the form it combines
PLAIN = {"CFL_COMB": "CFL", "ICFL_COMB": "ICFL", "CFL_ICFL_COMB-10": "CFL_ICFL-10",
         "CFL_ICFL_COMB-40": "CFL_ICFL-40"}

Model = F.Model
rand = F.rand
default_ids = F.default_ids


def lds_window(fact):
    """the widest window whose working memory stays in LDS under `fact` (fpm_kfinger_lds_window)"""
    return fpmash.kfinger_lds_window(fact)


def cuts(lengths):
    out, at = set(), 0
    for ln in lengths:
        at += ln
        out.add(at)
    return out


def side_cuts(word: bytes, fact: str, rev_threshold=datagen.COMB_REV_THRESHOLD):
    """(the cuts of the forward side, the mirrored cuts of the reverse side below n) of an
    upper-cased word under the combined form `fact`, the reverse side's CFL_ICFL at
    rev_threshold"""
    plain = PLAIN.get(fact) or fact.replace("_COMB", "")
    rev = plain if "-" not in plain else "CFL_ICFL-%d" % rev_threshold
    n = len(word)
    fwd = cuts(datagen.factor_lengths(word, plain))
    back = {n - c for c in cuts(datagen.factor_lengths(datagen.reverse_complement(word), rev))}
    return fwd, back - {0}


def lengths_with_reverse_at(word: bytes, T: int, rev_threshold: int):
    """CFL_ICFL_COMB-T of `word` as it would be with the reverse side at rev_threshold"""
    fwd, back = side_cuts(word, "CFL_ICFL_COMB-%d" % T, rev_threshold)
    out, prev = [], 0
    for c in sorted(fwd | back):
        out.append(c - prev)
        prev = c
    return out


def is_own_reverse_complement(word: bytes):
    return datagen.reverse_complement(word) == word


# ---- the inputs of tests/test_gpu_kfinger_comb.py ---------------------------------------------

def short_record_seqs(w):
    """records shorter than the window, whose mirror runs over their own length: 1, 2 and w - 1
    bytes (w >= 4), between two records of a window or more"""
    return [rand(61, w + 3), rand(62, 1), rand(63, 2), rand(64, w - 1), rand(65, w)]


# one record with lower case, N, an IUPAC code, 0x24 and bytes >= 0x80, over a window's length
BYTE_RULES = rand(71, 230, b"ACGTacgtNnRy$\x80\xff")


def byte_rule_seqs():
    return [BYTE_RULES, b"acgtNRY$\xe9", rand(72, 99, b"ACGTacgtNnRy$\x80\xff")] + F.byte_rule_seqs()


def own_reverse_complements():
    """words equal to their reverse complement: every cut c of one side is the cut n - c of the
    other"""
    half = rand(73, 75)
    return [half + datagen.reverse_complement(half), b"ACGT" * 30, b"AATT" * 26 + b"N" + b"AATT" * 26]


def stride_seqs(n_desc, w, R, stage):
    """records that make exactly n_desc descriptors of both kinds at little cost: one record of
    w + 5 bytes (a descriptor per R window starts), then records of w - 1 bytes, one line each,
    as many as fill a descriptor's stage, for every descriptor left"""
    per_pack = min(stage // (w - 1), R)
    long_descs = -(-(w + 5) // R)
    assert n_desc > long_descs
    short = (n_desc - long_descs) * per_pack
    return [rand(800, w + 5)] + [rand(801 + i % 97, w - 1) for i in range(short)]
