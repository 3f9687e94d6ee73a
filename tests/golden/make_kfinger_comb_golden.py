#!/usr/bin/env python3
"""Generate the combined-factorization k-finger fixtures in tests/golden/ (build container only,
with the reference tree present, as make_kfinger_golden.py).

Everything written here is output of lyn2vec's own code, imported from the reference tree and
run as it is: d_cfl, d_icfl and d_cfl_icfl (factorizations_comb.py:178-246) and
compute_fingerprint_by_list (fingerprint_utils.py:443-476); or a copy of data the fork ships.

  dna2.fasta, dna2-ICFL_COMB.txt   the fork's own lyn2vec/training/dna2.fasta (4 records of 200
      bases) and lyn2vec/training/fingerprint_ICFL_COMB.txt (its 800 lines), copied as data; the
      generator asserts that lyn2vec's d_icfl over the fasta's windows gives that text
  DNA1-CFL_COMB.txt.gz, DNA1-CFL_ICFL_COMB-10.txt.gz   lyn2vec's lines (`--type basic --shift
      shift`, window 100, IDs with "_0") for the first three records of DNA1.fasta, which hold
      only ACGTN; gzipped as make_kfinger_golden.py's (level 9, no name or time in the header)
  comb_words.json.gz   2,000 words over ACGTN with their lengths under CFL_COMB, ICFL_COMB and
      CFL_ICFL_COMB-{1, 3, 10, 20, 29, 30, 31, 40}: rows [word, CFL_COMB, ICFL_COMB, then one per
      threshold], each list of lengths joined by spaces.  Every length from 1 to 64 for one
      letter, for the periods TG, TTG, ACGT and AATT and for words equal to their own reverse
      complement; random words of 1 to 64 bytes over 1 to 5 letters; 100 random ACGT words of 100
      to 300 bytes, so that factors longer than 30 occur

Run:  python tests/golden/make_kfinger_comb_golden.py <reference root>
"""
import gzip
import json
import os
import random
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
LYN2VEC = os.path.join(sys.argv[1], "lyn2vec")
if not os.path.isdir(LYN2VEC):
    sys.exit(f"{LYN2VEC} missing: the fixtures are made where the reference tree is")
sys.dont_write_bytecode = True
sys.path.insert(0, LYN2VEC)
sys.path.insert(0, os.path.dirname(HERE))
from factorizations_comb import d_cfl, d_icfl, d_cfl_icfl, reverse_complement  # noqa: E402
from fingerprint_utils import compute_fingerprint_by_list  # noqa: E402
import seqio  # noqa: E402

THRESHOLDS = (1, 3, 10, 20, 29, 30, 31, 40)
RECORDS = 3


def lines_of(path, factorization, T, n_records=None):
    recs = seqio.read_records(path)[:n_records]
    assert all(set(s.upper()) <= set(b"ACGTN") for _n, _c, s in recs)
    # lyn2vec's read lines: "<comment's first token>_0 <SEQUENCE>" (fingerprint_utils.py:276-307)
    reads = [f"{c.split()[0].decode()}_0 {s.decode().upper()}" for _n, c, s in recs]
    lines, _ = compute_fingerprint_by_list("no_create", "shift", factorization, T, reads)
    return "".join(lines).encode()


def words():
    rng = random.Random(20242)
    out = []
    letters = "ACGTN"
    for n in range(1, 65):
        out.append("A" * n)
        for period in ("TG", "TTG", "ACGT", "AATT"):
            out.append((period * 64)[:n])
        half = "".join(rng.choice("ACGT") for _ in range(n // 2))
        # equal to its own reverse complement: x rc(x), with N in the middle of an odd length
        out.append(half + ("N" if n & 1 else "") + reverse_complement(half))
    long_words = ["".join(rng.choice("ACGT") for _ in range(rng.randint(100, 300)))
                  for _ in range(100)]
    while len(out) < 2000 - len(long_words):
        k = rng.randint(1, 5)
        n = rng.randint(1, 64)
        out.append("".join(rng.choice(letters[:k]) for _ in range(n)))
    out += long_words
    assert all(set(w) <= set(letters) for w in out)
    return out


def lengths(factors):
    return " ".join(str(len(f)) for f in factors)


def write_gz(name, data: bytes):
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as g:
            g.write(data)


def main():
    training = os.path.join(LYN2VEC, "training")
    shutil.copyfile(os.path.join(training, "dna2.fasta"), os.path.join(HERE, "dna2.fasta"))
    shutil.copyfile(os.path.join(training, "fingerprint_ICFL_COMB.txt"),
                    os.path.join(HERE, "dna2-ICFL_COMB.txt"))
    with open(os.path.join(HERE, "dna2-ICFL_COMB.txt"), "rb") as f:
        assert f.read() == lines_of(os.path.join(HERE, "dna2.fasta"), d_icfl, None)
    for name, fact, T in (("DNA1-CFL_COMB.txt", d_cfl, None),
                          ("DNA1-CFL_ICFL_COMB-10.txt", d_cfl_icfl, 10)):
        write_gz(name, lines_of(os.path.join(HERE, "DNA1.fasta"), fact, T, RECORDS))
    rows = [[w, lengths(d_cfl(w, None)), lengths(d_icfl(w, None))] +
            [lengths(d_cfl_icfl(w, T)) for T in THRESHOLDS] for w in words()]
    write_gz("comb_words.json",
             json.dumps({"thresholds": list(THRESHOLDS), "rows": rows}, separators=(",", ":")).encode())
    print({"words": len(rows)})


if __name__ == "__main__":
    main()
