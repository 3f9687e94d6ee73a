#!/usr/bin/env python3
"""Generate the ICFL / CFL_ICFL k-finger fixtures in tests/golden/ (build container only, with
the reference tree present, as make_golden.py).

Everything written here is output of lyn2vec's own code, imported from the reference tree and
run as it is: ICFL_recursive and CFL_icfl (factorizations.py:143-169, 265-301) and
compute_fingerprint_by_list (fingerprint_utils.py:443-476).

Each file is stored gzipped (level 9, no name or time in the header, so a rerun gives the same
bytes), as reads{1,2}.fastq.gz are: the three together are 800 KB of text.

  DNA1-ICFL.txt.gz, DNA1-CFL_ICFL-10.txt.gz   lyn2vec's lines (`--type basic --shift shift`,
      window 100, IDs with "_0") for the first three records of DNA1.fasta
  icfl_words.json.gz   2,000 words of 1 to 64 bytes (random over 2- to 5-letter alphabets, periodic,
      ascending, descending, one letter; none holds '$', lyn2vec's in-band end mark) with their
      factor lengths: rows [word, ICFL, CFL_ICFL-1, -3, -10, -20, -30], each list of lengths
      joined by spaces

Run:  python tests/golden/make_kfinger_golden.py <reference root>
"""
import gzip
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
LYN2VEC = os.path.join(sys.argv[1], "lyn2vec")
if not os.path.isdir(LYN2VEC):
    sys.exit(f"{LYN2VEC} missing: the fixtures are made where the reference tree is")
sys.path.insert(0, LYN2VEC)
sys.path.insert(0, os.path.dirname(HERE))
from factorizations import ICFL_recursive, CFL_icfl  # noqa: E402
from fingerprint_utils import compute_fingerprint_by_list  # noqa: E402
import seqio  # noqa: E402

THRESHOLDS = (1, 3, 10, 20, 30)
RECORDS = 3


def dna1_lines(factorization, T):
    recs = seqio.read_records(os.path.join(HERE, "DNA1.fasta"))[:RECORDS]
    # lyn2vec's read lines: "<comment's first token>_0 <SEQUENCE>" (fingerprint_utils.py:276-307)
    reads = [f"{c.split()[0].decode()}_0 {s.decode().upper()}" for _n, c, s in recs]
    lines, _ = compute_fingerprint_by_list("no_create", "shift", factorization, T, reads)
    return "".join(lines).encode()


def words():
    rng = random.Random(20241)
    out = []
    letters = "ACGTN"
    for n in range(1, 65):                       # one letter, ascending, descending
        out.append("A" * n)
        out.append("".join(chr(0x25 + i) for i in range(n)))
        out.append("".join(chr(0x7A - i) for i in range(n)))
    for period in ("TG", "TTG", "TTTG", "ACGT", "TGCA", "GTT", "AAT", "CA"):
        for n in range(2, 65, 3):                # periodic, whole and ending in a break
            w = (period * 64)[:n]
            out.append(w)
            for brk in "AZ":
                out.append(w[:-1] + brk)
    while len(out) < 2000:
        k = rng.randint(2, 5)
        n = rng.randint(1, 64)
        out.append("".join(rng.choice(letters[:k]) for _ in range(n)))
    assert all("$" not in w for w in out)
    return out


def lengths(factors):
    return " ".join(str(len(f)) for f in factors if f not in ("<<", ">>"))


def write_gz(name, data: bytes):
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as g:
            g.write(data)


def main():
    for name, fact, T in (("DNA1-ICFL.txt", ICFL_recursive, None),
                          ("DNA1-CFL_ICFL-10.txt", CFL_icfl, 10)):
        write_gz(name, dna1_lines(fact, T))
    rows = [[w, lengths(ICFL_recursive(w, None))] + [lengths(CFL_icfl(w, T)) for T in THRESHOLDS]
            for w in words()]
    write_gz("icfl_words.json",
             json.dumps({"thresholds": list(THRESHOLDS), "rows": rows}, separators=(",", ":")).encode())
    print({"words": len(rows)})


if __name__ == "__main__":
    main()
