#!/usr/bin/env python3
"""Generate the long-read and factor-text k-finger fixtures in tests/golden/ (build container
only, with the reference tree present, as make_kfinger_comb_golden.py).

Everything written here is output of lyn2vec's own code, imported from the reference tree and
run as it is: compute_long_fingerprint_by_list (fingerprint_utils.py:480-518, `--type generalized
--split N --fact create`) and compute_fingerprint_by_list('create', 'shift', ...) (:443-476,
`--type basic --fact create`), over read lines built by seqio, which goes round lyn2vec's own
readers as the other generators do.  The long-read ID is the record's name, the first token of
its header; the window-mode ID is the comment's first token with "_0".

  DNA1-long300-CFL_ICFL-30.txt.gz, DNA1-long300-CFL_ICFL-30.fact.txt.gz   the first three records
      of DNA1.fasta at split 300 under CFL_ICFL-30 (lyn2vec's documented command): fingerprint
      and factor lines
  DNA1-long150-ICFL_COMB.txt.gz, DNA1-long150-ICFL_COMB.fact.txt.gz   the same at split 150 under
      ICFL_COMB
  DNA1-CFL.fact.txt.gz, DNA1-ICFL_COMB.fact.txt.gz   the factor lines of the first record of
      DNA1.fasta in window mode (w = 100) under CFL and ICFL_COMB
  long_words.json.gz   200 words over ACGTN of 1 to 40 bytes (every length for one letter and for
      the period TTG; random words over 1 to 5 letters, short ones more often); {"splits": [1, 2, 3, 7, 40],
      "facts": [CFL, ICFL, CFL_ICFL-3, CFL_COMB, ICFL_COMB, CFL_ICFL_COMB-3], "rows": [word, then
      for every split and, within it, every factorization, the fingerprint line and the factor
      line of the read line "w <word>"]}

Run:  python tests/golden/make_kfinger_long_golden.py <reference root>
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
sys.dont_write_bytecode = True
sys.path.insert(0, LYN2VEC)
sys.path.insert(0, os.path.dirname(HERE))
from factorizations import CFL, ICFL_recursive, CFL_icfl  # noqa: E402
from factorizations_comb import d_cfl, d_icfl, d_cfl_icfl  # noqa: E402
from fingerprint_utils import compute_fingerprint_by_list, \
    compute_long_fingerprint_by_list  # noqa: E402
import seqio  # noqa: E402

# lyn2vec.py:47-72, 131-156: the name -> (function, T)
FACTS = {"CFL": (CFL, None), "ICFL": (ICFL_recursive, None), "CFL_ICFL-3": (CFL_icfl, 3),
         "CFL_ICFL-30": (CFL_icfl, 30), "CFL_COMB": (d_cfl, None), "ICFL_COMB": (d_icfl, None),
         "CFL_ICFL_COMB-3": (d_cfl_icfl, 3)}
WORD_FACTS = ("CFL", "ICFL", "CFL_ICFL-3", "CFL_COMB", "ICFL_COMB", "CFL_ICFL_COMB-3")
SPLITS = (1, 2, 3, 7, 40)
DNA1 = os.path.join(HERE, "DNA1.fasta")


def records(n):
    recs = seqio.read_records(DNA1)[:n]
    assert all(set(s.upper()) <= set(b"ACGTN") for _n, _c, s in recs)
    return recs


def long_lines(reads, fact, split):
    f, T = FACTS[fact]
    lines, fact_lines = compute_long_fingerprint_by_list("create", f, T, split, reads)
    assert len(lines) == len(fact_lines) == len(reads)
    return "".join(lines).encode(), "".join(fact_lines).encode()


def window_fact_lines(reads, fact):
    f, T = FACTS[fact]
    _lines, fact_lines = compute_fingerprint_by_list("create", "shift", f, T, reads)
    return "".join(fact_lines).encode()


def words():
    rng = random.Random(20243)
    out = []
    for n in range(1, 41):
        out.append("A" * n)
        out.append(("TTG" * 14)[:n])
    while len(out) < 200:
        k = rng.randint(1, 5)
        out.append("".join(rng.choice("ACGTN"[:k]) for _ in range(rng.randint(1, rng.randint(1, 40)))))
    return out


def write_gz(name, data: bytes):
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as g:
            g.write(data)


def main():
    reads = [f"{n.decode()} {s.decode().upper()}" for n, _c, s in records(3)]
    for split, fact in ((300, "CFL_ICFL-30"), (150, "ICFL_COMB")):
        text, fact_text = long_lines(reads, fact, split)
        write_gz(f"DNA1-long{split}-{fact}.txt", text)
        write_gz(f"DNA1-long{split}-{fact}.fact.txt", fact_text)
    first = [f"{c.split()[0].decode()}_0 {s.decode().upper()}" for _n, c, s in records(1)]
    for fact in ("CFL", "ICFL_COMB"):
        write_gz(f"DNA1-{fact}.fact.txt", window_fact_lines(first, fact))
    rows = []
    for w in words():
        row = [w]
        for split in SPLITS:
            for fact in WORD_FACTS:
                row += [x.decode() for x in long_lines([f"w {w}"], fact, split)]
        rows.append(row)
    write_gz("long_words.json",
             json.dumps({"splits": list(SPLITS), "facts": list(WORD_FACTS), "rows": rows},
                        separators=(",", ":")).encode())
    print({"words": len(rows)})


if __name__ == "__main__":
    main()
