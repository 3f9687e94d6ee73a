"""Synthetic inputs in the formats the reference's configs use.

- DNA FASTA in lyn2vec's `--type generate` shape (dna_utils.py:7-83,
  lyn2vec.py:196-227): header `>T00000XXXXXXXX G00000XXXXXXXX`, 70-column lines,
  GC-biased uniform bases.  Seeded numpy instead of the reference's unseeded
  random.random() so runs are reproducible.
- Family-structured variants (ancestor + members with a substitution rate) so
  that dist has non-trivial shared-hash counts (unrelated random genomes give
  common = 0 for nearly every pair).
- CFL k-finger text (lyn2vec `--type basic --type_factorization CFL`; also ICFL, CFL_ICFL-T and
  the combined CFL_COMB, ICFL_COMB, CFL_ICFL_COMB-T of factorizations_comb.py:178-246;
  fingerprint_utils.py:95-110, 443-476; factorizations.py:102-126): one line per
  100-char cyclic window, `<Gid>_0 l1 l2 ...` with the Lyndon factor lengths of
  Duval's algorithm.
"""
from __future__ import annotations

import numpy as np

_B = np.frombuffer(b"ACGT", dtype=np.uint8)
_ID_ALPHA = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ", dtype=np.uint8)


def random_dna(n, length, gc=0.5, seed=0):
    """n sequences of `length` bases; P(G)=P(C)=gc/2, P(A)=P(T)=(1-gc)/2."""
    rng = np.random.default_rng(seed)
    p = np.array([(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2])
    codes = rng.choice(4, size=(n, length), p=p).astype(np.uint8)
    arr = _B[codes]
    return [arr[i].tobytes() for i in range(n)]


def family_dna(n_families, members, length, sub_rate=(0.01, 0.10), gc=0.5, seed=0):
    """members per family: an ancestor mutated at a per-member substitution rate."""
    rng = np.random.default_rng(seed)
    anc = random_dna(n_families, length, gc, seed + 7919)
    out = []
    for f in range(n_families):
        a = np.frombuffer(anc[f], dtype=np.uint8)
        for _ in range(members):
            rate = rng.uniform(*sub_rate)
            m = a.copy()
            hit = rng.random(length) < rate
            m[hit] = _B[rng.integers(0, 4, size=int(hit.sum()))]
            out.append(m.tobytes())
    return out


def lyn2vec_ids(n, seed=0):
    rng = np.random.default_rng(seed + 104729)
    tails = _ID_ALPHA[rng.integers(0, len(_ID_ALPHA), size=(n, 8))]
    return [t.tobytes().decode() for t in tails]


def fasta_bytes(seqs, ids=None, width=70):
    """lyn2vec-style FASTA: `>T00000<id> G00000<id>` then `width`-column lines."""
    if ids is None:
        ids = lyn2vec_ids(len(seqs))
    parts = []
    for s, i in zip(seqs, ids):
        parts.append(f">T00000{i} G00000{i}\n".encode())
        for o in range(0, len(s), width):
            parts.append(s[o:o + width] + b"\n")
    return b"".join(parts)


def duval_cfl_lengths(word: bytes):
    """Lyndon factor lengths of `word` (Duval; factorizations.py:102-126)."""
    out = []
    n = len(word)
    k = 0
    while k < n:
        i, j = k, k + 1
        while j < n and word[i] <= word[j]:
            i = k if word[i] < word[j] else i + 1
            j += 1
        while k <= i:
            out.append(j - i)
            k += j - i
    return out


def icfl_lengths(word: bytes, stats=None):
    """Inverse Lyndon factor lengths of `word`: the iterative form of lyn2vec's ICFL_recursive
    (factorizations.py:143-169 with find_pre :172-189, find_bre :212-232, border :235-248).
    The end of the word is known out of band, so a 0x24 byte is a byte like any other.

    Forward, from s = 0: scan word[s:] while it descends; where it stops at j before the end,
    the step's `last` is the shortest border b of word[s:s+j] (0 included) whose next byte is
    below word[s+j], or the longest border when none is; s advances by j - last.  The rest is the
    last factor.  Then right to left: a step's piece starts a new factor when the factor after it
    is longer than the step's `last`, and is glued onto that factor otherwise.

    stats, a dict, accumulates over calls: "steps", "merges" (pieces glued), "chain" (the longest
    border chain walked, in links) and "last" (the largest `last`)."""
    n = len(word)
    steps = []          # (start, last)
    s = 0
    chain_max = 0
    while True:
        w = word[s:]
        m = n - s
        i, j = 0, 1
        while j < m and w[j] <= w[i]:
            i = 0 if w[j] < w[i] else i + 1
            j += 1
        if j >= m:
            break
        f = [0] * j
        k = 0
        for e in range(1, j):
            while k > 0 and w[k] != w[e]:
                k = f[k - 1]
            if w[k] == w[e]:
                k += 1
            f[e] = k
        b = last = f[j - 1]
        links = 1
        while True:
            if w[b] < w[j]:
                last = b
            if b == 0:
                break
            b = f[b - 1]
            links += 1
        chain_max = max(chain_max, links)
        steps.append((s, last))
        s += j - last
    out = [n - s] if n else []
    end = s
    merges = 0
    for start, last in reversed(steps):
        if out[0] > last:
            out.insert(0, end - start)
        else:
            out[0] += end - start
            merges += 1
        end = start
    if stats is not None:
        stats["steps"] = stats.get("steps", 0) + len(steps)
        stats["merges"] = stats.get("merges", 0) + merges
        stats["chain"] = max(stats.get("chain", 0), chain_max)
        stats["last"] = max([stats.get("last", 0)] + [l for _, l in steps])
    return out


def cfl_icfl_lengths(word: bytes, T: int, stats=None):
    """lyn2vec's CFL_icfl (factorizations.py:265-301) without its << >> markers
    (fingerprint_utils.py:443-476 drops them): a Lyndon factor of at most T bytes is kept, a
    longer one gives way to its own inverse Lyndon factors."""
    out = []
    k = 0
    for ln in duval_cfl_lengths(word):
        if ln <= T:
            out.append(ln)
        else:
            out.extend(icfl_lengths(word[k:k + ln], stats))
        k += ln
    return out


COMB_REV_THRESHOLD = 30   # cfl_icfl_'s default cfl_max (factorizations_comb.py:164)
_COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def reverse_complement(word: bytes):
    """lyn2vec's reverse_complement (factorizations_comb.py:8-10) of an upper-cased word: A <-> T,
    C <-> G, N -> N; every other byte, on which lyn2vec raises KeyError, is its own complement"""
    return word[::-1].translate(_COMPLEMENT)


def comb_lengths(word: bytes, fwd, rev):
    """lyn2vec's d_duval_ (factorizations_comb.py:213-246) in closed form: the gaps between the
    cuts of fwd(word) together with the cuts of rev(reverse_complement(word)) mirrored to
    n - c; a cut both share is one cut"""
    n = len(word)
    cuts = set()
    at = 0
    for ln in fwd(word):
        at += ln
        cuts.add(at)
    at = 0
    for ln in rev(reverse_complement(word)):
        cuts.add(n - at)
        at += ln
    cuts.discard(0)
    out, prev = [], 0
    for c in sorted(cuts):
        out.append(c - prev)
        prev = c
    return out


def factor_lengths(word: bytes, factorization="CFL", stats=None):
    """the factor lengths of `word` under "CFL", "ICFL" or "CFL_ICFL-<T>", or under the combined
    "CFL_COMB", "ICFL_COMB" or "CFL_ICFL_COMB-<T>", whose reverse side runs at threshold 30
    whatever T is, as lyn2vec's does (the binding's parse_factorization reads the name)"""
    from . import parse_factorization
    kind, T = parse_factorization(factorization)
    if kind == "CFL":
        return duval_cfl_lengths(word)
    if kind == "ICFL":
        return icfl_lengths(word, stats)
    if kind == "CFL_ICFL":
        return cfl_icfl_lengths(word, T, stats)
    if kind == "CFL_COMB":
        return comb_lengths(word, duval_cfl_lengths, duval_cfl_lengths)
    if kind == "ICFL_COMB":
        return comb_lengths(word, lambda w: icfl_lengths(w, stats), lambda w: icfl_lengths(w, stats))
    return comb_lengths(word, lambda w: cfl_icfl_lengths(w, T, stats),
                        lambda w: cfl_icfl_lengths(w, COMB_REV_THRESHOLD, stats))


def cfl_lines(seq: bytes, gid: str, window=100, factorization="CFL"):
    """k-finger lines of one sequence (fingerprint_utils.py:95-110, 443-476)."""
    s = seq.upper()
    lines = []
    if len(s) < window:
        shifts = [s]
    else:
        ss = s + s[:window]
        shifts = [ss[i:i + window] for i in range(len(s))]
    for w in shifts:
        lines.append(f"{gid}_0 " + " ".join(str(x) for x in factor_lengths(w, factorization)) + "\n")
    return lines


def cfl_text(seqs, ids, window=100, factorization="CFL"):
    return "".join(l for s, i in zip(seqs, ids)
                   for l in cfl_lines(s, "G00000" + i, window, factorization)).encode()


def cfl_text_fast(seqs, ids, window=100, threads=None, factorization="CFL"):
    """cfl_text through the C++ generator (bin/cflgen, same bytes): C3-scale inputs
    (5,000 x 2 kb -> 10 M lines) in seconds instead of minutes."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "cflgen")
    inp = b"".join(i.encode() + b"\t" + s + b"\n" for s, i in zip(seqs, ids))
    args = [exe, str(window)] + ([str(threads)] if threads else [])
    if factorization != "CFL":
        from . import parse_factorization
        parse_factorization(factorization)
        # cflgen takes the name third, so the thread count is always given: the CPUs at hand,
        # 16 at the most
        args = [exe, str(window), str(threads or min(os.cpu_count() or 1, 16)), factorization]
    return subprocess.run(args, input=inp, stdout=subprocess.PIPE, check=True).stdout
