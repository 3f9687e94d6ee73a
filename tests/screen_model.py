"""`screen` checker: the documented verb (doc/man/mash-screen.1) restated on the CPU from the
parts of the reference that are intact: hashSequence's counting (CommandScreen.cpp:280-384), the
pool's one MinHashHeap and its set size (CommandTaxScreen.cpp:347-370, MinHashHeap.h:45), the
sums, -w and output loops (CommandScreen.cpp:153-254), estimateIdentity (:259-278) and
pValueWithin (:386-406).

The contract is coded twice: `literal` walks dictionaries the way the reference lines do, one
hash at a time; `closed` is the form the GPU path computes, over sorted arrays (searchsorted +
bincount).  tests/test_screen_model.py compares the two.

Database rows are ascending distinct hash lists (already cut to the sketch size); `keys` is the
stream of window keys of the whole pool (window_keys below; reads_model.window_hashes in the
default canonical, case-folding setting).  In -w every holder of a counted key has shared >= 1,
so its score is > 0: the reference's `maxScore = 0` start never leaves a key without a winner.
"""
import numpy as np

import reads_model as RM


def estimate_identity(common, denom, k):
    """estimateIdentity, CommandScreen.cpp:259-278"""
    if common == denom:
        return 1.0
    if common == 0:
        return 0.0
    return (float(common) / float(denom)) ** (1.0 / k)


def p_value_within(oracle, x, set_size, kmer_space, size):
    """pValueWithin, CommandScreen.cpp:386-406 (r clamped without the message)"""
    if x == 0:
        return 1.0
    r = max(0.0, min(1.0, float(set_size) / kmer_space))
    return oracle.binomial_q(x - 1, r, size)


def window_keys(oracle, recs, k, seed=42, alphabet=b"ACGT", noncanonical=False,
                preserve_case=False):
    """hashSequence's keys in stream order.  The default setting is reads_model.window_hashes;
    noncanonical / preserve-case follow the same lines (CommandScreen.cpp:295-301, 330-361)."""
    if not noncanonical and not preserve_case:
        return RM.window_hashes(oracle, recs, k, seed, alphabet)
    use64 = RM.use64_of(k, alphabet)
    ok = bytearray(256)
    for c in alphabet:
        ok[c] = 1
    out = []
    for rec in recs:
        if len(rec) < k:
            continue
        seq = rec if preserve_case else rec.upper()
        rev = seq.translate(RM._COMPL)[::-1]
        n = len(seq)
        for i in range(n - k + 1):
            f = seq[i:i + k]
            if not all(ok[c] for c in f):
                continue
            r = rev[n - i - k:n - i]
            out.append(oracle.get_hash(f if (noncanonical or f <= r) else r, seed, use64))
    return out


def bottom_s(keys, s):
    """the pool's MinHashHeap: the s smallest distinct keys, ascending"""
    return np.unique(np.asarray(keys, np.uint64))[:s]


def set_size(keys, s, use64=True):
    return RM.set_size(bottom_s(keys, s), use64)


# ---- literal: dictionaries, one hash at a time ------------------------------------------------
def literal_counts(rows, keys):
    """hashTable / hashCounts (CommandScreen.cpp:87-102) and hashSequence's `hashCounts[key]++`
    (:366-369; u32: the reference's atomic<uint32_t>)"""
    table, counts = {}, {}
    for i, row in enumerate(rows):
        for h in row:
            h = int(h)
            if h not in table:
                counts[h] = 0
                table[h] = []
            table[h].append(i)
    for key in keys:
        key = int(key)
        if key in counts:
            counts[key] = (counts[key] + 1) & 0xFFFFFFFF
    return table, counts


def literal(rows, keys, k=21, winner=False, lengths=None, visit=None):
    """-> (shared, median) per reference.  visit: a function reordering a key's holder list
    before the -w loop reads it (the reference's unordered set); None = ascending index."""
    table, counts = literal_counts(rows, keys)
    n = len(rows)
    shared, depths = [0] * n, [[] for _ in range(n)]
    for i, row in enumerate(rows):
        for h in row:
            if counts[int(h)] >= 1:
                shared[i] += 1
                depths[i].append(counts[int(h)])
    if winner:                                                        # :153-202
        scores = [estimate_identity(shared[i], len(rows[i]), k) for i in range(n)]
        shared, depths = [0] * n, [[] for _ in range(n)]
        for h, indices in table.items():
            if counts[h] < 1:
                continue
            max_score, max_length, max_index = 0.0, 0, None
            for i in (visit(list(indices)) if visit else indices):
                if scores[i] > max_score:
                    max_score, max_index, max_length = scores[i], i, lengths[i]
                elif scores[i] == max_score and lengths[i] > max_length:
                    max_index, max_length = i, lengths[i]
            shared[max_index] += 1
            depths[max_index].append(counts[h])
    median = []
    for i in range(n):                                                # :208-211, :235
        d = sorted(depths[i])
        median.append(d[shared[i] // 2] if shared[i] > 0 else 0)
    return shared, median


# ---- closed form: sorted arrays ---------------------------------------------------------------
def closed_counts(rows, keys):
    """-> (U, count) with U the sorted distinct union of the rows"""
    rows = [np.asarray(r, np.uint64) for r in rows]
    U = np.unique(np.concatenate(rows + [np.zeros(0, np.uint64)]))
    keys = np.asarray(keys, np.uint64)
    cnt = np.zeros(len(U), np.uint64)
    if len(U) and len(keys):
        at = np.searchsorted(U, keys)
        hit = (at < len(U))
        hit[hit] = U[at[hit]] == keys[hit]
        cnt = np.bincount(at[hit], minlength=len(U)).astype(np.uint64)
    return U, (cnt & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def closed(rows, keys, k=21, winner=False, lengths=None, counts=None):
    """-> (shared, median) per reference.  counts = (U, count) skips the counting."""
    rows = [np.asarray(r, np.uint64) for r in rows]
    U, cnt = counts if counts is not None else closed_counts(rows, keys)
    slots = [np.searchsorted(U, r) for r in rows]
    n = len(rows)
    own = [np.ones(len(r), bool) for r in rows]
    if winner:
        shared = [int((cnt[s] > 0).sum()) for s in slots]
        score = np.array([estimate_identity(shared[i], len(rows[i]), k) for i in range(n)])
        length = np.asarray(lengths, np.uint64)
        # per entry of U its holders; the winner: score down, length down, index up
        owner = np.full(len(U), -1, np.int64)
        hold_u = np.concatenate(slots + [np.zeros(0, np.int64)]).astype(np.int64)
        hold_i = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(slots)] +
                                [np.zeros(0, np.int64)])
        order = np.lexsort((hold_i, (~length)[hold_i], -score[hold_i], hold_u))
        hu, hi = hold_u[order], hold_i[order]
        first = np.ones(len(hu), bool)
        first[1:] = hu[1:] != hu[:-1]
        owner[hu[first]] = hi[first]
        own = [owner[s] == i for i, s in enumerate(slots)]
    shared, median = [], []
    for s, o in zip(slots, own):
        c = cnt[s][o] if len(s) else np.zeros(0, np.uint32)
        c = np.sort(c[c > 0])
        shared.append(len(c))
        median.append(int(c[len(c) // 2]) if len(c) else 0)
    return shared, median


# ---- output (CommandScreen.cpp:215-253) -------------------------------------------------------
def lines(oracle, rows, names, comments, shared, median, setsize, k, kmer_space,
          identity_min=0.0, pvalue_max=1.0):
    out = []
    for i, row in enumerate(rows):
        if not (shared[i] != 0 or identity_min < 0.0):
            continue
        identity = estimate_identity(shared[i], len(row), k)
        if identity < identity_min:
            continue
        p = p_value_within(oracle, shared[i], setsize, kmer_space, len(row))
        if p > pvalue_max:
            continue
        out.append("%g\t%d/%d\t%d\t%g\t%s\t%s\n" % (identity, shared[i], len(row), median[i], p,
                                                   names[i], comments[i]))
    return "".join(out)


def screen_text(oracle, rows, names, comments, lengths, keys, s, k=21, use64=True,
                kmer_space=None, winner=False, identity_min=0.0, pvalue_max=1.0, counts=None,
                setsize=None):
    """stdout of `screen` for a database and a pool's window keys (or precomputed (U, count)
    and set size)"""
    shared, median = closed(rows, keys, k, winner, lengths, counts)
    if setsize is None:
        setsize = set_size(keys, s, use64)
    return lines(oracle, rows, names, comments, shared, median, setsize, k,
                 kmer_space if kmer_space is not None else 4.0 ** k, identity_min, pvalue_max)
