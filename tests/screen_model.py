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


# ---- closed form over a whole matrix: no loop over cells or keys ------------------------------
def _row_sums(C):
    """(shared, median) per row of a matrix of gathered counters (0: not counted)"""
    shared = (C > 0).sum(axis=1)
    # ascending with the zeros pushed past every counter: position shared // 2 is the median
    S = np.sort(np.where(C == 0, np.uint64(1) << np.uint64(32), C.astype(np.uint64)), axis=1)
    S = np.concatenate([S, np.zeros((len(S), 1), np.uint64)], axis=1)      # (a row of no cell)
    median = S[np.arange(len(S)), shared // 2]
    return shared.astype(np.uint32), np.where(shared > 0, median, 0).astype(np.uint32)


def closed_matrix(R, lens, keys, k=21, lengths=None):
    """`closed` and `closed_counts` for databases of 10^7 cells: R a (rows x stride) matrix, row
    i's hashes its first lens[i] cells.  -> dict: U, count, holders (the rows that hold each entry
    of U), shared, median and, with lengths
    (one per row), scores (estimate_identity of the plain shared counts), wshared and wmedian:
    -w by screen_winner_kernel's rule, the greatest score, then the greatest length, then the
    lowest index."""
    R = np.asarray(R)
    n = len(lens)
    R = R.reshape(n, R.size // n if n else 0)
    lens = np.asarray(lens, np.int64)
    inside = np.arange(R.shape[1])[None, :] < lens[:, None]
    U, inv = np.unique(R[inside].astype(np.uint64), return_inverse=True)
    inv = inv.reshape(-1)
    keys = np.asarray(keys, np.uint64)
    cnt = np.zeros(len(U), np.uint32)
    if len(U) and len(keys):
        at = np.searchsorted(U, keys)
        hit = at < len(U)
        hit[hit] = U[at[hit]] == keys[hit]
        cnt = (np.bincount(at[hit], minlength=len(U)) & 0xFFFFFFFF).astype(np.uint32)
    C = np.zeros(R.shape, np.uint32)
    C[inside] = cnt[inv]
    out = {"U": U, "count": cnt, "holders": np.bincount(inv, minlength=len(U))}
    out["shared"], out["median"] = _row_sums(C)
    if lengths is None:
        return out
    score = np.array([estimate_identity(int(a), int(l), k) for a, l in zip(out["shared"], lens)])
    length = np.asarray(lengths, np.uint64)
    # rows in the order -w prefers them; an entry goes to the first of its holders in that order
    by_rank = np.lexsort((np.arange(n), ~length, -score))
    rank = np.empty(n, np.int64)
    rank[by_rank] = np.arange(n)
    row_of = np.broadcast_to(np.arange(n)[:, None], R.shape)[inside]
    best = np.full(len(U), n, np.int64)
    np.minimum.at(best, inv, rank[row_of])
    owner = np.append(by_rank, -1)[best]                 # (every entry of U has a holder)
    W = np.zeros(R.shape, np.uint32)
    W[inside] = np.where(owner[inv] == row_of, cnt[inv], 0)
    out["scores"] = score
    out["wshared"], out["wmedian"] = _row_sums(W)
    return out


# ---- the inputs of tests/test_gpu_screen_scale.py ---------------------------------------------
SCALE_SHARED = 3000          # keys a few rows share
SCALE_SHARED_ROWS = 5        # ... at most so many rows each


def scale_holders():
    """an upper bound of the cells scale_db gives to shared keys: the database has at least
    rows * width - scale_holders() distinct values"""
    return SCALE_SHARED * SCALE_SHARED_ROWS


def _distinct(rng, n, dtype):
    """n distinct values in random order, away from both ends of the type's range"""
    top = min(int(np.iinfo(dtype).max), 2 ** 63) - 256
    v = np.zeros(0, np.uint64)
    while len(v) < n:
        v = np.unique(np.concatenate([v, rng.integers(256, top, size=n - len(v) + n // 64 + 64,
                                                      dtype=np.uint64)]))
    return rng.permutation(v)[:n].astype(dtype)


def scale_db(seed, n, width, dtype=np.uint64, heavy=0, heavy_rows=0):
    """n strictly ascending rows of `width` cells: values drawn without replacement over the
    whole matrix, so distinct within every row, then SCALE_SHARED keys each put into 2 ..
    SCALE_SHARED_ROWS rows; with heavy > 0, `heavy` further keys held by heavy_rows rows each
    (random values like all others, not clustered).  -> (matrix, the heavy keys)"""
    rng = np.random.default_rng(seed)
    k_row = np.zeros(n, np.int64)
    member = np.zeros((n, 0), bool)
    if heavy:
        # per heavy key the heavy_rows rows with the smallest of n random numbers
        member = np.zeros((heavy, n), bool)
        pick = np.argpartition(rng.random((heavy, n)), heavy_rows, axis=1)[:, :heavy_rows]
        member[np.arange(heavy)[:, None], pick] = True
        member = np.ascontiguousarray(member.T)
        k_row = member.sum(axis=1)
        assert k_row.max() < width - 8
    n_light = int(n * width - k_row.sum())
    vals = _distinct(rng, n_light + heavy + SCALE_SHARED, dtype)
    light, hv, shared = np.split(vals, [n_light, n_light + heavy])
    R = np.empty((n, width), dtype)
    is_light = np.arange(width)[None, :] >= k_row[:, None]
    R[is_light] = light
    R[~is_light] = hv[np.nonzero(member)[1]]
    for key in shared:
        rows = rng.choice(n, size=int(rng.integers(2, SCALE_SHARED_ROWS + 1)), replace=False)
        cols = k_row[rows] + (rng.random(len(rows)) * (width - k_row[rows])).astype(np.int64)
        R[rows, cols] = key                      # (over a light cell, maybe an earlier shared key)
    R.sort(axis=1)
    assert (R[:, 1:] > R[:, :-1]).all()
    return R, hv.astype(np.uint64)


def scale_pool(seed, U, draws, hot=None):
    """pool keys: `draws` draws with repeats from a tenth of U, skewed so counters run from 1 to
    some tens, every key of `hot` a few times, and misses: below U[0], above U[-1], 0, the
    largest u64, and neighbours of present keys"""
    rng = np.random.default_rng(seed)
    some = rng.choice(len(U), size=max(len(U) // 10, 1), replace=False)
    keys = [U[some[(len(some) * rng.random(draws) ** 2).astype(np.int64)]]]
    if hot is not None and len(hot):
        keys.append(np.repeat(hot, rng.integers(1, 6, size=len(hot))))
    at = rng.integers(0, len(U), size=2000)
    miss = np.concatenate([U[at] + np.uint64(1), U[at] - np.uint64(1),
                           np.array([0, U[0] - np.uint64(1), U[-1] + np.uint64(1), 2 ** 64 - 1],
                                    np.uint64),
                           rng.integers(0, 2 ** 64, size=1000, dtype=np.uint64)])
    miss = miss[U[np.clip(np.searchsorted(U, miss), 0, len(U) - 1)] != miss]
    keys.append(miss)
    return rng.permutation(np.concatenate(keys).astype(np.uint64)), miss


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
