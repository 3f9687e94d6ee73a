"""Reads-mode checker: MinHashHeap::tryInsert with multiplicityMinimum = m and no Bloom filter
(MinHashHeap.cpp:68-146), restated in plain Python over the stream of window hashes that
addMinHashes produces (Sketch.cpp:664-735: uppercase, skip windows holding a byte outside the
alphabet, canonical = the smaller of the window and its reverse complement by memcmp, getHash).
Hashes come from the oracle's get_hash; the heap is two dicts and two heaps, taken one hash at a
time.  tests/test_reads_model.py pins it to the oracle's literal heap (m = 1) and to the closed
form the GPU path computes (m >= 2).  Shared inputs of the reads tests live here too.
"""
import heapq

import numpy as np

# complement of 'A'..'Z' (Sketch.cpp:1223-1250); other bytes never reach a compared window
_COMPL = bytes.maketrans(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", b"TVGHNNCDNNMNKNNNNYSAABWNRN")


def use64_of(k, alphabet=b"ACGT"):
    return float(len(alphabet)) ** k > 2.0 ** 32


def window_hashes(oracle, recs, k, seed=42, alphabet=b"ACGT"):
    """The hashes tryInsert sees, in stream order, for records taken in list order."""
    use64 = use64_of(k, alphabet)
    ok = bytearray(256)
    for c in alphabet:
        ok[c] = 1
    out = []
    for rec in recs:
        if len(rec) < k:
            continue
        seq = rec.upper()
        rev = seq.translate(_COMPL)[::-1]
        n = len(seq)
        bad = np.frombuffer(bytes(0 if ok[c] else 1 for c in seq), np.uint8)
        nbad = np.concatenate([[0], np.cumsum(bad)])
        for i in range(n - k + 1):
            if nbad[i + k] != nbad[i]:
                continue
            f = seq[i:i + k]
            r = rev[n - i - k:n - i]
            out.append(oracle.get_hash(r if f > r else f, seed, use64))
    return out


class ReadsHeap:
    """tryInsert, one hash at a time (line numbers: MinHashHeap.cpp)."""

    def __init__(self, s, m):
        self.s, self.m = s, m
        self.hashes = {}          # hash -> count (HashSet)
        self.queue = []           # max-heap of the hashes in `hashes` (negated)
        self.pending = {}         # hash -> count below m
        self.qpending = []        # max-heap of pending hashes (negated; may hold zombies)

    def try_insert(self, h):
        if not (len(self.hashes) < self.s or h < -self.queue[0]):        # :70-74
            return
        if h not in self.hashes:                                         # :76
            if self.m == 1 or self.pending.get(h, 0) == self.m - 1:      # :96
                self.hashes[h] = self.m
                heapq.heappush(self.queue, -h)
                self.pending.pop(h, None)
            else:                                                        # :110-118
                if h not in self.pending:
                    heapq.heappush(self.qpending, -h)
                self.pending[h] = self.pending.get(h, 0) + 1
        else:
            self.hashes[h] += 1                                          # :122
        if len(self.hashes) > self.s:                                    # :126-144
            top = -self.queue[0]
            del self.hashes[top]
            while self.qpending and top < -self.qpending[0]:
                self.pending.pop(-self.qpending[0], None)
                heapq.heappop(self.qpending)
            heapq.heappop(self.queue)

    def result(self):
        hs = sorted(self.hashes)
        return (np.array(hs, np.uint64), np.array([self.hashes[h] for h in hs], np.uint32))


def model_sketch(stream, s, m):
    """-> (ascending hashes u64, counts u32) of the heap after `stream`."""
    heap = ReadsHeap(s, m)
    for h in stream:
        heap.try_insert(h)
    return heap.result()


def closed_form(stream, s, m):
    """What the GPU path computes: F = the s smallest hashes with >= m occurrences, full counts,
    and for a full F the maximum's occurrences up to T = the last m-th occurrence among F."""
    pos = {}
    for i, h in enumerate(stream):
        pos.setdefault(h, []).append(i)
    F = sorted(h for h, p in pos.items() if len(p) >= m)[:s]
    counts = [len(pos[h]) for h in F]
    if len(F) == s:
        T = max(pos[h][m - 1] for h in F)
        counts[-1] = sum(1 for p in pos[F[-1]] if p <= T)
    return np.array(F, np.uint64), np.array(counts, np.uint32)


def set_size(hashes, use64=True):
    """MinHashHeap::estimateSetSize (MinHashHeap.h:45), truncated as Reference::length is."""
    if len(hashes) == 0:
        return 0
    return int((2.0 ** (64 if use64 else 32)) * float(len(hashes)) / float(int(max(hashes))))


def interleave(a, b):
    """sketchFile's round robin over two open files (Sketch.cpp:1352-1422): a record of each in
    turn; a file that has ended is left out."""
    out = []
    for i in range(max(len(a), len(b))):
        if i < len(a):
            out.append(a[i])
        if i < len(b):
            out.append(b[i])
    return out


# ---- shared inputs --------------------------------------------------------------------------
def _rand(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def mutate(rng, seq, rate):
    a = np.frombuffer(seq, np.uint8).copy()
    m = rng.random(len(a)) < rate
    a[m] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(m.sum()))]
    return a.tobytes()


def base_reads(seed=7):
    """A 3 kb genome at ~8x: 240 reads of 100 bp with 1 % substitutions, a few N and lowercase
    bytes (~19k windows, mostly single-copy)."""
    rng = np.random.default_rng(seed)
    genome = _rand(rng, 3000)
    reads = []
    for i in range(240):
        at = int(rng.integers(0, 2900))
        r = bytearray(mutate(rng, genome[at:at + 100], 0.01))
        if i % 17 == 0:
            r[int(rng.integers(0, 100))] = ord("N")
        if i % 5 == 0:
            j = int(rng.integers(0, 90))
            r[j:j + 10] = bytes(r[j:j + 10]).lower()
        reads.append(bytes(r))
    return reads


def order_inputs(oracle, seed=3):
    """Two orders of one record set, ([y, unit * 30, y], [y, y, unit * 30]), and a sketch size
    below unit's distinct k-mers whose maximum (at m = 2) is a hash of unit seen 30 times (a
    window inside one copy) with hashes of y below it."""
    rng = np.random.default_rng(seed)
    unit, y = _rand(rng, 97), _rand(rng, 300)
    inner = set(window_hashes(oracle, [unit], 21))            # windows inside one copy: 30 times
    yh = set(window_hashes(oracle, [y], 21))
    quals = sorted(set(window_hashes(oracle, [unit + unit[:20]], 21)) | yh)
    s = next(i + 1 for i, h in enumerate(quals)
             if i >= 20 and h in inner and any(q in yh for q in quals[:i]))
    assert s < 97
    return ([y, unit * 30, y], [y, y, unit * 30]), s


def widening_reads(seed=11):
    """20 kb of random sequence in 100-bp records plus a 60-bp unit in three separate records:
    at k = 21 the unit's 40 windows are the only hashes seen more than once (~1 in 500)."""
    rng = np.random.default_rng(seed)
    recs = [_rand(rng, 100) for _ in range(200)]
    unit = _rand(rng, 60)
    for at in (20, 90, 170):
        recs.insert(at, unit)
    return recs
