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


def _windows(recs, k, alphabet):
    """(record index, window index, forward window, reverse-complement window) of every window
    addMinHashes hashes: records shorter than k and windows holding a byte outside the alphabet
    are passed over (such a window emits nothing but keeps its index)."""
    ok = bytearray(256)
    for c in alphabet:
        ok[c] = 1
    for ri, rec in enumerate(recs):
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
            yield ri, i, seq[i:i + k], rev[n - i - k:n - i]


def window_hashes(oracle, recs, k, seed=42, alphabet=b"ACGT", noncanonical=False):
    """The hashes tryInsert sees, in stream order, for records taken in list order.
    noncanonical (Sketch.cpp:723): the forward window is hashed as it stands."""
    use64 = use64_of(k, alphabet)
    return [oracle.get_hash(f if noncanonical or f <= r else r, seed, use64)
            for _, _, f, r in _windows(recs, k, alphabet)]


def window_positions(recs, k, alphabet=b"ACGT"):
    """-> int64 [n, 2]: (record index in `recs`, window index within that record) of every hash
    window_hashes emits, in the same order: row i maps stream index i to its window.  For one
    long record (cut into 4096-window chunk tiles) the tile of a window is window // 4096."""
    return np.array([(ri, i) for ri, i, _, _ in _windows(recs, k, alphabet)],
                    np.int64).reshape(-1, 2)


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


MUTANTS = ("t_minus_1", "tile_skip_ge", "m_plus_1", "m_minus_1", "no_cut")
_NEVER = float("inf")


def closed_form(stream, s, m, detail=False, mutant=None, tile_floor=None):
    """What the GPU path computes: F = the s smallest hashes with >= m occurrences, full counts,
    and for a full F the maximum's occurrences up to T = the last m-th occurrence among F.
    detail: also T (a stream index; None when F is not full) and the stream indices of the
    maximum's occurrences (of F[-1]; empty when F is).
    mutant: a wrong closed form, to prove on the CPU that an input tells it from the true one
    (never what a result is compared with):
      t_minus_1     the cut is T - 1: `pos <= T` taken as `pos < T`
      tile_skip_ge  the cut is tile_floor(T) - 1, tile_floor(i) = the stream index of the first
                    window of the tile that holds window i: the skip `byte_off > T` taken as `>=`
                    drops T's own tile, and every later one with it
      m_plus_1      T from the (m+1)-th occurrences (slot m of the chain in place of slot m - 1;
                    a hash without one leaves its slot empty: no cut)
      m_minus_1     T from the (m-1)-th occurrences (m >= 2)
      no_cut        the maximum keeps its full count"""
    pos = {}
    for i, h in enumerate(stream):
        pos.setdefault(h, []).append(i)
    F = sorted(h for h, p in pos.items() if len(p) >= m)[:s]
    counts = [len(pos[h]) for h in F]
    T = None
    if len(F) == s:
        T = cut = max(pos[h][m - 1] for h in F)
        if mutant == "t_minus_1":
            cut = T - 1
        elif mutant == "tile_skip_ge":
            cut = tile_floor(T) - 1
        elif mutant == "m_plus_1":
            cut = max(pos[h][m] if len(pos[h]) > m else _NEVER for h in F)
        elif mutant == "m_minus_1":
            assert m >= 2
            cut = max(pos[h][m - 2] for h in F)
        elif mutant == "no_cut":
            cut = _NEVER
        else:
            assert mutant is None, mutant
        counts[-1] = sum(1 for p in pos[F[-1]] if p <= cut)
    out = np.array(F, np.uint64), np.array(counts, np.uint32)
    if detail:
        return out + (T, list(pos[F[-1]]) if F else [])
    return out


def maximum_count(stream, s, m, mutant=None, tile_floor=None):
    """The count closed_form (or one of its mutants) gives the maximum of a full F."""
    h, c = closed_form(stream, s, m, mutant=mutant, tile_floor=tile_floor)
    assert len(h) == s
    return int(c[-1])


def tile_floor_of(positions, tile=4096):
    """closed_form's tile_floor for a stream whose windows all lie in one long record (cut into
    chunk tiles of `tile` windows): positions = window_positions(...) of that stream."""
    win = positions[:, 1]
    assert len(set(positions[:, 0].tolist())) <= 1 and np.all(np.diff(win) > 0)

    def floor(i):
        return int(np.searchsorted(win, win[i] // tile * tile))
    return floor


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


# ---- inputs of the edge tests (tests/test_gpu_reads_edges.py; their preconditions and the
# mutant asserts run on the CPU in tests/test_reads_model.py) -----------------------------------
# Every builder is deterministic (seeded), asserts what its test relies on, and is cached: the
# CPU and the GPU tests of one session share one copy, which they leave unchanged.
import functools                                                         # noqa: E402
from types import SimpleNamespace                                        # noqa: E402

TILE = 4096                 # windows of a chunk tile of a long record (kChunkKmers)
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"


def _rand_over(rng, n, alphabet):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def _single_copy_kmers(oracle, recs, k, alphabet=b"ACGT", noncanonical=False):
    """hash -> its (forward) window, for records whose windows are all single-copy"""
    hs = window_hashes(oracle, recs, k, alphabet=alphabet, noncanonical=noncanonical)
    wins = [f for _, _, f, _ in _windows(recs, k, alphabet)]
    assert len(set(hs)) == len(hs) == sum(len(r) - k + 1 for r in recs)
    return dict(zip(hs, wins))


def qualifiers(stream, m):
    """the hashes seen >= m times, ascending"""
    h, c = np.unique(np.array(stream, np.uint64), return_counts=True)
    return [int(x) for x in h[c >= m]]


def _canon(w):
    r = w.translate(_COMPL)[::-1]
    return w if w <= r else r


def _canon_windows(seq, k):
    return [_canon(seq[i:i + k]) for i in range(len(seq) - k + 1)]


def _clean_chain(body, template, pool, kmer, k, rng, tries=200):
    """k-mers to append to `body`, one per entry of `template` (a hash: that k-mer; None: any
    k-mer of `pool` not yet used), such that no window across a junction (the k - 1 windows that
    start in one piece and end in the next) is a window of `body` or of another junction.
    Appended as they are, two k-mers of `body` often make such a window: the last j letters of
    one followed by the next letters of the other spell the window j places on in `body` with
    probability 4^-j.  Greedy over a shuffled pool, again from the start at a dead end."""
    seen = set(_canon_windows(body, k))
    for _ in range(tries):
        free = [pool[i] for i in rng.permutation(len(pool))]
        used, prev, out = set(), body, []
        for at, want in enumerate(template):
            # a free entry before a fixed one must fit that one too
            after = template[at + 1] if want is None and at + 1 < len(template) else None
            for h in ([want] if want is not None else free):
                j = _canon_windows(prev[-(k - 1):] + kmer[h][:k - 1], k)
                if after is not None:
                    j += _canon_windows(kmer[h][-(k - 1):] + kmer[after][:k - 1], k)
                if len(set(j)) == len(j) and not (set(j) & seen) and not (set(j) & used):
                    break
            else:
                break                                        # dead end
            j = j[:k - 1]
            used.update(j)
            if want is None:
                free.remove(h)
            out.append(h)
            prev = kmer[h]
        else:
            return out
    raise AssertionError("no clean chain")


PLANTED_N = 12
# case -> planted_record's (variant, m, target, seed); b is a with T on its tile's last window.
# (e's seed: one whose maximum has neighbours enough that make clean junctions on both sides)
PLANTED = {"a": ("a", 2, 0, 41), "b": ("a", 2, TILE - 1, 41), "c": ("c", 2, 0, 41),
           "d": ("d", 2, 0, 41), "e": ("e", 2, 0, 44),
           "a-m3": ("a", 3, 0, 41), "b-m3": ("a", 3, TILE - 1, 41), "c-m3": ("c", 3, 0, 41),
           "d-m3": ("d", 3, 0, 41),
           "a-m4": ("a", 4, 0, 41), "b-m4": ("a", 4, TILE - 1, 41), "c-m4": ("c", 4, 0, 41)}


@functools.lru_cache(maxsize=None)
def planted_record(oracle, variant, m=2, target=0, seed=41):
    """One record b"N" * pad + B + kmer(f_1) + ... (k = 21): B is 6,000 random bases, the f_i
    are PLANTED_N of its 21-mers by hash rank (every third of the smallest), M the largest.  The
    tail repeats them m - 1 times, so with s = PLANTED_N the sketch F is exactly the planted
    set and is full; the last k-mer of the tail holds T.  pad puts T on window `target` of its
    4,096-window tile (the run of N shifts every window and adds no hash).  The tail's order is
    one whose junction windows are new (_clean_chain), so that B's windows and every junction
    window stay below m copies (single-copy at m = 2), which is asserted.
      a  M last in the tail: M's m-th copy is at T            -> M counts m of m
      c  a + one more copy of M right after it, in T's tile   -> m of m + 1
      d  a + 4,075 random bases and then the extra copy, which so starts the next tile
                                                              -> m of m + 1
      e  (m = 2) M's second copy early, another hash last, M again before and after it
                                                              -> 3 of 4
    -> recs, k, s, m, stream, positions (window_positions), T (stream index), t_window, M,
    expect (M's count), total (M's occurrences), extra_window (c, d: the extra copy's)."""
    k = 21
    rng = np.random.default_rng(seed)
    B = _rand(rng, 6000)
    kmer = _single_copy_kmers(oracle, [B], k)
    D = sorted(kmer)
    planted = [D[3 * i] for i in range(PLANTED_N)]
    M = planted[-1]
    assert variant in ("a", "c", "d", "e") and (variant != "e" or m == 2)
    others = [None] * (PLANTED_N - 1)
    expect, total = (3, 4) if variant == "e" else (m, m + (variant in ("c", "d")))
    s = PLANTED_N
    for _ in range(50):
        # the order of one pass over the planted k-mers, its junction windows new; the junctions
        # the rest adds (between passes, around the filler) by trial: the asserts below hold
        if variant == "e":
            tail = _clean_chain(B, others[:2] + [M] + others[2:-1] + [M, None, M], planted[:-1],
                                kmer, k, rng)
        else:
            order = _clean_chain(B, others + [M] + [M] * (variant == "c"), planted[:-1], kmer, k,
                                 rng)
            tail = order[:PLANTED_N] * (m - 1) + order[PLANTED_N:]
        body = B + b"".join(kmer[h] for h in tail)
        if variant == "d":
            body += _rand(rng, TILE - k) + kmer[M]
        stream0 = window_hashes(oracle, [body], k)
        if qualifiers(stream0, m) == planted:
            break
    t0 = closed_form(stream0, s, m, detail=True)[2]
    pad = (target - int(window_positions([body], k)[t0, 1])) % TILE
    recs = [b"N" * pad + body]
    stream = window_hashes(oracle, recs, k)
    positions = window_positions(recs, k)
    assert stream == stream0 and int(positions[0, 1]) == pad
    assert qualifiers(stream, m) == planted                  # B's and the junctions' stay below m
    h, c, T, occ = closed_form(stream, s, m, detail=True)
    t_window = int(positions[T, 1])
    assert T == t0 and t_window % TILE == target
    assert [int(x) for x in h] == planted and int(c[-1]) == expect and len(occ) == total
    extra_window = None
    if variant in ("a", "c", "d"):
        assert occ[m - 1] == T                               # the maximum occurs exactly at T
    if variant in ("c", "d"):
        extra_window = int(positions[occ[-1], 1])
        if variant == "c":
            assert extra_window == t_window + k and extra_window // TILE == t_window // TILE
        else:
            assert extra_window == t_window + TILE and target == 0
    if variant == "e":
        assert occ[1] < occ[2] < T < occ[3]
    return SimpleNamespace(recs=recs, k=k, s=s, m=m, stream=stream, positions=positions, T=T,
                           t_window=t_window, M=M, expect=expect, total=total,
                           extra_window=extra_window)


@functools.lru_cache(maxsize=None)
def mult_record(oracle, target, seed=43):
    """-M on a planted position: b"N" * pad + B + b"N" + kmer(M).  s is the largest rank <= 64 whose
    hash M first occurs later than every smaller hash of B, so T_top (closed_form at m = 1: the
    last first occurrence among the sketch) is M's own first window; pad puts it on window
    `target` of its tile; the appended copy lies after T_top: M counts 1 of 2."""
    k = 21
    rng = np.random.default_rng(seed)
    B = _rand(rng, 6000)
    kmer = _single_copy_kmers(oracle, [B], k)
    first = {h: i for i, h in enumerate(window_hashes(oracle, [B], k))}
    D = sorted(kmer)
    s, latest = 0, -1
    for i, h in enumerate(D[:64]):
        if first[h] > latest:
            s, latest = i + 1, first[h]
    assert s >= 8                                            # (by the seed) not a trivial sketch
    M = D[s - 1]
    pad = (target - first[M]) % TILE
    recs = [b"N" * pad + B + b"N" + kmer[M]]                 # (the N: no junction window at all)
    stream = window_hashes(oracle, recs, k)
    positions = window_positions(recs, k)
    h, c, T, occ = closed_form(stream, s, 1, detail=True)
    assert [int(x) for x in h] == D[:s]
    assert len(occ) == 2 and occ[0] == T and int(c[-1]) == 1
    assert int(positions[T, 1]) % TILE == target
    return SimpleNamespace(recs=recs, k=k, s=s, m=1, stream=stream, positions=positions, T=T,
                           t_window=int(positions[T, 1]), M=M, expect=1, total=2)


@functools.lru_cache(maxsize=None)
def periodic_record(unit_len, reps, seed=47):
    """unit * reps: unit_len distinct windows, each seen ~reps times: one to two tiles in which
    every window contends for one of unit_len chains of position slots."""
    return _rand(np.random.default_rng(seed), unit_len) * reps


PERIODIC = ((64, 66), (61, 70))


@functools.lru_cache(maxsize=None)
def copies_ladder(oracle, k=21, alphabet=b"ACGT", noncanonical=False, flip_odd=False, seed=53):
    """20 single-copy 100-letter reads; hash D[2 i] (i < 40, D their hashes in order) is given
    1 + i % 9 copies in all by i % 9 extra records of its k-mer alone, in shuffled order, so at
    every m = 2..9 some hashes have exactly m - 1 and some exactly m copies, and a maximum's
    copies lie on both sides of T.  flip_odd (DNA): the extra records of odd i hold the reverse
    complement: the same hash when canonical, another when not.
    -> (records, the 40 hashes)"""
    rng = np.random.default_rng(seed)
    reads = [_rand_over(rng, 100, alphabet) for _ in range(20)]
    kmer = _single_copy_kmers(oracle, reads, k, alphabet, noncanonical)
    D = sorted(kmer)
    extra = []
    for i in range(40):
        w = kmer[D[2 * i]]
        if flip_odd and i % 2:
            w = w.translate(_COMPL)[::-1]
        extra += [w] * (i % 9)
    extra = [extra[i] for i in rng.permutation(len(extra))]
    return tuple(reads + extra), tuple(D[2 * i] for i in range(40))


def ladder_sizes(stream, m):
    """sketch sizes below and above the number of qualifiers q: the largest s < q at which the
    maximum has copies after T (q // 2 where there is none), and q + 3"""
    q = len(qualifiers(stream, m))
    assert q >= 2
    cut = [s for s in range(1, q)
           if maximum_count(stream, s, m) != maximum_count(stream, s, m, "no_cut")]
    return (cut[-1] if cut else q // 2), q + 3


@functools.lru_cache(maxsize=None)
def widening_record(oracle, r=10, seed=59):
    """One 12,308-base record, 12,288 windows (three full chunk tiles), all single-copy but r
    21-mers of the body (hash ranks 50 + 1000 j) that the tail repeats: r qualifiers at m = 2,
    12,288 - r distinct hashes."""
    k = 21
    rng = np.random.default_rng(seed)
    B = _rand(rng, 12308 - k * r)
    kmer = _single_copy_kmers(oracle, [B], k)
    D = sorted(kmer)
    picks = [D[50 + 1000 * j] for j in range(r)]
    rec = B + b"".join(kmer[h] for h in _clean_chain(B, [None] * r, picks, kmer, k, rng))
    stream = window_hashes(oracle, [rec], k)
    assert len(rec) == 12308 and len(stream) == 3 * TILE
    assert qualifiers(stream, 2) == picks and not qualifiers(stream, 3)
    return rec, stream


def widening_widths(s, m, windows, group_round):
    """The widths fpm_sketch_reads_run takes, restated: 8 s, then x 4 per round, each capped at
    one more than the windows of the largest group still open; s itself at m = 1.  windows: per
    group; group_round: the round that completes each group."""
    def cap(rnd):
        return min(max(w for w, r in zip(windows, group_round) if r >= rnd) + 1, 0x7fffffff)
    wide = s if m == 1 else min(8 * s, cap(1))
    out = [wide]
    for rnd in range(2, max(group_round) + 1):
        wide = min(wide * 4, cap(rnd))
        out.append(wide)
    return out


def group_is_sampled(ntile, width, every_min=16, chunk=TILE):
    """choose_samples' rule (csrc/sketch_plan.cpp) for a group of `ntile` tiles sketched at
    `width`: every E-th tile is sampled, E = tiles x 4,096 / 8 width within [16, 64], when the
    group has 2 E tiles and the sample 4 width windows."""
    every = min(64, max(every_min, ntile * chunk // (8 * width)))
    return ntile >= 2 * every and (ntile // every) * chunk >= 4 * width


SAMPLED_LONG = 270_000


@functools.lru_cache(maxsize=None)
def sampled_round2(oracle, seed=61):
    """Group 0: a 300-base record twice (280 hashes, each seen twice).  Group 1: one random
    record of SAMPLED_LONG bases (66 chunk tiles), second copies of D[25 i], i = 0..120 (D its
    hashes in order) as 21-base records in that order, and last a third copy of D[2475], the
    100th qualifier: the maximum at s = 100, m = 2, counted 2 of 3.
    -> recs, groups, streams (per group)"""
    k = 21
    rng = np.random.default_rng(seed)
    y = _rand(rng, 300)
    L = _rand(rng, SAMPLED_LONG)
    kmer = _single_copy_kmers(oracle, [L], k)
    D = sorted(kmer)
    long_recs = [L] + [kmer[D[25 * i]] for i in range(121)] + [kmer[D[2475]]]
    streams = [window_hashes(oracle, [y, y], k), window_hashes(oracle, long_recs, k)]
    assert len(qualifiers(streams[0], 2)) == 280
    assert qualifiers(streams[1], 2) == [D[25 * i] for i in range(121)]
    h, c, T, occ = closed_form(streams[1], 100, 2, detail=True)
    assert int(h[-1]) == D[2475] and int(c[-1]) == 2 and len(occ) == 3 and occ[1] == T < occ[2]
    recs = [y, y] + long_recs
    return SimpleNamespace(recs=recs, groups=[0, 0] + [1] * len(long_recs), streams=streams)
