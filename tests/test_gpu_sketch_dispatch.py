"""GPU parity of sketch at its dispatch edges: the tile classes at exact fill and one window
over, every 16-byte start / end residue of a tile, an invalid byte at the word edges of the
validity image, packed tiles closing at exactly 2,048 starts, the merge plans' odd carries and
kernels, the selection cap, the survivors-only kernel at every size of survivor set, and
canonical k-mers over alphabets beyond ACGT.

Every sketch is compared with oracle.sketch_batch, bit-exact on hashes and multiplicities
(reads mode: with tests/reads_model.py).  The tests that stand on a route assert it through
SketchJob.plan() (fpm_sketch_job_plan) and the run's hooks, so a moved threshold fails here
instead of moving the coverage.  The inputs come from plain builder functions; the unmarked
tests at the end check the builders' own promises on the CPU (a restatement of the planner's
tile cut, sample rule and merge rounds, csrc/sketch_plan.cpp, which tests/test_sketchplan_host.py
compares with the planner itself; the oracle's hashes), without a device.
"""
import functools
import itertools
import math

import numpy as np
import pytest

import reads_model

gpu = pytest.mark.gpu

CAPS = (256, 512, 1024, 2048, 4096, 8192)      # k-mer starts per tile class (kTileCap)
PACK, CHUNK = 2048, 4096                        # kPackKmers, kChunkKmers
SMALL_CAP = 2048                                # kMergeSmallCap
SEL_CAP = 15360                                 # kGroupSelectCap
THR_KEYS, SURV, SURV_SHARED = 1024, 2, 512      # kThrTileKeys = 256 * kSurv + kSurvShared
INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the host's staging rules, restated (csrc/sketch_plan.cpp: plan_sketch) --------------------

def tile_class(starts):
    return next(c for c, cap in enumerate(CAPS) if starts <= cap)


def packed_offsets(lens, k, device=False):
    """Each record's offset in the packed buffer (a 0x00 after every record).  The host path
    drops records shorter than k (None); the device path keeps what the parser emitted."""
    at, off = 0, []
    for L in lens:
        if not device and L < k:
            off.append(None)
            continue
        off.append(at)
        at += L + 1
    return off


def plan_tiles(lens, groups, k, device=False):
    """The tiles [group, byte_off, n_bytes] of records given in group order: a record of more
    than PACK starts is cut into CHUNK-start chunks, shorter ones share a tile of their group
    while the starts from the tile's first byte through the record fit PACK."""
    assert list(groups) == sorted(groups)
    tiles, cur, cur_g = [], None, None
    for L, g, o in zip(lens, groups, packed_offsets(lens, k, device)):
        if g != cur_g:
            if cur:
                tiles.append(cur)
            cur, cur_g = None, g
        if L < k:
            continue
        nk = L - k + 1
        if nk > PACK:
            if cur:
                tiles.append(cur)
            cur = None
            for c0 in range(0, nk, CHUNK):
                tiles.append([g, o + c0, min(CHUNK, nk - c0) + k - 1])
        elif cur and o > cur[1] + cur[2] and o + L - cur[1] - k + 1 <= PACK:
            cur[2] = o + L - cur[1]
        else:
            if cur:
                tiles.append(cur)
            cur = [g, o, L]
    if cur:
        tiles.append(cur)
    return tiles


def class_counts(tiles, k):
    n = [0] * len(CAPS)
    for _g, _o, nb in tiles:
        n[tile_class(nb - k + 1)] += 1
    return n


def sample_rule(ntile, s):
    """(sampled, every): a group's sample takes every `every`-th tile when it has at least two
    of them and they hold >= 4 s windows"""
    every = min(64, max(16, ntile * CHUNK // (8 * s)))
    return ntile >= 2 * every and (ntile // every) * CHUNK >= 4 * s, every


def tight_kt(ntile, every, s):
    f = ((ntile + every - 1) // every) / ntile
    return int(min(s, math.ceil(f * s + 8.0 * math.sqrt(f * s) + 32.0))), f


def survivors_rule(ntile, s):
    """thr4 for one sampled group of ntile class-4 tiles"""
    sampled, every = sample_rule(ntile, s)
    if not sampled:
        return False
    if s + s // 8 + 64 <= SEL_CAP:                  # selections -> tight bounds
        kt, f = tight_kt(ntile, every, s)
        est = int(2.0 * kt / f / ntile) + 64
    else:
        est = 2 * every * s // ntile + 64
    return est <= THR_KEYS // 2


def merge_rounds(est_of_group, s):
    """plan_rounds over each group's estimated list lengths: per round, whether it goes to
    merge_small_kernel (its longest input list is estimated <= SMALL_CAP)"""
    lists = [list(e) for e in est_of_group]
    small = []
    while True:
        any_, rmax = False, 0
        for g, L in enumerate(lists):
            if len(L) < 2:
                continue
            any_ = True
            nxt = []
            for i in range(0, len(L) - 1, 2):
                rmax = max(rmax, L[i], L[i + 1])
                nxt.append(min(s, L[i] + L[i + 1]))
            if len(L) % 2:
                nxt.append(L[-1])
            lists[g] = [] if len(nxt) == 1 else nxt
        if not any_:
            return small
        small.append(rmax <= SMALL_CAP)


# ---- inputs ------------------------------------------------------------------------------------

def rand_acgt(rng, n, p_lower=0.0):
    s = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)].copy()
    if p_lower:
        s[rng.random(n) < p_lower] += 32
    return s.tobytes()


def use64_of(k, n_alpha=4):
    return float(n_alpha) ** k > 2.0 ** 32


def window_keys(oracle, seq, k, seed=42):
    """The key of every window of an ACGT record, by position (INVALID where the window holds
    another byte): reads_model.window_hashes with the positions kept."""
    use64 = use64_of(k)
    seq = seq.upper()
    rev = seq.translate(reads_model._COMPL)[::-1]
    n = len(seq)
    bad = np.frombuffer(seq, np.uint8)
    bad = ~np.isin(bad, np.frombuffer(b"ACGT", np.uint8))
    nbad = np.concatenate([[0], np.cumsum(bad)])
    out = np.full(max(n - k + 1, 0), INVALID, np.uint64)
    for i in range(n - k + 1):
        if nbad[i + k] != nbad[i]:
            continue
        f, r = seq[i:i + k], rev[n - i - k:n - i]
        out[i] = oracle.get_hash(r if f > r else f, seed, use64)
    return out


# (a) one record per tile class at cap - 1, cap, cap + 1 starts
STRADDLE_K = (21, 22, 16, 17, 32, 1)
STRADDLE_STARTS = [cap + d for cap in CAPS[:5] for d in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def straddle_records(k):
    rng = np.random.default_rng(4100 + k)
    return [rand_acgt(rng, n + k - 1, p_lower=0.1) for n in STRADDLE_STARTS]


def straddle_classes(starts):
    """tiles per class of one record of up to 8,192 starts, stated directly (not through
    plan_tiles, which test_builder_straddle_windows compares it with)"""
    n = [0] * len(CAPS)
    if starts <= PACK:
        n[tile_class(starts)] = 1
    else:
        assert starts <= 2 * CHUNK
        n[4] = 1                                   # 2,049 .. 4,096 starts: one class-4 chunk
        if starts > CHUNK:
            n[tile_class(starts - CHUNK)] += 1     # 4,097: + a class-0 tile of one window
    return n


# (b) a probe record at every 16-byte residue of the packed buffer
def filler_for(at, k, residue):
    """length (64 .. 79) of a filler record at packed offset `at` after which the next record
    starts on `residue`"""
    return 64 + (residue - (at + 64 + 1)) % 16


def exact_fill_probe(k, cls):
    rng = np.random.default_rng(5200 + 10 * k + cls)
    return rand_acgt(rng, CAPS[cls] + k - 1)


def aligned_call(k, cls, a):
    """[filler of 64 + a bytes, the class's exact-fill probe]"""
    rng = np.random.default_rng(5300 + a)
    return [rand_acgt(rng, 64 + a), exact_fill_probe(k, cls)]


def residue_sweep_call(k, residue):
    """class-0 probes of every length k .. k + 40, each behind a filler that puts its first
    byte on `residue`: with the 16 residues, every (start, end) residue pair"""
    rng = np.random.default_rng(5400 + 100 * k + residue)
    recs, at = [], 0
    for L in range(k, k + 41):
        f = filler_for(at, k, residue)
        recs += [rand_acgt(rng, f), rand_acgt(rng, L)]
        at += f + 1 + L + 1
    return recs


def probe_residues(recs, k):
    """(start, end) residues of the odd (probe) records of a call"""
    off = packed_offsets([len(r) for r in recs], k)
    return [(off[i] % 16, (off[i] + len(recs[i])) % 16) for i in range(1, len(recs), 2)]


# (c) one or two N in an exact-fill record
def invalid_byte_records(k, cls):
    """-> (records, meta), -i mode: fillers (even records, 64 .. 79 bytes, so the start residue
    moves from probe to probe) and probes (odd records, meta[i] for records[2 i + 1]): the
    clean exact-fill record of the class; one N at each listed position (("one", p)); two N at
    distance k + 1 and k (("pair", q, d)).  The positions that depend on the probe's start
    residue a0 (a0 + p on a 32- / 64-bit word edge of the validity image) are taken for the
    probe's own a0."""
    P = CAPS[cls]
    E, L = P // 256, P + k - 1
    base = exact_fill_probe(k, cls)
    rng = np.random.default_rng(5500 + cls)
    recs, meta = [], []

    def add(make):
        at = sum(len(r) + 1 for r in recs)
        f = 64 + 5 * len(meta) % 16
        r = bytearray(base)
        tag = make(r, (at + f + 1) % 16)
        if tag is not None:
            recs.extend([rand_acgt(rng, f), bytes(r)])
            meta.append(tag)

    def one(pos):
        def make(r, a0):
            p = pos(a0)
            if not 0 <= p < L:
                return None
            r[p] = ord("N")
            return ("one", p)
        return make

    def pair(q, d):
        def make(r, a0):
            r[q] = r[q + d] = ord("N")
            return ("pair", q, d)
        return make

    add(lambda r, a0: ("clean",))
    for p in sorted({0, k - 1, k, L - k, L - 1, 1, E - 1, E, E + 1, 2 * E - 1, 2 * E, 2 * E + 1,
                     31, 32, 63, 64}):
        add(one(lambda a0, p=p: p))
    for t in (31, 32, 63, 64):                      # the bit index a0 + p itself on the edge
        add(one(lambda a0, t=t: t - a0))
    for w in (32, 64):                              # and the last such edges of the image
        for d in (-1, 0):
            add(one(lambda a0, w=w, d=d: (a0 + L - 1) // w * w + d - a0))
    for q in (0, E - 1, 37, L - 2 * k - 3):
        for d in (k + 1, k):
            if 0 <= q and q + d < L:
                add(pair(q, d))
    return recs, meta


# (i) reads mode: a record twice in one group, a chunked spacer between the copies so that
# each copy keeps a tile of its own, the second on the first's residue
def doubled(rec, k, rng):
    S = PACK + 1 + k - 1
    S += -(len(rec) + S + 2) % 16
    return [rec, rand_acgt(rng, S), rec]


# (d) packed tiles closing at exactly 2,048 starts
def packed_group(k, target, device, tail):
    """Records of length k and k + 1, records shorter than k between them, whose span from the
    first kept byte through the last record is exactly `target` starts; then `tail` more
    records of length k."""
    shorts = [0, 1, k - 1]
    # bytes the short records take between kept ones (device path only)
    extra = sum(x + 1 for x in shorts) if device else 0
    want = target + k - 1 + 1 - extra               # = a (k + 1) + b (k + 2)
    b = next(b for b in range(k + 1) if (want - b * (k + 2)) % (k + 1) == 0 and
             want - b * (k + 2) >= 2 * (k + 1))
    a = (want - b * (k + 2)) // (k + 1)
    lens = [k] * (a - 1) + [k + 1] * b + [k]
    for i, x in enumerate(shorts):                  # never first or last of the span
        lens.insert(1 + 7 * (i + 1), x)
    return lens + [k] * tail


def packed_input(k, device):
    """Five groups: a tile of exactly 2,048 starts and nothing more; the same followed by one
    record (a second tile); a span of exactly 2,049 (the last record opens a second tile); a
    full tile again, and right behind it the last group's two records (which must not join)."""
    rng = np.random.default_rng(6100 + k)
    glens = [packed_group(k, PACK, device, 0), packed_group(k, PACK, device, 1),
             packed_group(k, PACK + 1, device, 0), packed_group(k, PACK, device, 0), [k, k + 1]]
    lens = [x for g in glens for x in g]
    groups = [g for g, gl in enumerate(glens) for _ in gl]
    return [rand_acgt(rng, L) for L in lens], groups, len(glens)


PACKED_TILES = [(0, [0, 0, 0, 1, 0, 0]), (1, [1, 0, 0, 1, 0, 0]), (2, [1, 0, 0, 1, 0, 0]),
                (3, [0, 0, 0, 1, 0, 0]), (4, [1, 0, 0, 0, 0, 0])]


def fasta_of(recs):
    return b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs))


# (e) groups of 2, 3, 4, 5 and 9 one-record tiles
MERGE_SIZES = (2, 3, 4, 5, 9)
MERGE_KINDS = ("identical", "disjoint", "empty", "low")


def merge_input(k, starts, sizes=MERGE_SIZES):
    """For each size and kind a group of `size` records of `starts` starts (one tile each):
    the same record repeated; different random records; random ones and one of N only (an
    empty list); records of a repeated 60-byte unit (a union far below s)."""
    rng = np.random.default_rng(6200 + starts)
    L = starts + k - 1
    recs, groups = [], []
    for g, (n, kind) in enumerate(itertools.product(sizes, MERGE_KINDS)):
        if kind == "identical":
            rs = [rand_acgt(rng, L)] * n
        elif kind == "low":
            rs = [(rand_acgt(rng, 60) * (L // 60 + 1))[:L] for _ in range(n)]
        else:
            rs = [rand_acgt(rng, L) for _ in range(n)]
            if kind == "empty":
                rs[n // 2] = b"N" * L
        recs += rs
        groups += [g] * n
    return recs, groups, len(sizes) * len(MERGE_KINDS)


def merge_expect(starts, s, sizes=MERGE_SIZES):
    est = [[min(s, starts)] * n for n in sizes for _ in MERGE_KINDS]
    return merge_rounds(est, s)


# (f) the least long group that is sampled at s = 13,597 / 13,598
SEL_TILES = 224


@functools.lru_cache(maxsize=None)
def selection_record():
    return rand_acgt(np.random.default_rng(6300), SEL_TILES * CHUNK + 20)


# (g) a group of 4,096-start chunks for the survivors-only kernel.  A group is sampled from 2 x
# every tiles on, every = its windows / 8 s (16 .. 64): 32 chunks at s = 1,000 (every 16th tile:
# tiles 0 and 16, ~80 survivors per random tile), 64 chunks at s = 1,000 (every 32nd, a lower
# bound: ~55 per tile, one wave's worth)
THR_N, THR_SPILL, THR_OVER = 3, 7, (5, 9)       # the tiles made special (never sampled)
SURVIVOR_CASES = [(21, 1000, 32), (12, 1000, 32), (21, 1000, 64)]


def thread_survivors(keys, bound):
    """per tile (row) and thread (column): windows with key <= bound among the thread's 16"""
    low = (keys != INVALID) & (keys <= np.uint64(bound))
    return low.reshape(-1, 256, CHUNK // 256).sum(axis=2)


def tile_shapes(keys, bound):
    """per tile: (survivors, keys sent to the shared area, overflows)"""
    per = thread_survivors(keys, bound)
    total = per.sum(axis=1)
    spill = np.maximum(per - SURV, 0).sum(axis=1)
    return total, spill, spill > SURV_SHARED


@functools.lru_cache(maxsize=None)
def survivors_group(k, s, ntile):
    """-> (record, bound, keys): a record of ntile x 4,096 starts, random but for one chunk of
    N, one with runs of a short repeat that start on a thread's first window, two filled with a
    short repeat; the repeats' units are those with windows whose key lies below the group's
    bound (the kt-th smallest key of the sample).  The first seed that yields the shapes the
    case needs is taken (deterministic)."""
    from oracle import oracle as O
    O.lib()
    sampled, every = sample_rule(ntile, s)
    assert sampled and ntile == 2 * every and survivors_rule(ntile, s)
    assert not sample_rule(ntile - 1, s)[0]         # the least group this s samples that way
    kt, _f = tight_kt(ntile, every, s)
    for seed in range(200):
        rng = np.random.default_rng(6400 + 1000 * k + 10 * ntile + seed)
        rec = bytearray(rand_acgt(rng, ntile * CHUNK + k - 1))
        sample = np.concatenate([window_keys(O, bytes(rec[t * CHUNK:(t + 1) * CHUNK + k - 1]), k)
                                 for t in (0, every)])
        distinct = np.unique(sample)
        # the a-priori sample bound leaves the sample its s smallest
        frac = (1.25 * s + 16.0 * math.sqrt(s)) / len(sample)
        rng_max = 2.0 ** 64 if use64_of(k) else 2.0 ** 32
        assert frac < 0.5 and int((distinct < frac * rng_max).sum()) >= s
        bound = int(distinct[kt - 1])
        # units of period <= 6: the share of their windows below the bound
        dense, sparse = [], []
        for u in range(1, 7):
            for unit in itertools.product(b"ACGT", repeat=u):
                unit = bytes(unit)
                w = window_keys(O, (unit * (k // u + 3))[:k + u - 1], k)
                share = float((w <= np.uint64(bound)).mean())
                if share > 0.3:
                    dense.append(unit)
                elif share > 0 and u == 5:
                    sparse.append(unit)
        if not sparse or not dense:
            continue

        def fill(at, n, unit):
            rec[at:at + n] = (unit * (n // len(unit) + 1))[:n]

        fill(THR_N * CHUNK, CHUNK + k - 1, b"N")
        for j, t in enumerate((10, 100, 200)):        # thread t's 16 windows: one unit
            fill(THR_SPILL * CHUNK + 16 * t, 16 + k - 1, sparse[j % len(sparse)])
        for j, t in enumerate(THR_OVER):
            fill(t * CHUNK, CHUNK + k - 1, dense[j % len(dense)])
        keys = window_keys(O, bytes(rec), k)
        total, spill, over = tile_shapes(keys, bound)
        if not (over[list(THR_OVER)].all() and over.sum() == len(THR_OVER)):
            continue
        if not (0 < spill[THR_SPILL] <= SURV_SHARED):
            continue
        keys.setflags(write=False)
        return bytes(rec), bound, keys
    raise AssertionError("no seed gives the survivor shapes")




# (h) canonical k-mers over alphabets beyond ACGT
ALPHABET_CASES = [("ACGTN", 9), ("ACGTN", 21), ("ACGTRYKMSWBDHVN", 7)]


def alphabet_records(alphabet, k, lens, seed):
    rng = np.random.default_rng(seed)
    pool = np.frombuffer(alphabet.encode(), np.uint8)
    out = []
    for L in lens:
        s = pool[rng.integers(0, len(pool), size=L)].copy()
        m = rng.random(L) < 0.004
        s[m] = np.frombuffer(b"XZ-*", np.uint8)[rng.integers(0, 4, size=int(m.sum()))]
        s[rng.random(L) < 0.1] |= 0x20             # lower case ('-', '*' stay outside)
        out.append(s.tobytes())
    return out


# ---- running and comparing ---------------------------------------------------------------------

def assert_same(got, exp, what):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e), f"{what} {i}: {len(g)} vs {len(e)} entries"
        assert np.array_equal(g, e), f"{what} {i} differs"


def run_parity(ctx, oracle, kw, seqs, groups=None, n_groups=None, what=""):
    """The job's sketches and multiplicities against the oracle's -> (plan, hooks after the
    run)."""
    import fpmash
    P, O = fpmash.make_params(**kw), oracle.params(**kw)
    assert P.use64 == O.use64
    job = ctx.sketch_job(P, seqs, groups, n_groups)
    try:
        plan = job.plan()
        job.run()
        rows, cnt = job.fetch()
        mult = job.mult()
        hooks = {"redo": job.redo_tiles(), "short": job.short_groups()}
    finally:
        job.free()
    exp, exp_m = oracle.sketch_batch(O, seqs, groups=groups, n_groups=n_groups, counts=True)
    assert_same([rows[i, :cnt[i]] for i in range(len(cnt))], exp, what + " sketch")
    assert_same([mult[i, :cnt[i]] for i in range(len(cnt))], exp_m, what + " multiplicities")
    return plan, hooks


def staged_plan(ctx, kw, seqs, groups=None, n_groups=None):
    import fpmash
    job = ctx.sketch_job(fpmash.make_params(**kw), seqs, groups, n_groups)
    try:
        return job.plan()
    finally:
        job.free()


@functools.lru_cache(maxsize=None)
def reads_expect(k, s, recs):
    """the heap of tests/reads_model.py over one group's records at min_copies = 2 (computed
    once per group of records, shared, never modified)"""
    from oracle import oracle as O
    res = reads_model.model_sketch(reads_model.window_hashes(O, list(recs), k), s, 2)
    for a in res:
        a.setflags(write=False)
    return res


def run_reads(ctx, oracle, k, s, recs, groups, n_groups, what=""):
    """ctx.sketch_reads at min_copies = 2 against the heap of tests/reads_model.py"""
    import fpmash
    r = ctx.sketch_reads(fpmash.make_params(k=k, s=s), recs, groups, n_groups, min_copies=2)
    for g in range(n_groups):
        eh, ec = reads_expect(k, s, tuple(x for x, gg in zip(recs, groups) if gg == g))
        assert np.array_equal(r["hashes"][g], eh), f"{what} group {g}: hashes differ"
        assert np.array_equal(r["counts"][g], ec), f"{what} group {g}: counts differ"
    return r


# ---- (a) class straddles -----------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("k", STRADDLE_K)
def test_class_straddle_routes(ctx, k):
    """each record alone: the class its tile(s) take"""
    for starts, rec in zip(STRADDLE_STARTS, straddle_records(k)):
        plan = staged_plan(ctx, dict(k=k, s=1000), [rec])
        assert plan["tiles"] == straddle_classes(starts), (starts, plan["tiles"])
        assert plan["tiles"][5] == 0
        assert plan["n_slots"] == 0 and plan["rounds"] == (1 if starts > CHUNK else 0)
        assert not plan["thr4"]


@gpu
@pytest.mark.parametrize("s", [1, 256, 1000, 5000])
@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", STRADDLE_K)
def test_class_straddle_parity(ctx, oracle, k, canon, s):
    recs = straddle_records(k)
    plan, _ = run_parity(ctx, oracle, dict(k=k, s=s, noncanonical=not canon), recs,
                         what=f"k={k}")
    exp = np.sum([straddle_classes(n) for n in STRADDLE_STARTS], axis=0)
    assert plan["tiles"] == list(exp) and plan["tiles"][5] == 0


# ---- (b) alignment -----------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", [21, 22])
def test_alignment_exact_fill(ctx, oracle, k, canon):
    for cls in range(5):
        for a in range(16):
            plan, _ = run_parity(ctx, oracle, dict(k=k, s=1000, noncanonical=not canon),
                                 aligned_call(k, cls, a), what=f"class {cls} filler 64+{a}")
            exp = [0] * 6
            exp[0] += 1
            exp[cls] += 1
            assert plan["tiles"] == exp


@gpu
@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("k", [21, 22])
def test_alignment_residue_pairs(ctx, oracle, k, canon):
    for residue in range(16):
        recs = residue_sweep_call(k, residue)
        plan, _ = run_parity(ctx, oracle, dict(k=k, s=1000, noncanonical=not canon), recs,
                             what=f"start residue {residue}")
        assert plan["tiles"] == [len(recs), 0, 0, 0, 0, 0]


# ---- (c) invalid bytes -------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("cls", [2, 4])
@pytest.mark.parametrize("k", [21, 32, 1])
def test_invalid_bytes(ctx, oracle, k, cls, canon):
    recs, meta = invalid_byte_records(k, cls)
    plan, _ = run_parity(ctx, oracle, dict(k=k, s=1000, noncanonical=not canon), recs,
                         what=f"k={k} class {cls}")
    exp = [0] * 6
    exp[0] += len(meta)                             # the fillers
    exp[cls] += len(meta)
    assert plan["tiles"] == exp


# ---- (d) packed tiles --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("k", [21, 12])
def test_packed_tiles(ctx, oracle, k, path):
    import fpmash
    device = path == "device"
    recs, groups, ng = packed_input(k, device)
    kw = dict(k=k, s=1000)
    exp_tiles = list(np.sum([t for _g, t in PACKED_TILES], axis=0))
    if not device:
        plan, _ = run_parity(ctx, oracle, kw, recs, groups, ng, what="packed")
        assert plan["tiles"] == exp_tiles
        for g, t in PACKED_TILES:                   # and each group alone
            sub = [r for r, gg in zip(recs, groups) if gg == g]
            assert staged_plan(ctx, kw, sub, [0] * len(sub), 1)["tiles"] == t, g
        return
    P = fpmash.make_params(**kw)
    exp = oracle.sketch_batch(oracle.params(**kw), recs, groups=groups, n_groups=ng)
    handle, rec, _q = ctx.seq_parse([fasta_of(recs)])
    try:
        assert [int(x) for x in rec["seq_len"]] == [len(r) for r in recs]
        job = ctx.sketch_seq_job(P, handle, groups, ng)
        try:
            plan = job.plan()
            job.run()
            rows, cnt = job.fetch()
        finally:
            job.free()
    finally:
        ctx.seq_free(handle)
    assert_same([rows[i, :cnt[i]] for i in range(ng)], exp, "device path sketch")
    assert plan["tiles"] == exp_tiles


# ---- (e) merge shapes --------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("starts,s,rounds,small", [(1100, 2048, 4, 4), (1100, 2049, 4, 1),
                                                   (2100, 2048, 4, 4), (2100, 2049, 4, 0)])
def test_merge_rounds_small_cap(ctx, oracle, starts, s, rounds, small):
    """2, 3, 4, 5 and 9 lists per group: 1, 2, 2, 3 and 4 rounds with the odd list carried; a
    round goes to merge_small_kernel while its input lists are estimated <= 2,048 long (tiles
    of 1,100 starts: the first round only at s = 2,049)"""
    import fpmash
    recs, groups, ng = merge_input(21, starts)
    ctx.merge_small_spills()                        # reset
    plan, _ = run_parity(ctx, oracle, dict(k=21, s=s), recs, groups, ng, what="merge")
    assert (plan["rounds"], plan["rounds_small"]) == (rounds, small)
    assert plan["merge_kernel"] == fpmash.MK_LDS and plan["n_slots"] == 0
    assert plan["tiles"][tile_class(starts)] == len(recs)
    if s == SMALL_CAP:
        assert ctx.merge_small_spills() == 0        # no list can exceed s


@gpu
@pytest.mark.parametrize("s", [16384, 16385])
def test_merge_kernel_lds_cap(ctx, oracle, s):
    """two 4,096-start tiles per group (est 4,096 > 2,048: no small round): lists staged in LDS
    up to s = 16,384, searched in global memory beyond"""
    import fpmash
    recs, groups, ng = merge_input(21, CHUNK, sizes=(2,))
    plan, _ = run_parity(ctx, oracle, dict(k=21, s=s), recs, groups, ng, what="merge")
    assert (plan["rounds"], plan["rounds_small"]) == (1, 0)
    assert plan["merge_kernel"] == (fpmash.MK_LDS if s <= 16384 else fpmash.MK_GLOBAL)
    assert plan["tiles"] == [0, 0, 0, 0, len(recs), 0]


# ---- (f) the selection cap ---------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("s", [13597, 13598])
def test_selection_cap(ctx, oracle, s):
    """224 chunks: the least group sampled at these s (14 sample tiles of 4,096 >= 4 s).  s +
    s / 8 + 64 <= 15,360 up to s = 13,597: selections, tight bounds and the survivors-only
    kernel; one more and the lists are merged pairwise under the safe bound."""
    plan, hooks = run_parity(ctx, oracle, dict(k=21, s=s), [selection_record()], [0], 1,
                             what=f"s={s}")
    assert plan["tiles"] == [0, 0, 0, 0, SEL_TILES, 0]
    assert plan["sample_tiles"] == [0, 0, 0, 0, SEL_TILES // 16, 0] and plan["n_slots"] == 1
    if s <= 13597:
        assert plan["n_ssel"] > 0 and plan["n_sel"] > 0 and plan["tight"] == 1
        assert (plan["rounds"], plan["sample_rounds"]) == (0, 0)
        assert plan["thr4"] == 1 and hooks["short"] >= 0 and hooks["redo"] >= 0
    else:
        assert plan["n_ssel"] == 0 and plan["n_sel"] == 0 and plan["tight"] == 0
        assert (plan["rounds"], plan["sample_rounds"]) == (8, 4)     # 224 and 14 lists
        assert plan["thr4"] == 0 and hooks["short"] == -1 and hooks["redo"] == -1


# ---- (g) the survivors-only kernel at small shapes ---------------------------------------------

@gpu
@pytest.mark.parametrize("k,s,ntile", SURVIVOR_CASES)
def test_survivors_kernel_shapes(ctx, oracle, k, s, ntile):
    """One group of 32 / 64 chunks, the least the survivors-only kernel takes at this s: tiles
    without a valid window, with <= 64 survivors (one wave: most of the 64-chunk group's),
    with more (most of the 32-chunk group's), with threads holding more than two (the shared
    area) and two whose shared area overflows (the redo list): exactly those are redone."""
    rec, bound, keys = survivors_group(k, s, ntile)
    total, spill, over = tile_shapes(keys, bound)
    assert total[THR_N] == 0 and 0 < spill[THR_SPILL] <= SURV_SHARED
    few, many = (total > 0) & (total <= 64), (total > 64) & ~over
    assert many.sum() >= 16 if ntile == 32 else few.sum() >= 16
    assert [int(t) for t in np.flatnonzero(over)] == sorted(THR_OVER)
    plan, hooks = run_parity(ctx, oracle, dict(k=k, s=s), [rec], [0], 1, what=f"k={k} s={s}")
    assert plan["tiles"] == [0, 0, 0, 0, ntile, 0] and plan["thr4"] == 1
    assert plan["sample_tiles"] == [0, 0, 0, 0, 2, 0] and plan["tight"] == 1
    assert plan["n_slots"] == 1 and plan["n_sel"] > 0
    assert hooks["short"] == 0                      # the bound of the model is the run's
    assert hooks["redo"] == len(THR_OVER)


# ---- (h) canonical k-mers over other alphabets -------------------------------------------------

@gpu
@pytest.mark.parametrize("alphabet,k", ALPHABET_CASES)
def test_canonical_other_alphabets(ctx, oracle, alphabet, k):
    kw = dict(k=k, s=500, alphabet=alphabet)
    lens = [k - 1, k, k + 1, 255 + k, 256 + k, 300, 1000, 2100, 4096 + k, 9000]
    recs = alphabet_records(alphabet, k, lens, 6500 + k)
    plan, _ = run_parity(ctx, oracle, kw, recs, what="-i")
    assert plan["tiles"][4] >= 3 and plan["tiles"][0] >= 3
    grp = alphabet_records(alphabet, k, [700, 5, 9000, 1500, 30000], 6600 + k)
    plan, _ = run_parity(ctx, oracle, kw, grp, [0] * len(grp), 1, what="group")
    assert sum(plan["tiles"]) >= 10 and plan["rounds"] >= 4


# ---- (i) reads mode on the same edges ----------------------------------------------------------

@gpu
def test_reads_class_straddles(ctx, oracle):
    k, s = 21, 1000
    rng = np.random.default_rng(6700)
    recs, groups = [], []
    for g, rec in enumerate(straddle_records(k)):
        recs += doubled(rec, k, rng)
        groups += [g] * 3
    run_reads(ctx, oracle, k, s, recs, groups, len(STRADDLE_STARTS), what="straddle")


@gpu
@pytest.mark.parametrize("cls", range(5))
def test_reads_alignment(ctx, oracle, cls):
    k, s = 21, 1000
    for a in range(16):
        rng = np.random.default_rng(6800 + cls)     # the same spacer: one expected sketch
        filler, probe = aligned_call(k, cls, a)
        run_reads(ctx, oracle, k, s, [filler] + doubled(probe, k, rng), [0, 1, 1, 1], 2,
                  what=f"class {cls} filler 64+{a}")


@gpu
@pytest.mark.parametrize("cls", [2, 4])
def test_reads_invalid_bytes(ctx, oracle, cls):
    k, s = 21, 1000
    rng = np.random.default_rng(6900 + cls)
    recs, groups = [], []
    for g, rec in enumerate(invalid_byte_records(k, cls)[0][1::2]):    # the probes
        recs += doubled(rec, k, rng)
        groups += [g] * 3
    run_reads(ctx, oracle, k, s, recs, groups, groups[-1] + 1, what=f"class {cls}")


# ---- the builders' promises, on the CPU --------------------------------------------------------

@pytest.mark.parametrize("k", STRADDLE_K)
def test_builder_straddle_windows(oracle, k):
    """each record has the starts it is named for (every window valid: the oracle's
    multiplicities sum to them) and the staging model routes it as the issue states"""
    recs = straddle_records(k)
    O = oracle.params(k=k, s=10000, noncanonical=True)
    _h, mult = oracle.sketch_batch(O, recs, counts=True)
    for starts, rec, m in zip(STRADDLE_STARTS, recs, mult):
        assert len(rec) == starts + k - 1
        assert int(m.sum()) == starts
        assert int((window_keys(oracle, rec, k) != INVALID).sum()) == starts
        assert class_counts(plan_tiles([len(rec)], [0], k), k) == straddle_classes(starts)
    assert straddle_classes(256) == [1, 0, 0, 0, 0, 0] == straddle_classes(255)
    assert straddle_classes(257) == [0, 1, 0, 0, 0, 0]
    assert straddle_classes(2049) == [0, 0, 0, 0, 1, 0] == straddle_classes(4096)
    assert straddle_classes(4097) == [1, 0, 0, 0, 1, 0]


def test_builder_class5_unreachable():
    """no record length gives a tile of more than 4,096 starts: packed tiles stop at 2,048,
    chunks at 4,096"""
    for k in (1, 21, 32):
        for starts in list(range(1, 64)) + [2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192,
                                            8193, 12289, 100000]:
            n = class_counts(plan_tiles([starts + k - 1], [0], k), k)
            assert n[5] == 0 and sum(n) == (1 if starts <= PACK else -(-starts // CHUNK))
        lens = [k] * 5000 + [k + 1] * 3000
        assert class_counts(plan_tiles(lens, [0] * len(lens), k), k)[4:] == [0, 0]


@pytest.mark.parametrize("k", [21, 22])
def test_builder_alignment_residues(k):
    for cls in range(5):
        seen = {probe_residues(aligned_call(k, cls, a), k)[0][0] for a in range(16)}
        assert seen == set(range(16))
        assert len(exact_fill_probe(k, cls)) - k + 1 == CAPS[cls]
    pairs = set()
    for residue in range(16):
        recs = residue_sweep_call(k, residue)
        pr = probe_residues(recs, k)
        assert all(a == residue for a, _e in pr)
        assert sorted(len(r) for r in recs[1::2]) == list(range(k, k + 41))
        assert all(64 <= len(r) < 80 for r in recs[0::2])
        pairs |= set(pr)
    assert len(pairs) == 256


@pytest.mark.parametrize("cls", [2, 4])
@pytest.mark.parametrize("k", [21, 32, 1])
def test_builder_invalid_bytes(oracle, k, cls):
    recs, meta = invalid_byte_records(k, cls)
    P, L = CAPS[cls], CAPS[cls] + k - 1
    E = P // 256
    off = packed_offsets([len(r) for r in recs], k)
    assert len(recs) == 2 * len(meta) and all(64 <= len(r) < 80 for r in recs[0::2])
    assert len({o % 16 for o in off[1::2]}) == 16   # every start residue among the probes
    ones, bits = set(), set()
    for rec, m, o in zip(recs[1::2], meta, off[1::2]):
        assert len(rec) == L
        valid = window_keys(oracle, rec, k) != INVALID
        if m[0] == "clean":
            assert valid.all()
        elif m[0] == "one":
            p = m[1]
            assert rec.count(b"N") == 1 and rec[p:p + 1] == b"N"
            assert int((~valid).sum()) == min(p, L - k) - max(p - k + 1, 0) + 1
            ones.add(p)
            bits.add(o % 16 + p)
        else:
            _, q, d = m
            assert rec.count(b"N") == 2 and rec[q:q + 1] == rec[q + d:q + d + 1] == b"N"
            between = valid[q + 1:q + d]            # windows starting between the two
            assert int(between.sum()) == d - k and d - k in (0, 1)
            assert not valid[max(q - k + 1, 0):q + 1].any()
    assert {0, k - 1, k, L - k, L - 1, E - 1, E, E + 1, 2 * E - 1, 2 * E + 1} <= ones | {2 * E}
    end = 15 + L                                    # the image's last bit at a0 = 15
    assert {31, 32, 63, 64} <= bits and any(b % 64 == 0 and b > end - 96 for b in bits)
    assert any(b % 64 == 63 and b > end - 96 for b in bits)
    assert sum(m[0] == "pair" for m in meta) >= 6


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("k", [21, 12])
def test_builder_packed_tiles(k, device):
    recs, groups, ng = packed_input(k, device)
    lens = [len(r) for r in recs]
    assert any(L < k for L in lens) and {k, k + 1} <= set(lens)
    tiles = plan_tiles(lens, groups, k, device)
    for g, exp in PACKED_TILES:
        mine = [t for t in tiles if t[0] == g]
        assert class_counts(mine, k) == exp
        if g < 4:
            assert mine[0][2] - k + 1 == (PACK if g != 2 else PACK + 1 - (k + 1))
    # the full tile of group 3 ends right before group 4's first record
    last3, first4 = [t for t in tiles if t[0] == 3][-1], [t for t in tiles if t[0] == 4][0]
    assert last3[1] + last3[2] + 1 == first4[1]


def test_builder_merge_rounds():
    assert merge_expect(1100, 2048) == [True] * 4
    assert merge_expect(1100, 2049) == [True, False, False, False]
    assert merge_expect(2100, 2048) == [True] * 4
    assert merge_expect(2100, 2049) == [False] * 4
    assert merge_expect(CHUNK, 16384, sizes=(2,)) == [False] == merge_expect(CHUNK, 16385, sizes=(2,))
    for n, r in zip(MERGE_SIZES, (1, 2, 2, 3, 4)):
        assert len(merge_rounds([[100] * n], 1000)) == r
    recs, groups, ng = merge_input(21, 1100)
    tiles = plan_tiles([len(r) for r in recs], groups, 21)
    assert len(tiles) == len(recs) and ng == 20     # a tile per record
    assert sorted(groups.count(g) for g in range(ng)) == sorted(MERGE_SIZES * 4)


def test_builder_selection_group():
    for s in (13597, 13598):
        assert sample_rule(SEL_TILES, s) == (True, 16)
        assert not sample_rule(SEL_TILES - 1, s)[0]
    assert 13597 + 13597 // 8 + 64 <= SEL_CAP < 13598 + 13598 // 8 + 64
    assert survivors_rule(SEL_TILES, 13597) and not survivors_rule(SEL_TILES, 13598)
    rec = selection_record()
    assert class_counts(plan_tiles([len(rec)], [0], 21), 21) == [0, 0, 0, 0, SEL_TILES, 0]


@pytest.mark.parametrize("k,s,ntile", SURVIVOR_CASES)
def test_builder_survivor_shapes(oracle, k, s, ntile):
    rec, bound, keys = survivors_group(k, s, ntile)
    assert class_counts(plan_tiles([len(rec)], [0], k), k) == [0, 0, 0, 0, ntile, 0]
    # the group's sketch under the bound: at least s distinct keys (the tight bound holds), and
    # the s smallest of the model's keys are the oracle's sketch
    valid = np.unique(keys[keys != INVALID])
    assert int((valid <= np.uint64(bound)).sum()) >= s
    exp = oracle.sketch_batch(oracle.params(k=k, s=s), [rec])[0]
    assert np.array_equal(valid[:s], exp)
    total, spill, over = tile_shapes(keys, bound)
    per = thread_survivors(keys, bound)
    assert total[THR_N] == 0
    assert per[THR_SPILL].max() > SURV and 0 < spill[THR_SPILL] <= SURV_SHARED and not over[THR_SPILL]
    assert [int(t) for t in np.flatnonzero(over)] == sorted(THR_OVER)
    few, many = (total > 0) & (total <= 64), (total > 64) & ~over
    assert many.sum() >= 16 if ntile == 32 else few.sum() >= 16
    assert THR_KEYS == 256 * SURV + SURV_SHARED
