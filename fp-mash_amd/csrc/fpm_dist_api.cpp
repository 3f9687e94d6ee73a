// fpm_dist_api.cpp — the dist part of the C ABI declared in include/fpmash.h: the grid compare
// (dense, or bucket index + probe + candidate kernel), its finalize, the resident reference
// sets and the host-memory wrappers, over the kernels in dist.hip and dist_index.hip.
#include "fpm_internal.hpp"

#include <cmath>
#include <cstdlib>
#include <functional>
#include <memory>

// One grid's outputs: the counts, and either the full per-cell distance / p-value / pass
// (fpm_dist_dev*) or the compact list of the cells with numer > 0 (fpm_dist_list_dev*).
struct DistOut {
    Counts cnt;
    CellOut cell;
    CellList list{};
};

// The outputs handed to compare_impl, so the sparse path can finalize in place: the probe (or
// the side fill) writes every cell's no-shared-hash values and a candidate kernel rewrites
// (or lists) the candidates, with no dense pass re-reading the grid.
struct DistFinal {
    DistParams par;
    DistOut prim;
    // the transposed grid too (fpm_refset_dist_mirror_dev*): filled beside the primary grid and
    // its candidate cells scattered by the candidate finalize; compare_impl sets *mirrored
    // when it wrote it (the sorted sparse path), else dist_dev_impl computes it by a second,
    // swapped call
    DistOut mir{};
    bool *mirrored = nullptr;
    // the grid's counts were prefilled (fpm_dist_list_prefill): no defaults of its own, the
    // short pairs corrected after ev_prefill, before the first cell write
    bool prefilled = false;
    bool compact() const { return prim.list.count != nullptr; }
    bool has_mirror() const { return mir.cnt.numer != nullptr; }
};

// bucket index geometry for E entries over n_ref rows: ~2.4 entries per bucket (2^nbits >=
// E/4, at most 2^24 buckets); entries are u32 (ref id in rbits, key fingerprint in the next
// >= 7 bits, the visited-prefix flag of the half probe's cut at sketch size `cut` on top).  4K level-2 counters (16 KiB of LDS) and a 16 MB directory at the bench's
// E = 1e7.  Same-box A/B: E/2 buckets cost 0.04 ms more in the bucket pass than the extra
// probe events saved; E/8 a wash.
// FPM_IDX_ONEPASS=0: always the exact two-pass index build (A/B)
static const bool g_idx_one_pass = [] {
    const char *v = getenv("FPM_IDX_ONEPASS");
    return !(v && v[0] == '0');
}();

static IdxGeom make_geom(uint32_t n_ref, uint64_t E, uint32_t cut)
{
    IdxGeom geom{};
    uint32_t rbits = 1, lg = 1;
    while (rbits < 32 && (1ULL << rbits) < n_ref) rbits++;
    while (lg < 40 && (1ULL << lg) < E) lg++;
    geom.l2 = lg > kIdxL1 + 2 ? std::min<uint32_t>(lg - 2 - kIdxL1, 14) : 1;
    geom.nbits = kIdxL1 + geom.l2;
    geom.rbits = rbits;
    geom.fbits = rbits < 31 ? 31 - rbits : 0;
    geom.cut = cut;
    // level-1 tiles (one 1024-thread workgroup per CU: their LDS staging holds 8 B per cell)
    // in whole rounds of 256: the cells per tile trimmed so that the last round is not a
    // fraction of the chip (C2's 1e7 cells: 752 tiles of 13,312 instead of 611 of 16,384)
    {
        const uint64_t rounds = std::max<uint64_t>(1, (E + 256ULL * kIdxTile - 1) / (256ULL * kIdxTile));
        uint64_t tile = (E + 256 * rounds - 1) / (256 * rounds);
        tile = std::min<uint64_t>(kIdxTile, std::max<uint64_t>(1024, (tile + 1023) / 1024 * 1024));
        geom.tile = (uint32_t)tile;
        geom.ntiles = (uint32_t)((E + tile - 1) / tile);
    }
    // one-pass level 1: each partition's slot holds 1.5 x the mean + 6 sigma + 64 entries.
    // Bottom-s sketch values are uniform below each row's own maximum, and the rows' maxima
    // differ, so the density over the indexed range [0, kmax] tapers towards kmax and the low
    // partitions run ~10 % above the mean (C2: a 6-sigma slot overflowed on every build);
    // skewed keys (repeated -fp values) overflow and take the exact build
    const double mean = (double)E / (double)(1u << kIdxL1);
    geom.cap = g_idx_one_pass
                   ? (uint32_t)(((uint64_t)(1.5 * mean + 6.0 * std::sqrt(mean)) + 64 + 63) & ~63ull)
                   : 0u;
    return geom;
}

// One index build (launch_idx_build) over the rows R and the read-back of its counters (events,
// sortedness, the one-pass overflow flag), after `then` (work queued behind the build, e.g.
// the query side's probe count).  The one-pass build first; if a level-1 partition overflowed
// its slot, the exact two-pass build (g.cap = 0) replaces it.
// raw_of_unsorted: the caller re-indexes unsorted rows over their records, so when the rows
// turn out unsorted an overflowed one-pass build is left as it is (its flags and counters
// are all the caller reads) instead of being rebuilt exactly.
template <typename Then>
static int build_index(fpm_ctx *ctx, const RowSet &R, uint32_t hash_bytes, IdxGeom &g,
                       uint32_t *dir, uint32_t *entries, unsigned long long *ctr,
                       bool self_events, hipStream_t st, Then then, bool raw_of_unsorted = false,
                       const std::function<int()> &before_read = nullptr,
                       unsigned long long *zero_x = nullptr)
{
    for (;;) {
        const uint64_t E = (uint64_t)R.n * R.stride;
        const uint64_t nh = (uint64_t)(1u << kIdxL1) * g.ntiles;
        void *tile_hist, *tile_off, *tent, *scan_s, *part_fill;
        HIP_TRY(scratch(ctx, kSlotTileHist, nh * 4, &tile_hist));
        HIP_TRY(scratch(ctx, kSlotTileOff, (nh + 1) * 4, &tile_off));
        HIP_TRY(scratch(ctx, kSlotTent, idx_tent_words(g, E) * 8, &tent));
        HIP_TRY(scratch(ctx, kSlotScan, scan_scratch_words(nh) * 4, &scan_s));
        HIP_TRY(scratch(ctx, kSlotPartFill, (size_t)(1u << kIdxL1) * 4, &part_fill));
        uint32_t *unsorted = (uint32_t *)(ctr + kCtrUnsorted);
        uint32_t *overflow = (uint32_t *)(ctr + kCtrOverflow);
        {
            TimedLaunch tl(ctx, FPM_K_INDEX, st);
            IdxBuild b;
            b.rows = R;
            b.hash_bytes = hash_bytes;
            b.g = g;
            b.tile_hist = (uint32_t *)tile_hist;
            b.tile_off = (uint32_t *)tile_off;
            b.scan_s = (uint32_t *)scan_s;
            b.tent = (uint64_t *)tent;
            b.dir = dir;
            b.entries = entries;
            b.unsorted = unsorted;
            b.self_events = self_events ? ctr : nullptr;
            b.zero = ctr;
            b.nzero = kCtrZeroWords;
            b.zero_x = zero_x;
            b.acc = ctr + kCtrKmaxAcc;
            b.part_fill = (uint32_t *)part_fill;
            b.overflow = overflow;
            b.n_entries = ctr + kCtrIndexed;
            static_assert(kCtrEntries == kCtrIndexed + 1, "IdxBuild::n_entries[0..1]");
            HIP_TRY(launch_idx_build(b, st));
            if (int rc = then()) return rc;
            tl.done();
        }
        // the counters' copy first, then the work enqueued behind it before the host waits for
        // them (the speculated probe: the GPU runs it while the host reads and enqueues the
        // rest; enqueued before the copy, it would hold the copy, and the host, until it ends)
        unsigned long long seq;
        if (int rc = publish_counters(ctx, ctr, kCtrBuildWords, st, &seq)) return rc;
        if (before_read)
            if (int rc = before_read()) return rc;
        if (int rc = wait_counters(ctx, seq, st)) return rc;
        if (g.cap && host_overflow(ctx)) {
            if (raw_of_unsorted && host_unsorted(ctx)) return FPM_OK;
            g.cap = 0;
            ctx->idx_rebuilds++;
            continue;
        }
        return FPM_OK;
    }
}

// A reference set resident on the device with its bucket index built once (fpm_refset_*):
// query blocks probe it without re-uploading the references or rebuilding the index.
struct fpm_refset {
    fpm_ctx *ctx = nullptr;
    RowSet ref{};                 // the reference rows (in `mem` when uploaded from host buffers)
    uint32_t hash_bytes = 0, sketch_size = 0;
    DevBufs mem;                  // owns those rows and kmax
    // the index: directory, entries, and the record rows / lengths / positions it is built
    // over when the rows are unsorted; the largest indexed key; host state
    enum { kDir, kEntries, kRecRows, kRecLen, kRecPos, kIdxSlots };
    fpm_ctx::Slot slot[kIdxSlots];
    unsigned long long *kmax = nullptr;
    IdxGeom geom{};
    bool sparse_ok = false;       // the index exists (the sparse path is possible)
    bool ref_unsorted = false;    // some reference row is unsorted / carries duplicates
    bool recorded = false;        // the index holds launch_record_rows copies
    uint64_t mr = 0;              // their row stride
    uint64_t self_events = 0;     // sum_b |b|^2: the posting events of the set against itself
    uint64_t n_indexed = 0;       // the index's entries (never cut: other blocks probe it in full)
    // per-query-block device buffers (fpm_refset_dist, fpm_refset_dist_list): the uploaded
    // block, its result grids, and the six arrays of the device cell list
    enum { kQRows, kQLen, kQLength, kQNumer, kQDenom, kQDist, kQPval, kQPass, kQList,
           kQSlots = kQList + 6 };
    fpm_ctx::Slot qslot[kQSlots];
    uint64_t list_cap = 0;        // entries the device list slots hold
    const uint32_t *dir() const { return (const uint32_t *)slot[kDir].p; }
    const uint32_t *entries() const { return (const uint32_t *)slot[kEntries].p; }
};

// Build the reference index of a resident set (once): over the raw rows, or, when a row is
// unsorted / carries duplicates (-fp lists), over their records (launch_record_rows: only
// pairs sharing a record value can count anything in the literal walk).
static int refset_build_index(fpm_refset *rs, hipStream_t st)
{
    fpm_ctx *ctx = rs->ctx;
    const RowSet &R = rs->ref;
    const uint64_t E = (uint64_t)R.n * R.stride;
    IdxGeom geom = make_geom(R.n, E, rs->sketch_size);
    rs->sparse_ok = E > 0 && geom.rbits <= 24 && E < (1ULL << 31);
    if (!rs->sparse_ok) return FPM_OK;
    void *ctr;
    HIP_TRY(scratch(ctx, kSlotCounters, kCtrWords * 8, &ctr));
    if (!rs->kmax) HIP_TRY(rs->mem.get(&rs->kmax, 8));
    auto build = [&](const RowSet &rows, IdxGeom &g, bool raw) -> int {
        void *dir, *entries;
        HIP_TRY(grow_slot(rs->ctx, rs->slot[fpm_refset::kDir], ((1ULL << g.nbits) + 1) * 4, &dir));
        HIP_TRY(grow_slot(rs->ctx, rs->slot[fpm_refset::kEntries], (uint64_t)R.n * rows.stride * 4, &entries));
        // the bucket pass also sums the self events (a query block that is the set itself
        // then needs no probe count)
        return build_index(ctx, rows, rs->hash_bytes, g, (uint32_t *)dir, (uint32_t *)entries,
                           (unsigned long long *)ctr, true, st, [] { return FPM_OK; }, raw);
    };
    geom.kmax = rs->kmax;
    if (int rc = build(R, geom, true)) return rc;
    rs->ref_unsorted = host_unsorted(ctx);
    rs->self_events = host_events(ctx);
    rs->n_indexed = host_indexed(ctx);
    rs->mr =std::min<uint64_t>(R.stride, rs->sketch_size);
    rs->recorded = rs->ref_unsorted;
    if (rs->recorded) {
        void *dref, *dref_len, *dref_pos;
        HIP_TRY(grow_slot(rs->ctx, rs->slot[fpm_refset::kRecRows], (size_t)R.n * rs->mr * rs->hash_bytes, &dref));
        HIP_TRY(grow_slot(rs->ctx, rs->slot[fpm_refset::kRecLen], (size_t)R.n * 4, &dref_len));
        HIP_TRY(grow_slot(rs->ctx, rs->slot[fpm_refset::kRecPos], (size_t)R.n * rs->mr * 4, &dref_pos));
        {
            TimedLaunch tl(ctx, FPM_K_INDEX, st);
            HIP_TRY(launch_record_rows(R, rs->hash_bytes, rs->sketch_size, dref,
                                       (uint32_t *)dref_pos, (uint32_t *)dref_len, rs->mr, nullptr,
                                       st));
            tl.done();
        }
        geom = make_geom(R.n, (uint64_t)R.n * rs->mr, 0);
        geom.kmax = rs->kmax;
        if (int rc = build(RowSet{dref, (const uint32_t *)dref_len, nullptr, rs->mr, R.n}, geom,
                           false))
            return rc;
        rs->n_indexed = host_indexed(ctx);
    }
    rs->geom = geom;
    return FPM_OK;
}

// ----------------------------------------------------------------------------
// The grid compare, in phases: index, (fill / prefill), candidates, or dense
// ----------------------------------------------------------------------------

// One compare_impl call: its inputs, what they imply, and the state of its side-stream fill,
// of a prefill it took over and of the compact output's list count.
struct Compare {
    fpm_ctx *ctx;
    hipStream_t st;
    RowSet R, Q;
    uint32_t hash_bytes, S;
    Counts cnt;
    const DistFinal *fin;
    fpm_refset *rs;
    uint64_t n_pairs;
    bool self_set, compact, want_mir;
    // The side-stream fill writes every cell's no-shared-hash values (full output: distance /
    // p-value / pass, 17 B per cell), and with fill_cnt the numer / denom defaults too, which
    // the probe then leaves out: the probe (event reads, latency-bound, slowed ~3x by any write
    // stream beside it) gets shorter and the bytes move beside the rank kernel.  Measured
    // (same box, full output): C4's 2.5e9-pair grid 16.7 -> 15.4 ms; C2's 1e8 pairs +1 %, so
    // by grid size.  A transposed grid's defaults are written by the fill only.  The compact
    // output needs a fill only for the counts.
    bool prefilled, fill_cnt, need_fill;
    // the compact output's list count starts at zero: cleared by the index build's first
    // kernel when this call builds an index (no memset launch), else by zero_list before the
    // first kernel that appends to the list
    unsigned long long *list_cnt;
    bool list_zeroed;
    bool prefill_done;            // settle_prefill ran (or there is no prefill)
    bool fill_pending = false;    // launch_fill ran: ev_fill is to be waited for
    // the probe writes the numer / denom defaults itself
    bool probe_defaults() const { return !fill_cnt && !prefilled; }
};

// What the index phase hands to the candidate phase: the index, the rows the probe reads, the
// posting events and sortedness it learned, and what it already enqueued.
struct SparsePlan {
    unsigned long long *ctr = nullptr;          // the counter block (CtrWord)
    IdxGeom geom{};
    const uint32_t *dir = nullptr, *entries = nullptr;
    const void *p_rows = nullptr;               // the rows the probe reads
    const uint32_t *p_len = nullptr;            // and their lengths (null: the query rows' own)
    uint64_t p_stride = 0;
    // those rows as the probe count's input
    RowSet counted(const RowSet &Q) const
    {
        return RowSet{p_rows, p_len ? p_len : Q.len, nullptr, p_stride, Q.n};
    }
    uint64_t ev = 0;
    bool all_sorted = true;
    RecRows rec_r{}, rec_q{};                   // record rows (unsorted lists) for the walk
    bool skip_count = false;                    // no probe count ran: the probe counts and tests
    bool spec_probe = false;                    // the probe is enqueued already (speculated)
    bool spec_half = false;                     // and took the half form
    CmpRows spec_cmp{};                         // and wrote the compacted rows (if any)
    unsigned long long *n_cand() const { return ctr + kCtrCand; }
    uint32_t *unsorted() const { return (uint32_t *)(ctr + kCtrUnsorted); }
    uint32_t *cand_over() const { return (uint32_t *)(ctr + kCtrCandOver); }
};

// The symmetric probe (one sorted set against itself on the rank kernel's path) takes the half
// form when the index's flags were cut at this call's sketch size (a resident set built at
// another S: the full form) and the context's switch is on.
static bool probe_half(const Compare &c, const SparsePlan &p, bool sym)
{
    // (sym already excludes record rows and the skip-count path: neither is a sorted set
    // against itself; the launcher refuses the half form with either)
    return sym && c.ctx->probe_half && p.geom.cut == c.S && !p.p_len && !p.skip_count;
}

// The probe's arguments that follow from the call and its plan.  The form (sym, defaults, half,
// cmp) and the skip-count path's outputs are set by the caller.
static ProbeRows probe_args(const Compare &c, const SparsePlan &p, const CandList &out,
                            uint64_t *row_seg)
{
    ProbeRows a;
    a.qry = RowSet{p.p_rows, c.Q.len, nullptr, p.p_stride, c.Q.n};
    a.qry_it_len = p.p_len;
    a.ref = c.R;
    a.hash_bytes = c.hash_bytes;
    a.S = c.S;
    a.g = p.geom;
    a.dir = p.dir;
    a.entries = p.entries;
    a.self_set = c.self_set;
    a.cnt = c.cnt;
    a.out = out;
    a.row_seg = row_seg;
    a.cand_over = p.cand_over();
    return a;
}

// The transient index of one set against itself leaves out every value above V*, the largest
// value a half probe looks up (IdxGeom::vcut), for exactly the calls that end in the half probe
// when they go sparse: probe_half's conditions and the rank kernel's (compare_impl's
// rows_merge), as far as the host knows them before the build.  What it learns afterwards
// leads elsewhere without a probe of this index: unsorted rows to the record index (rebuilt,
// uncut), a dense result to the dense walk.  Resident sets stay whole (other blocks probe them
// in full), and so do record indexes.
static bool index_cut_ok(const Compare &c)
{
    return c.ctx->index_cut && c.ctx->probe_half && !c.rs && c.self_set && c.hash_bytes == 8 &&
           c.S > 0 && c.R.n <= (1u << 19) && std::max(c.R.stride, c.Q.stride) <= 2048;
}

// The compacted candidate rows of a call whose probe takes the half form: one
// transient sorted u64 set against itself, every ref of a row in one probe workgroup, rows the
// probe's kept bits cover, the context's switch on.  Empty when the call does not qualify or the
// buffers cannot be had: the call then ranks the rows themselves.
static CmpRows compact_rows(const Compare &c, bool half)
{
    fpm_ctx *ctx = c.ctx;
    CmpRows cm;
    if (!half || !ctx->rank_compact || c.rs || !c.self_set || c.hash_bytes != 8 ||
        c.R.n > (1u << 19) || c.R.stride > kCmpMaxRow)
        return cm;
    void *rows = nullptr, *len = nullptr;
    if (scratch(ctx, kSlotCmpRows, (size_t)c.R.n * cmp_row_bytes(c.R.stride), &rows) != hipSuccess ||
        scratch(ctx, kSlotCmpLen, (size_t)c.R.n * 8, &len) != hipSuccess) {
        (void)hipGetLastError();
        return cm;
    }
    cm.rows = rows;
    cm.len = (uint32_t *)len;
    return cm;
}

// The sparse / dense rule, the candidate capacity and the speculation profile are stated in the
// posting events of the whole index.  A cut index counts those of its indexed values only:
// scaled by entries / indexed entries, rounded up (exact when the sharing is spread evenly
// over the rows' range, never below the cut count; candidates <= cut events still holds).
static uint64_t whole_index_events(uint64_t ev, uint64_t entries, uint64_t indexed)
{
    if (!indexed || indexed >= entries) return ev;
    const unsigned __int128 x = (unsigned __int128)ev * entries + (indexed - 1);
    const unsigned __int128 q = x / indexed;
    return q > (unsigned __int128)UINT64_MAX ? UINT64_MAX : (uint64_t)q;
}

// what fpm_ctx_last_index_cut reports, after an index build's counters were read
static void note_index(fpm_ctx *ctx, const IdxGeom &g)
{
    ctx->last_index_cut = g.vcut != 0;
    ctx->last_indexed = host_indexed(ctx);
    ctx->last_entries = host_entries(ctx);
}

static int zero_list(Compare &c)
{
    if (!c.list_zeroed) HIP_TRY(hipMemsetAsync(c.list_cnt, 0, 8, c.st));
    c.list_zeroed = true;
    return FPM_OK;
}

// a prefilled grid: wait for the prefill, then correct the pairs whose lists hold fewer
// than S hashes together, before the first write of a cell (once)
static int settle_prefill(Compare &c)
{
    if (c.prefill_done) return FPM_OK;
    c.prefill_done = true;
    HIP_TRY(hipStreamWaitEvent(c.st, c.ctx->ev_prefill, 0));
    HIP_TRY(launch_dist_counts_fixup(c.R, c.Q, c.S, (uint16_t *)c.cnt.denom, c.st));
    return FPM_OK;
}

// record_in = false: the caller recorded ev_in on `st` already (at the point the fill may
// start) and submits the fill after later work on `st`
static int launch_fill(Compare &c, bool record_in)
{
    fpm_ctx *ctx = c.ctx;
    const DistFinal *fin = c.fin;
    // (the compact output: the counts only)
    PairFill fill{c.compact ? CellOut{} : fin->prim.cell, fin->par.max_dist, fin->par.max_pvalue};
    HIP_TRY(ensure_aux(ctx));
    if (record_in) HIP_TRY(hipEventRecord(ctx->ev_in, c.st));
    HIP_TRY(hipStreamWaitEvent(ctx->aux, ctx->ev_in, 0));
    TimedLaunch tl(ctx, FPM_K_FILL, ctx->aux);
    // the flattened fill runs ~35 % faster alone but slows a rank kernel beside it more
    // (C2, 1e8 cells / 2.3e8 events: rank 0.66 -> 0.70 ms while the fill shrank 0.63 ->
    // 0.57; C4, 2.5e9 cells: 14.1 -> 12.8-13.3 ms).  The fill is the long pole when its
    // cells outweigh the posting events (the rank kernel's work): flattened when the cells
    // written (both grids with a transpose) times 1.6 exceed the events
    const long double cells_w = (long double)c.n_pairs * (c.want_mir ? 2 : 1);
    const bool flat = cells_w * 1.6L > (long double)ctx->last_events;
    HIP_TRY(launch_dist_fill(c.R, c.Q, c.S, c.fill_cnt ? c.cnt : Counts{}, fill, flat, ctx->aux));
    if (c.want_mir) {
        // the transposed grid: the query rows as refs, the ref rows as queries
        fill.out = c.compact ? CellOut{} : fin->mir.cell;
        HIP_TRY(launch_dist_fill(c.Q, c.R, c.S, fin->mir.cnt, fill, flat, ctx->aux));
    }
    tl.done();
    HIP_TRY(hipEventRecord(ctx->ev_fill, ctx->aux));
    c.fill_pending = true;
    return FPM_OK;
}

// Index phase without a resident set: build the index in the context's scratch, over the raw
// rows or (unsorted lists) over their records, with the query side's probe count behind it and,
// for a call of the last call's shape, the speculated probe.
static int index_transient(Compare &c, SparsePlan &p)
{
    fpm_ctx *ctx = c.ctx;
    hipStream_t st = c.st;
    const RowSet &R = c.R, &Q = c.Q;
    const uint32_t hash_bytes = c.hash_bytes;
    const bool self_set = c.self_set;
    unsigned long long *events = p.ctr;
    void *dir_, *entries_;
    HIP_TRY(scratch(ctx, kSlotDir, ((1ULL << p.geom.nbits) + 1) * 4, &dir_));
    HIP_TRY(scratch(ctx, kSlotEntries, (uint64_t)R.n * R.stride * 4, &entries_));
    p.dir = (const uint32_t *)dir_;
    p.entries = (const uint32_t *)entries_;
    // the query side's probe count behind an index build (a set against itself needs none)
    auto count_probe = [&]() -> int {
        if (!self_set)
            HIP_TRY(launch_probe_count(p.counted(Q), hash_bytes, p.geom, p.dir, events,
                                       p.unsorted(), st));
        return FPM_OK;
    };
    // Unsorted lists (-fp): the index runs over each row's records among its first
    // min(len, S) entries (launch_record_rows): ~ln(S) values per row instead of every
    // distinct one, and only pairs sharing a record can count anything.  The
    // candidates are walked on the original lists.
    const uint64_t mr = std::min<uint64_t>(R.stride, c.S);
    const uint64_t mq = std::min<uint64_t>(Q.stride, c.S);
    void *dref = nullptr, *dref_len = nullptr, *dref_pos = nullptr, *dqry = nullptr,
         *dqry_len = nullptr, *dqry_pos = nullptr;
    // the record rows of both sides; flag: also test every row's order into `unsorted`
    auto records = [&](uint32_t *flag) -> int {
        HIP_TRY(scratch(ctx, kSlotRecRef, (size_t)R.n * mr * hash_bytes, &dref));
        HIP_TRY(scratch(ctx, kSlotRecRefLen, (size_t)R.n * 4, &dref_len));
        HIP_TRY(scratch(ctx, kSlotRecRefPos, (size_t)R.n * mr * 4, &dref_pos));
        if (!self_set) {
            HIP_TRY(scratch(ctx, kSlotRecQry, (size_t)Q.n * mq * hash_bytes, &dqry));
            HIP_TRY(scratch(ctx, kSlotRecQryLen, (size_t)Q.n * 4, &dqry_len));
            HIP_TRY(scratch(ctx, kSlotRecQryPos, (size_t)Q.n * mq * 4, &dqry_pos));
        }
        TimedLaunch tl(ctx, FPM_K_INDEX, st);
        HIP_TRY(launch_record_rows(R, hash_bytes, c.S, dref, (uint32_t *)dref_pos,
                                   (uint32_t *)dref_len, mr, flag, st));
        if (!self_set)
            HIP_TRY(launch_record_rows(Q, hash_bytes, c.S, dqry, (uint32_t *)dqry_pos,
                                       (uint32_t *)dqry_len, mq, flag, st));
        tl.done();
        return FPM_OK;
    };
    // the index over the record rows (after records())
    auto record_index = [&]() -> int {
        p.rec_r = RecRows{dref, (const uint32_t *)dref_pos, (const uint32_t *)dref_len, mr};
        p.rec_q = self_set ? p.rec_r
                           : RecRows{dqry, (const uint32_t *)dqry_pos, (const uint32_t *)dqry_len, mq};
        p.p_rows = p.rec_q.val;
        p.p_len = p.rec_q.len;
        p.p_stride = p.rec_q.stride;
        p.geom = make_geom(R.n, (uint64_t)R.n * mr, 0);
        p.geom.kmax = events + kCtrKmax;
        if (int rc = build_index(ctx, RowSet{dref, p.rec_r.len, nullptr, mr, R.n}, hash_bytes,
                                 p.geom, (uint32_t *)dir_, (uint32_t *)entries_, events, self_set,
                                 st, count_probe, false, nullptr,
                                 c.list_zeroed ? nullptr : c.list_cnt))
            return rc;
        c.list_zeroed = true;
        p.all_sorted = false;
        p.ev = host_events(ctx);
        note_index(ctx, p.geom);
        return FPM_OK;
    };
    if (hash_bytes == 4) {
        // u32 rows (the -fp lists; k <= 16 sketches): their order is tested with the
        // records, and unsorted rows go straight to the record index (C3: the raw
        // index built only to learn the order cost ~0.2 ms of 1.45)
        HIP_TRY(hipMemsetAsync(p.unsorted(), 0, sizeof(uint32_t), st));
        if (int rc = records(p.unsorted())) return rc;
        if (int rc = read_counters(ctx, events, kCtrProbeWords, st)) return rc;
        if (host_unsorted(ctx)) return record_index();
    }
    p.geom.kmax = events + kCtrKmax;
    p.geom.vcut = index_cut_ok(c) ? 1u : 0u;
    // A call of the last sparse rank-kernel call's shape (the bench's steps, a
    // pipeline's batches) enqueues its probe behind the index build before the
    // host reads the build's counters, so the GPU is not idle while the host
    // waits for them and launches (14-20 us per call); the probe's
    // candidates are kept when the counters confirm the path (sorted rows, sparse)
    // and the capacity (candidates <= min(events, pairs) <= cap).
    const fpm_ctx::SpecProfile &pf = ctx->spec;
    const bool can_spec = pf.valid && hash_bytes == 8 && pf.n_ref == R.n && pf.n_qry == Q.n &&
                          pf.S == c.S && pf.ref_stride == R.stride && pf.qry_stride == Q.stride &&
                          pf.self_set == self_set && pf.defaults == c.probe_defaults() &&
                          ctx->dist_mode != FPM_DIST_DENSE && R.n <= (1u << 19) &&
                          std::max(R.stride, Q.stride) <= 2048;
    auto speculate = [&]() -> int {
        p.spec_probe = false;
        if (!can_spec) return FPM_OK;
        void *cand, *row_seg;
        HIP_TRY(scratch(ctx, kSlotCand, pf.cap * 8, &cand));
        HIP_TRY(scratch(ctx, kSlotRowSeg, (size_t)Q.n * 8, &row_seg));
        // the form the confirmed call takes (sym = self_set there: it is kept only on the
        // rank kernel's path)
        p.spec_half = probe_half(c, p, self_set);
        // (the compacted rows' buffers are had before the probe is enqueued; a dropped
        // speculation drops them with it)
        p.spec_cmp = compact_rows(c, p.spec_half);
        TimedLaunch tl(ctx, FPM_K_PROBE, st);
        ProbeRows a = probe_args(c, p, CandList{(uint64_t *)cand, p.n_cand(), pf.cap},
                                 (uint64_t *)row_seg);
        a.sym = self_set;
        a.defaults = pf.defaults;
        a.half = p.spec_half;
        a.cmp = p.spec_cmp;
        HIP_TRY(launch_probe_rows(a, st));
        tl.done();
        p.spec_probe = true;
        return FPM_OK;
    };
    // one set against itself: the query side is the ref side, so its sortedness
    // is the ref flag and its posting events are sum_b |b|^2 from the bucket pass.
    // The counters are zeroed by the first index kernel.
    if (int rc = build_index(ctx, R, hash_bytes, p.geom, (uint32_t *)dir_, (uint32_t *)entries_,
                             events, self_set, st, count_probe, true, speculate,
                             c.list_zeroed ? nullptr : c.list_cnt))
        return rc;
    c.list_zeroed = true;
    p.ev = whole_index_events(host_events(ctx), host_entries(ctx), host_indexed(ctx));
    p.all_sorted = !host_unsorted(ctx);
    note_index(ctx, p.geom);
    if (p.all_sorted) return FPM_OK;
    if (hash_bytes != 4)
        if (int rc = records(nullptr)) return rc;
    return record_index();
}

// Index phase: pick the index and learn the posting events and the sortedness.  A resident
// set brings its index; what remains is the query block's side: nothing for the set against
// itself, nothing yet with skip_count (the probe counts), else a probe count (over the
// block's record rows when the index holds records).
static int index_phase(Compare &c, SparsePlan &p)
{
    fpm_ctx *ctx = c.ctx;
    fpm_refset *rs = c.rs;
    hipStream_t st = c.st;
    const RowSet &Q = c.Q;
    if (!rs) return index_transient(c, p);
    ctx->last_indexed = ctx->last_entries = rs->n_indexed;
    // A resident sorted set against another block of sorted rows (the C4 block pairs, the
    // CLI's query blocks): no probe count.  The count pass reads every query hash's
    // bucket bounds at random (~0.27 ms for 2.2e7 hashes at N = 8, as long as the index
    // rebuild), and the probe reads them again; instead the probe reports the row's
    // posting events and whether the query rows are sorted, and the candidate compare is
    // chosen after it (rank kernel, or the literal walk for unsorted rows: the candidates
    // are the same).  Taken in the forced sparse mode, and in AUTO when the set's own
    // density (its self events per row) says the block is far from the dense regime.
    const long double ev_est =
        (long double)rs->self_events * Q.n / std::max<uint32_t>(1, rs->ref.n);
    p.skip_count = !c.self_set && !rs->recorded && !rs->ref_unsorted && c.hash_bytes == 8 &&
                   (ctx->dist_mode == FPM_DIST_SPARSE ||
                    (ctx->dist_mode == FPM_DIST_AUTO &&
                     ev_est * 16.0L <= (long double)c.n_pairs * c.S));
    p.geom = rs->geom;
    p.dir = rs->dir();
    p.entries = rs->entries();
    if (c.self_set && !rs->recorded) {
        // the resident set against itself: its posting events and sortedness are the
        // index build's (sum_b |b|^2, the reference flag), no probe count
        p.ev = rs->self_events;
        p.all_sorted = !rs->ref_unsorted;
        // (the candidate counter among them)
        HIP_TRY(hipMemsetAsync(p.ctr, 0, kCtrProbeWords * 8, st));
        return FPM_OK;
    }
    if (p.skip_count) {
        p.ev = (uint64_t)ev_est;        // replaced by the probe's own count
        p.all_sorted = true;            // verified by the probe
        HIP_TRY(hipMemsetAsync(p.ctr, 0, kCtrProbeWords * 8, st));
        return FPM_OK;
    }
    // count this block's posting events (and its sortedness)
    TimedLaunch tl(ctx, FPM_K_INDEX, st);
    HIP_TRY(hipMemsetAsync(p.ctr, 0, kCtrProbeWords * 8, st));
    if (rs->recorded) {
        const uint64_t mq = std::min<uint64_t>(Q.stride, c.S);
        void *dqry, *dqry_len, *dqry_pos;
        HIP_TRY(scratch(ctx, kSlotRecQry, (size_t)Q.n * mq * c.hash_bytes, &dqry));
        HIP_TRY(scratch(ctx, kSlotRecQryLen, (size_t)Q.n * 4, &dqry_len));
        HIP_TRY(scratch(ctx, kSlotRecQryPos, (size_t)Q.n * mq * 4, &dqry_pos));
        HIP_TRY(launch_record_rows(Q, c.hash_bytes, c.S, dqry, (uint32_t *)dqry_pos,
                                   (uint32_t *)dqry_len, mq, nullptr, st));
        p.rec_r = RecRows{rs->slot[fpm_refset::kRecRows].p,
                          (const uint32_t *)rs->slot[fpm_refset::kRecPos].p,
                          (const uint32_t *)rs->slot[fpm_refset::kRecLen].p, rs->mr};
        p.rec_q = RecRows{dqry, (const uint32_t *)dqry_pos, (const uint32_t *)dqry_len, mq};
        p.p_rows = dqry;
        p.p_len = (const uint32_t *)dqry_len;
        p.p_stride = mq;
    }
    HIP_TRY(launch_probe_count(p.counted(Q), c.hash_bytes, p.geom, p.dir, p.ctr, p.unsorted(), st));
    tl.done();
    if (int rc = read_counters(ctx, p.ctr, kCtrProbeWords, st)) return rc;
    p.ev = host_events(ctx);
    // record rows are sorted by construction: the query's own order is what the walk
    // needs, so the walk is literal whenever the index holds records
    p.all_sorted = !rs->ref_unsorted && !rs->recorded && !host_unsorted(ctx);
    return FPM_OK;
}

// the rank kernel over the probe's candidates: results into cl's per-candidate slots, if any
// (cmp: the compacted rows the call's probe wrote, if any)
static hipError_t rank_candidates(const Compare &c, const CandList &cl, const void *row_seg,
                                  bool sym, CmpRows cmp = CmpRows{})
{
    uint32_t rank_cap = 0;
    const hipError_t e = launch_merge_rows(cl, (const uint64_t *)row_seg, c.R, c.Q, c.S, sym, c.cnt,
                                           cmp, &rank_cap, c.st);
    c.ctx->last_rank_compact = cmp.rows != nullptr;
    c.ctx->last_cmp_len = cmp.len;
    c.ctx->last_cmp_n = c.R.n;
    c.ctx->last_cmp_stream = c.st;
    c.ctx->last_kernel = rank_cap == 1024 ? FPM_DK_CAND_RANK_1024 : FPM_DK_CAND_RANK_2048;
    return e;
}

// Candidate phase: the probe (unless speculated), the candidate compare (rank kernel, or the
// literal walk), the side fill ordered around it, and with `fin` the candidate finalize.
static int candidate_phase(Compare &c, SparsePlan &p, bool rows_merge, uint64_t cap)
{
    fpm_ctx *ctx = c.ctx;
    hipStream_t st = c.st;
    const RowSet &R = c.R, &Q = c.Q;
    const DistFinal *fin = c.fin;
    // one sorted set against itself: (numer, denom) of sorted distinct lists is
    // symmetric in the two sets, so each unordered pair is ranked once (by the row the
    // probe gives it: pair parity) and each result is written to both cells (q, r) and
    // (r, q)
    const bool sym = rows_merge && c.self_set;
    const bool half = p.spec_probe ? p.spec_half : probe_half(c, p, sym);
    ctx->last_probe = half ? FPM_PROBE_HALF : FPM_PROBE_FULL;
    // A cut index holds only the values a half probe looks up: no other form may run on it.
    // index_cut_ok admits only calls that take the half form here, so this is a guard, not a
    // path: should the two ever disagree, the index is rebuilt whole (any speculated probe
    // dropped with it) and the call goes on as without the cut.
    if (p.geom.vcut && !half) {
        p.geom.vcut = 0;
        p.spec_probe = false;
        if (int rc = build_index(ctx, R, c.hash_bytes, p.geom, const_cast<uint32_t *>(p.dir),
                                 const_cast<uint32_t *>(p.entries), p.ctr, c.self_set, st,
                                 [] { return FPM_OK; }))
            return rc;
        p.ev = host_events(ctx);
        note_index(ctx, p.geom);
        ctx->last_events = p.ev;
        cap = std::max<uint64_t>(1, std::min<uint64_t>(p.ev, c.n_pairs));
    }
    const CmpRows cmp = p.spec_probe ? p.spec_cmp : compact_rows(c, half);
    void *cand, *row_seg;
    HIP_TRY(scratch(ctx, kSlotCand, cap * 8, &cand));
    HIP_TRY(scratch(ctx, kSlotRowSeg, (size_t)Q.n * 8, &row_seg));
    CandList cl{(uint64_t *)cand, p.n_cand(), cap};
    if (!p.spec_probe) {
        TimedLaunch tl(ctx, FPM_K_PROBE, st);
        ProbeRows a = probe_args(c, p, cl, (uint64_t *)row_seg);
        a.sym = sym;
        a.defaults = c.probe_defaults();
        a.half = half;
        a.cmp = cmp;
        if (p.skip_count) {     // no probe count ran: the probe tests the order and counts
            a.q_unsorted = p.unsorted();
            a.events = p.ctr;
        }
        HIP_TRY(launch_probe_rows(a, st));
        tl.done();
    }
    // A resident sorted set against a block without a count (skip_count): the rank
    // kernel is enqueued behind the probe before the host waits for the probe's
    // sortedness flag (the block's rows are sorted in every bench / CLI use; a row
    // that is not makes its rank workgroup exit, and the results are then dropped for
    // the literal walk), so the GPU does not idle while the host reads and launches.
    // The fill may start where the probe ends (ev_in) and is submitted after the read.
    bool rank_done = false;
    if (p.skip_count) {
        unsigned long long seq;
        if (int rc = publish_counters(ctx, p.ctr, kCtrProbeWords, st, &seq)) return rc;
        if (fin && rows_merge) {
            void *cres;
            HIP_TRY(scratch(ctx, kSlotCandRes, cap * 8, &cres));
            if (c.need_fill) {
                HIP_TRY(ensure_aux(ctx));
                HIP_TRY(hipEventRecord(ctx->ev_in, st));
            }
            TimedLaunch tl(ctx, FPM_K_COMPARE, st);
            CandList slots = cl;
            slots.cnum = (uint32_t *)cres;
            slots.cden = slots.cnum + cap;
            HIP_TRY(rank_candidates(c, slots, row_seg, sym));
            tl.done();
            rank_done = true;
        }
        if (int rc = wait_counters(ctx, seq, st)) return rc;
        ctx->last_events = host_events(ctx);
        if (host_unsorted(ctx)) {
            p.all_sorted = false;       // unsorted query rows: the literal walk
            rows_merge = false;
            rank_done = false;          // (its per-candidate slots are not read)
        }
    }
    // The rank kernel keeps its results in per-candidate slots (cnum / cden) and leaves
    // the grid alone, so the fill (needing only the list lengths) runs beside it on the
    // side stream, and the candidate finalize scatters the results after both.  The
    // literal walk writes cells in place, so it waits for the fill instead.  (Beside the
    // index build or the probe the fill slowed both: they move as many bytes as it does.)
    if (fin && rows_merge) {
        void *cres;
        HIP_TRY(scratch(ctx, kSlotCandRes, cap * 8, &cres));
        cl.cnum = (uint32_t *)cres;
        cl.cden = cl.cnum + cap;
    }
    const bool cnum = cl.cnum != nullptr;
    // (Submitted before the probe instead, the fill slows the probe more than it gains:
    // C4 one GPU 6.66 -> 6.80-6.86 ms, same box, r04.  Written by the rank kernel's own
    // row workgroups after their candidates instead of beside them: rank 2.7 -> 3.3 ms
    // with the fill inside, C4 6.48-6.55 -> 6.69-6.72 ms, same box, r04.)
    // After the host read of the probe's counters the GPU is idle: a fill submitted
    // first would take every CU before the rank kernel's workgroups arrive (rank +
    // fill 0.39 + 1.51 -> 0.55 + 1.67 ms at N = 8).  The fill may start where the probe
    // ends (ev_in recorded here) but is submitted after the candidate compare.
    const bool defer_fill = c.need_fill && p.skip_count && rows_merge;
    if (defer_fill) {
        HIP_TRY(ensure_aux(ctx));
        if (!rank_done) HIP_TRY(hipEventRecord(ctx->ev_in, st));
    } else if (c.need_fill) {
        if (int rc = launch_fill(c, true)) return rc;
    }
    if (c.fill_pending && !cnum) HIP_TRY(hipStreamWaitEvent(st, ctx->ev_fill, 0));
    if (!cnum)                              // the literal walk writes cells in place
        if (int rc = settle_prefill(c)) return rc;
    if (!rank_done) {
        TimedLaunch tl(ctx, FPM_K_COMPARE, st);
        if (rows_merge)
            HIP_TRY(rank_candidates(c, cl, row_seg, sym, cmp));
        else {
            HIP_TRY(launch_walk_candidates(cl, R, Q, c.hash_bytes, c.S, c.cnt, p.rec_r, p.rec_q,
                                           st));
            ctx->last_kernel = FPM_DK_CAND_WALK;
        }
        tl.done();
    }
    if (defer_fill)
        if (int rc = launch_fill(c, false)) return rc;
    if (c.fill_pending && cnum) HIP_TRY(hipStreamWaitEvent(st, ctx->ev_fill, 0));
    if (int rc = settle_prefill(c)) return rc;
    if (fin) {
        if (int rc = zero_list(c)) return rc;
        const DistParams &par = fin->par;
        const bool mirror = c.want_mir && cnum;
        TimedLaunch tl(ctx, FPM_K_FINALIZE, st);
        if (c.compact) {
            const CellList none{};
            HIP_TRY(launch_dist_cand_list(cl, sym, c.cnt, R, Q, par, fin->prim.list,
                                          mirror ? fin->mir.cnt : Counts{},
                                          mirror ? fin->mir.list : none, st));
        } else {
            MirrorOut mir{};
            if (mirror) mir = MirrorOut{fin->mir.cnt, fin->mir.cell, Q.n};
            HIP_TRY(launch_dist_cand_finalize(cl, sym, c.cnt, R, Q, par, fin->prim.cell, mir, st));
        }
        tl.done();
        if (mirror && fin->mirrored) *fin->mirrored = true;
    }
    ctx->last_sparse = rows_merge ? 2 : 1;
    ctx->last_cand = (uint64_t)-1;   // read by fpm_ctx_last_dist_stats (sync + copy)
    ctx->last_cand_dev = p.n_cand();
    ctx->last_cand_stream = st;
    return FPM_OK;
}

// Dense phase: every cell's counts by the grid walk (dist_dev_impl finalizes, or lists the
// cells of the dense grid, afterwards).
static int dense_phase(Compare &c)
{
    fpm_ctx *ctx = c.ctx;
    hipStream_t st = c.st;
    const RowSet &R = c.R, &Q = c.Q;
    if (int rc = zero_list(c)) return rc;
    // the dense compare writes every cell: after a prefill, not beside it
    if (c.prefilled && !c.prefill_done) {
        HIP_TRY(hipStreamWaitEvent(st, ctx->ev_prefill, 0));
        c.prefill_done = true;
    }
    ctx->last_cand = c.n_pairs;
    void *ublk = nullptr, *bimg = nullptr;
    const bool img = compare_grid_img_ok(c.hash_bytes, c.S, R.stride, Q.stride);
    if (img) {
        size_t ub, bb;
        compare_grid_img_scratch(Q.n, c.S, R.stride, Q.stride, &ub, &bb);
        HIP_TRY(scratch(ctx, kSlotImgBlocks, ub, &ublk));
        HIP_TRY(scratch(ctx, kSlotImg, bb, &bimg));
    }
    TimedLaunch tl(ctx, FPM_K_COMPARE, st);
    if (img) {
        HIP_TRY(launch_compare_grid_img(R, Q, c.S, ublk, bimg, c.cnt, st));
        ctx->last_kernel = FPM_DK_GRID_IMG;
    } else {
        bool lds = false;
        HIP_TRY(launch_compare_grid(R, Q, c.hash_bytes, c.S, c.cnt, &lds, st));
        ctx->last_kernel = lds ? FPM_DK_GRID_LDS : FPM_DK_GRID_GLOBAL;
    }
    tl.done();
    return FPM_OK;
}

// The grid compare: dense walk, or bucket index + probe + candidate kernel (sparse).
// With `fin`, a sparse run also finalizes (full outputs, or the compact list) and sets
// *finalized.  With `rs`, the references are that resident set and its index is reused.
static int compare_impl(fpm_ctx *ctx, const RowSet &R, const RowSet &Q, uint32_t hash_bytes,
                        uint32_t sketch_size, Counts cnt, void *stream,
                        const DistFinal *fin = nullptr, bool *finalized = nullptr,
                        fpm_refset *rs = nullptr)
{
    if (finalized) *finalized = false;
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    hipStream_t st = pick_stream(ctx, stream);
    if (ctx->prefill.pending) {
        // a prefill this call does not take over: nothing here may run beside it
        HIP_TRY(hipStreamWaitEvent(st, ctx->ev_prefill, 0));
        ctx->prefill.pending = false;
    }
    const uint64_t n_pairs = (uint64_t)R.n * Q.n;
    ctx->last_sparse = 0;
    ctx->last_kernel = FPM_DK_NONE;
    ctx->last_probe = FPM_PROBE_NONE;
    ctx->last_index_cut = false;
    ctx->last_rank_compact = false;
    ctx->last_indexed = ctx->last_entries = 0;
    ctx->last_events = 0;
    ctx->last_cand = 0;
    if (n_pairs == 0) {
        if (fin && fin->compact()) HIP_TRY(hipMemsetAsync(fin->prim.list.count, 0, 8, st));
        return FPM_OK;
    }
    const uint64_t E = (uint64_t)R.n * R.stride;   // index entries (upper bound)
    bool try_sparse = ctx->dist_mode == FPM_DIST_SPARSE ||
                      (ctx->dist_mode == FPM_DIST_AUTO && n_pairs >= 4096 && E > 0);
    if (E == 0) try_sparse = false;
    SparsePlan p;
    p.geom = make_geom(R.n, E, sketch_size);
    if (p.geom.rbits > 24 || E >= (1ULL << 31)) try_sparse = false;
    if (rs && !rs->sparse_ok) try_sparse = false;
    Compare c{ctx, st, R, Q, hash_bytes, sketch_size, cnt, fin, rs, n_pairs};
    c.self_set = R.rows == Q.rows && R.len == Q.len && R.stride == Q.stride && R.n == Q.n;
    c.compact = fin && fin->compact();
    c.want_mir = fin && fin->has_mirror() && !c.self_set;
    c.prefilled = fin && fin->prefilled;
    c.fill_cnt = fin && !c.prefilled &&
                 (c.want_mir || (ctx->fill_counts < 0 ? n_pairs >= (1ULL << 28)
                                                      : ctx->fill_counts != 0));
    c.need_fill = fin && (!c.compact || c.fill_cnt);
    c.list_cnt = c.compact ? reinterpret_cast<unsigned long long *>(fin->prim.list.count) : nullptr;
    c.list_zeroed = !c.compact;
    c.prefill_done = !c.prefilled;
    if (!try_sparse) return dense_phase(c);

    void *ctr;
    HIP_TRY(scratch(ctx, kSlotCounters, kCtrWords * 8, &ctr));
    p.ctr = (unsigned long long *)ctr;
    p.p_rows = Q.rows;
    p.p_stride = Q.stride;
    if (int rc = index_phase(c, p)) return rc;
    ctx->last_events = p.ev;
    // Unsorted lists: a candidate costs a literal walk of ~S steps from global memory,
    // and whether the walk ever meets a shared value depends on the order, so a pair
    // sharing values rarely shares a counted one (C3: every pair shares the frequent
    // k-fingers, 4 % have numer > 0).  Take the index path only when the events say
    // most pairs share nothing (fewer events than half the pairs).
    const bool sparse = ctx->dist_mode == FPM_DIST_SPARSE ||
                        ((long double)p.ev * 4.0L <= (long double)n_pairs * sketch_size &&
                         (p.all_sorted || 2 * p.ev <= n_pairs));
    const bool rows_merge = sparse && p.all_sorted && hash_bytes == 8 && R.n <= (1u << 19) &&
                            std::max(R.stride, Q.stride) <= 2048;
    // without a count the candidates are bounded by the pairs only
    uint64_t cap = std::max<uint64_t>(1, p.skip_count ? n_pairs : std::min<uint64_t>(p.ev, n_pairs));
    if (p.spec_probe) {
        // the speculated probe stands when it took this call's path and its buffer held
        // every candidate: sparse, rank kernel (sorted rows), the symmetric choice it made
        // (self_set), candidates <= min(events, pairs) <= its capacity
        if (rows_merge && cap <= ctx->spec.cap) {
            cap = ctx->spec.cap;
            ctx->spec_hits++;
        } else {
            p.spec_probe = false;
            ctx->spec_misses++;
            HIP_TRY(hipMemsetAsync(p.n_cand(), 0, 8, st));
            HIP_TRY(hipMemsetAsync(p.cand_over(), 0, 4, st));
        }
    }
    if (rows_merge && !p.skip_count) {
        // the profile of this shape for the next call (capacity grow-only)
        fpm_ctx::SpecProfile &pf = ctx->spec;
        const bool same = pf.valid && pf.n_ref == R.n && pf.n_qry == Q.n && pf.S == sketch_size &&
                          pf.ref_stride == R.stride && pf.qry_stride == Q.stride &&
                          pf.self_set == c.self_set;
        const uint64_t keep = same ? std::max(pf.cap, cap) : cap;
        pf = fpm_ctx::SpecProfile{true, R.n, Q.n, sketch_size, R.stride, Q.stride,
                                  keep, c.self_set, c.probe_defaults()};
    }
    if (!sparse) return dense_phase(c);
    if (int rc = candidate_phase(c, p, rows_merge, cap)) return rc;
    if (fin) *finalized = true;
    return FPM_OK;
}

// compare + finalize on device buffers (fpm_dist_dev* and fpm_dist_list_dev*)
static int dist_dev_impl(fpm_ctx *ctx, const RowSet &R, const RowSet &Q, uint32_t hash_bytes,
                         uint32_t sketch_size, const DistParams &par, const DistOut &out,
                         void *stream, const char *who, fpm_refset *rs = nullptr,
                         const DistOut *mirror = nullptr)
{
    const bool compact = out.list.count != nullptr;
    if (!R.length || !Q.length) return fail(FPM_EINVAL, std::string(who) + ": lengths required");
    if (!out.cnt.numer || !out.cnt.denom)
        return fail(FPM_EINVAL, std::string(who) + ": numer / denom buffers required");
    if (compact ? (!out.list.qry || !out.list.ref || !out.list.dist || !out.list.pval)
                : (!out.cell.dist || !out.cell.pval))
        return fail(FPM_EINVAL, std::string(who) +
                                    (compact ? ": list qry / ref / distance / p-value buffers required"
                                             : ": distance and p-value buffers required"));
    hipStream_t st = pick_stream(ctx, stream);
    // the prefill of this very grid (fpm_dist_list_prefill) is taken over; any other waits in
    // compare_impl
    bool prefilled = false;
    if (ctx->prefill.pending) {
        const fpm_ctx::Prefill &pf = ctx->prefill;
        prefilled = compact && out.cnt.c16 && !mirror && !rs && pf.numer == out.cnt.numer &&
                    pf.denom == out.cnt.denom && pf.n_ref == R.n && pf.n_qry == Q.n &&
                    pf.S == sketch_size;
        if (prefilled) ctx->prefill.pending = false;
    }
    // (the list count is cleared inside compare_impl: by the index build, else a memset)
    DistFinal fin{par, out};
    fin.prefilled = prefilled;
    bool finalized = false, mirrored = false;
    if (mirror) {
        fin.mir = *mirror;
        fin.mirrored = &mirrored;
        if (compact) HIP_TRY(hipMemsetAsync(mirror->list.count, 0, 8, st));
    }
    if (int rc = compare_impl(ctx, R, Q, hash_bytes, sketch_size, out.cnt, stream, &fin,
                              &finalized, rs)) {
        // an error before the compare ordered itself after a taken-over prefill: the side
        // stream may still be writing the caller's counts, so wait for it before returning
        if (prefilled) (void)hipEventSynchronize(ctx->ev_prefill);
        return rc;
    }
    if (!finalized) {
        TimedLaunch tl(ctx, FPM_K_FINALIZE, st);
        if (compact)
            HIP_TRY(launch_dist_grid_list(out.cnt, R, Q, par, out.list, st));
        else
            HIP_TRY(launch_dist_finalize(out.cnt, R, Q, par, out.cell, st));
        tl.done();
    }
    // the transposed grid, when the compare could not scatter it (dense path, unsorted lists:
    // their literal walk is not symmetric): the swapped call, ref and query sets exchanged
    if (!mirror || mirrored) return FPM_OK;
    return dist_dev_impl(ctx, Q, R, hash_bytes, sketch_size, par, *mirror, stream, who);
}

static DistOut full_out(void *numer, void *denom, bool c16, double *dist, double *pval,
                        uint8_t *pass)
{
    return DistOut{Counts{numer, denom, c16}, CellOut{dist, pval, pass}};
}

static int list_out(void *numer, void *denom, bool c16, const fpm_cell_list *l, DistOut &o,
                    const char *who)
{
    if (!l || !l->count) return fail(FPM_EINVAL, std::string(who) + ": cell list with a count required");
    o.cnt = Counts{numer, denom, c16};
    o.list = CellList{l->qry, l->ref, l->dist, l->pvalue, l->pass,
                      (unsigned long long *)l->count, l->cap};
    return FPM_OK;
}

namespace {
// The device side of a host-memory grid call (fpm_dist, fpm_fp_positional_grid): the uploaded
// rows and the five result grids, freed on every return path.
struct GridStage {
    fpm_ctx *ctx;
    hipError_t e = hipSuccess;
    DevBufs mem{ctx};
    void *r = nullptr, *q = nullptr;
    uint32_t *rl = nullptr, *ql = nullptr, *nu = nullptr, *de = nullptr;
    uint64_t *rL = nullptr, *qL = nullptr;
    double *di = nullptr, *pv = nullptr;
    uint8_t *pa = nullptr;
    template <typename T> void up(T *&b, const void *h, size_t bytes)
    {
        if (e == hipSuccess) e = mem.upload(ctx, &b, h, bytes);
    }
    // the result grids of np cells: the counts, and with `full` distance / p-value / pass
    void results(uint64_t np, bool full)
    {
        up(nu, nullptr, np * 4);
        up(de, nullptr, np * 4);
        if (!full) return;
        up(di, nullptr, np * 8);
        up(pv, nullptr, np * 8);
        up(pa, nullptr, np);
    }
    // the result grids the caller asked for -> its memory, once the context stream is done
    int fetch(uint64_t np, uint32_t *numer, uint32_t *denom, double *dist, double *pvalue,
              uint8_t *pass)
    {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (numer) HIP_TRY(copy_out(ctx, numer, nu, np * 4));
        if (denom) HIP_TRY(copy_out(ctx, denom, de, np * 4));
        if (dist) HIP_TRY(copy_out(ctx, dist, di, np * 8));
        if (pvalue) HIP_TRY(copy_out(ctx, pvalue, pv, np * 8));
        if (pass) HIP_TRY(copy_out(ctx, pass, pa, np));
        return FPM_OK;
    }
};
}  // namespace

static int refset_check(fpm_refset *rs, uint32_t sketch_size, uint32_t count_bytes,
                        const char *who)
{
    if (!rs) return fail(FPM_EINVAL, std::string(who) + ": null set");
    // an index over records holds those of each row's first min(len, S) entries: S is the
    // set's.  Sorted rows are indexed whole, so a call at another S probes the same index
    // (the set against itself then takes the full probe: the flags were cut at the set's S)
    if (sketch_size != rs->sketch_size && rs->recorded)
        return fail(FPM_EINVAL, std::string(who) + ": sketch_size differs from the set's");
    if (count_bytes != 2 && count_bytes != 4) return fail(FPM_EINVAL, "count_bytes must be 2 or 4");
    if (count_bytes == 2 && sketch_size > 65535)
        return fail(FPM_EINVAL, std::string(who) + ": u16 counts need sketch_size <= 65535");
    return set_device(rs->ctx);
}

static int refset_list_impl(fpm_refset *rs, const RowSet &Q, uint32_t sketch_size,
                            const DistParams &par, uint32_t count_bytes, void *d_numer,
                            void *d_denom, const fpm_cell_list *list, void *stream,
                            const char *who)
{
    if (int rc = refset_check(rs, sketch_size, count_bytes, who)) return rc;
    DistOut o;
    if (int rc = list_out(d_numer, d_denom, count_bytes == 2, list, o, who)) return rc;
    return dist_dev_impl(rs->ctx, rs->ref, Q, rs->hash_bytes, sketch_size, par, o, stream, who, rs);
}

static int mirror_check(fpm_refset *rs, const void *d_qry, const char *who)
{
    if (d_qry == rs->ref.rows)
        return fail(FPM_EINVAL, std::string(who) + ": the query rows are the reference rows "
                                                   "(use the non-mirror call: that grid is its "
                                                   "own transpose)");
    return FPM_OK;
}

// One host query block into the set's device slots (rows, entry counts, sequence lengths: zero
// without `length`), with `n_out` result grids of `out_bytes[i]` each sized beside them.
static int refset_stage_query(fpm_refset *rs, const RowSet &h, RowSet &d, int n_out,
                              const size_t *out_bytes, void **out)
{
    fpm_ctx *ctx = rs->ctx;
    hipStream_t st = ctx->stream;
    void *q, *ql, *qL;
    const size_t qb = (size_t)h.n * h.stride * rs->hash_bytes;
    HIP_TRY(grow_slot(rs->ctx, rs->qslot[fpm_refset::kQRows], std::max<size_t>(16, qb), &q));
    HIP_TRY(grow_slot(rs->ctx, rs->qslot[fpm_refset::kQLen], (size_t)h.n * 4, &ql));
    HIP_TRY(grow_slot(rs->ctx, rs->qslot[fpm_refset::kQLength], (size_t)h.n * 8, &qL));
    for (int i = 0; i < n_out; i++)
        HIP_TRY(grow_slot(rs->ctx, rs->qslot[fpm_refset::kQNumer + i], out_bytes[i], &out[i]));
    HIP_TRY(hipStreamSynchronize(st));            // the query slots are free to overwrite
    HIP_TRY(copy_in(ctx, q, h.rows, qb));
    HIP_TRY(copy_in(ctx, ql, h.len, (size_t)h.n * 4));
    if (h.length)
        HIP_TRY(copy_in(ctx, qL, h.length, (size_t)h.n * 8));
    else
        HIP_TRY(hipMemsetAsync(qL, 0, (size_t)h.n * 8, st));
    d = RowSet{q, (const uint32_t *)ql, (const uint64_t *)qL, h.stride, h.n};
    return FPM_OK;
}

extern "C" {

int fpm_compare_grid_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                         uint64_t ref_stride, uint32_t n_ref, const void *d_qry,
                         const uint32_t *d_qry_len, uint64_t qry_stride, uint32_t n_qry,
                         uint32_t hash_bytes, uint32_t sketch_size, uint32_t *d_numer,
                         uint32_t *d_denom, void *stream)
{
    return compare_impl(ctx, RowSet{d_ref, d_ref_len, nullptr, ref_stride, n_ref},
                        RowSet{d_qry, d_qry_len, nullptr, qry_stride, n_qry}, hash_bytes,
                        sketch_size, Counts{d_numer, d_denom, false}, stream);
}

int fpm_dist_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                 const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                 const void *d_qry, const uint32_t *d_qry_len, const uint64_t *d_qry_length,
                 uint64_t qry_stride, uint32_t n_qry, uint32_t hash_bytes, uint32_t sketch_size,
                 uint32_t kmer_size, double kmer_space, double max_dist, double max_pvalue,
                 uint32_t *d_numer, uint32_t *d_denom, double *d_dist, double *d_pvalue,
                 uint8_t *d_pass, void *stream)
{
    return dist_dev_impl(ctx, RowSet{d_ref, d_ref_len, d_ref_length, ref_stride, n_ref},
                         RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry}, hash_bytes,
                         sketch_size, DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                         full_out(d_numer, d_denom, false, d_dist, d_pvalue, d_pass), stream,
                         "fpm_dist_dev");
}

int fpm_dist_dev16(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                   const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                   const void *d_qry, const uint32_t *d_qry_len, const uint64_t *d_qry_length,
                   uint64_t qry_stride, uint32_t n_qry, uint32_t hash_bytes, uint32_t sketch_size,
                   uint32_t kmer_size, double kmer_space, double max_dist, double max_pvalue,
                   uint16_t *d_numer, uint16_t *d_denom, double *d_dist, double *d_pvalue,
                   uint8_t *d_pass, void *stream)
{
    if (sketch_size > 65535)
        return fail(FPM_EINVAL, "fpm_dist_dev16: sketch_size must be <= 65535 (u16 counts)");
    return dist_dev_impl(ctx, RowSet{d_ref, d_ref_len, d_ref_length, ref_stride, n_ref},
                         RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry}, hash_bytes,
                         sketch_size, DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                         full_out(d_numer, d_denom, true, d_dist, d_pvalue, d_pass), stream,
                         "fpm_dist_dev16");
}

int fpm_dist_list_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                      const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                      const void *d_qry, const uint32_t *d_qry_len, const uint64_t *d_qry_length,
                      uint64_t qry_stride, uint32_t n_qry, uint32_t hash_bytes,
                      uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
                      double max_dist, double max_pvalue, uint16_t *d_numer, uint16_t *d_denom,
                      const fpm_cell_list *list, void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    if (sketch_size > 65535)
        return fail(FPM_EINVAL, "fpm_dist_list_dev: sketch_size must be <= 65535 (u16 counts)");
    DistOut o;
    if (int rc = list_out(d_numer, d_denom, true, list, o, "fpm_dist_list_dev")) return rc;
    return dist_dev_impl(ctx, RowSet{d_ref, d_ref_len, d_ref_length, ref_stride, n_ref},
                         RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry}, hash_bytes,
                         sketch_size, DistParams{kmer_size, kmer_space, max_dist, max_pvalue}, o,
                         stream, "fpm_dist_list_dev");
}

int fpm_dist_list_prefill(fpm_ctx *ctx, uint16_t *d_numer, uint16_t *d_denom, uint32_t n_ref,
                          uint32_t n_qry, uint32_t sketch_size, void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    if (!d_numer || !d_denom) return fail(FPM_EINVAL, "fpm_dist_list_prefill: numer / denom buffers required");
    if (sketch_size > 65535)
        return fail(FPM_EINVAL, "fpm_dist_list_prefill: sketch_size must be <= 65535 (u16 counts)");
    hipStream_t st = pick_stream(ctx, stream);
    HIP_TRY(ensure_aux(ctx));
    // one prefill at a time: an earlier one nobody took over is waited for by `stream` first
    if (ctx->prefill.pending) HIP_TRY(hipStreamWaitEvent(st, ctx->ev_prefill, 0));
    HIP_TRY(hipEventRecord(ctx->ev_in, st));
    HIP_TRY(hipStreamWaitEvent(ctx->aux, ctx->ev_in, 0));
    {
        TimedLaunch tl(ctx, FPM_K_FILL, ctx->aux);
        HIP_TRY(launch_dist_counts_const(d_numer, d_denom, (uint64_t)n_ref * n_qry, sketch_size,
                                         ctx->aux));
        tl.done();
    }
    HIP_TRY(hipEventRecord(ctx->ev_prefill, ctx->aux));
    ctx->prefill = fpm_ctx::Prefill{d_numer, d_denom, n_ref, n_qry, sketch_size, true};
    return FPM_OK;
}

int fpm_dist_finalize_dev(fpm_ctx *ctx, const uint32_t *d_numer, const uint32_t *d_denom,
                          const uint64_t *d_ref_length, const uint64_t *d_qry_length,
                          uint32_t n_ref, uint32_t n_qry, uint32_t kmer_size,
                          double kmer_space, double max_dist, double max_pvalue,
                          double *d_dist, double *d_pvalue, uint8_t *d_pass, void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    TimedLaunch tl(ctx, FPM_K_FINALIZE, st);
    HIP_TRY(launch_dist_finalize(Counts{(void *)d_numer, (void *)d_denom, false},
                                 RowSet{nullptr, nullptr, d_ref_length, 0, n_ref},
                                 RowSet{nullptr, nullptr, d_qry_length, 0, n_qry},
                                 DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                                 CellOut{d_dist, d_pvalue, d_pass}, st));
    tl.done();
    return FPM_OK;
}

int fpm_pvalue_batch_dev(fpm_ctx *ctx, const void *d_numer, const void *d_denom,
                         uint32_t count_bytes, const uint64_t *d_len_ref,
                         const uint64_t *d_len_qry, uint64_t n, uint32_t kmer_size,
                         double kmer_space, double *d_dist, double *d_pvalue, void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    if (count_bytes != 2 && count_bytes != 4) return fail(FPM_EINVAL, "count_bytes must be 2 or 4");
    if (n && (!d_numer || !d_denom || !d_len_ref || !d_len_qry))
        return fail(FPM_EINVAL, "null input");
    hipStream_t st = pick_stream(ctx, stream);
    TimedLaunch tl(ctx, FPM_K_FINALIZE, st);
    HIP_TRY(launch_pvalue_batch(Counts{(void *)d_numer, (void *)d_denom, count_bytes == 2},
                                d_len_ref, d_len_qry, n, DistParams{kmer_size, kmer_space}, d_dist,
                                d_pvalue, st));
    tl.done();
    return FPM_OK;
}

int fpm_dist(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len, const uint64_t *ref_length,
             uint64_t ref_stride, uint32_t n_ref, const void *qry, const uint32_t *qry_len,
             const uint64_t *qry_length, uint64_t qry_stride, uint32_t n_qry,
             uint32_t hash_bytes, uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
             double max_dist, double max_pvalue, uint32_t *out_numer, uint32_t *out_denom,
             double *out_dist, double *out_pvalue, uint8_t *out_pass)
{
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    const uint64_t np = (uint64_t)n_ref * n_qry;
    if (np == 0) return FPM_OK;
    const bool fin = out_dist || out_pvalue || out_pass;
    if (fin && (!ref_length || !qry_length)) return fail(FPM_EINVAL, "lengths required for distance");
    GridStage g{ctx};
    // one set against itself (dist X.msh X.msh): upload once; the grid call then sees
    // identical device inputs and may use the pair symmetry
    const bool same = ref == qry && ref_len == qry_len && ref_stride == qry_stride &&
                      n_ref == n_qry;
    g.up(g.r, ref, (size_t)n_ref * ref_stride * hash_bytes);
    g.up(g.rl, ref_len, (size_t)n_ref * 4);
    if (!same) {
        g.up(g.q, qry, (size_t)n_qry * qry_stride * hash_bytes);
        g.up(g.ql, qry_len, (size_t)n_qry * 4);
    }
    if (fin) {
        g.up(g.rL, ref_length, (size_t)n_ref * 8);
        g.up(g.qL, qry_length, (size_t)n_qry * 8);
    }
    g.results(np, fin);
    if (g.e != hipSuccess) return fail(FPM_ENOMEM, std::string("dist staging: ") + hipGetErrorString(g.e));
    const RowSet R{g.r, g.rl, g.rL, ref_stride, n_ref};
    const RowSet Q{same ? g.r : g.q, same ? g.rl : g.ql, g.qL, qry_stride, n_qry};
    const Counts cnt{g.nu, g.de, false};
    int rc = fin ? dist_dev_impl(ctx, R, Q, hash_bytes, sketch_size,
                                 DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                                 full_out(cnt.numer, cnt.denom, false, g.di, g.pv, g.pa),
                                 nullptr, "fpm_dist_dev")
                 : compare_impl(ctx, R, Q, hash_bytes, sketch_size, cnt, nullptr);
    if (rc) return rc;
    return g.fetch(np, out_numer, out_denom, out_dist, out_pvalue, out_pass);
}

int fpm_compare_grid(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len,
                     uint64_t ref_stride, uint32_t n_ref, const void *qry,
                     const uint32_t *qry_len, uint64_t qry_stride, uint32_t n_qry,
                     uint32_t hash_bytes, uint32_t sketch_size, uint32_t *out_numer,
                     uint32_t *out_denom)
{
    return fpm_dist(ctx, ref, ref_len, nullptr, ref_stride, n_ref, qry, qry_len, nullptr,
                    qry_stride, n_qry, hash_bytes, sketch_size, 0, 0.0, -1.0, -1.0, out_numer,
                    out_denom, nullptr, nullptr, nullptr);
}

int fpm_fp_positional_grid(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len,
                           uint64_t ref_stride, uint32_t n_ref, const void *qry,
                           const uint32_t *qry_len, uint64_t qry_stride, uint32_t n_qry,
                           uint32_t hash_bytes, double max_dist, double max_pvalue,
                           uint32_t *out_numer, uint32_t *out_denom, double *out_dist,
                           double *out_pvalue, uint8_t *out_pass)
{
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    if (n_qry > 65535) return fail(FPM_EINVAL, "positional grid: at most 65535 queries per call");
    const uint64_t np = (uint64_t)n_ref * n_qry;
    if (np == 0) return FPM_OK;
    GridStage g{ctx};
    g.up(g.r, ref, (size_t)n_ref * ref_stride * hash_bytes);
    g.up(g.rl, ref_len, (size_t)n_ref * 4);
    g.up(g.q, qry, (size_t)n_qry * qry_stride * hash_bytes);
    g.up(g.ql, qry_len, (size_t)n_qry * 4);
    g.results(np, true);
    if (g.e != hipSuccess) return fail(FPM_ENOMEM, std::string("positional staging: ") + hipGetErrorString(g.e));
    HIP_TRY(launch_positional_grid(RowSet{g.r, g.rl, nullptr, ref_stride, n_ref},
                                   RowSet{g.q, g.ql, nullptr, qry_stride, n_qry}, hash_bytes,
                                   max_dist, max_pvalue, g.nu, g.de, CellOut{g.di, g.pv, g.pa},
                                   ctx->stream));
    return g.fetch(np, out_numer, out_denom, out_dist, out_pvalue, out_pass);
}

// ---- resident reference set ----------------------------------------------------------

int fpm_refset_create_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                          const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                          uint32_t hash_bytes, uint32_t sketch_size, fpm_refset **out)
{
    if (!out) return fail(FPM_EINVAL, "refset_create: null output");
    *out = nullptr;
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    std::unique_ptr<fpm_refset, void (*)(fpm_refset *)> rs(new fpm_refset, fpm_refset_free);
    rs->ctx = rs->mem.ctx = ctx;
    rs->ref = RowSet{d_ref, d_ref_len, d_ref_length, ref_stride, n_ref};
    rs->hash_bytes = hash_bytes;
    rs->sketch_size = sketch_size;
    if (int rc = refset_build_index(rs.get(), ctx->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *out = rs.release();
    return FPM_OK;
}

int fpm_refset_create(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len,
                      const uint64_t *ref_length, uint64_t ref_stride, uint32_t n_ref,
                      uint32_t hash_bytes, uint32_t sketch_size, fpm_refset **out)
{
    if (!out) return fail(FPM_EINVAL, "refset_create: null output");
    *out = nullptr;
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    // device copies of the rows, which the set then owns
    DevBufs own(ctx);
    void *rows;
    uint32_t *len;
    uint64_t *length;
    HIP_TRY(own.get(&rows, std::max<size_t>(16, (size_t)n_ref * ref_stride * hash_bytes)));
    HIP_TRY(own.get(&len, std::max<size_t>(16, (size_t)n_ref * 4)));
    HIP_TRY(own.get(&length, std::max<size_t>(16, (size_t)n_ref * 8)));
    HIP_TRY(copy_in(ctx, rows, ref, (size_t)n_ref * ref_stride * hash_bytes));
    HIP_TRY(copy_in(ctx, len, ref_len, (size_t)n_ref * 4));
    if (ref_length) HIP_TRY(copy_in(ctx, length, ref_length, (size_t)n_ref * 8));
    if (int rc = fpm_refset_create_dev(ctx, rows, len, length, ref_stride, n_ref, hash_bytes,
                                       sketch_size, out))
        return rc;
    (*out)->mem.absorb(std::move(own));
    return FPM_OK;
}

int fpm_refset_dist_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                        const uint64_t *d_qry_length, uint64_t qry_stride, uint32_t n_qry,
                        uint32_t sketch_size, uint32_t count_bytes, uint32_t kmer_size,
                        double kmer_space, double max_dist, double max_pvalue, void *d_numer,
                        void *d_denom, double *d_dist, double *d_pvalue, uint8_t *d_pass,
                        void *stream)
{
    if (int rc = refset_check(rs, sketch_size, count_bytes, "fpm_refset_dist_dev")) return rc;
    return dist_dev_impl(rs->ctx, rs->ref, RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry},
                         rs->hash_bytes, sketch_size,
                         DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                         full_out(d_numer, d_denom, count_bytes == 2, d_dist, d_pvalue, d_pass),
                         stream, "fpm_refset_dist_dev", rs);
}

int fpm_refset_dist_list_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                             const uint64_t *d_qry_length, uint64_t qry_stride, uint32_t n_qry,
                             uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
                             double max_dist, double max_pvalue, uint16_t *d_numer,
                             uint16_t *d_denom, const fpm_cell_list *list, void *stream)
{
    return refset_list_impl(rs, RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry},
                            sketch_size, DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                            2, d_numer, d_denom, list, stream, "fpm_refset_dist_list_dev");
}

int fpm_refset_dist_mirror_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                               const uint64_t *d_qry_length, uint64_t qry_stride, uint32_t n_qry,
                               uint32_t sketch_size, uint32_t count_bytes, uint32_t kmer_size,
                               double kmer_space, double max_dist, double max_pvalue,
                               void *d_numer, void *d_denom, double *d_dist, double *d_pvalue,
                               uint8_t *d_pass, void *m_numer, void *m_denom, double *m_dist,
                               double *m_pvalue, uint8_t *m_pass, void *stream)
{
    const char *who = "fpm_refset_dist_mirror_dev";
    if (int rc = refset_check(rs, sketch_size, count_bytes, who)) return rc;
    if (!m_numer || !m_denom || !m_dist || !m_pvalue)
        return fail(FPM_EINVAL, "refset_dist_mirror: mirror numer / denom / distance / p-value required");
    if (int rc = mirror_check(rs, d_qry, who)) return rc;
    const DistOut mir = full_out(m_numer, m_denom, count_bytes == 2, m_dist, m_pvalue, m_pass);
    return dist_dev_impl(rs->ctx, rs->ref, RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry},
                         rs->hash_bytes, sketch_size,
                         DistParams{kmer_size, kmer_space, max_dist, max_pvalue},
                         full_out(d_numer, d_denom, count_bytes == 2, d_dist, d_pvalue, d_pass),
                         stream, who, rs, &mir);
}

int fpm_refset_dist_mirror_list_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                                    const uint64_t *d_qry_length, uint64_t qry_stride,
                                    uint32_t n_qry, uint32_t sketch_size, uint32_t kmer_size,
                                    double kmer_space, double max_dist, double max_pvalue,
                                    uint16_t *d_numer, uint16_t *d_denom,
                                    const fpm_cell_list *list, uint16_t *m_numer,
                                    uint16_t *m_denom, const fpm_cell_list *m_list, void *stream)
{
    const char *who = "fpm_refset_dist_mirror_list_dev";
    if (int rc = refset_check(rs, sketch_size, 2, who)) return rc;
    if (int rc = mirror_check(rs, d_qry, who)) return rc;
    DistOut o, m;
    if (int rc = list_out(d_numer, d_denom, true, list, o, who)) return rc;
    if (int rc = list_out(m_numer, m_denom, true, m_list, m, who)) return rc;
    if (!m_numer || !m_denom) return fail(FPM_EINVAL, std::string(who) + ": mirror numer / denom required");
    return dist_dev_impl(rs->ctx, rs->ref, RowSet{d_qry, d_qry_len, d_qry_length, qry_stride, n_qry},
                         rs->hash_bytes, sketch_size,
                         DistParams{kmer_size, kmer_space, max_dist, max_pvalue}, o, stream, who,
                         rs, &m);
}

int fpm_refset_reindex(fpm_refset *rs, void *stream)
{
    if (!rs) return fail(FPM_EINVAL, "refset_reindex: null set");
    if (int rc = set_device(rs->ctx)) return rc;
    return refset_build_index(rs, pick_stream(rs->ctx, stream));
}

int fpm_refset_dist(fpm_refset *rs, const void *qry, const uint32_t *qry_len,
                    const uint64_t *qry_length, uint64_t qry_stride, uint32_t n_qry,
                    uint32_t sketch_size, uint32_t kmer_size, double kmer_space, double max_dist,
                    double max_pvalue, uint32_t *out_numer, uint32_t *out_denom, double *out_dist,
                    double *out_pvalue, uint8_t *out_pass)
{
    if (!rs) return fail(FPM_EINVAL, "refset_dist: null set");
    fpm_ctx *ctx = rs->ctx;
    if (int rc = set_device(ctx)) return rc;
    const uint64_t np = (uint64_t)rs->ref.n * n_qry;
    if (np == 0) return FPM_OK;
    hipStream_t st = ctx->stream;
    RowSet Q;
    void *o[5];   // numer, denom, distance, p-value, pass
    const size_t ob[5] = {np * 4, np * 4, np * 8, np * 8, np};
    if (int rc = refset_stage_query(rs, RowSet{qry, qry_len, qry_length, qry_stride, n_qry}, Q, 5,
                                    ob, o))
        return rc;
    if (int rc = fpm_refset_dist_dev(rs, Q.rows, Q.len, Q.length, qry_stride, n_qry, sketch_size,
                                     4, kmer_size, kmer_space, max_dist, max_pvalue, o[0], o[1],
                                     (double *)o[2], (double *)o[3], (uint8_t *)o[4], st))
        return rc;
    // results: caller memory (pinned from fpm_host_alloc copies at full PCIe rate, pageable
    // memory through the context's pinned ring)
    HIP_TRY(hipStreamSynchronize(st));
    void *const dst[5] = {out_numer, out_denom, out_dist, out_pvalue, out_pass};
    for (int i = 0; i < 5; i++)
        if (dst[i]) HIP_TRY(copy_out(ctx, dst[i], o[i], ob[i]));
    return FPM_OK;
}

int fpm_refset_dist_list(fpm_refset *rs, const void *qry, const uint32_t *qry_len,
                         const uint64_t *qry_length, uint64_t qry_stride, uint32_t n_qry,
                         uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
                         double max_dist, double max_pvalue, uint32_t count_bytes,
                         void *out_numer, void *out_denom, uint32_t *l_qry, uint32_t *l_ref,
                         double *l_dist, double *l_pvalue, uint8_t *l_pass, uint64_t cap,
                         uint64_t *n_listed)
{
    if (!rs) return fail(FPM_EINVAL, "refset_dist_list: null set");
    if (count_bytes != 2 && count_bytes != 4) return fail(FPM_EINVAL, "count_bytes must be 2 or 4");
    if (!n_listed) return fail(FPM_EINVAL, "refset_dist_list: null n_listed");
    *n_listed = 0;
    fpm_ctx *ctx = rs->ctx;
    if (int rc = set_device(ctx)) return rc;
    const uint64_t np = (uint64_t)rs->ref.n * n_qry;
    if (np == 0) return FPM_OK;
    hipStream_t st = ctx->stream;
    RowSet Q;
    void *o[2];   // numer, denom
    const size_t ob[2] = {np * count_bytes, np * count_bytes};
    if (int rc = refset_stage_query(rs, RowSet{qry, qry_len, qry_length, qry_stride, n_qry}, Q, 2,
                                    ob, o))
        return rc;
    const DistParams par{kmer_size, kmer_space, max_dist, max_pvalue};
    // the device list: grown (and the call repeated) when the cells sharing hashes outnumber it
    uint64_t want = std::max<uint64_t>(rs->list_cap, std::max<uint64_t>(4096, np / 32));
    for (;;) {
        void *p[6];
        const size_t eb[6] = {4, 4, 8, 8, 1, 0};
        for (int i = 0; i < 5; i++)
            HIP_TRY(grow_slot(rs->ctx, rs->qslot[fpm_refset::kQList + i], want * eb[i], &p[i]));
        HIP_TRY(grow_slot(rs->ctx, rs->qslot[fpm_refset::kQList + 5], 8, &p[5]));
        rs->list_cap = want;
        const fpm_cell_list L{(uint32_t *)p[0], (uint32_t *)p[1], (double *)p[2], (double *)p[3],
                              (uint8_t *)p[4], want, (uint64_t *)p[5]};
        if (int rc = refset_list_impl(rs, Q, sketch_size, par, count_bytes, o[0], o[1], &L, st,
                                      "fpm_refset_dist_list"))
            return rc;
        uint64_t cnt = 0;
        HIP_TRY(hipMemcpyAsync(&cnt, L.count, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (cnt > want) {
            want = cnt + cnt / 8;
            continue;
        }
        *n_listed = cnt;
        const uint64_t m = std::min<uint64_t>(cnt, cap);
        if (out_numer) HIP_TRY(copy_out(ctx, out_numer, o[0], ob[0]));
        if (out_denom) HIP_TRY(copy_out(ctx, out_denom, o[1], ob[1]));
        if (m) {
            if (l_qry) HIP_TRY(copy_out(ctx, l_qry, L.qry, m * 4));
            if (l_ref) HIP_TRY(copy_out(ctx, l_ref, L.ref, m * 4));
            if (l_dist) HIP_TRY(copy_out(ctx, l_dist, L.dist, m * 8));
            if (l_pvalue) HIP_TRY(copy_out(ctx, l_pvalue, L.pvalue, m * 8));
            if (l_pass) HIP_TRY(copy_out(ctx, l_pass, L.pass, m));
        }
        return FPM_OK;
    }
}

void fpm_refset_free(fpm_refset *rs)
{
    if (!rs) return;
    if (rs->ctx) (void)hipSetDevice(rs->ctx->device);
    delete rs;
}

}  // extern "C"

