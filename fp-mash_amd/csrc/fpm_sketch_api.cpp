// fpm_sketch_api.cpp — the sketch part of the C ABI declared in include/fpmash.h: host-side
// staging (record packing, tile plan, merge schedule), the run and its redo / fallback
// passes, the device min-merge and the -M pass, over the kernels in sketch.hip.
#include "fpm_internal.hpp"

#include <array>
#include <cmath>
#include <cstdlib>

namespace {

// Reference complement table for 'A'..'Z' (Sketch.cpp:1223-1250); other bytes 'N'.
const char kComplAZ[26] = {'T', 'V', 'G', 'H', 'N', 'N', 'C', 'D', 'N', 'N', 'M', 'N', 'K',
                           'N', 'N', 'N', 'N', 'Y', 'S', 'A', 'A', 'B', 'W', 'N', 'R', 'N'};

// Tile sizing: small records are packed up to kPackKmers k-mer starts per tile,
// long records are cut into kChunkKmers-start chunks (k-1 bytes of halo).
constexpr uint32_t kPackKmers = 2048;
// (2048-start chunks: the tile kernel 1.3 ms faster on C5, the group selection 1.3 ms slower)
constexpr uint32_t kChunkKmers = 4096;

int tile_class(uint32_t nstarts)
{
    for (int c = 0; c < kTileClasses; c++)
        if (nstarts <= kTileCap[c]) return c;
    return -1;
}

}  // namespace

// merge rounds whose estimated input lists are at most merge_small_cap() long use
// merge_small_kernel; FPM_MERGE_SMALL=0 turns it off (A/B), =2 uses it for every round
// (tests: its global-memory search past the LDS cap)
static const int g_merge_small_env = [] {
    const char *v = getenv("FPM_MERGE_SMALL");
    return v ? atoi(v) : 1;
}();

// ----------------------------------------------------------------------------
// Sketch job: packing + tile plan + merge schedule
// ----------------------------------------------------------------------------
// Rows of one device matrix d_rows[n_rows][s]: rows [0, n_groups) are the final
// sketches, rows >= n_groups hold per-tile / intermediate lists of groups whose
// records span several tiles; those are reduced by pairwise merge rounds.

struct fpm_sketch_job {
    fpm_ctx *ctx = nullptr;
    SketchKParams kp{};
    uint32_t n_groups = 0;
    uint32_t n_rows = 0;
    uint64_t seq_bytes = 0;
    uint64_t n_kmers = 0;
    uint64_t n_tiles = 0;
    uint8_t *d_seq = nullptr;
    TileDesc *d_tiles = nullptr;
    uint64_t *d_rows = nullptr;
    uint32_t *d_count = nullptr;
    MergeDesc *d_merge = nullptr;
    uint32_t class_begin[kTileClasses + 1] = {0};
    std::vector<uint32_t> round_begin;
    std::vector<uint8_t> round_small, sround_small;   // per round: merge_small_kernel
    // long groups: a 1-in-kSampleEvery sample of their tiles is sketched first; its s-th
    // smallest hash bounds what every tile of the group keeps
    uint32_t n_slots = 0;
    TileDesc *d_stiles = nullptr;
    MergeDesc *d_smerge = nullptr;
    uint32_t *d_srow = nullptr;
    uint64_t *d_thr = nullptr;
    uint32_t sclass_begin[kTileClasses + 1] = {0};
    std::vector<uint32_t> sround_begin;
    // sampled groups: one-workgroup selection from their bounded tile lists
    // (group_select_kernel); a pairwise merge plan of the same lists is kept as the fallback
    // for groups whose keys below the cut do not fit in LDS
    uint32_t n_sel = 0;
    SelDesc *d_sel = nullptr;
    uint32_t *d_sel_rows = nullptr, *d_sel_failed = nullptr, *h_sel_failed = nullptr;
    MergeDesc *d_fmerge = nullptr;
    std::vector<uint32_t> fround_begin;
    std::vector<uint8_t> fround_small;
    uint32_t n_ssel = 0;                      // sample selections (first n_ssel of d_sel)
    std::vector<uint32_t> ssel_begin, sel_begin;   // d_sel offsets of each level
    // fallback merge plans (rows >= n_rows live in d_fb_rows, allocated on first use)
    std::vector<std::array<uint32_t, 3>> fplan, sfplan;
    uint32_t n_fb_rows = 0;
    uint64_t *d_fb_rows = nullptr;
    uint32_t *d_fb_count = nullptr;
    MergeDesc *d_sfmerge = nullptr;
    std::vector<uint32_t> sfround_begin;
    std::vector<uint8_t> sfround_small;
    // class-4 tiles all bounded (C5's genomes): the survivors-only tile kernel, whose
    // overflowing tiles (d_redo, count d_redo_n) run again through the plain one
    bool thr4 = false;
    TileDesc *d_redo = nullptr;
    uint32_t *d_redo_n = nullptr;
    uint32_t n4 = 0;                 // class-4 tiles (the redo list's capacity)
    // tight bounds (groups with a selection): each slot's bound is the sample's kt-th smallest
    // hash instead of its s-th (d_kt), the s-th kept as d_thr_safe; a group left with fewer
    // than s hashes (sketch_short_kernel: d_short = count, then the slots) is redone with the
    // safe bound: its tiles and selections again, from the host copies below
    bool tight = false;
    uint32_t *d_kt = nullptr, *d_slot_group = nullptr, *d_short = nullptr;
    uint64_t *d_thr_safe = nullptr;
    std::vector<TileDesc> h_tiles;          // the main tiles by class (class_begin)
    std::vector<SelDesc> h_sel;             // the selections (sample levels, then main)
    TileDesc *d_rtiles = nullptr;           // the redo's subsets (allocated on first use)
    SelDesc *d_rsel = nullptr;
    int32_t last_short = -1;                // groups redone by the last run (-1: no tight bounds)
    // a-priori sample bounds (d_thr[n_slots ..]): a sample left short is redone unbounded
    bool sbounded = false;
    uint32_t *d_sshort = nullptr;           // count, then the slots
    uint64_t *d_sbound0 = nullptr;          // the a-priori sample bounds as staged: restored
                                            // into d_thr at every run (a short sample's redo
                                            // lifts its bound in d_thr)
    std::vector<TileDesc> h_stiles;         // the sample tiles by class (sclass_begin)
    std::vector<uint32_t> h_ssel_tag;       // each sample selection's slot
    int32_t last_sample_short = -1;
    // -M pass (allocated on first use)
    uint32_t *d_mult = nullptr;
    unsigned long long *d_first = nullptr;
    uint64_t *d_ttop = nullptr;
    // reads mode (fpm_sketch_job_set_min_copies, fpm_sketch_reads_run): the parameters and
    // records as staged (pos = offsets in d_seq), from which the widening rounds stage their
    // wide jobs over this job's d_seq (borrowed: such a job never adopts it); the
    // filtered rows, counts and T, allocated on first use
    fpm_sketch_params params{};
    StageRecords recs;
    uint32_t min_copies = 1;
    uint64_t *d_rrows = nullptr, *d_rttop = nullptr;
    uint32_t *d_rcount = nullptr, *d_rmult = nullptr, *d_rdone = nullptr;
    std::vector<uint32_t> h_rdone;          // per group: the round that completed it
    int32_t reads_rounds = -1;              // rounds of the last reads run (-1: none yet)
    int32_t reads_sampled = -1;             // long groups its last round's wide job sampled
    DevBufs mem;                            // owns every d_* buffer above but a borrowed d_seq
};

static void job_release(fpm_sketch_job *j)
{
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    if (j->h_sel_failed) (void)hipHostFree(j->h_sel_failed);
}

void job_view(const fpm_sketch_job *j, JobView *out)
{
    *out = JobView{j->ctx, j->kp, j->n_groups, j->d_seq, j->d_tiles, j->class_begin, j->d_rows,
                   j->d_count};
}

extern "C" {

int fpm_sketch_stage(fpm_ctx *ctx, const fpm_sketch_params *p, const char *seq,
                     const uint64_t *rec_off, uint32_t n_rec, const uint32_t *group_of_rec,
                     uint32_t n_groups, fpm_sketch_job **job_out)
{
    if (int rc = set_device(ctx)) return rc;
    if (!p || !job_out || (n_rec && (!seq || !rec_off))) return fail(FPM_EINVAL, "null argument");
    *job_out = nullptr;
    if (!group_of_rec) n_groups = n_rec;
    for (uint32_t r = 0; r < n_rec; r++)
        if (rec_off[r + 1] < rec_off[r]) return fail(FPM_EINVAL, "record offsets must be non-decreasing");
    if (group_of_rec)
        for (uint32_t r = 0; r < n_rec; r++)
            if (group_of_rec[r] >= n_groups) return fail(FPM_EINVAL, "group id out of range");
    StageRecords R;
    R.n_groups = n_groups;
    R.host_seq = seq;
    R.pos.resize(n_rec);
    R.len.resize(n_rec);
    R.group.resize(n_rec);
    R.order.resize(n_rec);
    for (uint32_t r = 0; r < n_rec; r++) {
        R.pos[r] = rec_off[r];
        R.len[r] = rec_off[r + 1] - rec_off[r];
        R.group[r] = group_of_rec ? group_of_rec[r] : r;
        R.order[r] = r;
    }
    // records of a group in stream order, groups ascending
    if (group_of_rec)
        std::stable_sort(R.order.begin(), R.order.end(),
                         [&](uint32_t a, uint32_t b) { return R.group[a] < R.group[b]; });
    return stage_core(ctx, p, R, job_out);
}

}  // extern "C"

int stage_core(fpm_ctx *ctx, const fpm_sketch_params *p, StageRecords &R,
               fpm_sketch_job **job_out)
{
    if (p->kmer_size < 1 || p->kmer_size > 32) return fail(FPM_EINVAL, "kmer_size must be 1..32");
    if (p->sketch_size < 1) return fail(FPM_EINVAL, "sketch_size must be >= 1");
    const uint32_t k = p->kmer_size, s = p->sketch_size;
    const uint32_t n_groups = R.n_groups;
    const std::vector<uint32_t> &order = R.order;
    SketchKParams kp{};
    kp.k = k; kp.s = s; kp.seed = p->seed; kp.use64 = p->use64 ? 1 : 0;
    kp.canonical = p->noncanonical ? 0 : 1; kp.preserve_case = p->preserve_case ? 1 : 0;
    for (int c = 0; c < 256; c++) {
        kp.alphabet[c] = p->alphabet[c] ? 1 : 0;
        kp.complement[c] = (c >= 'A' && c <= 'Z') ? (uint8_t)kComplAZ[c - 'A'] : (uint8_t)'N';
    }
    kp.alphabet[0] = 0;   // the separator byte is never a k-mer byte
    kp.compl_acgt = 1;
    for (int c = 0; c < 256; c++)
        if (kp.alphabet[c] && c != 'A' && c != 'C' && c != 'G' && c != 'T') kp.compl_acgt = 0;

    // host path: pack records >= k (each followed by 0x00) in group order
    std::vector<uint8_t> packed;
    if (R.host_seq) {
        uint64_t total = 0;
        for (uint32_t r : order)
            if (R.len[r] >= k) total += R.len[r] + 1;
        packed.resize(total);
        uint64_t at = 0;
        for (uint32_t r : order) {
            if (R.len[r] < k) continue;
            memcpy(packed.data() + at, R.host_seq + R.pos[r], R.len[r]);
            packed[at + R.len[r]] = 0;
            R.pos[r] = at;                      // now the packed offset
            at += R.len[r] + 1;
        }
    }
    // cut tiles: a tile covers [byte_off, byte_off + n_bytes) of the packed buffer, records of
    // one group only; short records share a tile while its k-mer starts fit (bytes between
    // them, separators or records shorter than k, hold no valid window)
    std::vector<TileDesc> tiles;
    std::vector<uint32_t> tile_group;
    uint64_t n_kmers = 0;
    uint32_t cur_group = UINT32_MAX;
    bool open = false;
    TileDesc cur{};
    auto close = [&]() {
        if (open) { tiles.push_back(cur); tile_group.push_back(cur_group); open = false; }
    };
    for (uint32_t r : order) {
        const uint64_t l = R.len[r];
        const uint32_t g = R.group[r];
        if (g != cur_group) { close(); cur_group = g; }
        if (l < k) continue;
        const uint64_t poff = R.pos[r];
        const uint64_t nk = l - k + 1;
        n_kmers += nk;
        if (nk > kPackKmers) {
            close();
            for (uint64_t c0 = 0; c0 < nk; c0 += kChunkKmers) {
                uint64_t cn = std::min<uint64_t>(kChunkKmers, nk - c0);
                tiles.push_back(TileDesc{poff + c0, (uint32_t)(cn + k - 1), 0});
                tile_group.push_back(g);
            }
        } else if (open && poff > cur.byte_off + cur.n_bytes &&
                   poff + l - cur.byte_off - k + 1 <= kPackKmers) {
            cur.n_bytes = (uint32_t)(poff + l - cur.byte_off);   // through this record
        } else {
            close();
            cur = TileDesc{poff, (uint32_t)l, 0};
            open = true;
        }
    }
    close();
    for (size_t t = 0; t < tiles.size(); t++) tiles[t].pad = tile_group[t];

    // rows: single-tile groups write their final row, others get temp rows
    std::vector<uint32_t> ntile_of(n_groups, 0);
    for (uint32_t g : tile_group) ntile_of[g]++;
    std::vector<std::vector<uint32_t>> lists(n_groups);
    uint32_t n_rows = n_groups;
    for (size_t t = 0; t < tiles.size(); t++) {
        uint32_t g = tile_group[t];
        if (ntile_of[g] == 1) tiles[t].out_row = g;
        else { tiles[t].out_row = n_rows; lists[g].push_back(n_rows); n_rows++; }
    }
    // long groups (many 4096-k-mer chunks: C5 genomes): every kSampleEvery-th tile is also
    // sketched in a sample pass (own temp rows and merge plan); the sample's s-th smallest
    // hash is >= the group's s-th smallest, so the full pass drops every hash above it and
    // its merges move ~kSampleEvery*s hashes per group instead of every tile's bottom-s.
    // The sample rate per group: every E-th tile, E = the group's k-mers / 8 s within
    // [16, 64], so a sample holds ~8 s k-mers: enough for its s-th smallest (the safe bound)
    // and a tight kt-th one.  C5's 5 Mb genomes: E = 61, C5 23.6 -> 21.9 ms against E = 16
    // (22.8 ms at 16 s k-mers, E = 31), same box, r05x / r05y.
    constexpr uint32_t kSampleEvery = 16;
    std::vector<uint32_t> every(n_groups, kSampleEvery);
    for (uint32_t g = 0; g < n_groups; g++)
        every[g] = (uint32_t)std::min<uint64_t>(
            64, std::max<uint64_t>(kSampleEvery, (uint64_t)ntile_of[g] * kChunkKmers / (8ULL * s)));
    std::vector<uint32_t> slot_of(n_groups, 0);          // 0: not sampled, else slot + 1
    std::vector<TileDesc> stiles;
    std::vector<std::vector<uint32_t>> slists(n_groups);
    std::vector<uint32_t> srow, sgroup;                  // sgroup: each sample tile's group
    {
        std::vector<uint32_t> seen(n_groups, 0);
        for (size_t t = 0; t < tiles.size(); t++) {
            const uint32_t g = tile_group[t];
            const uint64_t sample_kmers = (uint64_t)(ntile_of[g] / every[g]) * kChunkKmers;
            if (ntile_of[g] < 2 * every[g] || sample_kmers < 4ULL * s) continue;
            if (!slot_of[g]) { srow.push_back(0); slot_of[g] = (uint32_t)srow.size(); }
            if (seen[g]++ % every[g] == 0) {
                TileDesc st = tiles[t];
                st.out_row = n_rows;
                st.thr_slot = 0;
                slists[g].push_back(n_rows++);
                stiles.push_back(st);
                sgroup.push_back(g);
            }
        }
        for (size_t t = 0; t < tiles.size(); t++) tiles[t].thr_slot = slot_of[tile_group[t]];
    }
    // list-length estimate per row (steers merge_small_kernel only; results do not depend
    // on it): a tile keeps at most its k-mers and s; a tile of a sampled (thresholded) group
    // keeps ~kSampleEvery * s / tiles of the group's hashes (2x margin)
    std::vector<uint64_t> est(n_rows, s);
    for (size_t t = 0; t < tiles.size(); t++) {
        const uint32_t g = tile_group[t];
        uint64_t e = std::min<uint64_t>(s, tiles[t].n_bytes >= k ? tiles[t].n_bytes - k + 1 : 0);
        if (slot_of[g]) e = std::min<uint64_t>(e, 2ULL * every[g] * s / ntile_of[g] + 64);
        if (tiles[t].out_row < est.size()) est[tiles[t].out_row] = e;
    }
    for (auto &st : stiles)
        if (st.out_row < est.size())
            est[st.out_row] = std::min<uint64_t>(s, st.n_bytes >= k ? st.n_bytes - k + 1 : 0);
    struct Plan { uint32_t a, b, c; };
    // pairwise merge rounds of each group's lists; the last merge writes final_row(g)
    auto plan_rounds = [&](std::vector<std::vector<uint32_t>> &L_of, auto final_row,
                           std::vector<Plan> &plan, std::vector<uint32_t> &rounds,
                           std::vector<uint8_t> &small) {
        rounds.assign(1, 0);
        small.clear();
        for (;;) {
            bool any = false;
            uint64_t round_max = 0;
            for (uint32_t g = 0; g < n_groups; g++) {
                auto &L = L_of[g];
                if (L.size() < 2) continue;
                any = true;
                std::vector<uint32_t> next;
                for (size_t i = 0; i + 1 < L.size(); i += 2) {
                    uint32_t c = (L.size() == 2) ? final_row(g) : n_rows++;
                    plan.push_back({L[i], L[i + 1], c});
                    next.push_back(c);
                    if (est.size() <= c) est.resize(c + 1, s);
                    const uint64_t ea = est[L[i]], eb = est[L[i + 1]];
                    est[c] = std::min<uint64_t>(s, ea + eb);
                    round_max = std::max(round_max, std::max(ea, eb));
                }
                if (L.size() % 2) next.push_back(L.back());
                if (next.size() == 1) next.clear();   // reached the final row
                L.swap(next);
            }
            if (!any) break;
            rounds.push_back((uint32_t)plan.size());
            small.push_back(round_max <= merge_small_cap() ? 1 : 0);
        }
    };
    std::vector<Plan> splan, mplan, fplan;
    std::vector<uint32_t> srb, rb, frb;
    std::vector<uint8_t> ssmall, msmall, fsmall;
    for (uint32_t g = 0; g < n_groups; g++)
        if (slot_of[g]) srow[slot_of[g] - 1] = slists[g].size() == 1 ? slists[g][0] : 0;
    // sampled groups select their sketch (and their sample's) with group_select_kernel; their
    // lists leave the merge plans for fallback plans (pairwise merges only: C5 17.6 vs 2.6 ms).
    // A group with more keys than one workgroup should read (~2^19: a 1 Gb genome's sample
    // holds 62 M) is split into chunks of rows selected in parallel, then the chunks' sketches
    // are selected again (a tree of levels, one launch per level).
    std::vector<uint32_t> sel_rows;
    std::vector<std::vector<SelDesc>> ssel_lv, sel_lv;
    const bool use_sel = (uint64_t)s + s / 8 + 64 <= group_select_cap();
    // A sample's tiles keep only the hashes below an a-priori bound: hash values are uniform,
    // so of a sample's N windows ~frac N lie below frac of the hash range, and frac =
    // (1.25 s + 16 sqrt(s)) / N leaves >= s of them (C5: ~14k of a sample's 82k) with ~40
    // standard deviations to spare.  The sample's selection then reads ~6x fewer keys.  A
    // sample left with fewer than s (values repeated across its tiles) gives its group no
    // bound, as a sample shorter than s always did (the sketches do not depend on it).
    std::vector<uint64_t> sbound(srow.size(), ~0ULL);
    if (use_sel && !srow.empty()) {
        std::vector<uint64_t> ns(srow.size(), 0);
        for (size_t i = 0; i < stiles.size(); i++)
            ns[slot_of[sgroup[i]] - 1] += stiles[i].n_bytes >= k ? stiles[i].n_bytes - k + 1 : 0;
        const double range = kp.use64 ? 18446744073709551616.0 : 4294967296.0;
        for (size_t i = 0; i < srow.size(); i++) {
            const double frac = (1.25 * s + 16.0 * std::sqrt((double)s)) / std::max<double>(1, ns[i]);
            if (frac < 0.5) sbound[i] = (uint64_t)(frac * range);
        }
        const uint32_t n_sl = (uint32_t)srow.size();
        for (size_t i = 0; i < stiles.size(); i++) {
            const uint32_t sl = slot_of[sgroup[i]];
            if (sbound[sl - 1] != ~0ULL) {
                stiles[i].thr_slot = n_sl + sl;              // d_thr[n_slots + slot]
                if (stiles[i].out_row < est.size())
                    est[stiles[i].out_row] = std::min<uint64_t>(
                        est[stiles[i].out_row], (uint64_t)(2.0 * (double)sbound[sl - 1] / range *
                                                           stiles[i].n_bytes) + 64);
            }
        }
    }
    // tags (optional): per level, the slot of each descriptor (sample selections carry slot
    // 0xFFFFFFFF on the device; the host finds a group's descriptors by the tag)
    auto build_sel = [&](const std::vector<uint32_t> &rows0, uint32_t final_row, uint32_t slot,
                         std::vector<std::vector<SelDesc>> &lv,
                         std::vector<std::vector<uint32_t>> *tags = nullptr, uint32_t tag = 0) {
        constexpr uint64_t kKeysPerWG = 1u << 19;
        constexpr size_t kRowsPerWG = 4096;
        std::vector<uint32_t> cur = rows0;
        for (size_t level = 0;; level++) {
            if (lv.size() <= level) lv.resize(level + 1);
            if (tags && tags->size() <= level) tags->resize(level + 1);
            std::vector<std::pair<size_t, size_t>> ch;
            size_t a = 0;
            uint64_t acc = 0;
            for (size_t i = 0; i < cur.size(); i++) {
                const uint64_t e = est[cur[i]];
                if (i > a && (acc + e > kKeysPerWG || i - a >= kRowsPerWG)) {
                    ch.push_back({a, i});
                    a = i;
                    acc = 0;
                }
                acc += e;
            }
            ch.push_back({a, cur.size()});
            if (ch.size() == 1) {
                lv[level].push_back(SelDesc{(uint32_t)sel_rows.size(), (uint32_t)cur.size(),
                                            final_row, slot});
                if (tags) (*tags)[level].push_back(tag);
                sel_rows.insert(sel_rows.end(), cur.begin(), cur.end());
                return;
            }
            std::vector<uint32_t> next;
            for (auto &c : ch) {
                const uint32_t r = n_rows++;
                if (est.size() <= r) est.resize(r + 1, s);
                uint64_t sum = 0;
                for (size_t i = c.first; i < c.second; i++) sum += est[cur[i]];
                est[r] = std::min<uint64_t>(s, sum);
                lv[level].push_back(SelDesc{(uint32_t)sel_rows.size(),
                                            (uint32_t)(c.second - c.first), r, slot});
                if (tags) (*tags)[level].push_back(tag);
                sel_rows.insert(sel_rows.end(), cur.begin() + c.first, cur.begin() + c.second);
                next.push_back(r);
            }
            cur.swap(next);
        }
    };
    std::vector<Plan> sfplan;
    std::vector<uint32_t> sfrb;
    std::vector<uint8_t> sfsmall;
    std::vector<std::vector<uint32_t>> sflists(n_groups), flists(n_groups);
    std::vector<std::vector<uint32_t>> ssel_tag_lv;
    if (use_sel)
        for (uint32_t g = 0; g < n_groups; g++) {
            if (!slot_of[g] || slists[g].size() < 2) continue;
            const uint32_t r = n_rows++;                    // the sample's sketch row
            srow[slot_of[g] - 1] = r;
            build_sel(slists[g], r, 0xFFFFFFFFu, ssel_lv, &ssel_tag_lv, slot_of[g] - 1);
            sflists[g].swap(slists[g]);
        }
    plan_rounds(slists, [&](uint32_t g) {
        const uint32_t r = n_rows++;
        srow[slot_of[g] - 1] = r;
        return r;
    }, splan, srb, ssmall);
    if (use_sel)
        for (uint32_t g = 0; g < n_groups; g++) {
            if (!slot_of[g] || lists[g].size() < 2) continue;
            build_sel(lists[g], g, slot_of[g] - 1, sel_lv);
            flists[g].swap(lists[g]);
        }
    plan_rounds(lists, [](uint32_t g) { return g; }, mplan, rb, msmall);
    // d_sel: the sample levels, then the main levels; level boundaries for the launches
    std::vector<SelDesc> sel;
    std::vector<uint32_t> ssel_begin{0}, sel_begin, ssel_tag;
    for (auto &l : ssel_lv) {
        sel.insert(sel.end(), l.begin(), l.end());
        ssel_begin.push_back((uint32_t)sel.size());
    }
    for (auto &l : ssel_tag_lv) ssel_tag.insert(ssel_tag.end(), l.begin(), l.end());
    sel_begin.push_back((uint32_t)sel.size());
    for (auto &l : sel_lv) {
        sel.insert(sel.end(), l.begin(), l.end());
        sel_begin.push_back((uint32_t)sel.size());
    }
    // the fallback plans' intermediate rows come last: they are allocated only if a selection
    // fails (a C5 share holds ~1.2 M tile rows of s u64: the fallback rows would double that)
    const uint32_t n_core = n_rows;
    if (use_sel) {
        plan_rounds(sflists, [&](uint32_t g) { return srow[slot_of[g] - 1]; }, sfplan, sfrb,
                    sfsmall);
        plan_rounds(flists, [](uint32_t g) { return g; }, fplan, frb, fsmall);
    }

    // tiles ordered by capacity class
    auto order_by_class = [&](const std::vector<TileDesc> &in, std::vector<TileDesc> &out,
                              uint32_t *begin) {
        out.clear();
        out.reserve(in.size());
        begin[0] = 0;
        for (int c = 0; c < kTileClasses; c++) {
            for (auto &t : in)
                if (tile_class(t.n_bytes - k + 1) == c) out.push_back(t);
            begin[c + 1] = (uint32_t)out.size();
        }
        return out.size() == in.size();
    };
    std::vector<TileDesc> by_class, sby_class;
    uint32_t class_begin[kTileClasses + 1] = {0}, sclass_begin[kTileClasses + 1] = {0};
    if (!order_by_class(tiles, by_class, class_begin) ||
        !order_by_class(stiles, sby_class, sclass_begin))
        return fail(FPM_EINVAL, "internal: tile exceeds capacity");

    auto *job = new fpm_sketch_job();
    job->ctx = ctx;
    job->kp = kp;
    job->n_groups = n_groups;
    job->n_rows = n_core;
    job->n_fb_rows = n_rows - n_core;
    for (auto &pl : fplan) job->fplan.push_back({pl.a, pl.b, pl.c});
    for (auto &pl : sfplan) job->sfplan.push_back({pl.a, pl.b, pl.c});
    job->seq_bytes = R.host_seq ? packed.size() : R.d_seq_bytes;
    job->n_kmers = n_kmers;
    job->n_tiles = tiles.size();
    memcpy(job->class_begin, class_begin, sizeof(class_begin));
    memcpy(job->sclass_begin, sclass_begin, sizeof(sclass_begin));
    job->round_begin = rb;
    job->sround_begin = srb;
    job->round_small = msmall;
    job->sround_small = ssmall;
    job->n_slots = (uint32_t)srow.size();
    job->ssel_begin = ssel_begin;
    job->sel_begin = sel_begin;
    job->n_ssel = ssel_begin.back();
    job->n_sel = sel_begin.back() - sel_begin.front();
    job->sfround_begin = sfrb;
    job->sfround_small = sfsmall;
    job->fround_begin = frb;
    job->fround_small = fsmall;

    hipError_t e = hipSuccess;
    auto alloc = [&](auto **ptr, size_t bytes) {
        if (e == hipSuccess) e = job->mem.get(ptr, bytes);
    };
    if (R.host_seq) alloc(&job->d_seq, packed.size() + 64);
    else job->d_seq = R.d_seq;   // the parse's packed records, or borrowed (adopted below)
    alloc(&job->d_tiles, by_class.size() * sizeof(TileDesc));
    alloc(&job->d_rows, (size_t)n_core * s * sizeof(uint64_t));
    alloc(&job->d_count, (size_t)n_core * sizeof(uint32_t));
    // groups without any k-mer keep count 0: zeroed once here (every run rewrites the count
    // of each group that has tiles: the tile kernel or the last merge of its group)
    if (e == hipSuccess) e = memset_sync(ctx, job->d_count, 0, (size_t)n_core * sizeof(uint32_t));
    alloc(&job->d_merge, mplan.size() * sizeof(MergeDesc));
    alloc(&job->d_stiles, sby_class.size() * sizeof(TileDesc));
    alloc(&job->d_smerge, splan.size() * sizeof(MergeDesc));
    alloc(&job->d_srow, srow.size() * sizeof(uint32_t));
    alloc(&job->d_thr, 2 * srow.size() * sizeof(uint64_t));   // main, then sample bounds
    alloc(&job->d_sel, sel.size() * sizeof(SelDesc));
    alloc(&job->d_sel_rows, sel_rows.size() * sizeof(uint32_t));
    alloc(&job->d_sel_failed, (sel.size() + 2) * sizeof(uint32_t));
    if (e == hipSuccess && !sel.empty())
        e = hipHostMalloc((void **)&job->h_sel_failed, 3 * sizeof(uint32_t), hipHostMallocDefault);
    // tight bounds where every sampled group has a selection: kt = f s + 8 sqrt(f s) + 32 of
    // the sample's hashes (f = the group's sampled share of tiles), so ~kt / f >= s of the
    // group's distinct hashes lie below it with ~8 standard deviations to spare (C5 at E = 61:
    // ~300 of the sample's 10,000; the group keeps ~18k hashes instead of ~160k)
    std::vector<uint32_t> kt, slot_group;
    if (use_sel && !srow.empty() && !sel.empty()) {
        kt.assign(srow.size(), s);
        slot_group.assign(srow.size(), 0);
        for (uint32_t g = 0; g < n_groups; g++) {
            if (!slot_of[g]) continue;
            const uint32_t i = slot_of[g] - 1;
            slot_group[i] = g;
            const double f = (double)((ntile_of[g] + every[g] - 1) / every[g]) / ntile_of[g];
            const double fs = f * s;
            kt[i] = (uint32_t)std::min<double>(s, std::ceil(fs + 8.0 * std::sqrt(fs) + 32.0));
        }
        job->tight = true;
        alloc(&job->d_kt, kt.size() * sizeof(uint32_t));
        alloc(&job->d_slot_group, slot_group.size() * sizeof(uint32_t));
        alloc(&job->d_short, (srow.size() + 1) * sizeof(uint32_t));
        alloc(&job->d_thr_safe, srow.size() * sizeof(uint64_t));
        job->h_tiles = by_class;
        job->h_sel = sel;
        job->last_short = 0;
        bool any_sb = false;
        for (uint64_t b : sbound) any_sb = any_sb || b != ~0ULL;
        if (any_sb) {
            job->sbounded = true;
            job->h_stiles = sby_class;
            job->h_ssel_tag = ssel_tag;
            job->last_sample_short = 0;
            alloc(&job->d_sshort, (srow.size() + 1) * sizeof(uint32_t));
            alloc(&job->d_sbound0, srow.size() * sizeof(uint64_t));
        }
    }
    {
        // the survivors-only tile kernel for the class-4 tiles when every one carries its
        // group's bound and that bound leaves few survivors per tile: a group's main pass keeps
        // about kSampleEvery * s of its hashes (the sample's s-th smallest bounds them), so a
        // tile keeps ~kSampleEvery * s / (the group's tiles); est (2x margin + 64, above) must
        // stay within half of what one tile holds, or most tiles would be hashed twice (their
        // survivors overflow and the plain kernel redoes them).  (C5 one GPU: 31.2 -> 25.8 ms,
        // same box, r04; C5 tiles: est 326 of 1,024)
        const uint32_t b4 = class_begin[4], n4 = class_begin[5] - b4;
        // (tight bounds: ~kt / f survivors per group; a short group's redo under the safe bound
        // keeps ~E s per group, and its tiles that overflow are redone by the plain kernel)
        std::vector<uint64_t> slot_est(srow.size() + 1, ~0ULL);
        for (uint32_t g = 0; g < n_groups; g++) {
            if (!slot_of[g]) continue;
            const double f = (double)((ntile_of[g] + every[g] - 1) / every[g]) / ntile_of[g];
            slot_est[slot_of[g]] = job->tight
                                       ? (uint64_t)(2.0 * kt[slot_of[g] - 1] / f / ntile_of[g]) + 64
                                       : 2ULL * every[g] * s / ntile_of[g] + 64;
        }
        bool all = n4 > 0;
        for (uint32_t i = 0; all && i < n4; i++) {
            const uint32_t sl = by_class[b4 + i].thr_slot;
            all = sl != 0 && slot_est[sl] <= kThrTileKeys / 2;
        }
        job->thr4 = all;
        job->n4 = n4;
        if (all) {
            alloc(&job->d_redo, (size_t)n4 * sizeof(TileDesc));
            alloc(&job->d_redo_n, sizeof(uint32_t));
        }
    }
    if (e != hipSuccess) {
        job_release(job);
        delete job;
        return fail(FPM_ENOMEM, std::string("sketch staging alloc: ") + hipGetErrorString(e));
    }
    auto descs = [&](const std::vector<Plan> &plan) {
        std::vector<MergeDesc> md(plan.size());
        for (size_t i = 0; i < plan.size(); i++) {
            md[i].a = job->d_rows + (uint64_t)plan[i].a * s;
            md[i].alen = job->d_count + plan[i].a;
            md[i].b = job->d_rows + (uint64_t)plan[i].b * s;
            md[i].blen = job->d_count + plan[i].b;
            md[i].c = job->d_rows + (uint64_t)plan[i].c * s;
            md[i].clen = job->d_count + plan[i].c;
        }
        return md;
    };
    const std::vector<MergeDesc> md = descs(mplan), smd = descs(splan);
    if (!packed.empty()) e = h2d_staged(ctx, job->d_seq, packed.data(), packed.size());
    auto put = [&](void *dst, const auto &v) {      // (an empty vector copies nothing)
        if (e == hipSuccess) e = copy_in(ctx, dst, v.data(), v.size() * sizeof(v[0]));
    };
    put(job->d_tiles, by_class);
    put(job->d_merge, md);
    put(job->d_stiles, sby_class);
    put(job->d_smerge, smd);
    put(job->d_srow, srow);
    put(job->d_sel, sel);
    put(job->d_sel_rows, sel_rows);
    put(job->d_thr + srow.size(), sbound);
    if (job->d_sbound0) put(job->d_sbound0, sbound);
    put(job->d_kt, kt);
    put(job->d_slot_group, slot_group);
    if (e != hipSuccess) {
        job_release(job);
        delete job;
        return fail(FPM_EHIP, std::string("sketch staging copy: ") + hipGetErrorString(e));
    }
    if (!R.host_seq && !R.borrow) job->mem.adopt(R.d_seq);
    // kept for reads mode's widening rounds (moved, not copied: the callers are done with them)
    job->params = *p;
    job->recs.n_groups = n_groups;
    job->recs.order = std::move(R.order);
    job->recs.pos = std::move(R.pos);
    job->recs.len = std::move(R.len);
    job->recs.group = std::move(R.group);
    *job_out = job;
    return FPM_OK;
}

// the fallback merge plans' descriptors (first failure of a selection): intermediate rows in
// a buffer of their own
static int fallback_descs(fpm_sketch_job *job)
{
    if (job->d_fmerge || job->d_sfmerge) return FPM_OK;
    const uint64_t s = job->kp.s;
    if (job->n_fb_rows) {
        HIP_TRY(job->mem.get(&job->d_fb_rows, (size_t)job->n_fb_rows * s * sizeof(uint64_t)));
        HIP_TRY(job->mem.get(&job->d_fb_count, (size_t)job->n_fb_rows * sizeof(uint32_t)));
    }
    auto row = [&](uint32_t r) { return r < job->n_rows ? job->d_rows + r * s
                                                       : job->d_fb_rows + (r - job->n_rows) * s; };
    auto cnt = [&](uint32_t r) { return r < job->n_rows ? job->d_count + r
                                                       : job->d_fb_count + (r - job->n_rows); };
    auto upload = [&](const std::vector<std::array<uint32_t, 3>> &plan, MergeDesc **dst) -> int {
        std::vector<MergeDesc> md(plan.size());
        for (size_t i = 0; i < plan.size(); i++)
            md[i] = MergeDesc{row(plan[i][0]), cnt(plan[i][0]), row(plan[i][1]), cnt(plan[i][1]),
                              row(plan[i][2]), cnt(plan[i][2])};
        HIP_TRY(job->mem.upload(job->ctx, dst, md.data(), md.size() * sizeof(MergeDesc)));
        return FPM_OK;
    };
    if (int rc = upload(job->fplan, &job->d_fmerge)) return rc;
    return upload(job->sfplan, &job->d_sfmerge);
}

// device room for a redo's tile and selection subsets (allocated on first use)
static int redo_buffers(fpm_sketch_job *job)
{
    if (!job->d_rtiles)
        HIP_TRY(job->mem.get(&job->d_rtiles,
                             std::max(job->h_tiles.size(), job->h_stiles.size()) * sizeof(TileDesc)));
    if (!job->d_rsel) HIP_TRY(job->mem.get(&job->d_rsel, job->h_sel.size() * sizeof(SelDesc)));
    return FPM_OK;
}

// one group_select launch per level of d_sel[begin[l] .. begin[l + 1])
static int select_levels(fpm_sketch_job *job, const SelDesc *d_sel,
                         const std::vector<uint32_t> &begin, uint32_t *d_failed, hipStream_t st)
{
    for (size_t l = 0; l + 1 < begin.size(); l++) {
        const uint32_t b = begin[l], n = begin[l + 1] - b;
        if (!n) continue;
        TimedLaunch tl(job->ctx, FPM_K_MERGE, st);
        HIP_TRY(launch_group_select(d_sel + b, n, job->d_sel_rows, job->d_rows, job->d_count,
                                    job->kp.s, job->d_thr, d_failed, st));
        tl.done();
    }
    return FPM_OK;
}

// The groups a bound left short, their tiles and selections once more.  Main pass: the tight
// bound (slots in d_short[1 ..], bounds already raised to the safe ones by
// sketch_short_kernel).  Sample pass: the a-priori bound (slots in d_sshort[1 ..], bounds
// lifted by sketch_sample_short_kernel), the sample tiles and sample selections.
template <typename TilesPass>
static int redo_short(fpm_sketch_job *job, bool sample, uint32_t n_short, hipStream_t st,
                      TilesPass &tiles_pass)
{
    fpm_ctx *ctx = job->ctx;
    std::vector<uint32_t> slots(n_short);
    HIP_TRY(hipMemcpyAsync(slots.data(), (sample ? job->d_sshort : job->d_short) + 1,
                           n_short * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint8_t> is_short(job->n_slots + 1, 0);
    for (uint32_t i : slots)
        if (i < job->n_slots) is_short[i] = 1;
    // a main tile carries slot + 1 (0: none), a bounded sample tile n_slots + slot + 1
    const uint32_t *cb = sample ? job->sclass_begin : job->class_begin;
    const std::vector<TileDesc> &tiles = sample ? job->h_stiles : job->h_tiles;
    const uint32_t base = sample ? job->n_slots : 0;
    std::vector<TileDesc> sub;
    uint32_t begin[kTileClasses + 1] = {0};
    for (int c = 0; c < kTileClasses; c++) {
        for (uint32_t t = cb[c]; t < cb[c + 1]; t++) {
            const TileDesc &td = tiles[t];
            if (td.thr_slot > base && is_short[td.thr_slot - base - 1]) sub.push_back(td);
        }
        begin[c + 1] = (uint32_t)sub.size();
    }
    // a main selection carries its slot, a sample selection's slot is its host-side tag
    const std::vector<uint32_t> &lv = sample ? job->ssel_begin : job->sel_begin;
    std::vector<SelDesc> rsel;
    std::vector<uint32_t> rbegin{0};
    for (size_t l = 0; l + 1 < lv.size(); l++) {
        for (uint32_t i = lv[l]; i < lv[l + 1]; i++) {
            const uint32_t slot = !sample ? job->h_sel[i].slot
                                  : i < job->h_ssel_tag.size() ? job->h_ssel_tag[i] : UINT32_MAX;
            if (slot < job->n_slots && is_short[slot]) rsel.push_back(job->h_sel[i]);
        }
        rbegin.push_back((uint32_t)rsel.size());
    }
    if (int rc = redo_buffers(job)) return rc;
    if (!sub.empty()) HIP_TRY(copy_in(ctx, job->d_rtiles, sub.data(), sub.size() * sizeof(TileDesc)));
    if (!rsel.empty()) HIP_TRY(copy_in(ctx, job->d_rsel, rsel.data(), rsel.size() * sizeof(SelDesc)));
    if (int rc = tiles_pass(job->d_rtiles, begin, !sample)) return rc;
    return select_levels(job, job->d_rsel, rbegin, job->d_sel_failed + (sample ? 1 : 0), st);
}

extern "C" {

int fpm_sketch_run(fpm_sketch_job *job, void *stream)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    auto tiles_pass = [&](const TileDesc *d_t, const uint32_t *begin, bool main) -> int {
        for (int c = 0; c < kTileClasses; c++) {
            uint32_t b = begin[c], n = begin[c + 1] - b;
            if (!n) continue;
            TimedLaunch tl(ctx, FPM_K_SKETCH, st);
            if (main && c == 4 && job->thr4) {
                HIP_TRY(hipMemsetAsync(job->d_redo_n, 0, sizeof(uint32_t), st));
                HIP_TRY(launch_sketch_tiles_thr(job->d_seq, d_t + b, n, job->kp, job->d_thr,
                                                job->d_rows, job->d_count, job->d_redo,
                                                job->d_redo_n, st));
                // the tiles whose survivors did not fit, again through the plain kernel; the
                // count stays on the device (the list holds at most n: one entry per tile)
                HIP_TRY(launch_sketch_redo(job->d_seq, job->d_redo, job->d_redo_n, n, job->kp,
                                           job->d_thr, job->d_rows, job->d_count, st));
            } else {
                HIP_TRY(launch_sketch_tiles(c, job->d_seq, d_t + b, n, job->kp, job->d_thr,
                                            job->d_rows, job->d_count, st));
            }
            tl.done();
        }
        return FPM_OK;
    };
    auto merge_pass = [&](const MergeDesc *d_m, const std::vector<uint32_t> &rounds,
                          const std::vector<uint8_t> &small) -> int {
        for (size_t r = 0; r + 1 < rounds.size(); r++) {
            uint32_t b = rounds[r], n = rounds[r + 1] - b;
            TimedLaunch tl(ctx, FPM_K_MERGE, st);
            const bool sm = g_merge_small_env == 2 ||
                            (g_merge_small_env != 0 && r < small.size() && small[r]);
            HIP_TRY(launch_merge(d_m + b, n, job->kp.s, sm, st));
            tl.done();
        }
        return FPM_OK;
    };
    // failure flags: [0] main selections, [1] sample selections, [2..] per selection
    uint32_t *fail_main = job->d_sel_failed, *fail_samp = job->d_sel_failed + 1;
    // a selection that did not fit (more repeated values below the cut than LDS holds):
    // the pairwise merges of every sampled group's lists (rare; one host round trip)
    auto fallback = [&](bool sample) -> int {
        if (int rc = fallback_descs(job)) return rc;
        return sample ? merge_pass(job->d_sfmerge, job->sfround_begin, job->sfround_small)
                      : merge_pass(job->d_fmerge, job->fround_begin, job->fround_small);
    };
    // After a pass's selections and merges.  The groups its bound left short (`bounded`) are
    // counted before the one host read that also fetches the selections' failure flag (a
    // listing without `raise` changes nothing but the list, so a count stale from a failed
    // selection is harmless: after the fallback they are counted again); their tiles and
    // selections then run again (redo_short), listed again with their bounds raised / lifted.
    auto settle = [&](bool sample, bool bounded, auto list, int32_t &last) -> int {
        uint32_t *d_fail = sample ? fail_samp : fail_main;
        uint32_t *h_fail = job->h_sel_failed + (sample ? 1 : 0);
        if (bounded)
            if (int rc = list(false)) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if (*h_fail) {
            if (int rc = fallback(sample)) return rc;
            if (bounded) {
                if (int rc = list(false)) return rc;
                HIP_TRY(hipStreamSynchronize(st));
            }
        }
        if (!bounded) return FPM_OK;
        const uint32_t n_short = job->h_sel_failed[2];
        last = (int32_t)n_short;
        if (!n_short) return FPM_OK;
        if (int rc = list(true)) return rc;   // the same list, raised
        HIP_TRY(hipMemsetAsync(d_fail, 0, sizeof(uint32_t), st));
        if (int rc = redo_short(job, sample, n_short, st, tiles_pass)) return rc;
        HIP_TRY(hipMemcpyAsync(h_fail, d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return *h_fail ? fallback(sample) : FPM_OK;
    };
    if (job->n_ssel + job->n_sel)
        HIP_TRY(hipMemsetAsync(job->d_sel_failed, 0, (job->n_ssel + job->n_sel + 2) * sizeof(uint32_t),
                               st));
    if (job->n_slots) {   // sample pass of long groups -> per-group hash bounds
        if (job->sbounded)   // the bounds as staged (a previous run's redo lifted some)
            HIP_TRY(hipMemcpyAsync(job->d_thr + job->n_slots, job->d_sbound0,
                                   job->n_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        if (int rc = tiles_pass(job->d_stiles, job->sclass_begin, false)) return rc;
        if (job->n_ssel) {
            if (int rc = select_levels(job, job->d_sel, job->ssel_begin, fail_samp, st)) return rc;
            HIP_TRY(hipMemcpyAsync(job->h_sel_failed + 1, fail_samp, sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, st));
        }
        if (int rc = merge_pass(job->d_smerge, job->sround_begin, job->sround_small)) return rc;
        if (job->n_ssel) {
            // samples their a-priori bound left short: redone unbounded
            auto list_sample_short = [&](bool raise) -> int {
                HIP_TRY(hipMemsetAsync(job->d_sshort, 0, sizeof(uint32_t), st));
                HIP_TRY(launch_sketch_sample_short(job->d_srow, job->n_slots, job->d_count,
                                                   job->kp.s, job->d_thr + job->n_slots,
                                                   job->d_sshort, job->d_sshort + 1, raise, st));
                HIP_TRY(hipMemcpyAsync(job->h_sel_failed + 2, job->d_sshort, sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, st));
                return FPM_OK;
            };
            if (int rc = settle(true, job->sbounded, list_sample_short, job->last_sample_short))
                return rc;
        }
        HIP_TRY(launch_sketch_threshold(job->d_srow, job->n_slots, job->d_rows, job->d_count,
                                        job->kp.s, job->tight ? job->d_kt : nullptr, job->d_thr,
                                        job->tight ? job->d_thr_safe : nullptr, st));
    }
    // (the selections of each batch of genomes on a side stream beside the next batch's
    // tiles measured a wash on C5: the 120 KB-LDS selection workgroups take the tiles' CUs)
    if (int rc = tiles_pass(job->d_tiles, job->class_begin, true)) return rc;
    if (job->n_sel) {
        if (int rc = select_levels(job, job->d_sel, job->sel_begin, fail_main, st)) return rc;
        HIP_TRY(hipMemcpyAsync(job->h_sel_failed, fail_main, sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    }
    if (int rc = merge_pass(job->d_merge, job->round_begin, job->round_small)) return rc;
    if (job->n_sel) {
        // the groups the tight bound left short: redone under the safe bound
        auto list_short = [&](bool raise) -> int {
            HIP_TRY(hipMemsetAsync(job->d_short, 0, sizeof(uint32_t), st));
            HIP_TRY(launch_sketch_short(job->d_slot_group, job->n_slots, job->d_count, job->kp.s,
                                        job->d_thr, job->d_thr_safe, job->d_short, job->d_short + 1,
                                        raise, st));
            HIP_TRY(hipMemcpyAsync(job->h_sel_failed + 2, job->d_short, sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, st));
            return FPM_OK;
        };
        return settle(false, job->tight && job->n_slots, list_short, job->last_short);
    }
    return FPM_OK;
}

int fpm_sketch_job_short_groups(fpm_sketch_job *job, int32_t *n_short)
{
    if (!job || !n_short) return fail(FPM_EINVAL, "null argument");
    *n_short = job->last_short;
    return FPM_OK;
}

int fpm_sketch_job_sample_short(fpm_sketch_job *job, int32_t *n_short)
{
    if (!job || !n_short) return fail(FPM_EINVAL, "null argument");
    *n_short = job->sbounded ? job->last_sample_short : -1;
    return FPM_OK;
}

int fpm_sketch_job_plan(fpm_sketch_job *job, fpm_sketch_plan *out)
{
    if (!job || !out) return fail(FPM_EINVAL, "null argument");
    static_assert(FPM_TILE_CLASSES == kTileClasses, "fpmash.h states the tile classes");
    *out = fpm_sketch_plan{};
    for (int c = 0; c < kTileClasses; c++) {
        out->tiles[c] = job->class_begin[c + 1] - job->class_begin[c];
        out->sample_tiles[c] = job->sclass_begin[c + 1] - job->sclass_begin[c];
    }
    out->thr4 = job->thr4 ? 1 : 0;
    out->n_slots = job->n_slots;
    out->tight = job->tight ? 1 : 0;
    out->n_ssel = job->n_ssel;
    out->n_sel = job->n_sel;
    // as merge_pass (fpm_sketch_run) routes each round
    auto rounds = [](const std::vector<uint32_t> &begin, const std::vector<uint8_t> &small,
                     uint32_t *n, uint32_t *n_small) {
        *n = begin.empty() ? 0 : (uint32_t)begin.size() - 1;
        for (size_t r = 0; r < *n; r++)
            if (g_merge_small_env == 2 || (g_merge_small_env != 0 && r < small.size() && small[r]))
                ++*n_small;
    };
    rounds(job->round_begin, job->round_small, &out->rounds, &out->rounds_small);
    rounds(job->sround_begin, job->sround_small, &out->sample_rounds, &out->sample_rounds_small);
    out->merge_kernel = job->kp.s <= kMergeLdsKeys ? FPM_MK_LDS : FPM_MK_GLOBAL;
    return FPM_OK;
}

int fpm_merge_small_spills(fpm_ctx *ctx, uint64_t *count)
{
    if (!count) return fail(FPM_EINVAL, "null argument");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(merge_small_spills(count));
    return FPM_OK;
}

int fpm_sketch_device_output(fpm_sketch_job *job, uint64_t **d_hashes, uint32_t **d_count,
                             uint32_t *n_groups, uint32_t *row_stride)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    if (d_hashes) *d_hashes = job->d_rows;
    if (d_count) *d_count = job->d_count;
    if (n_groups) *n_groups = job->n_groups;
    if (row_stride) *row_stride = job->kp.s;
    return FPM_OK;
}

int fpm_sketch_fetch(fpm_sketch_job *job, uint64_t *out_hashes, uint32_t *out_count)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipDeviceSynchronize());
    if (out_hashes && job->n_groups)
        HIP_TRY(d2h_staged(ctx, out_hashes, job->d_rows,
                           (size_t)job->n_groups * job->kp.s * sizeof(uint64_t)));
    if (out_count && job->n_groups)
        HIP_TRY(copy_out(ctx, out_count, job->d_count, (size_t)job->n_groups * sizeof(uint32_t)));
    return FPM_OK;
}

int fpm_sketch_mult(fpm_sketch_job *job, void *stream, uint32_t *out_mult)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    const uint64_t s = job->kp.s, ng = job->n_groups;
    if (!ng) return FPM_OK;
    if (!job->d_mult) {
        HIP_TRY(job->mem.get(&job->d_mult, ng * s * sizeof(uint32_t)));
        HIP_TRY(job->mem.get(&job->d_first, ng * s * sizeof(unsigned long long)));
        HIP_TRY(job->mem.get(&job->d_ttop, ng * sizeof(uint64_t)));
    }
    HIP_TRY(hipMemsetAsync(job->d_mult, 0, ng * s * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(job->d_first, 0xff, ng * s * sizeof(unsigned long long), st));
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1)
            HIP_TRY(launch_mult_ttop(job->d_count, job->n_groups, job->kp.s, job->d_first,
                                     job->d_ttop, st));
        for (int c = 0; c < kTileClasses; c++) {
            const uint32_t b = job->class_begin[c], n = job->class_begin[c + 1] - b;
            if (!n) continue;
            TimedLaunch tl(ctx, FPM_K_SKETCH, st);
            HIP_TRY(launch_sketch_mult(c, pass, job->d_seq, job->d_tiles + b, n, job->kp,
                                       job->d_rows, job->d_count, job->d_mult, job->d_first,
                                       job->d_ttop, st));
            tl.done();
        }
    }
    if (out_mult) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(d2h_staged(ctx, out_mult, job->d_mult, ng * s * sizeof(uint32_t)));
    }
    return FPM_OK;
}

int fpm_sketch_job_info(fpm_sketch_job *job, uint64_t *seq_bytes, uint64_t *n_tiles,
                        uint64_t *n_kmers)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    if (seq_bytes) *seq_bytes = job->seq_bytes;
    if (n_tiles) *n_tiles = job->n_tiles;
    if (n_kmers) *n_kmers = job->n_kmers;
    return FPM_OK;
}

int fpm_sketch_job_redo_tiles(fpm_sketch_job *job, int32_t *n_redo)
{
    if (!job || !n_redo) return fail(FPM_EINVAL, "null argument");
    *n_redo = -1;
    if (!job->thr4 || !job->d_redo_n) return FPM_OK;
    if (int rc = set_device(job->ctx)) return rc;
    uint32_t v = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&v, job->d_redo_n, sizeof v, hipMemcpyDeviceToHost));
    *n_redo = (int32_t)v;
    return FPM_OK;
}

int fpm_sketch_job_set_min_copies(fpm_sketch_job *job, uint32_t min_copies)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    if (min_copies == 0) return fail(FPM_EINVAL, "min_copies must be >= 1");
    job->min_copies = min_copies;
    return FPM_OK;
}

// One widening round of reads mode over `wide` (the staged job itself, or a job staged with a
// wider sketch size over the groups still open): its exact bottom-S' rows, the counts and
// positions of their entries, the filter, the full sketches' maximum.
static int reads_round(fpm_sketch_job *job, fpm_sketch_job *wide, uint32_t round, hipStream_t st)
{
    fpm_ctx *ctx = job->ctx;
    const uint32_t m = job->min_copies, s = job->kp.s, S = wide->kp.s, ng = job->n_groups;
    if (int rc = fpm_sketch_run(wide, st)) return rc;
    job->reads_sampled = (int32_t)wide->n_slots;
    // per wide-row entry: a u32 count and min_copies u64 position slots, from the context's
    // pool of released buffers (no device-wide allocation per round once it is warm)
    const size_t n_ent = (size_t)ng * S;
    const size_t wcnt_bytes = n_ent * sizeof(uint32_t);
    const size_t slots_bytes = n_ent * m * sizeof(unsigned long long);
    DevBufs tmp(ctx);
    uint32_t *d_wcnt;
    unsigned long long *d_slots;
    auto body = [&]() -> int {
        size_t mem_free = 0, mem_total = 0;
        HIP_TRY(hipMemGetInfo(&mem_free, &mem_total));
        if (wcnt_bytes + slots_bytes > mem_free)
            return fail(FPM_ENOMEM, "reads mode: " + std::to_string((wcnt_bytes + slots_bytes) >> 20) +
                                        " MB of counts and position slots (groups x wide sketch x "
                                        "(4 + 8 min_copies) B) exceed the free device memory");
        HIP_TRY(tmp.get_pooled(&d_wcnt, wcnt_bytes));
        HIP_TRY(tmp.get_pooled(&d_slots, slots_bytes));
        HIP_TRY(hipMemsetAsync(d_wcnt, 0, n_ent * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(d_slots, 0xff, n_ent * m * sizeof(unsigned long long), st));
        for (int c = 0; c < kTileClasses; c++) {
            const uint32_t b = wide->class_begin[c], n = wide->class_begin[c + 1] - b;
            if (!n) continue;
            TimedLaunch tl(ctx, FPM_K_SKETCH, st);
            HIP_TRY(launch_reads_count(c, wide->d_seq, wide->d_tiles + b, n, wide->kp, wide->d_rows,
                                       wide->d_count, m, d_wcnt, d_slots, st));
            tl.done();
        }
        HIP_TRY(launch_reads_filter(wide->d_rows, wide->d_count, S, ng, d_wcnt, d_slots, m, s, round,
                                    job->d_rdone, job->d_rrows, job->d_rcount, job->d_rmult,
                                    job->d_rttop, st));
        for (int c = 0; c < kTileClasses; c++) {
            const uint32_t b = wide->class_begin[c], n = wide->class_begin[c + 1] - b;
            if (!n) continue;
            TimedLaunch tl(ctx, FPM_K_SKETCH, st);
            HIP_TRY(launch_reads_maxcount(c, wide->d_seq, wide->d_tiles + b, n, wide->kp, s, round,
                                          job->d_rdone, job->d_rrows, job->d_rcount, job->d_rmult,
                                          job->d_rttop, st));
            tl.done();
        }
        // the one host read of the round: which groups are final
        HIP_TRY(hipMemcpyAsync(job->h_rdone.data(), job->d_rdone, ng * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return FPM_OK;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(st);   // before `tmp` hands the two buffers back
    return rc;
}

int fpm_sketch_reads_run(fpm_sketch_job *job, void *stream)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    const uint64_t s = job->kp.s, ng = job->n_groups;
    job->reads_rounds = 0;
    if (!ng) return FPM_OK;
    if (!job->d_rrows) {
        // all five or none: a later run must not find some of them missing
        DevBufs out;
        hipError_t e = out.get(&job->d_rrows, ng * s * sizeof(uint64_t));
        if (e == hipSuccess) e = out.get(&job->d_rmult, ng * s * sizeof(uint32_t));
        if (e == hipSuccess) e = out.get(&job->d_rcount, ng * sizeof(uint32_t));
        if (e == hipSuccess) e = out.get(&job->d_rdone, ng * sizeof(uint32_t));
        if (e == hipSuccess) e = out.get(&job->d_rttop, ng * sizeof(uint64_t));
        if (e != hipSuccess) {
            job->d_rrows = job->d_rttop = nullptr;
            job->d_rmult = job->d_rcount = job->d_rdone = nullptr;
            job->reads_rounds = -1;
            return fail(FPM_ENOMEM, std::string("reads mode output alloc: ") + hipGetErrorString(e));
        }
        job->mem.absorb(std::move(out));
    }
    job->h_rdone.assign(ng, 0);
    HIP_TRY(hipMemsetAsync(job->d_rdone, 0, ng * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(job->d_rcount, 0, ng * sizeof(uint32_t), st));
    // The wide row must reach the s-th hash with min_copies occurrences: sequencing errors put
    // several single-copy k-mers below each repeated one, so the first width is 8 s and each
    // further round has 4 x the last, up to one more than the windows of the largest group
    // still open (a row of that width is never full: it holds every distinct hash of its
    // group).  min_copies 1 needs no widening: every entry qualifies.
    std::vector<uint64_t> windows(ng, 0);
    for (uint32_t r : job->recs.order)
        if (job->recs.len[r] >= job->kp.k)
            windows[job->recs.group[r]] += job->recs.len[r] - job->kp.k + 1;
    auto open_cap = [&]() {
        uint64_t c = 0;
        for (uint64_t g = 0; g < ng; g++)
            if (!job->h_rdone[g]) c = std::max(c, windows[g]);
        return std::min<uint64_t>(c + 1, 0x7fffffffULL);
    };
    uint64_t cap = open_cap();
    uint64_t wide = job->min_copies == 1 ? s : std::min<uint64_t>(8 * s, cap);
    for (uint32_t round = 1;; round++) {
        if (wide == s) {
            if (int rc = reads_round(job, job, round, st)) return rc;
        } else {
            StageRecords R;
            R.n_groups = job->n_groups;
            R.pos = job->recs.pos;
            R.len = job->recs.len;
            R.group = job->recs.group;
            for (uint32_t r : job->recs.order)
                if (!job->h_rdone[R.group[r]]) R.order.push_back(r);
            R.d_seq = job->d_seq;
            R.d_seq_bytes = job->seq_bytes;
            R.borrow = true;
            fpm_sketch_params p = job->params;
            p.sketch_size = (uint32_t)wide;
            fpm_sketch_job *wj = nullptr;
            if (int rc = stage_core(ctx, &p, R, &wj)) return rc;
            const int rc = reads_round(job, wj, round, st);
            fpm_sketch_job_free(wj);
            if (rc) return rc;
        }
        job->reads_rounds = (int32_t)round;
        bool open = false;
        for (uint32_t d : job->h_rdone) open = open || !d;
        if (!open) return FPM_OK;
        if (wide >= cap) return fail(FPM_EHIP, "internal: reads mode left a group open");
        cap = open_cap();
        wide = std::min<uint64_t>(wide * 4, cap);
    }
}

int fpm_sketch_reads_fetch(fpm_sketch_job *job, uint64_t *out_hashes, uint32_t *out_count,
                           uint32_t *out_mult, uint64_t *out_estimate)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    if (job->reads_rounds < 0) return fail(FPM_EINVAL, "reads_fetch before reads_run");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    const size_t s = job->kp.s, ng = job->n_groups;
    if (!ng) return FPM_OK;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint32_t> cnt(ng);
    HIP_TRY(copy_out(ctx, cnt.data(), job->d_rcount, ng * sizeof(uint32_t)));
    if (out_count) memcpy(out_count, cnt.data(), ng * sizeof(uint32_t));
    std::vector<uint64_t> tmp;
    if (!out_hashes && out_estimate) {
        tmp.resize(ng * s);
        out_hashes = tmp.data();
    }
    if (out_hashes) HIP_TRY(d2h_staged(ctx, out_hashes, job->d_rrows, ng * s * sizeof(uint64_t)));
    if (out_mult) HIP_TRY(d2h_staged(ctx, out_mult, job->d_rmult, ng * s * sizeof(uint32_t)));
    if (out_estimate) {
        // MinHashHeap::estimateSetSize (MinHashHeap.h:45), truncated as Sketch.cpp:1432 stores it
        const double range = job->kp.use64 ? 18446744073709551616.0 : 4294967296.0;
        for (size_t g = 0; g < ng; g++) {
            out_estimate[g] = 0;
            if (!cnt[g]) continue;
            const double e = range * (double)cnt[g] / (double)out_hashes[g * s + cnt[g] - 1];
            out_estimate[g] = e < 18446744073709551616.0 ? (uint64_t)e : ~0ULL;
        }
    }
    return FPM_OK;
}

int fpm_sketch_job_reads_rounds(fpm_sketch_job *job, int32_t *n_rounds, uint32_t *group_round)
{
    if (!job || !n_rounds) return fail(FPM_EINVAL, "null argument");
    *n_rounds = job->reads_rounds;
    if (group_round && job->reads_rounds >= 0)
        for (uint32_t g = 0; g < job->n_groups; g++) group_round[g] = job->h_rdone[g];
    return FPM_OK;
}

int fpm_sketch_job_reads_sampled(fpm_sketch_job *job, int32_t *n_sampled)
{
    if (!job || !n_sampled) return fail(FPM_EINVAL, "null argument");
    *n_sampled = job->reads_rounds < 0 ? -1 : job->reads_sampled;
    return FPM_OK;
}

void fpm_sketch_job_free(fpm_sketch_job *job)
{
    if (!job) return;
    job_release(job);
    delete job;
}

int fpm_sketch_merge_dev(fpm_ctx *ctx, const uint64_t *d_lists, const uint32_t *d_counts,
                         uint32_t n_lists, uint32_t s, uint64_t *d_out, uint32_t *d_out_count,
                         void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    if ((n_lists && (!d_lists || !d_counts)) || !d_out || !d_out_count || s == 0)
        return fail(FPM_EINVAL, "sketch_merge_dev: bad argument");
    hipStream_t st = pick_stream(ctx, stream);
    if (n_lists == 0) {
        HIP_TRY(hipMemsetAsync(d_out_count, 0, 4, st));
        return FPM_OK;
    }
    if (n_lists == 1) {
        HIP_TRY(hipMemcpyAsync(d_out, d_lists, (size_t)s * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_out_count, d_counts, 4, hipMemcpyDeviceToDevice, st));
        return FPM_OK;
    }
    // pairwise rounds (the bottom s of a union = the bottom s of the union of the parts'
    // bottom s); intermediate lists in scratch rows, the last merge writes d_out
    void *tmp, *tcnt, *dd;
    HIP_TRY(scratch(ctx, kSlotMergeRows, (size_t)(n_lists - 1) * s * 8, &tmp));
    HIP_TRY(scratch(ctx, kSlotMergeCounts, (size_t)(n_lists - 1) * 4, &tcnt));
    struct L { const uint64_t *p; const uint32_t *c; };
    std::vector<L> cur(n_lists);
    for (uint32_t i = 0; i < n_lists; i++) cur[i] = L{d_lists + (uint64_t)i * s, d_counts + i};
    std::vector<MergeDesc> md;
    std::vector<uint32_t> rounds{0};
    uint32_t used = 0;
    while (cur.size() > 1) {
        std::vector<L> nxt;
        for (size_t i = 0; i + 1 < cur.size(); i += 2) {
            uint64_t *c = cur.size() == 2 ? d_out : (uint64_t *)tmp + (uint64_t)used * s;
            uint32_t *cc = cur.size() == 2 ? d_out_count : (uint32_t *)tcnt + used;
            if (cur.size() != 2) used++;
            md.push_back(MergeDesc{cur[i].p, cur[i].c, cur[i + 1].p, cur[i + 1].c, c, cc});
            nxt.push_back(L{c, cc});
        }
        if (cur.size() % 2) nxt.push_back(cur.back());
        cur.swap(nxt);
        rounds.push_back((uint32_t)md.size());
    }
    HIP_TRY(scratch(ctx, kSlotMergeDescs, md.size() * sizeof(MergeDesc), &dd));
    HIP_TRY(hipStreamSynchronize(st));   // the descriptor buffer may still be read by a prior call
    HIP_TRY(copy_in(ctx, dd, md.data(), md.size() * sizeof(MergeDesc)));
    for (size_t r = 0; r + 1 < rounds.size(); r++) {
        TimedLaunch tl(ctx, FPM_K_MERGE, st);
        HIP_TRY(launch_merge((const MergeDesc *)dd + rounds[r], rounds[r + 1] - rounds[r], s, false,
                             st));
        tl.done();
    }
    return FPM_OK;
}

int fpm_sketch_batch(fpm_ctx *ctx, const fpm_sketch_params *p, const char *seq,
                     const uint64_t *rec_off, uint32_t n_rec, const uint32_t *group_of_rec,
                     uint32_t n_groups, uint64_t *out_hashes, uint32_t *out_count)
{
    fpm_sketch_job *job = nullptr;
    int rc = fpm_sketch_stage(ctx, p, seq, rec_off, n_rec, group_of_rec, n_groups, &job);
    if (rc) return rc;
    rc = fpm_sketch_run(job, nullptr);
    if (!rc) rc = fpm_sketch_fetch(job, out_hashes, out_count);
    fpm_sketch_job_free(job);
    return rc;
}

}  // extern "C"
