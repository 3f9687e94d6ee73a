// sketch_plan.cpp — the planner behind sketch staging (sketch_plan.hpp): tile cut, row
// numbering, sample rule and bounds, selection trees, merge rounds, the survivors decision.
// Host arithmetic only; the order in which rows are numbered is stated in the header.
#include "sketch_plan.hpp"

#include <algorithm>
#include <cmath>

namespace fpm {
namespace {

using RowLists = std::vector<std::vector<uint32_t>>;   // per group: the rows still to combine

int tile_class(uint32_t nstarts)
{
    for (int c = 0; c < kTileClasses; c++)
        if (nstarts <= kTileCap[c]) return c;
    return -1;
}

uint64_t tile_starts(const TileDesc &t, uint32_t k) { return t.n_bytes >= k ? t.n_bytes - k + 1 : 0; }

// Row numbers in handing-out order, and per row the estimated list length (s until set).  The
// estimate steers merge_small_kernel and the selections' chunking only; results do not depend
// on it.
struct Rows {
    uint32_t n;
    uint64_t s;
    std::vector<uint64_t> est;
    uint32_t fresh() { return n++; }
    uint64_t &len(uint32_t r)
    {
        if (est.size() <= r) est.resize((size_t)r + 1, s);
        return est[r];
    }
};

// per group: its tiles, its sample rate and its slot
struct Groups {
    std::vector<uint32_t> ntile, every, slot_of;   // slot_of: 0 = not sampled, else slot + 1
    explicit Groups(uint32_t n) : ntile(n, 0), every(n, kSampleEvery), slot_of(n, 0) {}
    // the sampled share of the group's tiles
    double share(uint32_t g) const { return (double)((ntile[g] + every[g] - 1) / every[g]) / ntile[g]; }
};

// cut tiles: a tile covers [byte_off, byte_off + n_bytes) of the packed buffer, records of
// one group only; short records share a tile while its k-mer starts fit (bytes between
// them, separators or records shorter than k, hold no valid window).  -> the k-mer starts
uint64_t cut_tiles(const PlanRecords &R, uint32_t k, std::vector<TileDesc> &tiles,
                   std::vector<uint32_t> &tile_group)
{
    uint64_t n_kmers = 0;
    uint32_t cur_group = UINT32_MAX;
    bool open = false;
    TileDesc cur{};
    auto close = [&]() {
        if (open) { tiles.push_back(cur); tile_group.push_back(cur_group); open = false; }
    };
    for (uint32_t r : R.order) {
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
                tiles.push_back(TileDesc{poff + c0, (uint32_t)(cn + k - 1), 0, 0, 0});
                tile_group.push_back(g);
            }
        } else if (open && poff > cur.byte_off + cur.n_bytes &&
                   poff + l - cur.byte_off - k + 1 <= kPackKmers) {
            cur.n_bytes = (uint32_t)(poff + l - cur.byte_off);   // through this record
        } else {
            close();
            cur = TileDesc{poff, (uint32_t)l, 0, 0, 0};
            open = true;
        }
    }
    close();
    for (size_t t = 0; t < tiles.size(); t++) tiles[t].pad = tile_group[t];
    return n_kmers;
}

// rows: single-tile groups write their final row, others get temp rows (lists)
void number_rows(std::vector<TileDesc> &tiles, const std::vector<uint32_t> &tile_group, Groups &G,
                 Rows &rows, RowLists &lists)
{
    for (uint32_t g : tile_group) G.ntile[g]++;
    for (size_t t = 0; t < tiles.size(); t++) {
        const uint32_t g = tile_group[t];
        if (G.ntile[g] == 1) tiles[t].out_row = g;
        else { tiles[t].out_row = rows.fresh(); lists[g].push_back(tiles[t].out_row); }
    }
}

// long groups (many 4096-k-mer chunks: C5 genomes): every kSampleEvery-th tile is also
// sketched in a sample pass (own temp rows and merge plan); the sample's s-th smallest
// hash is >= the group's s-th smallest, so the full pass drops every hash above it and
// its merges move ~kSampleEvery*s hashes per group instead of every tile's bottom-s.
// The sample rate per group: every E-th tile, E = the group's k-mers / 8 s within
// [16, 64], so a sample holds ~8 s k-mers: enough for its s-th smallest (the safe bound)
// and a tight kt-th one.  C5's 5 Mb genomes: E = 61, C5 23.6 -> 21.9 ms against E = 16
// (22.8 ms at 16 s k-mers, E = 31), same box, r05x / r05y.
// -> the slots; sgroup: each sample tile's group
uint32_t choose_samples(std::vector<TileDesc> &tiles, const std::vector<uint32_t> &tile_group,
                        uint32_t s, Groups &G, Rows &rows, std::vector<TileDesc> &stiles,
                        std::vector<uint32_t> &sgroup, RowLists &slists)
{
    const uint32_t n_groups = (uint32_t)G.ntile.size();
    for (uint32_t g = 0; g < n_groups; g++)
        G.every[g] = (uint32_t)std::min<uint64_t>(
            64, std::max<uint64_t>(kSampleEvery, (uint64_t)G.ntile[g] * kChunkKmers / (8ULL * s)));
    uint32_t n_slots = 0;
    std::vector<uint32_t> seen(n_groups, 0);
    for (size_t t = 0; t < tiles.size(); t++) {
        const uint32_t g = tile_group[t];
        const uint64_t sample_kmers = (uint64_t)(G.ntile[g] / G.every[g]) * kChunkKmers;
        if (G.ntile[g] < 2 * G.every[g] || sample_kmers < 4ULL * s) continue;
        if (!G.slot_of[g]) G.slot_of[g] = ++n_slots;
        if (seen[g]++ % G.every[g] == 0) {
            TileDesc st = tiles[t];
            st.out_row = rows.fresh();
            st.thr_slot = 0;
            slists[g].push_back(st.out_row);
            stiles.push_back(st);
            sgroup.push_back(g);
        }
    }
    for (size_t t = 0; t < tiles.size(); t++) tiles[t].thr_slot = G.slot_of[tile_group[t]];
    return n_slots;
}

// list-length estimate per row: a tile keeps at most its k-mers and s; a tile of a sampled
// (thresholded) group keeps ~kSampleEvery * s / tiles of the group's hashes (2x margin)
void estimate_lengths(const std::vector<TileDesc> &tiles, const std::vector<uint32_t> &tile_group,
                      const std::vector<TileDesc> &stiles, const Groups &G, uint32_t k, uint32_t s,
                      Rows &rows)
{
    for (size_t t = 0; t < tiles.size(); t++) {
        const uint32_t g = tile_group[t];
        uint64_t e = std::min<uint64_t>(s, tile_starts(tiles[t], k));
        if (G.slot_of[g]) e = std::min<uint64_t>(e, 2ULL * G.every[g] * s / G.ntile[g] + 64);
        rows.len(tiles[t].out_row) = e;
    }
    for (auto &st : stiles) rows.len(st.out_row) = std::min<uint64_t>(s, tile_starts(st, k));
}

// A sample's tiles keep only the hashes below an a-priori bound: hash values are uniform,
// so of a sample's N windows ~frac N lie below frac of the hash range, and frac =
// (1.25 s + 16 sqrt(s)) / N leaves >= s of them (C5: ~14k of a sample's 82k) with ~40
// standard deviations to spare.  The sample's selection then reads ~6x fewer keys.  A
// sample left with fewer than s (values repeated across its tiles) gives its group no
// bound, as a sample shorter than s always did (the sketches do not depend on it).
// A bounded sample tile carries thr_slot n_slots + slot + 1 (d_thr[n_slots + slot]).
std::vector<uint64_t> sample_bounds(std::vector<TileDesc> &stiles, const std::vector<uint32_t> &sgroup,
                                    const Groups &G, uint32_t n_slots, const PlanParams &p, Rows &rows)
{
    const uint32_t k = p.k, s = p.s;
    std::vector<uint64_t> sbound(n_slots, ~0ULL), ns(n_slots, 0);
    for (size_t i = 0; i < stiles.size(); i++)
        ns[G.slot_of[sgroup[i]] - 1] += tile_starts(stiles[i], k);
    const double range = p.use64 ? 18446744073709551616.0 : 4294967296.0;
    for (size_t i = 0; i < n_slots; i++) {
        const double frac = (1.25 * s + 16.0 * std::sqrt((double)s)) / std::max<double>(1, ns[i]);
        if (frac < 0.5) sbound[i] = (uint64_t)(frac * range);
    }
    for (size_t i = 0; i < stiles.size(); i++) {
        const uint32_t sl = G.slot_of[sgroup[i]];
        if (sbound[sl - 1] == ~0ULL) continue;
        stiles[i].thr_slot = n_slots + sl;
        uint64_t &e = rows.len(stiles[i].out_row);
        e = std::min<uint64_t>(e, (uint64_t)(2.0 * (double)sbound[sl - 1] / range * stiles[i].n_bytes) + 64);
    }
    return sbound;
}

// One group's selection: a single descriptor, or, for a group with more keys than one
// workgroup should read (~2^19: a 1 Gb genome's sample holds 62 M), chunks of rows selected in
// parallel into rows of their own, then the chunks' sketches selected again (a tree of levels,
// one launch per level).  lv[level]: the level's descriptors; tags (optional): per level, the
// slot of each descriptor (sample selections carry slot 0xFFFFFFFF on the device; the host
// finds a group's descriptors by the tag)
void build_sel(const std::vector<uint32_t> &rows0, uint32_t final_row, uint32_t slot, Rows &rows,
               std::vector<uint32_t> &sel_rows, std::vector<std::vector<SelDesc>> &lv,
               std::vector<std::vector<uint32_t>> *tags = nullptr, uint32_t tag = 0)
{
    std::vector<uint32_t> cur = rows0;
    for (size_t level = 0;; level++) {
        if (lv.size() <= level) lv.resize(level + 1);
        if (tags && tags->size() <= level) tags->resize(level + 1);
        std::vector<std::pair<size_t, size_t>> ch;
        size_t a = 0;
        uint64_t acc = 0;
        for (size_t i = 0; i < cur.size(); i++) {
            const uint64_t e = rows.len(cur[i]);
            if (i > a && (acc + e > kKeysPerWG || i - a >= kRowsPerWG)) {
                ch.push_back({a, i});
                a = i;
                acc = 0;
            }
            acc += e;
        }
        ch.push_back({a, cur.size()});
        const bool last = ch.size() == 1;
        std::vector<uint32_t> next;
        for (auto &c : ch) {
            const uint32_t r = last ? final_row : rows.fresh();
            if (!last) {
                uint64_t sum = 0;
                for (size_t i = c.first; i < c.second; i++) sum += rows.len(cur[i]);
                rows.len(r) = std::min<uint64_t>(rows.s, sum);
            }
            lv[level].push_back(SelDesc{(uint32_t)sel_rows.size(), (uint32_t)(c.second - c.first), r, slot});
            if (tags) (*tags)[level].push_back(tag);
            sel_rows.insert(sel_rows.end(), cur.begin() + c.first, cur.begin() + c.second);
            next.push_back(r);
        }
        if (last) return;
        cur.swap(next);
    }
}

// pairwise merge rounds of each group's lists; the last merge writes final_row(g)
template <typename FinalRow>
MergeSchedule plan_rounds(RowLists &L_of, FinalRow final_row, Rows &rows)
{
    MergeSchedule m;
    m.round_begin.assign(1, 0);
    for (;;) {
        bool any = false;
        uint64_t round_max = 0;
        for (uint32_t g = 0; g < L_of.size(); g++) {
            auto &L = L_of[g];
            if (L.size() < 2) continue;
            any = true;
            std::vector<uint32_t> next;
            for (size_t i = 0; i + 1 < L.size(); i += 2) {
                const uint32_t c = (L.size() == 2) ? final_row(g) : rows.fresh();
                m.steps.push_back({L[i], L[i + 1], c});
                next.push_back(c);
                const uint64_t ea = rows.len(L[i]), eb = rows.len(L[i + 1]);
                rows.len(c) = std::min<uint64_t>(rows.s, ea + eb);
                round_max = std::max(round_max, std::max(ea, eb));
            }
            if (L.size() % 2) next.push_back(L.back());
            if (next.size() == 1) next.clear();   // reached the final row
            L.swap(next);
        }
        if (!any) break;
        m.round_begin.push_back((uint32_t)m.steps.size());
        m.round_small.push_back(round_max <= kMergeSmallCap ? 1 : 0);
    }
    return m;
}

// d_sel: the sample levels, then the main levels; level boundaries for the launches
void flatten_sel(const std::vector<std::vector<SelDesc>> &ssel_lv,
                 const std::vector<std::vector<uint32_t>> &ssel_tag_lv,
                 const std::vector<std::vector<SelDesc>> &sel_lv, SketchPlan &P)
{
    P.ssel_begin.assign(1, 0);
    for (auto &l : ssel_lv) {
        P.sel.insert(P.sel.end(), l.begin(), l.end());
        P.ssel_begin.push_back((uint32_t)P.sel.size());
    }
    for (auto &l : ssel_tag_lv) P.ssel_tag.insert(P.ssel_tag.end(), l.begin(), l.end());
    P.sel_begin.push_back((uint32_t)P.sel.size());
    for (auto &l : sel_lv) {
        P.sel.insert(P.sel.end(), l.begin(), l.end());
        P.sel_begin.push_back((uint32_t)P.sel.size());
    }
}

// Selections, merge schedules and their rows, in the contract's order.  Sampled groups select
// their sketch (and their sample's) with group_select_kernel; their lists leave the merge
// plans for fallback plans (pairwise merges only: C5 17.6 vs 2.6 ms).
void plan_reductions(const Groups &G, bool use_sel, Rows &rows, RowLists &lists, RowLists &slists,
                     SketchPlan &P)
{
    const uint32_t n_groups = P.n_groups;
    std::vector<std::vector<SelDesc>> ssel_lv, sel_lv;
    std::vector<std::vector<uint32_t>> ssel_tag_lv;
    RowLists sflists(n_groups), flists(n_groups);
    for (uint32_t g = 0; g < n_groups; g++)
        if (G.slot_of[g]) P.srow[G.slot_of[g] - 1] = slists[g].size() == 1 ? slists[g][0] : 0;
    if (use_sel)
        for (uint32_t g = 0; g < n_groups; g++) {
            if (!G.slot_of[g] || slists[g].size() < 2) continue;
            const uint32_t r = rows.fresh();                    // the sample's sketch row
            P.srow[G.slot_of[g] - 1] = r;
            build_sel(slists[g], r, 0xFFFFFFFFu, rows, P.sel_rows, ssel_lv, &ssel_tag_lv,
                      G.slot_of[g] - 1);
            sflists[g].swap(slists[g]);
        }
    P.smerge = plan_rounds(slists, [&](uint32_t g) {
        return P.srow[G.slot_of[g] - 1] = rows.fresh();
    }, rows);
    if (use_sel)
        for (uint32_t g = 0; g < n_groups; g++) {
            if (!G.slot_of[g] || lists[g].size() < 2) continue;
            build_sel(lists[g], g, G.slot_of[g] - 1, rows, P.sel_rows, sel_lv);
            flists[g].swap(lists[g]);
        }
    P.merge = plan_rounds(lists, [](uint32_t g) { return g; }, rows);
    flatten_sel(ssel_lv, ssel_tag_lv, sel_lv, P);
    // the fallback plans' intermediate rows come last: they are allocated only if a selection
    // fails (a C5 share holds ~1.2 M tile rows of s u64: the fallback rows would double that)
    P.n_rows = rows.n;
    if (use_sel) {
        P.sfmerge = plan_rounds(sflists, [&](uint32_t g) { return P.srow[G.slot_of[g] - 1]; }, rows);
        P.fmerge = plan_rounds(flists, [](uint32_t g) { return g; }, rows);
    }
    P.n_fb_rows = rows.n - P.n_rows;
}

// tight bounds where every sampled group has a selection: kt = f s + 8 sqrt(f s) + 32 of
// the sample's hashes (f = the group's sampled share of tiles), so ~kt / f >= s of the
// group's distinct hashes lie below it with ~8 standard deviations to spare (C5 at E = 61:
// ~300 of the sample's 10,000; the group keeps ~18k hashes instead of ~160k)
void tight_bounds(const Groups &G, uint32_t s, SketchPlan &P)
{
    P.kt.assign(P.n_slots, s);
    P.slot_group.assign(P.n_slots, 0);
    for (uint32_t g = 0; g < P.n_groups; g++) {
        if (!G.slot_of[g]) continue;
        const uint32_t i = G.slot_of[g] - 1;
        P.slot_group[i] = g;
        const double fs = G.share(g) * s;
        P.kt[i] = (uint32_t)std::min<double>(s, std::ceil(fs + 8.0 * std::sqrt(fs) + 32.0));
    }
    P.tight = true;
    for (uint64_t b : P.sbound) P.sbounded = P.sbounded || b != ~0ULL;
}

// the survivors-only tile kernel for the class-4 tiles when every one carries its
// group's bound and that bound leaves few survivors per tile: a group's main pass keeps
// about kSampleEvery * s of its hashes (the sample's s-th smallest bounds them), so a
// tile keeps ~kSampleEvery * s / (the group's tiles); est (2x margin + 64, above) must
// stay within half of what one tile holds, or most tiles would be hashed twice (their
// survivors overflow and the plain kernel redoes them).  (C5 one GPU: 31.2 -> 25.8 ms,
// same box, r04; C5 tiles: est 326 of 1,024)
// (tight bounds: ~kt / f survivors per group; a short group's redo under the safe bound
// keeps ~E s per group, and its tiles that overflow are redone by the plain kernel)
void survivors_decision(const Groups &G, uint32_t s, SketchPlan &P)
{
    const uint32_t b4 = P.class_begin[4];
    P.n4 = P.class_begin[5] - b4;
    std::vector<uint64_t> slot_est(P.n_slots + 1, ~0ULL);
    for (uint32_t g = 0; g < P.n_groups; g++) {
        if (!G.slot_of[g]) continue;
        slot_est[G.slot_of[g]] =
            P.tight ? (uint64_t)(2.0 * P.kt[G.slot_of[g] - 1] / G.share(g) / G.ntile[g]) + 64
                    : 2ULL * G.every[g] * s / G.ntile[g] + 64;
    }
    bool all = P.n4 > 0;
    for (uint32_t i = 0; all && i < P.n4; i++) {
        const uint32_t sl = P.tiles[b4 + i].thr_slot;
        all = sl != 0 && slot_est[sl] <= kThrTileKeys / 2;
    }
    P.thr4 = all;
}

// tiles ordered by capacity class; false: a tile fits no class
bool order_by_class(const std::vector<TileDesc> &in, uint32_t k, std::vector<TileDesc> &out,
                    uint32_t *begin)
{
    out.clear();
    out.reserve(in.size());
    begin[0] = 0;
    for (int c = 0; c < kTileClasses; c++) {
        for (auto &t : in)
            if (tile_class(t.n_bytes - k + 1) == c) out.push_back(t);
        begin[c + 1] = (uint32_t)out.size();
    }
    return out.size() == in.size();
}

}  // namespace

bool plan_sketch(const PlanRecords &R, const PlanParams &p, SketchPlan *out)
{
    const uint32_t k = p.k, s = p.s;
    SketchPlan &P = *out;
    P = SketchPlan{};
    P.n_groups = R.n_groups;
    std::vector<TileDesc> tiles, stiles;
    std::vector<uint32_t> tile_group, sgroup;
    P.n_kmers = cut_tiles(R, k, tiles, tile_group);
    Rows rows{R.n_groups, s, {}};
    Groups G(R.n_groups);
    RowLists lists(R.n_groups), slists(R.n_groups);
    number_rows(tiles, tile_group, G, rows, lists);
    P.n_slots = choose_samples(tiles, tile_group, s, G, rows, stiles, sgroup, slists);
    estimate_lengths(tiles, tile_group, stiles, G, k, s, rows);
    const bool use_sel = (uint64_t)s + s / 8 + 64 <= kGroupSelectCap;
    P.srow.assign(P.n_slots, 0);
    P.sbound.assign(P.n_slots, ~0ULL);
    if (use_sel && P.n_slots) P.sbound = sample_bounds(stiles, sgroup, G, P.n_slots, p, rows);
    plan_reductions(G, use_sel, rows, lists, slists, P);
    if (!order_by_class(tiles, k, P.tiles, P.class_begin) ||
        !order_by_class(stiles, k, P.stiles, P.sclass_begin))
        return false;
    if (use_sel && P.n_slots && !P.sel.empty()) tight_bounds(G, s, P);
    survivors_decision(G, s, P);
    return true;
}

}  // namespace fpm
