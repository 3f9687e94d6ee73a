// sketchplan_check.cpp — the sketch planner (csrc/sketch_plan.cpp) alone, on the CPU: the
// structure every plan must have (tiles cover each k-mer start once, every row has one producer
// per pass and is read after it was written, the fallback schedules reduce the same lists into
// the same rows), over inputs at the planner's edges.  The planner reads record lengths only,
// so the inputs are lengths.  Built with a host sanitizer by tests/test_sketchplan_host.py;
// prints "sketchplan ok" and exits 0, or names the first check that failed.
//
// With arguments it prints one plan instead, as a line of JSON:
//   sketchplan_check K S USE64 host|device GROUP:LENGTH ...      (groups ascending)
#include "../csrc/sketch_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

using namespace fpm;

static std::string g_case;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            fprintf(stderr, "sketchplan_check:%d: %s: %s\n", __LINE__, g_case.c_str(), #cond); \
            return false;                                                                    \
        }                                                                                    \
    } while (0)

struct Case {
    std::string name;
    uint32_t k, s;
    bool use64, device;
    std::vector<std::pair<uint32_t, uint64_t>> recs;   // (group, length), groups ascending
    uint32_t n_groups;
    void add(uint32_t g, uint64_t len, uint32_t times = 1)
    {
        for (uint32_t i = 0; i < times; i++) recs.push_back({g, len});
        n_groups = std::max(n_groups, g + 1);
    }
};

struct Records {
    std::vector<uint32_t> order, group;
    std::vector<uint64_t> pos, len;
};

// packed offsets (a 0x00 after every record): the host path packs the records >= k only, the
// device path keeps what the parser emitted, shorter records too
static Records records_of(const Case &c)
{
    Records R;
    uint64_t at = 0;
    for (auto &r : c.recs) {
        const bool kept = c.device || r.second >= c.k;
        R.order.push_back((uint32_t)R.len.size());
        R.group.push_back(r.first);
        R.len.push_back(r.second);
        R.pos.push_back(kept ? at : 0);
        if (kept) at += r.second + 1;
    }
    return R;
}

static int class_of(uint64_t starts)
{
    for (int c = 0; c < kTileClasses; c++)
        if (starts <= kTileCap[c]) return c;
    return -1;
}

static bool check_classes(const std::vector<TileDesc> &tiles, const uint32_t *begin, uint32_t k)
{
    CHECK(begin[0] == 0 && begin[kTileClasses] == tiles.size());
    for (int c = 0; c < kTileClasses; c++) {
        CHECK(begin[c] <= begin[c + 1]);
        for (uint32_t t = begin[c]; t < begin[c + 1]; t++) {
            CHECK(tiles[t].n_bytes >= k);
            CHECK(class_of(tiles[t].n_bytes - k + 1) == c);    // within the cap, and no lower class
        }
    }
    return true;
}

// every k-mer start of every record >= k lies in exactly one main tile, of the record's group
static bool check_cover(const Case &c, const Records &R, const SketchPlan &P)
{
    std::vector<TileDesc> by_off = P.tiles;
    std::sort(by_off.begin(), by_off.end(),
              [](const TileDesc &a, const TileDesc &b) { return a.byte_off < b.byte_off; });
    // a tile's starts: [byte_off, byte_off + n_bytes - k]; the tiles' ranges are disjoint
    for (size_t t = 0; t + 1 < by_off.size(); t++)
        CHECK(by_off[t].byte_off + by_off[t].n_bytes - c.k < by_off[t + 1].byte_off);
    uint64_t n_kmers = 0, in_tiles = 0;
    for (uint32_t r : R.order) {
        if (R.len[r] < c.k) continue;
        const uint64_t lo = R.pos[r], hi = R.pos[r] + R.len[r] - c.k;   // the record's starts
        n_kmers += hi - lo + 1;
        uint64_t covered = 0;
        auto it = std::upper_bound(by_off.begin(), by_off.end(), lo,
                                   [](uint64_t v, const TileDesc &t) { return v < t.byte_off; });
        if (it != by_off.begin()) --it;
        for (; it != by_off.end() && it->byte_off <= hi; ++it) {
            const uint64_t a = std::max(lo, it->byte_off), b = std::min(hi, it->byte_off + it->n_bytes - c.k);
            if (a > b) continue;
            CHECK(it->pad == R.group[r]);
            covered += b - a + 1;
        }
        CHECK(covered == hi - lo + 1);
    }
    CHECK(P.n_kmers == n_kmers);
    // and no tile without a record of its group behind it
    std::vector<uint8_t> has(c.n_groups, 0);
    for (uint32_t r : R.order)
        if (R.len[r] >= c.k) has[R.group[r]] = 1;
    for (auto &t : P.tiles) {
        CHECK(t.pad < c.n_groups && has[t.pad]);
        in_tiles += t.n_bytes - c.k + 1;
    }
    CHECK(in_tiles >= n_kmers);   // (a packed tile also spans the starts between its records)
    return true;
}

static bool check_ranges(const Case &c, const SketchPlan &P)
{
    const uint32_t all_rows = P.n_rows + P.n_fb_rows;
    CHECK(P.n_groups == c.n_groups && P.n_rows >= P.n_groups && all_rows >= P.n_rows);
    CHECK(P.srow.size() == P.n_slots && P.sbound.size() == P.n_slots);
    for (auto &t : P.tiles) CHECK(t.out_row < P.n_rows && t.thr_slot <= P.n_slots);
    for (auto &t : P.stiles) {
        CHECK(t.out_row < P.n_rows);
        if (t.thr_slot) {
            CHECK(t.thr_slot > P.n_slots && t.thr_slot <= 2 * P.n_slots);
            CHECK(P.sbound[t.thr_slot - P.n_slots - 1] != ~0ULL);
        }
    }
    for (uint32_t r : P.srow) CHECK(r < P.n_rows);
    CHECK(!P.ssel_begin.empty() && P.ssel_begin.front() == 0 && !P.sel_begin.empty());
    CHECK(P.ssel_begin.back() == P.sel_begin.front() && P.sel_begin.back() == P.sel.size());
    CHECK(std::is_sorted(P.ssel_begin.begin(), P.ssel_begin.end()));
    CHECK(std::is_sorted(P.sel_begin.begin(), P.sel_begin.end()));
    CHECK(P.ssel_tag.size() == P.n_ssel());
    for (size_t i = 0; i < P.sel.size(); i++) {
        const SelDesc &d = P.sel[i];
        CHECK(d.out_row < P.n_rows && d.n_rows >= 1);
        CHECK((uint64_t)d.row_begin + d.n_rows <= P.sel_rows.size());
        if (i < P.n_ssel()) CHECK(d.slot == 0xFFFFFFFFu && P.ssel_tag[i] < P.n_slots);
        else CHECK(d.slot < P.n_slots);
    }
    for (uint32_t r : P.sel_rows) CHECK(r < P.n_rows);
    for (const MergeSchedule *m : {&P.merge, &P.smerge})
        for (auto &st : m->steps) CHECK(st.a < P.n_rows && st.b < P.n_rows && st.c < P.n_rows);
    for (const MergeSchedule *m : {&P.fmerge, &P.sfmerge})
        for (auto &st : m->steps) CHECK(st.a < all_rows && st.b < all_rows && st.c < all_rows);
    for (const MergeSchedule *m : {&P.merge, &P.smerge, &P.fmerge, &P.sfmerge}) {
        if (m->round_begin.empty()) { CHECK(m->steps.empty() && m->round_small.empty()); continue; }
        CHECK(m->round_begin.front() == 0 && m->round_begin.back() == m->steps.size());
        CHECK(std::is_sorted(m->round_begin.begin(), m->round_begin.end()));
        CHECK(m->round_small.size() == m->rounds());
    }
    return true;
}

// One pass over the rows as the run makes it: tiles, then the selections level by level, then
// the merges round by round.  A row is written once, read only after the stage that wrote it,
// and read once unless it is one of the pass's final rows, which are never read.
struct Pass {
    std::vector<int> wrote, reads;
    std::vector<uint32_t> leaves;    // the tile rows the selections / merges read
    int stage = 0;
    explicit Pass(uint32_t rows) : wrote(rows, -1), reads(rows, 0) {}
    bool write(uint32_t r)
    {
        CHECK(r < wrote.size() && wrote[r] < 0);
        wrote[r] = stage;
        return true;
    }
    bool read(uint32_t r)
    {
        CHECK(r < wrote.size() && wrote[r] >= 0 && wrote[r] < stage);
        if (wrote[r] == 0) leaves.push_back(r);
        reads[r]++;
        return true;
    }
    bool tiles(const std::vector<TileDesc> &ts)
    {
        for (auto &t : ts)
            if (!write(t.out_row)) return false;
        return true;
    }
    bool selections(const SketchPlan &P, const std::vector<uint32_t> &begin)
    {
        for (size_t l = 0; l + 1 < begin.size(); l++) {
            stage++;
            for (uint32_t i = begin[l]; i < begin[l + 1]; i++) {
                for (uint32_t j = 0; j < P.sel[i].n_rows; j++)
                    if (!read(P.sel_rows[P.sel[i].row_begin + j])) return false;
                if (!write(P.sel[i].out_row)) return false;
            }
        }
        return true;
    }
    bool merges(const MergeSchedule &m)
    {
        for (size_t r = 0; r < m.rounds(); r++) {
            stage++;
            for (uint32_t i = m.round_begin[r]; i < m.round_begin[r + 1]; i++)
                if (!read(m.steps[i].a) || !read(m.steps[i].b) || !write(m.steps[i].c)) return false;
        }
        return true;
    }
    // `finals`: the rows the pass must end in
    bool settled(const std::vector<uint32_t> &finals)
    {
        std::vector<uint8_t> is_final(wrote.size(), 0);
        for (uint32_t r : finals) {
            CHECK(r < wrote.size() && wrote[r] >= 0 && !is_final[r]);
            is_final[r] = 1;
        }
        for (size_t r = 0; r < wrote.size(); r++)
            if (wrote[r] >= 0) CHECK(reads[r] == (is_final[r] ? 0 : 1));
        std::sort(leaves.begin(), leaves.end());
        return true;
    }
};

static bool check_passes(const SketchPlan &P)
{
    const uint32_t all_rows = P.n_rows + P.n_fb_rows;
    std::vector<uint32_t> group_rows;                 // row g of each group that has tiles
    std::vector<uint8_t> has(P.n_groups, 0);
    for (auto &t : P.tiles) has[t.pad] = 1;
    for (uint32_t g = 0; g < P.n_groups; g++)
        if (has[g]) group_rows.push_back(g);
    // the passes as staged, and with the fallback merges in place of the selections
    Pass main(P.n_rows), sample(P.n_rows), fmain(all_rows), fsample(all_rows);
    CHECK(sample.tiles(P.stiles) && sample.selections(P, P.ssel_begin) && sample.merges(P.smerge));
    CHECK(main.tiles(P.tiles) && main.selections(P, P.sel_begin) && main.merges(P.merge));
    CHECK(fsample.tiles(P.stiles) && fsample.merges(P.sfmerge) && fsample.merges(P.smerge));
    CHECK(fmain.tiles(P.tiles) && fmain.merges(P.fmerge) && fmain.merges(P.merge));
    CHECK(sample.settled(P.srow) && main.settled(group_rows));
    CHECK(fsample.settled(P.srow) && fmain.settled(group_rows));
    // a fallback reads the leaf rows its selections read, and nothing of the core rows is
    // written by it but the selections' final rows
    CHECK(sample.leaves == fsample.leaves && main.leaves == fmain.leaves);
    for (const MergeSchedule *m : {&P.fmerge, &P.sfmerge}) {
        std::vector<uint32_t> ends, sel_ends;
        for (auto &st : m->steps)
            if (st.c < P.n_rows) ends.push_back(st.c);
        const std::vector<uint32_t> &lv = m == &P.fmerge ? P.sel_begin : P.ssel_begin;
        for (uint32_t i = lv[lv.size() - 1]; i-- > lv.front();) {
            const uint32_t r = P.sel[i].out_row;
            const bool final_row = m == &P.fmerge ? r < P.n_groups
                                                  : std::count(P.srow.begin(), P.srow.end(), r) > 0;
            if (final_row) sel_ends.push_back(r);
        }
        std::sort(ends.begin(), ends.end());
        std::sort(sel_ends.begin(), sel_ends.end());
        CHECK(ends == sel_ends);
    }
    return true;
}

static bool check_bounds(const Case &c, const SketchPlan &P)
{
    if (P.tight) {
        CHECK(P.kt.size() == P.n_slots && P.slot_group.size() == P.n_slots);
        for (uint32_t i = 0; i < P.n_slots; i++) CHECK(P.kt[i] >= 1 && P.kt[i] <= c.s);
        for (uint32_t i = 0; i < P.n_slots; i++) CHECK(P.slot_group[i] < P.n_groups);
        for (auto &t : P.tiles)
            if (t.thr_slot) CHECK(P.slot_group[t.thr_slot - 1] == t.pad);
    } else {
        CHECK(P.kt.empty() && P.slot_group.empty() && !P.sbounded);
    }
    CHECK(P.n4 == P.class_begin[5] - P.class_begin[4]);
    if (P.thr4)
        for (uint32_t t = P.class_begin[4]; t < P.class_begin[5]; t++) CHECK(P.tiles[t].thr_slot != 0);
    return true;
}

static bool plan_case(const Case &c, SketchPlan *P)
{
    g_case = c.name;
    const Records R = records_of(c);
    CHECK(plan_sketch(PlanRecords{R.order, R.pos, R.len, R.group, c.n_groups},
                      PlanParams{c.k, c.s, c.use64}, P));
    return check_classes(P->tiles, P->class_begin, c.k) &&
           check_classes(P->stiles, P->sclass_begin, c.k) && check_cover(c, R, *P) &&
           check_ranges(c, *P) && check_passes(*P) && check_bounds(c, *P);
}

// the levels of the main selections as descriptor row counts
static std::vector<std::vector<uint32_t>> main_levels(const SketchPlan &P)
{
    std::vector<std::vector<uint32_t>> lv;
    for (size_t l = 0; l + 1 < P.sel_begin.size(); l++) {
        lv.emplace_back();
        for (uint32_t i = P.sel_begin[l]; i < P.sel_begin[l + 1]; i++) lv.back().push_back(P.sel[i].n_rows);
    }
    return lv;
}

// (b) records of 99 bytes, on the device path three records shorter than k among them, and a
// last record sized so that the span from the first byte through it holds `starts` starts:
// the bytes of all records and their separators are starts + k
static Case packed_case(uint32_t starts, bool device)
{
    Case c{std::string("packed ") + (device ? "device " : "host ") + std::to_string(starts),
           21, 1000, true, device, {}, 0};
    const uint64_t shorts[3] = {0, 1, 20};
    uint64_t bytes = 0;
    for (int i = 0; i < 19; i++) {
        c.add(0, 99);
        bytes += 100;
        if (device && i < 3) { c.add(0, shorts[i]); bytes += shorts[i] + 1; }
    }
    c.add(0, starts + c.k - bytes - 1);
    return c;
}

static Case chunks_case(const char *what, uint32_t k, uint32_t s, uint32_t ntile)
{
    Case c{std::string(what) + " " + std::to_string(ntile) + " chunks s=" + std::to_string(s), k, s,
           k > 16, false, {}, 0};
    c.add(0, (uint64_t)ntile * kChunkKmers + k - 1);
    return c;
}

static bool run_checks()
{
    SketchPlan P;
    {   // (a) lengths k - 1, k, k + 1, an empty group, a group of records shorter than k
        Case c{"short records", 21, 1000, true, false, {}, 0};
        c.add(0, 20); c.add(1, 21); c.add(2, 22); c.n_groups = 4; c.add(4, 5); c.add(4, 20); c.add(4, 0);
        if (!plan_case(c, &P)) return false;
        CHECK(P.tiles.size() == 2 && P.n_kmers == 3 && P.n_rows == 5);
        c.name += " (device)";
        c.device = true;
        if (!plan_case(c, &P)) return false;
        CHECK(P.tiles.size() == 2 && P.n_rows == 5);
    }
    for (bool device : {false, true}) {   // (b) a packed tile closes at 2,048 starts, not at 2,049
        if (!plan_case(packed_case(kPackKmers, device), &P)) return false;
        CHECK(P.tiles.size() == 1 && P.tiles[0].n_bytes - 21 + 1 == kPackKmers);
        if (!plan_case(packed_case(kPackKmers + 1, device), &P)) return false;
        CHECK(P.tiles.size() == 2);
    }
    // (c) groups of 1, 2, 3 and 5 one-record tiles: the merge rounds' odd carries, either side
    // of the small-kernel cap (1,100-start tiles) and of the LDS merge cap (4,096-start tiles)
    for (uint32_t s : {2048u, 2049u, 16384u, 16385u}) {
        Case c{"merge groups s=" + std::to_string(s), 21, s, true, false, {}, 0};
        const uint64_t len = (s <= 2049 ? 1100 : kChunkKmers) + 20;
        uint32_t g = 0;
        for (uint32_t n : {1u, 2u, 3u, 5u}) c.add(g++, len, n);
        if (!plan_case(c, &P)) return false;
        CHECK(P.n_slots == 0 && P.sel.empty() && P.merge.rounds() == 3);   // 5 lists: 3 rounds
    }
    // (d) the sample rule's edge, the selection cap, the survivors-only kernel's least groups
    if (!plan_case(chunks_case("sample edge", 21, 1000, 31), &P)) return false;
    CHECK(P.n_slots == 0 && P.stiles.empty() && !P.thr4);
    if (!plan_case(chunks_case("sample edge", 21, 1000, 32), &P)) return false;
    CHECK(P.n_slots == 1 && P.stiles.size() == 2);
    if (!plan_case(chunks_case("selection cap", 21, 13597, 224), &P)) return false;
    CHECK(P.n_slots == 1 && P.n_sel() > 0 && P.n_ssel() > 0 && P.tight && P.merge.steps.empty());
    if (!plan_case(chunks_case("selection cap", 21, 13598, 224), &P)) return false;
    CHECK(P.n_slots == 1 && P.sel.empty() && !P.tight && P.fmerge.steps.empty() && !P.thr4);
    for (auto &ks : {std::make_pair(21u, 32u), std::make_pair(12u, 32u), std::make_pair(21u, 64u)}) {
        if (!plan_case(chunks_case("survivors", ks.first, 1000, ks.second), &P)) return false;
        CHECK(P.thr4 && P.tight && P.n4 == ks.second);
    }
    {   // (e) 4,097 rows: the main selection splits at 4,096 rows per workgroup
        if (!plan_case(chunks_case("row split", 21, 1000, (uint32_t)kRowsPerWG + 1), &P)) return false;
        const auto lv = main_levels(P);
        CHECK(lv.size() == 2 && lv[0] == (std::vector<uint32_t>{(uint32_t)kRowsPerWG, 1}));
        CHECK(lv[1] == std::vector<uint32_t>{2});
    }
    {   // (f) 2,000 chunks at s = 13,597: a sampled group's tile is estimated to keep
        // 2 every s / tiles + 64 hashes, every = 64 from 1,700 tiles on at this s, so 2 * 64 *
        // 13,597 / 2,000 + 64 = 934 per row, and 2^19 / 934 = 561 rows reach the key limit
        // long before 4,096 rows: chunks of 561, 561, 561 and 317 rows, then one selection
        if (!plan_case(chunks_case("key split", 21, 13597, 2000), &P)) return false;
        const auto lv = main_levels(P);
        CHECK(lv.size() == 2 && lv[0] == (std::vector<uint32_t>{561, 561, 561, 317}));
        CHECK(lv[1] == std::vector<uint32_t>{4});
    }
    {   // (g) no group at all, and groups without a record
        Case c{"no groups", 21, 1000, true, false, {}, 0};
        if (!plan_case(c, &P)) return false;
        CHECK(P.n_rows == 0 && P.tiles.empty() && P.merge.rounds() == 0);
        c.name = "empty groups";
        c.n_groups = 3;
        if (!plan_case(c, &P)) return false;
        CHECK(P.n_rows == 3 && P.tiles.empty());
    }
    return true;
}

// per slot its sample rate, read off the plan: the position of the sample's second tile among
// the group's tiles (a sampled group has at least two sample tiles)
static std::vector<uint32_t> every_of(const SketchPlan &P)
{
    std::map<uint32_t, std::vector<uint64_t>> main_off, sample_off;
    for (auto &t : P.tiles) main_off[t.pad].push_back(t.byte_off);
    for (auto &t : P.stiles) sample_off[t.pad].push_back(t.byte_off);
    std::map<uint32_t, uint32_t> slot_of_group;
    for (auto &t : P.tiles)
        if (t.thr_slot) slot_of_group[t.pad] = t.thr_slot - 1;
    std::vector<uint32_t> every(P.n_slots, 0);
    for (auto &kv : slot_of_group) {
        auto &m = main_off[kv.first], &sm = sample_off[kv.first];
        std::sort(m.begin(), m.end());
        std::sort(sm.begin(), sm.end());
        if (sm.size() >= 2) every[kv.second] = (uint32_t)(std::find(m.begin(), m.end(), sm[1]) - m.begin());
    }
    return every;
}

static void print_list(const char *key, const std::vector<uint32_t> &v, const char *end = ", ")
{
    printf("\"%s\": [", key);
    for (size_t i = 0; i < v.size(); i++) printf("%s%u", i ? ", " : "", v[i]);
    printf("]%s", end);
}

static int print_plan(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: sketchplan_check K S USE64 host|device GROUP:LENGTH ...\n");
        return 2;
    }
    Case c{"arguments", (uint32_t)atoi(argv[1]), (uint32_t)atoi(argv[2]), atoi(argv[3]) != 0,
           !strcmp(argv[4], "device"), {}, 0};
    for (int i = 5; i < argc; i++) {
        unsigned g = 0;
        unsigned long long len = 0;
        if (sscanf(argv[i], "%u:%llu", &g, &len) != 2) {
            fprintf(stderr, "sketchplan_check: bad record %s\n", argv[i]);
            return 2;
        }
        c.add(g, len);
    }
    SketchPlan P;
    if (!plan_case(c, &P)) return 1;
    std::vector<uint32_t> n(kTileClasses), sn(kTileClasses);
    for (int cl = 0; cl < kTileClasses; cl++) {
        n[cl] = P.class_begin[cl + 1] - P.class_begin[cl];
        sn[cl] = P.sclass_begin[cl + 1] - P.sclass_begin[cl];
    }
    printf("{");
    print_list("tiles", n);
    print_list("sample_tiles", sn);
    printf("\"n_slots\": %u, ", P.n_slots);
    print_list("every", every_of(P));
    print_list("kt", P.kt);
    printf("\"thr4\": %d, \"tight\": %d, \"n_sel\": %u, \"n_ssel\": %u, ", P.thr4, P.tight, P.n_sel(),
           P.n_ssel());
    const char *names[4] = {"main", "sample", "fallback", "sample_fallback"};
    const MergeSchedule *ms[4] = {&P.merge, &P.smerge, &P.fmerge, &P.sfmerge};
    printf("\"rounds_small\": {");
    for (int i = 0; i < 4; i++)
        print_list(names[i], std::vector<uint32_t>(ms[i]->round_small.begin(), ms[i]->round_small.end()),
                   i < 3 ? ", " : "");
    printf("}}\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return print_plan(argc, argv);
    if (!run_checks()) return 1;
    printf("sketchplan ok\n");
    return 0;
}
