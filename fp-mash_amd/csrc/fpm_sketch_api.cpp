// fpm_sketch_api.cpp — the sketch part of the C ABI declared in include/fpmash.h: host-side
// staging (record packing, the plan of sketch_plan.cpp, its upload), the run and its redo /
// fallback passes, the device min-merge and the -M pass, over the kernels in sketch.hip.
#include "fpm_internal.hpp"
#include "sketch_plan.hpp"

#include <cstdlib>

namespace {

// Reference complement table for 'A'..'Z' (Sketch.cpp:1223-1250); other bytes 'N'.
const char kComplAZ[26] = {'T', 'V', 'G', 'H', 'N', 'N', 'C', 'D', 'N', 'N', 'M', 'N', 'K',
                           'N', 'N', 'N', 'N', 'Y', 'S', 'A', 'A', 'B', 'W', 'N', 'R', 'N'};
}  // namespace

// merge rounds whose estimated input lists are at most kMergeSmallCap long use
// merge_small_kernel; FPM_MERGE_SMALL=0 turns it off (A/B), =2 uses it for every round
// (tests: its global-memory search past the LDS cap)
static const int g_merge_small_env = [] {
    const char *v = getenv("FPM_MERGE_SMALL");
    return v ? atoi(v) : 1;
}();

// whether round r of a schedule runs through merge_small_kernel
static bool round_is_small(const MergeSchedule &m, size_t r)
{
    return g_merge_small_env == 2 ||
           (g_merge_small_env != 0 && r < m.round_small.size() && m.round_small[r]);
}

// ----------------------------------------------------------------------------
// Sketch job: packing + tile plan + merge schedule
// ----------------------------------------------------------------------------
// Rows of one device matrix d_rows[n_rows][s]: rows [0, n_groups) are the final
// sketches, rows >= n_groups hold per-tile / intermediate lists of groups whose
// records span several tiles; those are reduced by selections and pairwise merge rounds
// (sketch_plan.hpp states which row is whose).

struct fpm_sketch_job {
    fpm_ctx *ctx = nullptr;
    SketchKParams kp{};
    SketchPlan plan;               // what the device buffers below were filled from
    uint64_t seq_bytes = 0;
    uint8_t *d_seq = nullptr;
    TileDesc *d_tiles = nullptr;   // plan.tiles
    uint64_t *d_rows = nullptr;
    uint32_t *d_count = nullptr;
    MergeDesc *d_merge = nullptr;  // plan.merge
    // long groups' sample pass: plan.stiles, plan.smerge, plan.srow; d_thr: the groups' bounds
    // (main pass), then the samples' a-priori bounds
    TileDesc *d_stiles = nullptr;
    MergeDesc *d_smerge = nullptr;
    uint32_t *d_srow = nullptr;
    uint64_t *d_thr = nullptr;
    // sampled groups' selections (plan.sel, plan.sel_rows); the fallback merges of plan.fmerge /
    // plan.sfmerge for groups whose keys below the cut do not fit in LDS, their descriptors and
    // rows (>= plan.n_rows: d_fb_rows) allocated on first use
    SelDesc *d_sel = nullptr;
    uint32_t *d_sel_rows = nullptr, *d_sel_failed = nullptr, *h_sel_failed = nullptr;
    MergeDesc *d_fmerge = nullptr, *d_sfmerge = nullptr;
    uint64_t *d_fb_rows = nullptr;
    uint32_t *d_fb_count = nullptr;
    // plan.thr4: the survivors-only tile kernel, whose overflowing tiles (d_redo, count
    // d_redo_n) run again through the plain one
    TileDesc *d_redo = nullptr;
    uint32_t *d_redo_n = nullptr;
    // plan.tight: each slot's bound is the sample's kt-th smallest hash instead of its s-th
    // (d_kt), the s-th kept as d_thr_safe; a group left with fewer than s hashes
    // (sketch_short_kernel: d_short = count, then the slots) is redone with the safe bound: its
    // tiles and selections again, from the plan
    uint32_t *d_kt = nullptr, *d_slot_group = nullptr, *d_short = nullptr;
    uint64_t *d_thr_safe = nullptr;
    TileDesc *d_rtiles = nullptr;           // the redo's subsets (allocated on first use)
    SelDesc *d_rsel = nullptr;
    int32_t last_short = -1;                // groups redone by the last run (-1: no tight bounds)
    // plan.sbounded (a-priori sample bounds, d_thr[n_slots ..]): a sample left short is redone
    // unbounded
    uint32_t *d_sshort = nullptr;           // count, then the slots
    uint64_t *d_sbound0 = nullptr;          // the a-priori sample bounds as staged: restored
                                            // into d_thr at every run (a short sample's redo
                                            // lifts its bound in d_thr)
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
    fpm_sketch_plan reads_plan{};           // that wide job's plan and width (reads_width 0: no
    uint32_t reads_width = 0;               // round yet), kept past the wide job's life
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
    *out = JobView{j->ctx, j->kp, j->plan.n_groups, j->d_seq, j->d_tiles, j->plan.class_begin,
                   j->d_rows, j->d_count};
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

static SketchKParams kernel_params(const fpm_sketch_params *p)
{
    SketchKParams kp{};
    kp.k = p->kmer_size; kp.s = p->sketch_size; kp.seed = p->seed; kp.use64 = p->use64 ? 1 : 0;
    kp.canonical = p->noncanonical ? 0 : 1; kp.preserve_case = p->preserve_case ? 1 : 0;
    for (int c = 0; c < 256; c++) {
        kp.alphabet[c] = p->alphabet[c] ? 1 : 0;
        kp.complement[c] = (c >= 'A' && c <= 'Z') ? (uint8_t)kComplAZ[c - 'A'] : (uint8_t)'N';
    }
    kp.alphabet[0] = 0;   // the separator byte is never a k-mer byte
    kp.compl_acgt = 1;
    for (int c = 0; c < 256; c++)
        if (kp.alphabet[c] && c != 'A' && c != 'C' && c != 'G' && c != 'T') kp.compl_acgt = 0;
    return kp;
}

// host path: the records >= k (each followed by 0x00) packed in group order; R.pos becomes
// each packed record's offset
static std::vector<uint8_t> pack_records(StageRecords &R, uint32_t k)
{
    uint64_t total = 0;
    for (uint32_t r : R.order)
        if (R.len[r] >= k) total += R.len[r] + 1;
    std::vector<uint8_t> packed(total);
    uint64_t at = 0;
    for (uint32_t r : R.order) {
        if (R.len[r] < k) continue;
        memcpy(packed.data() + at, R.host_seq + R.pos[r], R.len[r]);
        packed[at + R.len[r]] = 0;
        R.pos[r] = at;
        at += R.len[r] + 1;
    }
    return packed;
}

// merge steps as descriptors; row(r) / count(r): where row r and its count live
template <typename Row, typename Count>
static std::vector<MergeDesc> merge_descs(const std::vector<MergeStep> &steps, Row row, Count count)
{
    std::vector<MergeDesc> md(steps.size());
    for (size_t i = 0; i < steps.size(); i++)
        md[i] = MergeDesc{row(steps[i].a), count(steps[i].a), row(steps[i].b), count(steps[i].b),
                          row(steps[i].c), count(steps[i].c)};
    return md;
}

// the device buffers job->plan asks for
static hipError_t alloc_plan(fpm_sketch_job *job, const StageRecords &R, size_t packed_bytes)
{
    const SketchPlan &P = job->plan;
    const size_t s = job->kp.s, n_slots = P.n_slots;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto **ptr, size_t bytes) {
        if (e == hipSuccess) e = job->mem.get(ptr, bytes);
    };
    if (R.host_seq) alloc(&job->d_seq, packed_bytes + 64);
    else job->d_seq = R.d_seq;   // the parse's packed records, or borrowed (adopted after upload)
    alloc(&job->d_tiles, P.tiles.size() * sizeof(TileDesc));
    alloc(&job->d_rows, (size_t)P.n_rows * s * sizeof(uint64_t));
    alloc(&job->d_count, (size_t)P.n_rows * sizeof(uint32_t));
    // groups without any k-mer keep count 0: zeroed once here (every run rewrites the count
    // of each group that has tiles: the tile kernel or the last merge of its group)
    if (e == hipSuccess)
        e = memset_sync(job->ctx, job->d_count, 0, (size_t)P.n_rows * sizeof(uint32_t));
    alloc(&job->d_merge, P.merge.steps.size() * sizeof(MergeDesc));
    alloc(&job->d_stiles, P.stiles.size() * sizeof(TileDesc));
    alloc(&job->d_smerge, P.smerge.steps.size() * sizeof(MergeDesc));
    alloc(&job->d_srow, n_slots * sizeof(uint32_t));
    alloc(&job->d_thr, 2 * n_slots * sizeof(uint64_t));   // main, then sample bounds
    alloc(&job->d_sel, P.sel.size() * sizeof(SelDesc));
    alloc(&job->d_sel_rows, P.sel_rows.size() * sizeof(uint32_t));
    alloc(&job->d_sel_failed, (P.sel.size() + 2) * sizeof(uint32_t));
    if (e == hipSuccess && !P.sel.empty())
        e = hipHostMalloc((void **)&job->h_sel_failed, 3 * sizeof(uint32_t), hipHostMallocDefault);
    if (P.tight) {
        alloc(&job->d_kt, n_slots * sizeof(uint32_t));
        alloc(&job->d_slot_group, n_slots * sizeof(uint32_t));
        alloc(&job->d_short, (n_slots + 1) * sizeof(uint32_t));
        alloc(&job->d_thr_safe, n_slots * sizeof(uint64_t));
        job->last_short = 0;
    }
    if (P.sbounded) {
        alloc(&job->d_sshort, (n_slots + 1) * sizeof(uint32_t));
        alloc(&job->d_sbound0, n_slots * sizeof(uint64_t));
        job->last_sample_short = 0;
    }
    if (P.thr4) {
        alloc(&job->d_redo, (size_t)P.n4 * sizeof(TileDesc));
        alloc(&job->d_redo_n, sizeof(uint32_t));
    }
    return e;
}

// job->plan and the packed records (host path) into the buffers of alloc_plan
static hipError_t copy_plan(fpm_sketch_job *job, const std::vector<uint8_t> &packed)
{
    const SketchPlan &P = job->plan;
    fpm_ctx *ctx = job->ctx;
    const uint64_t s = job->kp.s;
    auto row = [&](uint32_t r) { return job->d_rows + r * s; };
    auto cnt = [&](uint32_t r) { return job->d_count + r; };
    hipError_t e = hipSuccess;
    if (!packed.empty()) e = h2d_staged(ctx, job->d_seq, packed.data(), packed.size());
    auto put = [&](void *dst, const auto &v) {      // (an empty vector copies nothing)
        if (e == hipSuccess) e = copy_in(ctx, dst, v.data(), v.size() * sizeof(v[0]));
    };
    put(job->d_tiles, P.tiles);
    put(job->d_merge, merge_descs(P.merge.steps, row, cnt));
    put(job->d_stiles, P.stiles);
    put(job->d_smerge, merge_descs(P.smerge.steps, row, cnt));
    put(job->d_srow, P.srow);
    put(job->d_sel, P.sel);
    put(job->d_sel_rows, P.sel_rows);
    put(job->d_thr + P.n_slots, P.sbound);
    if (job->d_sbound0) put(job->d_sbound0, P.sbound);
    put(job->d_kt, P.kt);
    put(job->d_slot_group, P.slot_group);
    return e;
}

static int upload_plan(fpm_sketch_job *job, const StageRecords &R, const std::vector<uint8_t> &packed)
{
    hipError_t e = alloc_plan(job, R, packed.size());
    if (e != hipSuccess)
        return fail(FPM_ENOMEM, std::string("sketch staging alloc: ") + hipGetErrorString(e));
    e = copy_plan(job, packed);
    if (e != hipSuccess)
        return fail(FPM_EHIP, std::string("sketch staging copy: ") + hipGetErrorString(e));
    if (!R.host_seq && !R.borrow) job->mem.adopt(R.d_seq);
    return FPM_OK;
}

// parameters, pack, plan (sketch_plan.cpp), allocate and upload
int stage_core(fpm_ctx *ctx, const fpm_sketch_params *p, StageRecords &R,
               fpm_sketch_job **job_out)
{
    if (p->kmer_size < 1 || p->kmer_size > 32) return fail(FPM_EINVAL, "kmer_size must be 1..32");
    if (p->sketch_size < 1) return fail(FPM_EINVAL, "sketch_size must be >= 1");
    const SketchKParams kp = kernel_params(p);
    std::vector<uint8_t> packed;
    if (R.host_seq) packed = pack_records(R, kp.k);
    SketchPlan plan;
    if (!plan_sketch(PlanRecords{R.order, R.pos, R.len, R.group, R.n_groups},
                     PlanParams{kp.k, kp.s, kp.use64 != 0}, &plan))
        return fail(FPM_EINVAL, "internal: tile exceeds capacity");
    auto *job = new fpm_sketch_job();
    job->ctx = job->mem.ctx = ctx;
    job->kp = kp;
    job->plan = std::move(plan);
    job->seq_bytes = R.host_seq ? packed.size() : R.d_seq_bytes;
    if (int rc = upload_plan(job, R, packed)) {
        job_release(job);
        delete job;
        return rc;
    }
    // kept for reads mode's widening rounds (moved, not copied: the callers are done with them)
    job->params = *p;
    job->recs.n_groups = R.n_groups;
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
    const SketchPlan &P = job->plan;
    const uint64_t s = job->kp.s;
    if (P.n_fb_rows) {
        HIP_TRY(job->mem.get(&job->d_fb_rows, (size_t)P.n_fb_rows * s * sizeof(uint64_t)));
        HIP_TRY(job->mem.get(&job->d_fb_count, (size_t)P.n_fb_rows * sizeof(uint32_t)));
    }
    auto row = [&](uint32_t r) { return r < P.n_rows ? job->d_rows + r * s
                                                     : job->d_fb_rows + (r - P.n_rows) * s; };
    auto cnt = [&](uint32_t r) { return r < P.n_rows ? job->d_count + r
                                                     : job->d_fb_count + (r - P.n_rows); };
    const std::vector<MergeDesc> md = merge_descs(P.fmerge.steps, row, cnt),
                                 smd = merge_descs(P.sfmerge.steps, row, cnt);
    HIP_TRY(job->mem.upload(job->ctx, &job->d_fmerge, md.data(), md.size() * sizeof(MergeDesc)));
    HIP_TRY(job->mem.upload(job->ctx, &job->d_sfmerge, smd.data(), smd.size() * sizeof(MergeDesc)));
    return FPM_OK;
}

// device room for a redo's tile and selection subsets (allocated on first use)
static int redo_buffers(fpm_sketch_job *job)
{
    const SketchPlan &P = job->plan;
    if (!job->d_rtiles)
        HIP_TRY(job->mem.get(&job->d_rtiles,
                             std::max(P.tiles.size(), P.stiles.size()) * sizeof(TileDesc)));
    if (!job->d_rsel) HIP_TRY(job->mem.get(&job->d_rsel, P.sel.size() * sizeof(SelDesc)));
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

// the tile kernels over d_t, a tile array ordered by class; `main`: the main pass, whose class-4
// tiles take the survivors-only kernel when the plan says so
static int tiles_pass(fpm_sketch_job *job, const TileDesc *d_t, const uint32_t *begin, bool main,
                      hipStream_t st)
{
    return for_each_class(begin, [&](int c, uint32_t b, uint32_t n) -> int {
        TimedLaunch tl(job->ctx, FPM_K_SKETCH, st);
        if (main && c == 4 && job->plan.thr4) {
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
        return FPM_OK;
    });
}

// one launch per round of a merge schedule over its descriptors d_m
static int merge_pass(fpm_sketch_job *job, const MergeDesc *d_m, const MergeSchedule &m,
                      hipStream_t st)
{
    for (size_t r = 0; r < m.rounds(); r++) {
        const uint32_t b = m.round_begin[r], n = m.round_begin[r + 1] - b;
        TimedLaunch tl(job->ctx, FPM_K_MERGE, st);
        HIP_TRY(launch_merge(d_m + b, n, job->kp.s, round_is_small(m, r), st));
        tl.done();
    }
    return FPM_OK;
}

// The groups a bound left short, their tiles and selections once more.  Main pass: the tight
// bound (slots in d_short[1 ..], bounds already raised to the safe ones by
// sketch_short_kernel).  Sample pass: the a-priori bound (slots in d_sshort[1 ..], bounds
// lifted by sketch_sample_short_kernel), the sample tiles and sample selections.
static int redo_short(fpm_sketch_job *job, bool sample, uint32_t n_short, hipStream_t st)
{
    fpm_ctx *ctx = job->ctx;
    const SketchPlan &P = job->plan;
    std::vector<uint32_t> slots(n_short);
    HIP_TRY(hipMemcpyAsync(slots.data(), (sample ? job->d_sshort : job->d_short) + 1,
                           n_short * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint8_t> is_short(P.n_slots + 1, 0);
    for (uint32_t i : slots)
        if (i < P.n_slots) is_short[i] = 1;
    // a main tile carries slot + 1 (0: none), a bounded sample tile n_slots + slot + 1
    const uint32_t *cb = sample ? P.sclass_begin : P.class_begin;
    const std::vector<TileDesc> &tiles = sample ? P.stiles : P.tiles;
    const uint32_t base = sample ? P.n_slots : 0;
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
    const std::vector<uint32_t> &lv = sample ? P.ssel_begin : P.sel_begin;
    std::vector<SelDesc> rsel;
    std::vector<uint32_t> rbegin{0};
    for (size_t l = 0; l + 1 < lv.size(); l++) {
        for (uint32_t i = lv[l]; i < lv[l + 1]; i++) {
            const uint32_t slot = !sample ? P.sel[i].slot
                                  : i < P.ssel_tag.size() ? P.ssel_tag[i] : UINT32_MAX;
            if (slot < P.n_slots && is_short[slot]) rsel.push_back(P.sel[i]);
        }
        rbegin.push_back((uint32_t)rsel.size());
    }
    if (int rc = redo_buffers(job)) return rc;
    if (!sub.empty()) HIP_TRY(copy_in(ctx, job->d_rtiles, sub.data(), sub.size() * sizeof(TileDesc)));
    if (!rsel.empty()) HIP_TRY(copy_in(ctx, job->d_rsel, rsel.data(), rsel.size() * sizeof(SelDesc)));
    if (int rc = tiles_pass(job, job->d_rtiles, begin, !sample, st)) return rc;
    return select_levels(job, job->d_rsel, rbegin, job->d_sel_failed + (sample ? 1 : 0), st);
}

extern "C" {

int fpm_sketch_run(fpm_sketch_job *job, void *stream)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    const SketchPlan &P = job->plan;
    // failure flags: [0] main selections, [1] sample selections, [2..] per selection
    uint32_t *fail_main = job->d_sel_failed, *fail_samp = job->d_sel_failed + 1;
    // a selection that did not fit (more repeated values below the cut than LDS holds):
    // the pairwise merges of every sampled group's lists (rare; one host round trip)
    auto fallback = [&](bool sample) -> int {
        if (int rc = fallback_descs(job)) return rc;
        return sample ? merge_pass(job, job->d_sfmerge, P.sfmerge, st)
                      : merge_pass(job, job->d_fmerge, P.fmerge, st);
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
        if (int rc = redo_short(job, sample, n_short, st)) return rc;
        HIP_TRY(hipMemcpyAsync(h_fail, d_fail, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return *h_fail ? fallback(sample) : FPM_OK;
    };
    if (!P.sel.empty())
        HIP_TRY(hipMemsetAsync(job->d_sel_failed, 0, (P.sel.size() + 2) * sizeof(uint32_t), st));
    if (P.n_slots) {   // sample pass of long groups -> per-group hash bounds
        if (P.sbounded)   // the bounds as staged (a previous run's redo lifted some)
            HIP_TRY(hipMemcpyAsync(job->d_thr + P.n_slots, job->d_sbound0,
                                   P.n_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        if (int rc = tiles_pass(job, job->d_stiles, P.sclass_begin, false, st)) return rc;
        if (P.n_ssel()) {
            if (int rc = select_levels(job, job->d_sel, P.ssel_begin, fail_samp, st)) return rc;
            HIP_TRY(hipMemcpyAsync(job->h_sel_failed + 1, fail_samp, sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, st));
        }
        if (int rc = merge_pass(job, job->d_smerge, P.smerge, st)) return rc;
        if (P.n_ssel()) {
            // samples their a-priori bound left short: redone unbounded
            auto list_sample_short = [&](bool raise) -> int {
                HIP_TRY(hipMemsetAsync(job->d_sshort, 0, sizeof(uint32_t), st));
                HIP_TRY(launch_sketch_sample_short(job->d_srow, P.n_slots, job->d_count, job->kp.s,
                                                   job->d_thr + P.n_slots, job->d_sshort,
                                                   job->d_sshort + 1, raise, st));
                HIP_TRY(hipMemcpyAsync(job->h_sel_failed + 2, job->d_sshort, sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, st));
                return FPM_OK;
            };
            if (int rc = settle(true, P.sbounded, list_sample_short, job->last_sample_short))
                return rc;
        }
        HIP_TRY(launch_sketch_threshold(job->d_srow, P.n_slots, job->d_rows, job->d_count,
                                        job->kp.s, P.tight ? job->d_kt : nullptr, job->d_thr,
                                        P.tight ? job->d_thr_safe : nullptr, st));
    }
    // (the selections of each batch of genomes on a side stream beside the next batch's
    // tiles measured a wash on C5: the 120 KB-LDS selection workgroups take the tiles' CUs)
    if (int rc = tiles_pass(job, job->d_tiles, P.class_begin, true, st)) return rc;
    if (P.n_sel()) {
        if (int rc = select_levels(job, job->d_sel, P.sel_begin, fail_main, st)) return rc;
        HIP_TRY(hipMemcpyAsync(job->h_sel_failed, fail_main, sizeof(uint32_t),
                               hipMemcpyDeviceToHost, st));
    }
    if (int rc = merge_pass(job, job->d_merge, P.merge, st)) return rc;
    if (P.n_sel()) {
        // the groups the tight bound left short: redone under the safe bound
        auto list_short = [&](bool raise) -> int {
            HIP_TRY(hipMemsetAsync(job->d_short, 0, sizeof(uint32_t), st));
            HIP_TRY(launch_sketch_short(job->d_slot_group, P.n_slots, job->d_count, job->kp.s,
                                        job->d_thr, job->d_thr_safe, job->d_short, job->d_short + 1,
                                        raise, st));
            HIP_TRY(hipMemcpyAsync(job->h_sel_failed + 2, job->d_short, sizeof(uint32_t),
                                   hipMemcpyDeviceToHost, st));
            return FPM_OK;
        };
        return settle(false, P.tight && P.n_slots, list_short, job->last_short);
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
    *n_short = job->plan.sbounded ? job->last_sample_short : -1;
    return FPM_OK;
}

int fpm_sketch_job_plan(fpm_sketch_job *job, fpm_sketch_plan *out)
{
    if (!job || !out) return fail(FPM_EINVAL, "null argument");
    static_assert(FPM_TILE_CLASSES == kTileClasses, "fpmash.h states the tile classes");
    *out = fpm_sketch_plan{};
    for (int c = 0; c < kTileClasses; c++) {
        out->tiles[c] = job->plan.class_begin[c + 1] - job->plan.class_begin[c];
        out->sample_tiles[c] = job->plan.sclass_begin[c + 1] - job->plan.sclass_begin[c];
    }
    out->thr4 = job->plan.thr4 ? 1 : 0;
    out->n_slots = job->plan.n_slots;
    out->tight = job->plan.tight ? 1 : 0;
    out->n_ssel = job->plan.n_ssel();
    out->n_sel = job->plan.n_sel();
    // as merge_pass (fpm_sketch_run) routes each round
    auto rounds = [](const MergeSchedule &m, uint32_t *n, uint32_t *n_small) {
        *n = (uint32_t)m.rounds();
        for (size_t r = 0; r < *n; r++)
            if (round_is_small(m, r)) ++*n_small;
    };
    rounds(job->plan.merge, &out->rounds, &out->rounds_small);
    rounds(job->plan.smerge, &out->sample_rounds, &out->sample_rounds_small);
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
    if (n_groups) *n_groups = job->plan.n_groups;
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
    if (out_hashes && job->plan.n_groups)
        HIP_TRY(d2h_staged(ctx, out_hashes, job->d_rows,
                           (size_t)job->plan.n_groups * job->kp.s * sizeof(uint64_t)));
    if (out_count && job->plan.n_groups)
        HIP_TRY(copy_out(ctx, out_count, job->d_count, (size_t)job->plan.n_groups * sizeof(uint32_t)));
    return FPM_OK;
}

int fpm_sketch_mult(fpm_sketch_job *job, void *stream, uint32_t *out_mult)
{
    if (!job) return fail(FPM_EINVAL, "null job");
    fpm_ctx *ctx = job->ctx;
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    const uint64_t s = job->kp.s, ng = job->plan.n_groups;
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
            HIP_TRY(launch_mult_ttop(job->d_count, job->plan.n_groups, job->kp.s, job->d_first,
                                     job->d_ttop, st));
        const uint32_t *cb = job->plan.class_begin;
        const int rc = for_each_class(cb, [&](int c, uint32_t b, uint32_t n) -> int {
            TimedLaunch tl(ctx, FPM_K_SKETCH, st);
            HIP_TRY(launch_sketch_mult(c, pass, job->d_seq, job->d_tiles + b, n, job->kp,
                                       job->d_rows, job->d_count, job->d_mult, job->d_first,
                                       job->d_ttop, st));
            tl.done();
            return FPM_OK;
        });
        if (rc) return rc;
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
    if (n_tiles) *n_tiles = job->plan.tiles.size();
    if (n_kmers) *n_kmers = job->plan.n_kmers;
    return FPM_OK;
}

int fpm_sketch_job_redo_tiles(fpm_sketch_job *job, int32_t *n_redo)
{
    if (!job || !n_redo) return fail(FPM_EINVAL, "null argument");
    *n_redo = -1;
    if (!job->plan.thr4 || !job->d_redo_n) return FPM_OK;
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
    const uint32_t m = job->min_copies, s = job->kp.s, S = wide->kp.s, ng = job->plan.n_groups;
    // for fpm_sketch_job_reads_plan: the caller frees a staged wide job after the round
    if (int rc = fpm_sketch_job_plan(wide, &job->reads_plan)) return rc;
    job->reads_width = S;
    if (int rc = fpm_sketch_run(wide, st)) return rc;
    job->reads_sampled = (int32_t)wide->plan.n_slots;
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
        const uint32_t *cb = wide->plan.class_begin;
        if (int rc = for_each_class(cb, [&](int c, uint32_t b, uint32_t n) -> int {
                TimedLaunch tl(ctx, FPM_K_SKETCH, st);
                HIP_TRY(launch_reads_count(c, wide->d_seq, wide->d_tiles + b, n, wide->kp,
                                           wide->d_rows, wide->d_count, m, d_wcnt, d_slots, st));
                tl.done();
                return FPM_OK;
            }))
            return rc;
        HIP_TRY(launch_reads_filter(wide->d_rows, wide->d_count, S, ng, d_wcnt, d_slots, m, s, round,
                                    job->d_rdone, job->d_rrows, job->d_rcount, job->d_rmult,
                                    job->d_rttop, st));
        if (int rc = for_each_class(cb, [&](int c, uint32_t b, uint32_t n) -> int {
                TimedLaunch tl(ctx, FPM_K_SKETCH, st);
                HIP_TRY(launch_reads_maxcount(c, wide->d_seq, wide->d_tiles + b, n, wide->kp, s,
                                              round, job->d_rdone, job->d_rrows, job->d_rcount,
                                              job->d_rmult, job->d_rttop, st));
                tl.done();
                return FPM_OK;
            }))
            return rc;
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
    const uint64_t s = job->kp.s, ng = job->plan.n_groups;
    job->reads_rounds = 0;
    if (!ng) return FPM_OK;
    if (!job->d_rrows) {
        // all five or none: a later run must not find some of them missing
        DevBufs out(ctx);
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
            R.n_groups = job->plan.n_groups;
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
    const size_t s = job->kp.s, ng = job->plan.n_groups;
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
        for (uint32_t g = 0; g < job->plan.n_groups; g++) group_round[g] = job->h_rdone[g];
    return FPM_OK;
}

int fpm_sketch_job_reads_sampled(fpm_sketch_job *job, int32_t *n_sampled)
{
    if (!job || !n_sampled) return fail(FPM_EINVAL, "null argument");
    *n_sampled = job->reads_rounds < 0 ? -1 : job->reads_sampled;
    return FPM_OK;
}

int fpm_sketch_job_reads_plan(fpm_sketch_job *job, fpm_sketch_plan *out, uint32_t *width)
{
    if (!job || !out || !width) return fail(FPM_EINVAL, "null argument");
    if (!job->reads_width) return fail(FPM_EINVAL, "reads_plan before a reads_run round");
    *out = job->reads_plan;
    *width = job->reads_width;
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
