// fpm_internal.hpp — what the files implementing the C ABI of include/fpmash.h share:
// the context, its pool / ring / copy helpers, the device scratch slots, the counter block and
// DevBufs, the owner of device buffers.  fpm_ctx.cpp and fpm_devmem.cpp define the helpers;
// fpm_sketch_api.cpp, fpm_text_api.cpp, fpm_dist_api.cpp, fpm_contain_api.cpp,
// fpm_screen_api.cpp, fpm_kfinger_api.cpp and fpm_comm.cpp use them.  Nothing declared here is
// exported from the library.
#pragma once

#include "fpm_kernels.hpp"
#include "../../include/fpmash.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

using namespace fpm;

#define FPM_HIDDEN __attribute__((visibility("hidden")))

// sets the text fpm_last_error() returns (one error text for the whole ABI); returns `code`
FPM_HIDDEN int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(FPM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

// Host memcpy split over a few persistent threads: the pinned ring's copies of pageable caller
// memory ran at one thread's ~8 GB/s, below the DMA behind them (C3's 301 MB of -fp text:
// ~40 ms of the parse wall).  Parts of >= 1 MB; the caller copies the first part itself.
class CopyPool {
  public:
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    void copy(void *dst, const void *src, size_t n)
    {
        constexpr size_t kPart = size_t(1) << 20;
        const unsigned want = (unsigned)std::min<size_t>(kMaxThreads + 1, n / kPart);
        if (want <= 1) { memcpy(dst, src, n); return; }
        std::unique_lock<std::mutex> lk(mu_);
        while (th_.size() + 1 < want && th_.size() < threads()) {
            // (at the process's thread limit: fewer parts, never an exception through the C ABI)
            try {
                th_.emplace_back([this] { work(); });
            } catch (const std::system_error &) {
                break;
            }
        }
        const unsigned parts = (unsigned)std::min<size_t>(want, th_.size() + 1);
        const size_t per = (n + parts - 1) / parts;
        char *d = static_cast<char *>(dst);
        const char *sp = static_cast<const char *>(src);
        for (unsigned i = 1; i < parts; i++) {
            const size_t a = i * per, b = std::min(n, a + per);
            if (a < b) { q_.push_back({d + a, sp + a, b - a}); pending_++; }
        }
        lk.unlock();
        cv_.notify_all();
        memcpy(d, sp, std::min(n, per));
        lk.lock();
        done_.wait(lk, [this] { return pending_ == 0; });
    }

  private:
    static constexpr unsigned kMaxThreads = 7;
    static unsigned threads()
    {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        return std::min(kMaxThreads, std::max(1u, hw / 2));
    }
    struct Task { char *d; const char *s; size_t n; };
    void work()
    {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
            if (q_.empty()) return;
            const Task t = q_.back();
            q_.pop_back();
            lk.unlock();
            memcpy(t.d, t.s, t.n);
            lk.lock();
            if (--pending_ == 0) done_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    std::vector<Task> q_;
    size_t pending_ = 0;
    bool stop_ = false;
};

// The context's grow-only device scratch buffers, by what they hold.  A slot belongs to one
// call at a time: calls on a context are stream-ordered, and growing a buffer goes through
// hipFree, which waits for the device.  Slots named twice below are claimed from two places
// of one dist call on purpose: the speculated launch (probe, rank kernel) and the regular one
// ask for the same candidates / row segments / results, and only one of the two runs, or the
// second reuses what the first wrote; the query-side record rows are built by whichever index
// source the call takes (resident-recorded or transient), never both.
//
// No slot is read before the call that claims it has written what it reads: a slot keeps the
// last call's bytes (or, under fpm_ctx_set_poison, the poison byte), never a value a kernel may
// rely on.  "init:" names who writes a slot first in a call; "in full" means every word a later
// kernel reads was written by that call ("Who initialises device memory";
// tests/test_gpu_poison.py runs every path over poisoned slots).
enum ScratchSlot : int {
    // index build: level-1 histograms per tile.  init: idx_part_hist_kernel, in full (every
    // partition x tile); the one-pass build does not use it
    kSlotTileHist = 0,
    // index build: their scan.  init: launch_exscan, in full ([0, nh) and the total at nh)
    kSlotTileOff = 1,
    // index build: level-1 staging entries.  init: the scatter kernels; the bucket pass reads
    // only [s0, s1) of each partition, the entries its fill / scan counted as written
    kSlotTent = 2,
    // rank kernel: per-candidate numer | denom (shared, see above).  init: rank_rows_kernel,
    // one pair per candidate; the candidate finalize reads the first n_cand pairs.  A row the
    // kernel leaves (unsorted, skip-count path) sends the call to the literal walk, which
    // does not read the slot
    kSlotCandRes = 3,
    // bucket directory.  init: idx_bucket_kernel, in full (every sub-bucket and the end word)
    kSlotDir = 4,
    // bucket entries.  init: idx_bucket_kernel, [0, indexed entries); the directory bounds
    // every read
    kSlotEntries = 5,
    // index build: scan scratch.  init: scan_local_kernel, every block sum before it is read
    kSlotScan = 6,
    // the counter block (CtrWord).  init: zeroed when the slot is made (scratch(): 4096 bytes or
    // less); then [0, kCtrZeroWords) by idx_kmax_kernel's last workgroup, or [0, kCtrProbeWords)
    // by a memset on the resident-set paths, before any kernel of the call adds to them;
    // kCtrKmaxAcc .. +2 are left at zero by idx_kmax_kernel itself (the only words that live
    // across calls); kCtrContain by a memset in contain / screen; kCtrCandOver is only written
    kSlotCounters = 7,
    // the probe's candidates (shared).  init: probe_rows_kernel, [0, n_cand); rows past the
    // capacity (a speculated probe) write nothing and get an empty segment
    kSlotCand = 8,
    // their per-query-row segments (shared).  init: probe_rows_kernel, one word per query row
    // (the rank kernel's path has one ref chunk: every row writes its own)
    kSlotRowSeg = 9,
    // record rows of the references.  init: record_rows_kernel, [0, length) of each row
    kSlotRecRef = 10,
    // their lengths.  init: record_rows_kernel, in full
    kSlotRecRefLen = 11,
    // record rows of the queries (shared).  init: record_rows_kernel, as the references'
    kSlotRecQry = 12,
    // their lengths (shared).  init: record_rows_kernel, in full
    kSlotRecQryLen = 13,
    // dense image compare: union blocks.  init: the image build kernel, what the compare reads
    kSlotImgBlocks = 14,
    // dense image compare: bit images.  init: the image build kernel, [0, min(len, W)) per row
    kSlotImg = 15,
    // index build: one-pass partition fill counts.  init: zeroed by idx_kmax_kernel's last
    // workgroup (zero32) before the scatter adds to them; the two-pass build does not read it
    kSlotPartFill = 16,
    // fpm_sketch_merge_dev: intermediate lists (no index build beside it: calls on a context
    // are stream-ordered, and each call writes the slot before it reads it).  init:
    // merge kernel, [0, count) of each list before the next round reads it
    kSlotMergeRows = 16,
    // fpm_sketch_merge_dev: their counts.  init: merge kernel, one per intermediate list
    kSlotMergeCounts = 17,
    // fpm_sketch_merge_dev: merge descriptors.  init: copied from the host, in full
    kSlotMergeDescs = 18,
    // record positions of the references.  init: record_rows_kernel, [0, length) of each row
    kSlotRecRefPos = 19,
    // record positions of the queries (shared).  init: record_rows_kernel, as the references'
    kSlotRecQryPos = 20,
    // the compacted candidate rows: values and positions (shared).  init: probe_rows_kernel
    // (CMP), [0, kept length) of each row; the rank kernel masks what lies past it
    kSlotCmpRows = 21,
    // their lengths, and the rows' own (shared).  init: probe_rows_kernel (CMP), 2 n words in
    // full; fpm_ctx_last_rank_compact reads them once (fpm_ctx_poison_now reads them first)
    kSlotCmpLen = 22,
    kSlotCount
};

// The dist counter block (kSlotCounters), in u64 words.  The flags are the low u32 of their word.
enum CtrWord : uint32_t {
    kCtrEvents = 0,        // posting events
    kCtrPartials = 1,      // ..64: per-block partial events
    kCtrCand = 65,         // candidates the probe appended
    kCtrUnsorted = 66,     // flag: some row is unsorted / carries duplicates
    kCtrOverflow = 67,     // flag: a one-pass index build overflowed a partition slot
    kCtrIndexed = 68,      // entries the index build indexed (fewer than kCtrEntries when cut)
    kCtrEntries = 69,      // entries the indexed rows hold
    kCtrKmax = 70,         // the largest indexed key (the bucket scale)
    kCtrCandOver = 71,     // flag: a probe ran past its candidate buffer (only a speculated one can)
    kCtrKmaxAcc = 72,      // ..74: idx_kmax_kernel's accumulators, kept at zero between calls
    kCtrContain = 75,      // contain: low u32 the not-ascending flag, high u32 the longest query row
    kCtrWords = 80,
    kCtrProbeWords = kCtrOverflow,   // [0, 67): cleared before, and read after, a probe count
    kCtrBuildWords = kCtrKmax,       // [0, 70): published after an index build
    kCtrZeroWords = kCtrKmaxAcc      // [0, 72): cleared by the index build's first kernel
};

struct fpm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[FPM_K_COUNT];
    // grow-only device scratch, one buffer per named slot (no allocation in steady state)
    // (a slot frees its buffer when destroyed: set the device before deleting its holder)
    struct Slot {
        void *p = nullptr;
        size_t bytes = 0;
        Slot() = default;
        Slot(const Slot &) = delete;
        Slot &operator=(const Slot &) = delete;
        ~Slot();
    };
    Slot scratch[kSlotCount];
    unsigned long long *host_counters = nullptr;   // pinned + mapped, for the events read-back
    unsigned long long *dev_counters = nullptr;    // its device-side address
    unsigned long long pub_seq = 0;                // last sequence number published into it
    int dist_mode = FPM_DIST_AUTO;
    int fill_counts = -1;      // the side-stream fill also writes the numer / denom defaults
                               // (-1: for grids of >= 2^28 pairs; FPM_FILL_COUNTS=0/1 forces)
    int last_sparse = 0;
    int last_kernel = FPM_DK_NONE;   // fpm_ctx_last_dist_kernel
    bool probe_half = true;          // fpm_ctx_set_probe_half (FPM_PROBE_HALF=0 starts it off)
    int last_probe = FPM_PROBE_NONE; // fpm_ctx_last_dist_probe
    bool index_cut = true;           // fpm_ctx_set_index_cut (FPM_INDEX_CUT=0 starts it off)
    // fpm_ctx_last_index_cut: the last compare's index left out the values no half probe can
    // reach, the entries it holds and the entries its rows hold (0 / 0: no index was built)
    bool last_index_cut = false;
    uint64_t last_indexed = 0, last_entries = 0;
    bool rank_compact = true;        // fpm_ctx_set_rank_compact (FPM_RANK_COMPACT=0 starts it off)
    // fpm_ctx_last_rank_compact: the last compare ranked its candidates on compacted rows; their
    // lengths (kept, then the rows' own: 2 n u32 on the device) are summed when asked for
    bool last_rank_compact = false;
    const uint32_t *last_cmp_len = nullptr;
    uint32_t last_cmp_n = 0;
    hipStream_t last_cmp_stream = nullptr;
    uint64_t last_kept = 0, last_cmp_entries = 0;
    int contain_mode = FPM_CONTAIN_AUTO;        // fpm_ctx_set_contain_mode
    int last_contain_kernel = FPM_CK_NONE;      // fpm_ctx_last_contain_kernel
    int last_screen_kernel = FPM_SK_NONE;       // fpm_ctx_last_screen_kernel
    int last_tax_kernel = FPM_TK_NONE;          // fpm_ctx_last_tax_kernel
    uint64_t last_events = 0, last_cand = 0;
    const unsigned long long *last_cand_dev = nullptr;   // the last sparse call's counter
    hipStream_t last_cand_stream = nullptr;
    // side stream for the sparse dist's fill (a pure write stream that runs beside the
    // latency-bound candidate compare); ev_in / ev_fill order it against `stream`
    hipStream_t aux = nullptr;
    hipEvent_t ev_in = nullptr, ev_fill = nullptr;
    // a compact grid's counts written ahead on `aux` (fpm_dist_list_prefill), until the dist
    // call on that grid takes it over (or any other dist call waits for it): ev_prefill
    struct Prefill {
        const void *numer = nullptr, *denom = nullptr;
        uint32_t n_ref = 0, n_qry = 0, S = 0;
        bool pending = false;
    } prefill;
    hipEvent_t ev_prefill = nullptr;
    // pinned staging ring for host -> device copies of pageable caller memory
    static constexpr int kRing = 4;
    static constexpr size_t kRingBytes = 8u << 20;
    void *ring[kRing] = {};
    hipEvent_t ring_ev[kRing] = {};
    CopyPool copier;                       // the ring's host-side copies
    // device buffers of released -fp text jobs, reused by the next jobs: a fresh hipMalloc of
    // tens of MB is cleared by the driver before first use, and a kernel writing it could wait
    // ~27 ms for that (tools/micro/fp_text_time.py under rocprofv3: fp_line_kernel 0.06 ms,
    // now and then 27 ms)
    static constexpr size_t kPoolBytes = size_t(2) << 30;
    uint64_t idx_rebuilds = 0;             // one-pass index builds that overflowed a slot
    // The last sparse rank-kernel call's shape and candidate capacity: a call of the same
    // shape enqueues its probe right behind the index build, before the host reads the
    // build's counters (compare_impl), and checks afterwards that the path and the capacity
    // held; otherwise the probe's output is dropped and the call proceeds as without it.
    struct SpecProfile {
        bool valid = false;
        uint32_t n_ref = 0, n_qry = 0, S = 0;
        uint64_t ref_stride = 0, qry_stride = 0, cap = 0;
        bool self_set = false, defaults = false;
    } spec;
    uint64_t spec_hits = 0, spec_misses = 0;
    std::vector<std::pair<void *, size_t>> pool;
    size_t pool_bytes = 0;
    std::mutex pool_mu;
    // fpm_ctx_set_poison (FPM_POISON=<0..255> starts it on): every buffer handed out is filled
    // with this byte first; -1: off
    int poison = -1;
};

// Event bracket: records start before and stop after a launch; done() hands the pair to the
// context, and a bracket left before done() (a launch failed) destroys it.
struct TimedLaunch {
    fpm_ctx *ctx; int kid; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    TimedLaunch(fpm_ctx *c, int k, hipStream_t s) : ctx(c), kid(k), st(s)
    {
        if (ctx->timing) {
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            (void)hipEventRecord(a, st);
        }
    }
    void done()
    {
        if (ctx->timing) {
            (void)hipEventRecord(b, st);
            ctx->ev[kid].push_back({a, b});
            a = b = nullptr;
        }
    }
    ~TimedLaunch()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
    TimedLaunch(const TimedLaunch &) = delete;
    TimedLaunch &operator=(const TimedLaunch &) = delete;
};

#pragma GCC visibility push(hidden)

int set_device(fpm_ctx *ctx);
inline hipStream_t pick_stream(fpm_ctx *ctx, void *stream)
{
    return stream ? (hipStream_t)stream : ctx->stream;
}

// device buffers of released jobs, reused by the next (fpm_ctx::pool; fpm_devmem.cpp)
hipError_t pool_alloc(fpm_ctx *ctx, void **p, size_t bytes);
void pool_free(fpm_ctx *ctx, void *p, size_t bytes);
// the poison fill (fpm_ctx_set_poison) of a buffer about to be handed out, synchronous on the
// context stream; nothing while poison is off or without a context
hipError_t poison_fill(fpm_ctx *ctx, void *p, size_t bytes);

// copies on the context stream, pageable caller memory through the pinned ring
hipError_t ensure_ring(fpm_ctx *ctx);
hipError_t memset_sync(fpm_ctx *ctx, void *dst, int v, size_t bytes);
hipError_t h2d_staged(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
hipError_t d2h_staged(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
hipError_t copy_out(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
hipError_t copy_in(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
hipError_t ensure_aux(fpm_ctx *ctx);

// grow-only device buffers: a slot of at least `bytes` (poisoned under `ctx`'s setting when it
// grows); scratch() is the context's named slot
hipError_t grow_slot(fpm_ctx *ctx, fpm_ctx::Slot &s, size_t bytes, void **out);
hipError_t scratch(fpm_ctx *ctx, ScratchSlot id, size_t bytes, void **out);

// The owner of device buffers: everything it still holds is freed with it, pooled buffers back
// into its context's pool (the caller has synchronised the streams that used them), the others
// with hipFree.  Handles keep their typed d_* fields as views and one DevBufs beside them;
// staging calls keep a local one.  A zero-byte request allocates 16 bytes.
class DevBufs {
  public:
    struct Buf { void *p; size_t bytes; bool pooled; };
    fpm_ctx *ctx = nullptr;            // get_pooled's pool, and whose poison setting get follows
    DevBufs() = default;
    explicit DevBufs(fpm_ctx *c) : ctx(c) {}
    DevBufs(DevBufs &&o) noexcept : ctx(o.ctx), held_(std::move(o.held_)) { o.held_.clear(); }
    DevBufs(const DevBufs &) = delete;
    DevBufs &operator=(const DevBufs &) = delete;
    ~DevBufs();
    // on failure *out is null and nothing is recorded
    template <typename T> hipError_t get(T **out, size_t bytes) { return typed(out, bytes, false); }
    template <typename T> hipError_t get_pooled(T **out, size_t bytes) { return typed(out, bytes, true); }
    // get, then the caller's host memory copied in (none given: allocated only)
    template <typename T> hipError_t upload(fpm_ctx *c, T **out, const void *host, size_t bytes)
    {
        hipError_t e = get(out, bytes);
        if (e == hipSuccess && host && bytes) e = copy_in(c, (void *)*out, host, bytes);
        return e;
    }
    // takes over a hipMalloc'd buffer (the packed records of a parse)
    void adopt(void *p) { if (p) held_.push_back({p, 0, false}); }
    // gives `p` up to the caller; null when `p` is not held here (nothing changes then)
    template <typename T> T *release(T *p) { return remove(p, false) ? p : nullptr; }
    // frees `p` now
    template <typename T> void drop(T *&p) { remove(p, true); p = nullptr; }
    // takes over all of `o`'s buffers, in order (allocate all or none: into a local owner first)
    void absorb(DevBufs &&o);
    const std::vector<Buf> &held() const { return held_; }

  private:
    template <typename T> hipError_t typed(T **out, size_t bytes, bool pooled)
    {
        void *q = nullptr;
        const hipError_t e = take(&q, bytes, pooled);
        *out = static_cast<T *>(q);
        return e;
    }
    hipError_t take(void **out, size_t bytes, bool pooled);
    void free_buf(const Buf &b);
    bool remove(const void *p, bool free_it);
    std::vector<Buf> held_;
};

// device counters -> the context's host-mapped block (fpm_ctx.cpp)
int publish_counters(fpm_ctx *ctx, const unsigned long long *d_src, uint32_t n, hipStream_t st,
                     unsigned long long *seq_out);
int wait_counters(fpm_ctx *ctx, unsigned long long seq, hipStream_t st);
int read_counters(fpm_ctx *ctx, const unsigned long long *d_src, uint32_t n, hipStream_t st);

// the host copy of the counter block, after read_counters / wait_counters
inline uint64_t host_events(const fpm_ctx *ctx) { return ctx->host_counters[kCtrEvents]; }
inline bool host_flag(const fpm_ctx *ctx, CtrWord w)
{
    return ((const uint32_t *)(ctx->host_counters + w))[0] != 0;
}
inline bool host_unsorted(const fpm_ctx *ctx) { return host_flag(ctx, kCtrUnsorted); }
inline bool host_overflow(const fpm_ctx *ctx) { return host_flag(ctx, kCtrOverflow); }
inline uint64_t host_indexed(const fpm_ctx *ctx) { return ctx->host_counters[kCtrIndexed]; }
inline uint64_t host_entries(const fpm_ctx *ctx) { return ctx->host_counters[kCtrEntries]; }

#pragma GCC visibility pop

// Records to sketch, in the order their groups stream them: `rec_len(r)` bytes at `rec_pos(r)`
// of the device sequence buffer.  Host path: fpm_sketch_stage packs the records itself
// (host_packed); device path: fpm_sketch_stage_seq adopts the buffer seqparse.hip packed.
struct StageRecords {
    std::vector<uint32_t> order;        // records in group order (records of no group left out)
    std::vector<uint64_t> pos, len;     // per record (indexed by record id)
    std::vector<uint32_t> group;        // per record
    uint32_t n_groups = 0;
    const char *host_seq = nullptr;     // host path: record r is host_seq[pos..pos+len)
    uint8_t *d_seq = nullptr;           // device path: packed buffer (the job adopts it)
    uint64_t d_seq_bytes = 0;
    bool borrow = false;                // device path: d_seq stays with its owner (reads mode's
                                        // wide jobs over the staged job's buffer)
};

// fpm_sketch_api.cpp: the staging behind fpm_sketch_stage and fpm_sketch_stage_seq (pack,
// plan_sketch of sketch_plan.hpp, allocate and upload)
FPM_HIDDEN int stage_core(fpm_ctx *ctx, const fpm_sketch_params *p, StageRecords &R,
                          fpm_sketch_job **job_out);

// fn(c, begin, n) for each tile class c that has tiles, class_begin[c] .. class_begin[c + 1] of a
// tile array ordered by class; stops at the first status that is not FPM_OK and returns it
template <typename Fn> int for_each_class(const uint32_t *class_begin, Fn fn)
{
    for (int c = 0; c < kTileClasses; c++) {
        const uint32_t b = class_begin[c], n = class_begin[c + 1] - b;
        if (!n) continue;
        if (int rc = fn(c, b, n)) return rc;
    }
    return FPM_OK;
}

// fpm_text_api.cpp: the records of a device parse for a job that adopts them (fpm_kfinger_stage_seq):
// each record's offset and length in the packed buffer, and the buffer itself, which leaves the
// parse handle (the caller frees it with hipFree)
struct fpm_seqtext;
FPM_HIDDEN int seqtext_records(fpm_ctx *ctx, fpm_seqtext *seq, uint64_t *n_rec,
                               std::vector<uint64_t> *pos, std::vector<uint64_t> *len,
                               uint8_t **d_packed);

// fpm_sketch_api.cpp: what fpm_screen_add_job reads of a staged job (its tiles by class cover
// every window of its records exactly once; row 0 / count 0 are its first group's sketch)
struct JobView {
    fpm_ctx *ctx;
    SketchKParams kp;
    uint32_t n_groups;
    const uint8_t *d_seq;
    const TileDesc *d_tiles;
    const uint32_t *class_begin;   // kTileClasses + 1
    const uint64_t *d_rows;
    const uint32_t *d_count;
};
FPM_HIDDEN void job_view(const fpm_sketch_job *job, JobView *out);
