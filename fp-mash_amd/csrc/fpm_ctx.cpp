// fpm_ctx.cpp — the context part of the C ABI declared in include/fpmash.h: context, streams,
// events, device and pinned memory, copies, kernel timing, and the helpers of fpm_internal.hpp
// that the other ABI files (fpm_sketch_api.cpp, fpm_text_api.cpp, fpm_dist_api.cpp,
// fpm_comm.cpp) share.
// There is deliberately no CPU compute path in the library: without a usable device every
// compute entry point returns FPM_ENODEV.
#include "fpm_internal.hpp"

#include <atomic>
#include <cstdlib>

static thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

// Synchronous copies and memsets run on the context stream, after the work queued there, and
// never on the null stream: the null stream's first use in a process creates one more
// hardware queue (~9 ms in the CLI's trace), and a separate copy stream cost another ~8 ms of
// start-up for no overlap the synchronous copies could use.
hipError_t ensure_ring(fpm_ctx *ctx)
{
    hipError_t e = hipSuccess;
    if (ctx->ring_ev[fpm_ctx::kRing - 1]) return e;
    for (int i = 0; e == hipSuccess && i < fpm_ctx::kRing; i++) {
        if (!ctx->ring[i]) e = hipHostMalloc(&ctx->ring[i], fpm_ctx::kRingBytes, hipHostMallocDefault);
        if (e == hipSuccess && !ctx->ring_ev[i])
            e = hipEventCreateWithFlags(&ctx->ring_ev[i], hipEventDisableTiming);
    }
    return e;
}

// synchronous copy on the context stream (ordered after the work queued there)
static hipError_t copy_sync(fpm_ctx *ctx, void *dst, const void *src, size_t bytes,
                            hipMemcpyKind kind)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}

hipError_t memset_sync(fpm_ctx *ctx, void *dst, int v, size_t bytes)
{
    hipError_t e = hipMemsetAsync(dst, v, bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}

// Host -> device copy of pageable memory through the context's pinned ring: the caller's
// thread memcpy's piece i into a pinned buffer while the DMA engine moves piece i - 1
// (hipMemcpy from pageable memory stages through the runtime's own buffers one piece at a
// time: ~3.8 GB/s measured on the -fp text).  Synchronous on return.
hipError_t h2d_staged(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return hipSuccess;
    if (bytes < (1u << 20)) return copy_sync(ctx, dst, src, bytes, hipMemcpyHostToDevice);
    hipError_t e = ensure_ring(ctx);
    if (e != hipSuccess) return e;
    const char *s = static_cast<const char *>(src);
    char *d = static_cast<char *>(dst);
    bool used[fpm_ctx::kRing] = {};
    for (size_t off = 0, i = 0; off < bytes; off += fpm_ctx::kRingBytes, i++) {
        const int slot = (int)(i % fpm_ctx::kRing);
        const size_t n = std::min(fpm_ctx::kRingBytes, bytes - off);
        if (used[slot] && (e = hipEventSynchronize(ctx->ring_ev[slot])) != hipSuccess) return e;
        ctx->copier.copy(ctx->ring[slot], s + off, n);
        if ((e = hipMemcpyAsync(d + off, ctx->ring[slot], n, hipMemcpyHostToDevice, ctx->stream)) !=
            hipSuccess)
            return e;
        if ((e = hipEventRecord(ctx->ring_ev[slot], ctx->stream)) != hipSuccess) return e;
        used[slot] = true;
    }
    return hipStreamSynchronize(ctx->stream);
}

// Device -> host copy into pageable caller memory through the same pinned ring: the DMA of
// piece i overlaps the caller thread's memcpy of piece i - 1 out of the ring.
hipError_t d2h_staged(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return hipSuccess;
    if (bytes < (64u << 10)) return copy_sync(ctx, dst, src, bytes, hipMemcpyDeviceToHost);
    hipError_t e = ensure_ring(ctx);
    if (e != hipSuccess) return e;
    const char *s = static_cast<const char *>(src);
    char *d = static_cast<char *>(dst);
    const size_t R = fpm_ctx::kRingBytes;
    const size_t n_pieces = (bytes + R - 1) / R;
    auto issue = [&](size_t i) -> hipError_t {
        const int slot = (int)(i % fpm_ctx::kRing);
        const size_t off = i * R, n = std::min(R, bytes - off);
        hipError_t x = hipMemcpyAsync(ctx->ring[slot], s + off, n, hipMemcpyDeviceToHost, ctx->stream);
        if (x == hipSuccess) x = hipEventRecord(ctx->ring_ev[slot], ctx->stream);
        return x;
    };
    for (size_t i = 0; i < std::min<size_t>(n_pieces, fpm_ctx::kRing); i++)
        if ((e = issue(i)) != hipSuccess) return e;
    for (size_t i = 0; i < n_pieces; i++) {
        const int slot = (int)(i % fpm_ctx::kRing);
        const size_t off = i * R, n = std::min(R, bytes - off);
        if ((e = hipEventSynchronize(ctx->ring_ev[slot])) != hipSuccess) return e;
        ctx->copier.copy(d + off, ctx->ring[slot], n);
        if (i + fpm_ctx::kRing < n_pieces && (e = issue(i + fpm_ctx::kRing)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// Caller memory that is not page-locked goes through the context's pinned ring (d2h_staged)
// and is never handed to hipMemcpy directly: the runtime locks a large pageable buffer for the
// DMA (a userptr mapping), and when the caller later frees it (numpy / malloc give such
// buffers back with munmap) the kernel driver evicts and restores the process's GPU queues,
// which stalled whatever ran on the GPU for ~20-30 ms (tools/micro/fp_clock.hip: a ticker
// wave on its own stream saw a 26 ms gap next to the -fp text fetch into freshly malloc'd
// arrays).

static bool host_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// device -> caller host memory, synchronous; the caller has ordered `src`'s producers
hipError_t copy_out(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return hipSuccess;
    if (bytes < (64u << 10) || host_pinned(dst))
        return copy_sync(ctx, dst, src, bytes, hipMemcpyDeviceToHost);
    return d2h_staged(ctx, dst, src, bytes);
}

// caller host memory -> device, synchronous
hipError_t copy_in(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return hipSuccess;
    if (host_pinned(src)) return copy_sync(ctx, dst, src, bytes, hipMemcpyHostToDevice);
    return h2d_staged(ctx, dst, src, bytes);
}

hipError_t ensure_aux(fpm_ctx *ctx)
{
    if (ctx->aux) return hipSuccess;
    // default priority: a low-priority side stream (or a high-priority main one) measured
    // slower, the fill then trails the candidate compare instead of sharing its CUs; so did
    // CU-masked streams splitting the CUs between the fill and the compare
    hipError_t e = hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_fill, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_prefill, hipEventDisableTiming);
    return e;
}

// Device counters -> host (the index build's posting events and sortedness flags, read
// mid-call to pick the path): publish_kernel copies them into the context's mapped pinned
// block and then bumps a sequence word, which the host spins on.  A D2H copy + stream sync
// left the GPU idle ~45 us per call (the sync's wake-up, then the next launch).
// The two halves: publish_counters enqueues the copy (returns its sequence number), and
// wait_counters spins until it has landed, so work enqueued between them runs while the host
// waits (the speculated rank kernel of a resident set's block, compare_impl).
int publish_counters(fpm_ctx *ctx, const unsigned long long *d_src, uint32_t n,
                            hipStream_t st, unsigned long long *seq_out)
{
    if (!ctx->host_counters) {
        HIP_TRY(hipHostMalloc((void **)&ctx->host_counters, kPubWords * 8,
                              hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&ctx->dev_counters, ctx->host_counters, 0));
        memset(ctx->host_counters, 0, kPubWords * 8);
    }
    const unsigned long long seq = ++ctx->pub_seq;
    HIP_TRY(launch_publish(d_src, n, ctx->dev_counters, seq, st));
    *seq_out = seq;
    return FPM_OK;
}

int wait_counters(fpm_ctx *ctx, unsigned long long seq, hipStream_t st)
{
    volatile unsigned long long *flag = ctx->host_counters + kPubWords - 1;
    for (uint64_t spin = 1;; spin++) {
        if (*flag == seq) break;
        if ((spin & 1023) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q != hipSuccess && q != hipErrorNotReady) return fail(FPM_EHIP, hipGetErrorString(q));
            if (q == hipSuccess && *flag != seq) {
                std::atomic_thread_fence(std::memory_order_seq_cst);
                if (*flag != seq) return fail(FPM_EHIP, "counter publish did not land");
            }
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return FPM_OK;
}

int read_counters(fpm_ctx *ctx, const unsigned long long *d_src, uint32_t n,
                         hipStream_t st)
{
    unsigned long long seq;
    if (int rc = publish_counters(ctx, d_src, n, st, &seq)) return rc;
    return wait_counters(ctx, seq, st);
}

// returns a device buffer of at least `bytes` for scratch slot `id`
hipError_t scratch(fpm_ctx *ctx, ScratchSlot id, size_t bytes, void **out)
{
    auto &s = ctx->scratch[id];
    const bool grows = s.bytes < bytes;
    hipError_t e = grow_slot(ctx, s, bytes, out);
    // small buffers (the counters) start zeroed: some words are kept at zero between
    // calls by the kernels themselves (idx_kmax_kernel's accumulator)
    if (e == hipSuccess && grows && s.bytes <= 4096) e = memset_sync(ctx, s.p, 0, s.bytes);
    return e;
}

int set_device(fpm_ctx *ctx)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    return FPM_OK;
}

// What the context remembers as addresses into its scratch slots, read into host fields: the
// last sparse call's candidate count and the compacted rows' lengths (the fpm_ctx_last_*
// queries read them lazily; fpm_ctx_poison_now reads them before it overwrites the slots).
static int resolve_last_cand(fpm_ctx *ctx)
{
    if (ctx->last_cand != (uint64_t)-1) return FPM_OK;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->last_cand_stream));
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, ctx->last_cand_dev, 8, hipMemcpyDeviceToHost));
    ctx->last_cand = v;
    return FPM_OK;
}

static int resolve_last_cmp_len(fpm_ctx *ctx)
{
    if (!ctx->last_rank_compact || !ctx->last_cmp_len) return FPM_OK;
    // the probe's per-row lengths: read once, after the call's work
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->last_cmp_stream));
    std::vector<uint32_t> len(2 * (size_t)ctx->last_cmp_n);
    HIP_TRY(hipMemcpy(len.data(), ctx->last_cmp_len, len.size() * 4, hipMemcpyDeviceToHost));
    ctx->last_kept = ctx->last_cmp_entries = 0;
    for (uint32_t r = 0; r < ctx->last_cmp_n; r++) {
        ctx->last_kept += len[r];
        ctx->last_cmp_entries += len[ctx->last_cmp_n + r];
    }
    ctx->last_cmp_len = nullptr;
    return FPM_OK;
}

extern "C" {

int fpm_abi_version(void) { return FPM_ABI_VERSION; }

const char *fpm_last_error(void) { return g_err.c_str(); }

int fpm_device_count(int *count)
{
    if (!count) return fail(FPM_EINVAL, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return FPM_OK;
}

int fpm_ctx_create(int device, fpm_ctx **out)
{
    if (!out) return fail(FPM_EINVAL, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(FPM_ENODEV, "no HIP device visible (fpmash has no CPU fallback)");
    if (device < 0 || device >= n) return fail(FPM_EINVAL, "device index out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(FPM_ENODEV, std::string("device is ") + prop.gcnArchName +
                                    ", fpmash kernels are built for gfx950 only");
    fpm_ctx *ctx = new fpm_ctx();
    ctx->device = device;
    if (const char *v = getenv("FPM_FILL_COUNTS")) ctx->fill_counts = atoi(v) != 0 ? 1 : 0;
    if (const char *v = getenv("FPM_PROBE_HALF")) ctx->probe_half = atoi(v) != 0;
    if (const char *v = getenv("FPM_INDEX_CUT")) ctx->index_cut = atoi(v) != 0;
    if (const char *v = getenv("FPM_RANK_COMPACT")) ctx->rank_compact = atoi(v) != 0;
    if (const char *v = getenv("FPM_POISON")) {
        const int b = atoi(v);
        if (*v && b >= 0 && b <= 255) ctx->poison = b;
    }
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail(FPM_EHIP, std::string("context init: ") + hipGetErrorString(e));
    }
    *out = ctx;
    return FPM_OK;
}

void fpm_ctx_destroy(fpm_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    fpm_ctx_reset_timing(ctx);
    if (ctx->host_counters) (void)hipHostFree(ctx->host_counters);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
    if (ctx->ev_fill) (void)hipEventDestroy(ctx->ev_fill);
    if (ctx->ev_prefill) (void)hipEventDestroy(ctx->ev_prefill);
    for (int i = 0; i < fpm_ctx::kRing; i++) {
        if (ctx->ring[i]) (void)hipHostFree(ctx->ring[i]);
        if (ctx->ring_ev[i]) (void)hipEventDestroy(ctx->ring_ev[i]);
    }
    for (auto &b : ctx->pool) (void)hipFree(b.first);
    delete ctx;
}

int fpm_ctx_warm(fpm_ctx *ctx)
{
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(ensure_ring(ctx));
    // one 1 MB copy each way between the ring and the device: the first DMA of a process
    // sets up its copy path (~8-11 ms inside the first staged upload in the CLI's trace)
    constexpr size_t kWarm = 1u << 20;
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, kWarm));
    hipError_t e = hipMemcpyAsync(d, ctx->ring[0], kWarm, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->ring[1], d, kWarm, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    const hipError_t f = hipFree(d);
    HIP_TRY(e);
    HIP_TRY(f);
    return FPM_OK;
}

void *fpm_ctx_stream(fpm_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int fpm_stream_create(fpm_ctx *ctx, void **stream)
{
    if (!stream) return fail(FPM_EINVAL, "null stream");
    if (int rc = set_device(ctx)) return rc;
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = s;
    return FPM_OK;
}

int fpm_stream_destroy(fpm_ctx *ctx, void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    if (stream) HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return FPM_OK;
}

int fpm_event_create(fpm_ctx *ctx, void **event)
{
    if (!event) return fail(FPM_EINVAL, "null event");
    if (int rc = set_device(ctx)) return rc;
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *event = e;
    return FPM_OK;
}

int fpm_event_destroy(fpm_ctx *ctx, void *event)
{
    if (int rc = set_device(ctx)) return rc;
    if (event) HIP_TRY(hipEventDestroy((hipEvent_t)event));
    return FPM_OK;
}

int fpm_event_record(fpm_ctx *ctx, void *event, void *stream)
{
    if (!event) return fail(FPM_EINVAL, "null event");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipEventRecord((hipEvent_t)event, pick_stream(ctx, stream)));
    return FPM_OK;
}

int fpm_stream_wait_event(fpm_ctx *ctx, void *stream, void *event)
{
    if (!event) return fail(FPM_EINVAL, "null event");
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamWaitEvent(pick_stream(ctx, stream), (hipEvent_t)event, 0));
    return FPM_OK;
}

int fpm_ctx_synchronize(fpm_ctx *ctx)
{
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return FPM_OK;
}

int fpm_malloc(fpm_ctx *ctx, void **dptr, size_t bytes)
{
    if (int rc = set_device(ctx)) return rc;
    if (!dptr) return fail(FPM_EINVAL, "null dptr");
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(FPM_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    if ((e = poison_fill(ctx, *dptr, bytes ? bytes : 1)) != hipSuccess) {
        (void)hipFree(*dptr);
        *dptr = nullptr;
        return fail(FPM_EHIP, std::string("fpm_malloc: poison fill: ") + hipGetErrorString(e));
    }
    return FPM_OK;
}

int fpm_free(fpm_ctx *ctx, void *dptr)
{
    if (int rc = set_device(ctx)) return rc;
    if (dptr) HIP_TRY(hipFree(dptr));
    return FPM_OK;
}

int fpm_memcpy_h2d(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // earlier work on dst is ordered before
    if (bytes) HIP_TRY(h2d_staged(ctx, dst, src, bytes));
    return FPM_OK;
}

int fpm_memcpy_d2h(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(copy_out(ctx, dst, src, bytes));
    return FPM_OK;
}

int fpm_memcpy_d2d(fpm_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (int rc = set_device(ctx)) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return FPM_OK;
}

int fpm_memset(fpm_ctx *ctx, void *dptr, int value, size_t bytes)
{
    if (int rc = set_device(ctx)) return rc;
    if (bytes) HIP_TRY(hipMemsetAsync(dptr, value, bytes, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

int fpm_host_alloc(fpm_ctx *ctx, void **p, size_t bytes)
{
    if (!p) return fail(FPM_EINVAL, "host_alloc: null output");
    *p = nullptr;
    if (int rc = set_device(ctx)) return rc;
    if (hipHostMalloc(p, bytes ? bytes : 16) != hipSuccess)
        return fail(FPM_ENOMEM, "host_alloc: pinned allocation failed");
    return FPM_OK;
}

int fpm_host_free(fpm_ctx *ctx, void *p)
{
    if (int rc = set_device(ctx)) return rc;
    if (p) HIP_TRY(hipHostFree(p));
    return FPM_OK;
}

int fpm_ctx_set_dist_mode(fpm_ctx *ctx, int mode)
{
    if (!ctx || mode < FPM_DIST_AUTO || mode > FPM_DIST_SPARSE) return fail(FPM_EINVAL, "bad dist mode");
    ctx->dist_mode = mode;
    return FPM_OK;
}

int fpm_ctx_last_dist_stats(fpm_ctx *ctx, int *sparse, uint64_t *events, uint64_t *candidates)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    if (sparse) *sparse = ctx->last_sparse;
    if (events) *events = ctx->last_events;
    if (int rc = resolve_last_cand(ctx)) return rc;
    if (candidates) *candidates = ctx->last_cand;
    return FPM_OK;
}

int fpm_ctx_last_dist_kernel(fpm_ctx *ctx, int *kernel)
{
    if (!ctx || !kernel) return fail(FPM_EINVAL, "null argument");
    *kernel = ctx->last_kernel;
    return FPM_OK;
}

int fpm_ctx_set_probe_half(fpm_ctx *ctx, int on)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    ctx->probe_half = on != 0;
    return FPM_OK;
}

int fpm_ctx_last_dist_probe(fpm_ctx *ctx, int *form)
{
    if (!ctx || !form) return fail(FPM_EINVAL, "null argument");
    *form = ctx->last_probe;
    return FPM_OK;
}

int fpm_ctx_set_index_cut(fpm_ctx *ctx, int on)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    ctx->index_cut = on != 0;
    return FPM_OK;
}

int fpm_ctx_last_index_cut(fpm_ctx *ctx, int *cut, uint64_t *indexed, uint64_t *entries)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    if (cut) *cut = ctx->last_index_cut ? 1 : 0;
    if (indexed) *indexed = ctx->last_indexed;
    if (entries) *entries = ctx->last_entries;
    return FPM_OK;
}

int fpm_ctx_set_rank_compact(fpm_ctx *ctx, int on)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    ctx->rank_compact = on != 0;
    return FPM_OK;
}

int fpm_ctx_last_rank_compact(fpm_ctx *ctx, int *compact, uint64_t *kept, uint64_t *entries)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    if (int rc = resolve_last_cmp_len(ctx)) return rc;
    if (compact) *compact = ctx->last_rank_compact ? 1 : 0;
    if (kept) *kept = ctx->last_rank_compact ? ctx->last_kept : 0;
    if (entries) *entries = ctx->last_rank_compact ? ctx->last_cmp_entries : 0;
    return FPM_OK;
}

int fpm_ctx_index_rebuilds(fpm_ctx *ctx, uint64_t *count)
{
    if (!ctx || !count) return fail(FPM_EINVAL, "null argument");
    *count = ctx->idx_rebuilds;
    return FPM_OK;
}

int fpm_ctx_spec_stats(fpm_ctx *ctx, uint64_t *hits, uint64_t *misses)
{
    if (!ctx || !hits || !misses) return fail(FPM_EINVAL, "null argument");
    *hits = ctx->spec_hits;
    *misses = ctx->spec_misses;
    return FPM_OK;
}

int fpm_ctx_set_poison(fpm_ctx *ctx, int byte)
{
    if (!ctx || byte < -1 || byte > 255) return fail(FPM_EINVAL, "bad poison byte");
    ctx->poison = byte;
    return FPM_OK;
}

int fpm_ctx_poison_now(fpm_ctx *ctx)
{
    if (int rc = set_device(ctx)) return rc;
    if (ctx->poison < 0) return fail(FPM_EINVAL, "poison_now: poison is off");
    HIP_TRY(hipDeviceSynchronize());
    // nothing the context remembers may point into what is overwritten below
    if (int rc = resolve_last_cand(ctx)) return rc;
    if (int rc = resolve_last_cmp_len(ctx)) return rc;
    ctx->last_cmp_len = nullptr;
    ctx->last_cand_dev = nullptr;
    for (int id = 0; id < kSlotCount; id++) {
        fpm_ctx::Slot &s = ctx->scratch[id];
        if (!s.p) continue;
        if (id != kSlotCounters) {
            HIP_TRY(hipMemsetAsync(s.p, ctx->poison, s.bytes, ctx->stream));
            continue;
        }
        // the counter block: all of it but idx_kmax_kernel's three accumulators, the words the
        // kernels themselves keep at zero from one call to the next (CtrWord)
        const size_t lo = (size_t)kCtrKmaxAcc * 8, hi = lo + 3 * 8;
        HIP_TRY(hipMemsetAsync(s.p, ctx->poison, std::min(lo, s.bytes), ctx->stream));
        if (s.bytes > hi)
            HIP_TRY(hipMemsetAsync((char *)s.p + hi, ctx->poison, s.bytes - hi, ctx->stream));
    }
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        for (auto &b : ctx->pool)
            HIP_TRY(hipMemsetAsync(b.first, ctx->poison, b.second, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FPM_OK;
}

int fpm_ctx_set_timing(fpm_ctx *ctx, int enable)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    ctx->timing = enable != 0;
    return FPM_OK;
}

int fpm_ctx_reset_timing(fpm_ctx *ctx)
{
    if (!ctx) return fail(FPM_EINVAL, "null context");
    for (auto &v : ctx->ev) {
        for (auto &pr : v) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        v.clear();
    }
    return FPM_OK;
}

int fpm_ctx_kernel_time(fpm_ctx *ctx, int kernel, double *total_ms, uint64_t *launches)
{
    if (!ctx || kernel < 0 || kernel >= FPM_K_COUNT) return fail(FPM_EINVAL, "bad kernel id");
    if (int rc = set_device(ctx)) return rc;
    double t = 0;
    for (auto &pr : ctx->ev[kernel]) {
        HIP_TRY(hipEventSynchronize(pr.second));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        t += ms;
    }
    if (total_ms) *total_ms = t;
    if (launches) *launches = ctx->ev[kernel].size();
    return FPM_OK;
}

void fpm_scan_limits(uint32_t *block, uint32_t *fold_blocks)
{
    if (block) *block = kScanBlock;
    if (fold_blocks) *fold_blocks = kScanFoldBlocks;
}

int fpm_exscan_dev(fpm_ctx *ctx, const uint32_t *d_in, uint64_t n, uint32_t *d_out,
                   uint32_t *d_out2, uint32_t *d_total)
{
    if (!ctx || (n && (!d_in || !d_out))) return fail(FPM_EINVAL, "fpm_exscan_dev: null argument");
    if (n > (1ull << 31)) return fail(FPM_EINVAL, "fpm_exscan_dev: more than 2^31 elements");
    if (int rc = set_device(ctx)) return rc;
    DevBufs mem(ctx);
    uint32_t *scan_s = nullptr;
    HIP_TRY(mem.get_pooled(&scan_s, scan_scratch_words(n ? n : 1) * 4));
    const hipError_t launched = launch_exscan(d_in, d_out, d_out2, n, scan_s, d_total, ctx->stream);
    const hipError_t synced = hipStreamSynchronize(ctx->stream);   // the scratch goes back to the
    HIP_TRY(launched);                                             // pool on return
    HIP_TRY(synced);
    return FPM_OK;
}

}  // extern "C"
