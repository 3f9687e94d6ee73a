// fpm_screen_api.cpp — the screen part of the C ABI (include/fpmash.h): the table of a sketch
// database, the pool passes that fill its counters and the pool's bottom-s row, and the
// per-reference sums, -w and p-values read from them, and taxscreen's per-hash LCA and clade
// tallies over the same table.  The kernels are in screen.hip and taxscreen.hip, the pool pass
// in sketch.hip (screen_count_kernel), the binomial tail in dist.hip.
#include "fpm_internal.hpp"
#include "screen_table.hpp"

struct fpm_screen {
    fpm_ctx *ctx = nullptr;
    uint32_t n_db = 0, s = 0, hash_bytes = 8;
    uint64_t stride = 0;
    uint32_t E = 0, max_len = 0;          // cells of the database, its longest row
    uint32_t sbits = 0;                   // the build's sort bucket bits (0: no cell)
    std::vector<uint32_t> h_len;
    ScreenTable tab;                      // U, dir, count (owned)
    uint32_t *d_len = nullptr, *d_slot = nullptr, *d_ustart = nullptr, *d_post = nullptr;
    uint32_t *d_owner = nullptr, *d_shared = nullptr, *d_median = nullptr;
    // the pool's running bottom-s row: pair[0] (count pcnt[0]); pair[1] takes a job's row and
    // pair[2] (pcnt[2]) their merge
    uint64_t *d_pair = nullptr;
    uint32_t *d_pcnt = nullptr;
    DevBufs mem;                          // owns the table's arrays and every d_* above
};

namespace {

void screen_release(fpm_screen *sc)
{
    if (!sc) return;
    (void)hipSetDevice(sc->ctx->device);
    delete sc;
}

int screen_build(fpm_ctx *ctx, const void *d_db, const uint32_t *d_db_len, uint64_t stride,
                 uint32_t n_db, uint32_t hash_bytes, uint32_t sketch_size, fpm_screen **out)
{
    if (!out) return fail(FPM_EINVAL, "fpm_screen_create: null argument");
    *out = nullptr;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    if (sketch_size < 1) return fail(FPM_EINVAL, "sketch_size must be >= 1");
    if (n_db && (!d_db || !d_db_len)) return fail(FPM_EINVAL, "fpm_screen_create: null buffer");
    if ((uint64_t)n_db * stride >= (1ull << 32) || n_db > 0x7FFFFFFFu)
        return fail(FPM_EINVAL, "fpm_screen_create: n_db * stride must be below 2^32");
    hipStream_t st = ctx->stream;
    fpm_screen *sc = new fpm_screen;
    sc->ctx = sc->mem.ctx = ctx;
    sc->n_db = n_db;
    sc->s = sketch_size;
    sc->hash_bytes = hash_bytes;
    sc->stride = stride;
    sc->h_len.assign(n_db, 0);
    auto body = [&]() -> int {
        const size_t cells = (size_t)n_db * stride;
        DevBufs &mem = sc->mem;
        HIP_TRY(mem.get(&sc->d_len, std::max<size_t>(n_db, 1) * 4));
        HIP_TRY(mem.get(&sc->d_shared, std::max<size_t>(n_db, 1) * 4));
        HIP_TRY(mem.get(&sc->d_median, std::max<size_t>(n_db, 1) * 4));
        HIP_TRY(mem.get(&sc->d_slot, std::max<size_t>(cells, 1) * 4));
        HIP_TRY(mem.get(&sc->d_pair, (size_t)3 * sketch_size * 8));
        HIP_TRY(mem.get(&sc->d_pcnt, 16));
        HIP_TRY(hipMemsetAsync(sc->d_pcnt, 0, 16, st));
        uint64_t E = 0;
        if (n_db) {
            HIP_TRY(hipMemcpyAsync(sc->d_len, d_db_len, (size_t)n_db * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(sc->h_len.data(), d_db_len, (size_t)n_db * 4,
                                   hipMemcpyDeviceToHost, st));
            // strictly ascending rows (the lookup and the postings rest on it)
            void *ctr;
            HIP_TRY(scratch(ctx, kSlotCounters, kCtrWords * 8, &ctr));
            uint32_t *flag = (uint32_t *)((unsigned long long *)ctr + kCtrContain);
            HIP_TRY(hipMemsetAsync(flag, 0, 8, st));
            HIP_TRY(launch_rows_ascending(RowSet{d_db, d_db_len, nullptr, stride, n_db}, RowSet{},
                                          hash_bytes, flag, st));
            uint32_t host[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(host, flag, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint32_t l : sc->h_len) {
                if (l > stride) return fail(FPM_EINVAL, "fpm_screen_create: a row is longer than the stride");
                E += l;
                sc->max_len = std::max(sc->max_len, l);
            }
            if (host[0])
                return fail(FPM_EINVAL, "fpm_screen_create: a row is not strictly ascending");
        }
        sc->E = (uint32_t)E;
        uint32_t nU = 0;
        unsigned long long kmax = 0;
        DevBufs tmp(ctx);   // the build's scratch: freed on return
        uint64_t *okey = nullptr;
        uint32_t *ocell = nullptr, *head = nullptr, *hx = nullptr, *scan_s = nullptr;
        if (E) {
            // ~2 cells per sort bucket
            uint32_t sbits = 1;
            while (sbits < 22 && (2ull << sbits) < E) sbits++;
            sc->sbits = sbits;
            const uint64_t nb = 1ull << sbits;
            DevBufs sort_tmp(ctx);   // the sort's own scratch: freed at the end of this block
            unsigned long long *km;
            uint32_t *hist, *start;
            uint64_t *skey;
            HIP_TRY(sort_tmp.get(&km, 16));
            HIP_TRY(sort_tmp.get(&hist, nb * 4));
            HIP_TRY(sort_tmp.get(&start, nb * 4));
            HIP_TRY(tmp.get(&scan_s, scan_scratch_words(std::max<uint64_t>(nb, E)) * 4));
            HIP_TRY(sort_tmp.get(&skey, E * 8));
            HIP_TRY(tmp.get(&okey, E * 8));
            HIP_TRY(tmp.get(&ocell, E * 4));
            HIP_TRY(tmp.get(&head, E * 4));
            HIP_TRY(tmp.get(&hx, E * 4));
            HIP_TRY(mem.get(&sc->d_post, E * 4));   // the scatter's cells, then the postings
            HIP_TRY(launch_screen_sort(d_db, d_db_len, stride, n_db, hash_bytes, (uint32_t)E, sbits,
                                       km, hist, start, scan_s, skey, sc->d_post, okey, ocell, st));
            uint32_t *d_n = (uint32_t *)km + 2;
            HIP_TRY(launch_screen_heads(okey, (uint32_t)E, head, hx, scan_s, d_n, st));
            HIP_TRY(hipMemcpyAsync(&kmax, km, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&nU, d_n, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        // directory: 2^dbits >= 2 |U| where 24 bits allow
        uint32_t dbits = 4;
        while (dbits < 24 && (1ull << dbits) < 2ull * nU) dbits++;
        sc->tab.n = nU;
        sc->tab.dbits = dbits;
        sc->tab.umax = kmax;
        sc->tab.shift = kmax ? (uint32_t)__builtin_clzll(kmax) : 63u;
        HIP_TRY(mem.get(&sc->tab.U, std::max<size_t>(nU, 1) * 8));
        HIP_TRY(mem.get(&sc->tab.count, std::max<size_t>(nU, 1) * 4));
        HIP_TRY(mem.get(&sc->d_owner, std::max<size_t>(nU, 1) * 4));
        HIP_TRY(mem.get(&sc->d_ustart, ((size_t)nU + 1) * 4));
        HIP_TRY(mem.get(&sc->tab.dir, ((size_t)(1u << dbits) + 1) * 4));
        HIP_TRY(hipMemsetAsync(sc->tab.count, 0, std::max<size_t>(nU, 1) * 4, st));
        HIP_TRY(hipMemsetAsync(sc->d_ustart, 0, ((size_t)nU + 1) * 4, st));
        HIP_TRY(hipMemsetAsync((void *)sc->tab.dir, 0, ((size_t)(1u << dbits) + 1) * 4, st));
        HIP_TRY(launch_screen_compact(okey, ocell, head, hx, (uint32_t)E, stride, nU, dbits,
                                      sc->tab.shift, (uint64_t *)sc->tab.U, sc->d_ustart,
                                      sc->d_slot, sc->d_post, (uint32_t *)sc->tab.dir, st));
        HIP_TRY(hipStreamSynchronize(st));   // the build's buffers are released on return
        return FPM_OK;
    };
    const int rc = body();
    if (rc) {
        (void)hipStreamSynchronize(st);
        screen_release(sc);
        return rc;
    }
    *out = sc;
    return FPM_OK;
}

// shared / median of every reference from the counters (owner: the -w pass's, or null)
int screen_rows(fpm_screen *sc, const uint32_t *d_owner, uint32_t *out_shared, uint32_t *out_median)
{
    fpm_ctx *ctx = sc->ctx;
    hipStream_t st = ctx->stream;
    ctx->last_screen_kernel = FPM_SK_NONE;
    if (!sc->n_db) return FPM_OK;
    bool lds = false;
    {
        TimedLaunch tl(ctx, FPM_K_COMPARE, st);
        HIP_TRY(launch_screen_rows(sc->d_slot, sc->d_len, sc->stride, sc->n_db, sc->max_len,
                                   sc->tab.count, d_owner, sc->d_shared, sc->d_median, st, &lds));
        tl.done();
    }
    ctx->last_screen_kernel = lds ? FPM_SK_ROWS_LDS : FPM_SK_ROWS_GLOBAL;
    HIP_TRY(hipStreamSynchronize(st));
    if (out_shared) HIP_TRY(copy_out(ctx, out_shared, sc->d_shared, (size_t)sc->n_db * 4));
    if (out_median) HIP_TRY(copy_out(ctx, out_median, sc->d_median, (size_t)sc->n_db * 4));
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_screen_create_dev(fpm_ctx *ctx, const void *d_db, const uint32_t *d_db_len,
                          uint64_t stride, uint32_t n_db, uint32_t hash_bytes,
                          uint32_t sketch_size, fpm_screen **out)
{
    if (int rc = set_device(ctx)) return rc;
    return screen_build(ctx, d_db, d_db_len, stride, n_db, hash_bytes, sketch_size, out);
}

int fpm_screen_create(fpm_ctx *ctx, const void *db, const uint32_t *db_len, uint64_t stride,
                      uint32_t n_db, uint32_t hash_bytes, uint32_t sketch_size, fpm_screen **out)
{
    if (int rc = set_device(ctx)) return rc;
    if (hash_bytes != 4 && hash_bytes != 8) return fail(FPM_EINVAL, "hash_bytes must be 4 or 8");
    if (n_db && (!db || !db_len)) return fail(FPM_EINVAL, "fpm_screen_create: null buffer");
    DevBufs mem(ctx);
    void *rows;
    uint32_t *len;
    hipError_t e = mem.get(&rows, (size_t)n_db * stride * hash_bytes);
    if (e == hipSuccess) e = mem.get(&len, (size_t)n_db * 4);
    if (e == hipSuccess) e = copy_in(ctx, rows, db, (size_t)n_db * stride * hash_bytes);
    if (e == hipSuccess) e = copy_in(ctx, len, db_len, (size_t)n_db * 4);
    if (e != hipSuccess) return fail(FPM_ENOMEM, std::string("screen staging: ") + hipGetErrorString(e));
    return screen_build(ctx, rows, len, stride, n_db, hash_bytes, sketch_size, out);
}

void fpm_screen_free(fpm_screen *sc) { screen_release(sc); }

int fpm_screen_add_job(fpm_screen *sc, fpm_sketch_job *job, void *stream)
{
    if (!sc || !job) return fail(FPM_EINVAL, "fpm_screen_add_job: null argument");
    fpm_ctx *ctx = sc->ctx;
    if (int rc = set_device(ctx)) return rc;
    JobView v;
    job_view(job, &v);
    if (v.ctx != ctx) return fail(FPM_EINVAL, "fpm_screen_add_job: the job belongs to another context");
    if (v.n_groups != 1) return fail(FPM_EINVAL, "fpm_screen_add_job: the job must be staged as one group");
    if (v.kp.s != sc->s) return fail(FPM_EINVAL, "fpm_screen_add_job: the job's sketch size is not the screen's");
    if ((v.kp.use64 ? 8u : 4u) != sc->hash_bytes)
        return fail(FPM_EINVAL, "fpm_screen_add_job: the job's hash width is not the database's");
    hipStream_t st = pick_stream(ctx, stream);
    if (int rc = fpm_sketch_run(job, st)) return rc;
    // running row <- bottom-s of (running row, the job's row)
    const size_t rb = (size_t)sc->s * 8;
    HIP_TRY(hipMemcpyAsync(sc->d_pair + sc->s, v.d_rows, rb, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(sc->d_pcnt + 1, v.d_count, 4, hipMemcpyDeviceToDevice, st));
    if (int rc = fpm_sketch_merge_dev(ctx, sc->d_pair, sc->d_pcnt, 2, sc->s, sc->d_pair + 2 * (size_t)sc->s,
                                      sc->d_pcnt + 2, st))
        return rc;
    HIP_TRY(hipMemcpyAsync(sc->d_pair, sc->d_pair + 2 * (size_t)sc->s, rb, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(sc->d_pcnt, sc->d_pcnt + 2, 4, hipMemcpyDeviceToDevice, st));
    return for_each_class(v.class_begin, [&](int c, uint32_t b, uint32_t n) -> int {
        TimedLaunch tl(ctx, FPM_K_SCREEN, st);
        HIP_TRY(launch_screen_count(c, v.d_seq, v.d_tiles + b, n, v.kp, sc->tab, st));
        tl.done();
        return FPM_OK;
    });
}

int fpm_screen_add_hashes_dev(fpm_screen *sc, const uint64_t *d_keys, uint64_t n, void *stream)
{
    if (!sc || (n && !d_keys)) return fail(FPM_EINVAL, "fpm_screen_add_hashes_dev: null argument");
    if (int rc = set_device(sc->ctx)) return rc;
    HIP_TRY(launch_screen_hashes(d_keys, n, sc->tab, pick_stream(sc->ctx, stream)));
    return FPM_OK;
}

int fpm_screen_set_size(fpm_screen *sc, uint64_t *set_size)
{
    if (!sc || !set_size) return fail(FPM_EINVAL, "fpm_screen_set_size: null argument");
    fpm_ctx *ctx = sc->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t len = 0;
    HIP_TRY(copy_out(ctx, &len, sc->d_pcnt, 4));
    *set_size = 0;
    if (!len) return FPM_OK;
    uint64_t top = 0;
    HIP_TRY(copy_out(ctx, &top, sc->d_pair + (len - 1), 8));
    // MinHashHeap::estimateSetSize (MinHashHeap.h:45), truncated as CommandTaxScreen.cpp:370 stores it
    const double range = sc->hash_bytes == 8 ? 18446744073709551616.0 : 4294967296.0;
    const double e = range * (double)len / (double)top;
    *set_size = e < 18446744073709551616.0 ? (uint64_t)e : ~0ULL;
    return FPM_OK;
}

int fpm_screen_counts(fpm_screen *sc, uint64_t *out_keys, uint32_t *out_counts, uint64_t *n_distinct)
{
    if (!sc || !n_distinct) return fail(FPM_EINVAL, "fpm_screen_counts: null argument");
    fpm_ctx *ctx = sc->ctx;
    if (int rc = set_device(ctx)) return rc;
    *n_distinct = sc->tab.n;
    if (!sc->tab.n) return FPM_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (out_keys) HIP_TRY(copy_out(ctx, out_keys, sc->tab.U, (size_t)sc->tab.n * 8));
    if (out_counts) HIP_TRY(copy_out(ctx, out_counts, sc->tab.count, (size_t)sc->tab.n * 4));
    return FPM_OK;
}

int fpm_screen_rows(fpm_screen *sc, uint32_t *out_shared, uint32_t *out_median)
{
    if (!sc) return fail(FPM_EINVAL, "fpm_screen_rows: null argument");
    if (int rc = set_device(sc->ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());   // pool passes may have run on other streams
    return screen_rows(sc, nullptr, out_shared, out_median);
}

int fpm_screen_rows_winner(fpm_screen *sc, const double *scores, const uint64_t *lengths,
                           uint32_t *out_shared, uint32_t *out_median)
{
    if (!sc || (sc->n_db && (!scores || !lengths)))
        return fail(FPM_EINVAL, "fpm_screen_rows_winner: null argument");
    fpm_ctx *ctx = sc->ctx;
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (!sc->n_db) return screen_rows(sc, nullptr, out_shared, out_median);
    DevBufs mem(ctx);
    double *ds;
    uint64_t *dl;
    hipError_t e = mem.get(&ds, (size_t)sc->n_db * 8);
    if (e == hipSuccess) e = mem.get(&dl, (size_t)sc->n_db * 8);
    if (e == hipSuccess) e = copy_in(ctx, ds, scores, (size_t)sc->n_db * 8);
    if (e == hipSuccess) e = copy_in(ctx, dl, lengths, (size_t)sc->n_db * 8);
    if (e != hipSuccess) return fail(FPM_ENOMEM, std::string("screen -w staging: ") + hipGetErrorString(e));
    HIP_TRY(launch_screen_winner(sc->tab.count, sc->d_ustart, sc->d_post, sc->tab.n, ds, dl,
                                 sc->d_owner, ctx->stream));
    return screen_rows(sc, sc->d_owner, out_shared, out_median);
}

int fpm_screen_pvalues(fpm_screen *sc, const uint32_t *shared, double kmer_space, double *out_p)
{
    if (!sc || (sc->n_db && (!shared || !out_p)))
        return fail(FPM_EINVAL, "fpm_screen_pvalues: null argument");
    fpm_ctx *ctx = sc->ctx;
    uint64_t set_size = 0;
    if (int rc = fpm_screen_set_size(sc, &set_size)) return rc;
    if (!sc->n_db) return FPM_OK;
    double r = (double)set_size / kmer_space;
    r = std::max(0.0, std::min(1.0, r));
    DevBufs mem(ctx);
    uint32_t *dsh;
    double *dp;
    hipError_t e = mem.get(&dsh, (size_t)sc->n_db * 4);
    if (e == hipSuccess) e = mem.get(&dp, (size_t)sc->n_db * 8);
    if (e == hipSuccess) e = copy_in(ctx, dsh, shared, (size_t)sc->n_db * 4);
    if (e != hipSuccess) return fail(FPM_ENOMEM, std::string("screen p-value staging: ") + hipGetErrorString(e));
    {
        TimedLaunch tl(ctx, FPM_K_FINALIZE, ctx->stream);
        HIP_TRY(launch_screen_pvalues(dsh, sc->d_len, sc->n_db, r, dp, ctx->stream));
        tl.done();
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(copy_out(ctx, out_p, dp, (size_t)sc->n_db * 8));
    return FPM_OK;
}

int fpm_screen_tax(fpm_screen *sc, const uint32_t *parent, uint32_t n_nodes, uint32_t top,
                   const uint32_t *ref_node, uint32_t *out_lca, uint32_t *out_tax_hashes,
                   uint32_t *out_tax_count, uint32_t *out_clade_hashes, uint32_t *out_clade_count,
                   uint64_t out_totals[2])
{
    if (!sc || !out_totals || (n_nodes && !parent) || (sc->n_db && !ref_node))
        return fail(FPM_EINVAL, "fpm_screen_tax: null argument");
    fpm_ctx *ctx = sc->ctx;
    // node indices stay below the three reserved values and the fold's internal one
    if (n_nodes > 0xFFFFFFF0u) return fail(FPM_EINVAL, "fpm_screen_tax: too many nodes");
    if (top != FPM_TAX_UNKNOWN && top >= n_nodes)
        return fail(FPM_EINVAL, "fpm_screen_tax: top is not a node");
    for (uint32_t i = 0; i < sc->n_db; i++)
        if (ref_node[i] < FPM_TAX_UNKNOWN && ref_node[i] >= n_nodes)
            return fail(FPM_EINVAL, "fpm_screen_tax: a ref_node is not a node");
    // depth[v] = links from v to its root; a chain that does not end in FPM_TAX_ROOT within
    // n_nodes links is a cycle.  Chains are walked once: up to the first node whose depth is
    // known, then back down.
    constexpr uint32_t kUnset = 0xFFFFFFFFu;
    std::vector<uint32_t> depth(n_nodes, kUnset), path;
    for (uint32_t v = 0; v < n_nodes; v++) {
        if (parent[v] != FPM_TAX_ROOT && parent[v] >= n_nodes)
            return fail(FPM_EINVAL, "fpm_screen_tax: a parent index is out of range");
    }
    for (uint32_t v = 0; v < n_nodes; v++) {
        if (depth[v] != kUnset) continue;
        path.clear();
        uint32_t x = v, base = 0;
        for (;;) {
            if (path.size() > n_nodes) return fail(FPM_EINVAL, "fpm_screen_tax: the parent links hold a cycle");
            path.push_back(x);
            const uint32_t p = parent[x];
            if (p == FPM_TAX_ROOT) { base = 0; break; }
            if (depth[p] != kUnset) { base = depth[p] + 1; break; }
            x = p;
        }
        // path.back() has depth `base` (a cycle never reaches a break: the length bound ends it)
        for (size_t i = path.size(); i-- > 0;) depth[path[i]] = base + (uint32_t)(path.size() - 1 - i);
    }
    if (int rc = set_device(ctx)) return rc;
    HIP_TRY(hipDeviceSynchronize());   // pool passes may have run on other streams
    hipStream_t st = ctx->stream;
    const uint32_t nU = sc->tab.n;
    const size_t nb = (size_t)n_nodes * 4;
    DevBufs mem(ctx);
    uint32_t *dpar, *ddep, *dref, *dlca, *c0;
    unsigned long long *d_tot;
    hipError_t e = mem.upload(ctx, &dpar, parent, nb);
    if (e == hipSuccess) e = mem.upload(ctx, &ddep, depth.data(), nb);
    if (e == hipSuccess) e = mem.upload(ctx, &dref, ref_node, (size_t)sc->n_db * 4);
    if (e == hipSuccess) e = mem.get(&dlca, (size_t)nU * 4);
    if (e == hipSuccess) e = mem.get(&c0, 4 * nb);     // tax_hashes, tax_count, clade_hashes, clade_count
    if (e == hipSuccess) e = mem.get(&d_tot, 16);      // totals[0], the wave's entries
    if (e != hipSuccess) return fail(FPM_ENOMEM, std::string("taxscreen staging: ") + hipGetErrorString(e));
    HIP_TRY(hipMemsetAsync(c0, 0, std::max<size_t>(4 * nb, 16), st));
    HIP_TRY(hipMemsetAsync(d_tot, 0, 16, st));
    TaxTree t;
    t.parent = dpar;
    t.depth = ddep;
    t.n_nodes = n_nodes;
    t.top = top;
    uint32_t *c1 = c0 + n_nodes, *c2 = c1 + n_nodes, *c3 = c2 + n_nodes;
    ctx->last_tax_kernel = FPM_TK_NONE;
    {
        TimedLaunch tl(ctx, FPM_K_COMPARE, st);
        HIP_TRY(launch_tax_lca(sc->tab.count, sc->d_ustart, sc->d_post, nU, dref, t, dlca, c0, c1, d_tot, (uint32_t *)(d_tot + 1), st));
        tl.done();
    }
    {
        TimedLaunch tl(ctx, FPM_K_FINALIZE, st);
        HIP_TRY(launch_tax_clade(t, c0, c1, c2, c3, st));
        tl.done();
    }
    HIP_TRY(hipStreamSynchronize(st));
    unsigned long long host[2] = {0, 0};
    HIP_TRY(copy_out(ctx, host, d_tot, 16));
    if (nU) ctx->last_tax_kernel = (uint32_t)host[1] ? FPM_TK_WAVE : FPM_TK_THREAD;
    out_totals[0] = host[0];
    out_totals[1] = nU;
    if (out_lca && nU) HIP_TRY(copy_out(ctx, out_lca, dlca, (size_t)nU * 4));
    uint32_t *outs[4] = {out_tax_hashes, out_tax_count, out_clade_hashes, out_clade_count};
    const uint32_t *srcs[4] = {c0, c1, c2, c3};
    for (int i = 0; i < 4; i++)
        if (outs[i] && n_nodes) HIP_TRY(copy_out(ctx, outs[i], srcs[i], nb));
    return FPM_OK;
}

int fpm_ctx_last_tax_kernel(fpm_ctx *ctx, int *kernel)
{
    if (!ctx || !kernel) return fail(FPM_EINVAL, "null argument");
    *kernel = ctx->last_tax_kernel;
    return FPM_OK;
}

int fpm_screen_tax_wave_cut(fpm_ctx *ctx, uint32_t *cut)
{
    if (!ctx || !cut) return fail(FPM_EINVAL, "null argument");
    *cut = kTaxWaveCut;
    return FPM_OK;
}

int fpm_ctx_last_screen_kernel(fpm_ctx *ctx, int *kernel)
{
    if (!ctx || !kernel) return fail(FPM_EINVAL, "null argument");
    *kernel = ctx->last_screen_kernel;
    return FPM_OK;
}

int fpm_screen_table_info(fpm_screen *sc, uint64_t *cells, uint64_t *n_distinct, uint32_t *sbits,
                          uint32_t *dbits)
{
    if (!sc) return fail(FPM_EINVAL, "fpm_screen_table_info: null argument");
    if (cells) *cells = sc->E;
    if (n_distinct) *n_distinct = sc->tab.n;
    if (sbits) *sbits = sc->sbits;
    if (dbits) *dbits = sc->tab.dbits;
    return FPM_OK;
}

int fpm_screen_lds_cap(fpm_ctx *ctx, uint32_t *cap)
{
    if (!ctx || !cap) return fail(FPM_EINVAL, "null argument");
    *cap = kScreenRowsLdsCap;
    return FPM_OK;
}

}  // extern "C"
