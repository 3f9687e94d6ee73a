// fpm_devmem.cpp — who frees device memory in the C ABI files: the context's pool of released
// buffers, the grow-only slots, and DevBufs, the owner every handle and staging call keeps its
// buffers in (fpm_internal.hpp).  Nothing here launches a kernel, so the file links without the
// kernel objects (tools/devmem_check.cpp).
#include "fpm_internal.hpp"

// fpm_ctx_set_poison: a buffer about to be handed out is filled with the context's poison byte,
// the context stream synchronised before it leaves (off, or an owner without a context: nothing)
hipError_t poison_fill(fpm_ctx *ctx, void *p, size_t bytes)
{
    if (!ctx || ctx->poison < 0 || !p || !bytes) return hipSuccess;
    hipError_t e = hipMemsetAsync(p, ctx->poison, bytes, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}

// smallest pooled buffer of >= bytes (and at most 4x: a 1 GB buffer is not kept busy by a
// 1 KB request), else a new one
hipError_t pool_alloc(fpm_ctx *ctx, void **p, size_t bytes)
{
    size_t best = SIZE_MAX;
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        size_t bi = 0;
        for (size_t i = 0; i < ctx->pool.size(); i++) {
            const size_t b = ctx->pool[i].second;
            if (b >= bytes && b <= 4 * bytes + 4096 && b < best) { best = b; bi = i; }
            if (best == bytes) break;
        }
        if (best != SIZE_MAX) {
            *p = ctx->pool[bi].first;
            ctx->pool_bytes -= best;
            ctx->pool[bi] = ctx->pool.back();
            ctx->pool.pop_back();
        }
    }
    if (best != SIZE_MAX) {
        // (the bytes asked for: the buffer goes back to the pool at that size)
        const hipError_t e = poison_fill(ctx, *p, bytes);
        if (e != hipSuccess) {   // not handed out: the pool keeps it, at its own size
            std::lock_guard<std::mutex> g(ctx->pool_mu);
            ctx->pool.push_back({*p, best});
            ctx->pool_bytes += best;
            *p = nullptr;
        }
        return e;
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && (e = poison_fill(ctx, *p, bytes)) != hipSuccess) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    return e;
}

// back to the pool (the caller's stream work on it is complete), or freed past kPoolBytes
void pool_free(fpm_ctx *ctx, void *p, size_t bytes)
{
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        if (ctx->pool_bytes + bytes <= fpm_ctx::kPoolBytes) {
            ctx->pool.push_back({p, bytes});
            ctx->pool_bytes += bytes;
            return;
        }
    }
    (void)hipFree(p);
}

fpm_ctx::Slot::~Slot()
{
    if (p) (void)hipFree(p);
}

// a device buffer of at least `bytes` in the grow-only slot `s` (12 % headroom on growth)
hipError_t grow_slot(fpm_ctx *ctx, fpm_ctx::Slot &s, size_t bytes, void **out)
{
    if (s.bytes < bytes) {
        if (s.p) { hipError_t e = hipFree(s.p); if (e != hipSuccess) return e; }
        s.p = nullptr;
        s.bytes = 0;
        size_t b = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&s.p, b);
        if (e != hipSuccess) return e;
        s.bytes = b;
        if ((e = poison_fill(ctx, s.p, b)) != hipSuccess) return e;
    }
    *out = s.p;
    return hipSuccess;
}

hipError_t DevBufs::take(void **out, size_t bytes, bool pooled)
{
    *out = nullptr;
    bytes = bytes ? bytes : 16;
    void *q = nullptr;
    hipError_t e = pooled ? pool_alloc(ctx, &q, bytes) : hipMalloc(&q, bytes);
    if (e == hipSuccess && !pooled && (e = poison_fill(ctx, q, bytes)) != hipSuccess) (void)hipFree(q);
    if (e != hipSuccess) return e;
    held_.push_back({q, bytes, pooled});
    *out = q;
    return hipSuccess;
}

void DevBufs::free_buf(const Buf &b)
{
    if (b.pooled) pool_free(ctx, b.p, b.bytes);
    else (void)hipFree(b.p);
}

bool DevBufs::remove(const void *p, bool free_it)
{
    for (size_t i = 0; i < held_.size(); i++) {
        if (held_[i].p != p) continue;
        if (free_it) free_buf(held_[i]);
        held_.erase(held_.begin() + i);
        return true;
    }
    return false;
}

void DevBufs::absorb(DevBufs &&o)
{
    held_.insert(held_.end(), o.held_.begin(), o.held_.end());
    o.held_.clear();
}

DevBufs::~DevBufs()
{
    for (const Buf &b : held_) free_buf(b);
}
