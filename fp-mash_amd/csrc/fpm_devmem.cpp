// fpm_devmem.cpp — who frees device memory in the C ABI files: the context's pool of released
// buffers, the grow-only slots, and DevBufs, the owner every handle and staging call keeps its
// buffers in (fpm_internal.hpp).  Nothing here launches a kernel, so the file links without the
// kernel objects (tools/devmem_check.cpp).
#include "fpm_internal.hpp"

// smallest pooled buffer of >= bytes (and at most 4x: a 1 GB buffer is not kept busy by a
// 1 KB request), else a new one
hipError_t pool_alloc(fpm_ctx *ctx, void **p, size_t bytes)
{
    {
        std::lock_guard<std::mutex> g(ctx->pool_mu);
        size_t best = SIZE_MAX, bi = 0;
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
            return hipSuccess;
        }
    }
    return hipMalloc(p, bytes);
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
hipError_t grow_slot(fpm_ctx::Slot &s, size_t bytes, void **out)
{
    if (s.bytes < bytes) {
        if (s.p) { hipError_t e = hipFree(s.p); if (e != hipSuccess) return e; }
        s.p = nullptr;
        s.bytes = 0;
        size_t b = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&s.p, b);
        if (e != hipSuccess) return e;
        s.bytes = b;
    }
    *out = s.p;
    return hipSuccess;
}

hipError_t DevBufs::take(void **out, size_t bytes, bool pooled)
{
    *out = nullptr;
    bytes = bytes ? bytes : 16;
    void *q = nullptr;
    const hipError_t e = pooled ? pool_alloc(ctx, &q, bytes) : hipMalloc(&q, bytes);
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
