// devmem_check.cpp — the bookkeeping of DevBufs and the context's buffer pool (csrc/fpm_devmem.cpp)
// on a machine without a device: every hipMalloc fails there, and the addresses the owner is
// given are made up and taken back before it could free them.  Built with a host sanitizer by
// tests/test_devmem_host.py; prints "devmem ok" and exits 0, or names the first check that failed.
#include "../csrc/fpm_internal.hpp"

#include <cstdio>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "devmem_check:%d: %s\n", __LINE__, #cond);     \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static void *made_up(uintptr_t v) { return reinterpret_cast<void *>(v); }

int main()
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) {
        fprintf(stderr, "devmem_check: a device is visible, nothing checked\n");
        return 2;
    }
    void *const a = made_up(0x1000), *const b = made_up(0x2000), *const c = made_up(0x3000);
    {   // a failed get: the error comes back, the pointer is null, nothing is recorded
        DevBufs m;
        uint32_t *p = reinterpret_cast<uint32_t *>(a);
        CHECK(m.get(&p, 64) != hipSuccess);
        CHECK(p == nullptr);
        CHECK(m.held().empty());
    }
    {   // adopt / release, and a release of what is not held
        DevBufs m;
        m.adopt(a);
        CHECK(m.held().size() == 1 && m.held()[0].p == a && !m.held()[0].pooled);
        CHECK(m.release(b) == nullptr);
        CHECK(m.held().size() == 1);
        CHECK(m.release(a) == a);
        CHECK(m.held().empty());
        CHECK(m.release(a) == nullptr);
        void *q = b;          // drop of what is not held only nulls the field
        m.drop(q);
        CHECK(q == nullptr && m.held().empty());
    }
    {   // move construction and the move-merge: the source is left empty, the order is kept
        DevBufs m1;
        m1.adopt(a);
        m1.adopt(b);
        DevBufs m2(std::move(m1));
        CHECK(m1.held().empty());
        CHECK(m2.held().size() == 2 && m2.held()[0].p == a && m2.held()[1].p == b);
        DevBufs m3;
        m3.adopt(c);
        m3.absorb(std::move(m2));
        CHECK(m2.held().empty());
        CHECK(m3.held().size() == 3 && m3.held()[0].p == c && m3.held()[1].p == a &&
              m3.held()[2].p == b);
        CHECK(m3.release(a) == a && m3.release(b) == b && m3.release(c) == c);
        CHECK(m3.held().empty());
    }
    {   // pooled: taken from the pool without an allocation, put back by the destructor
        fpm_ctx ctx;
        ctx.pool.push_back({a, 4096});
        ctx.pool_bytes = 4096;
        {
            DevBufs m(&ctx);
            uint8_t *p = nullptr;
            CHECK(m.get_pooled(&p, 4096) == hipSuccess);
            CHECK(p == a);
            CHECK(ctx.pool.empty() && ctx.pool_bytes == 0);
            CHECK(m.held().size() == 1 && m.held()[0].pooled && m.held()[0].bytes == 4096);
        }
        CHECK(ctx.pool.size() == 1 && ctx.pool[0].first == a && ctx.pool[0].second == 4096);
        CHECK(ctx.pool_bytes == 4096);
        // a request the pool cannot serve goes to hipMalloc and fails here
        {
            DevBufs m(&ctx);
            uint8_t *p = nullptr;
            CHECK(m.get_pooled(&p, 1u << 20) != hipSuccess);
            CHECK(p == nullptr && m.held().empty() && ctx.pool.size() == 1);
        }
        // a zero-byte request asks the pool for 16 bytes: the 16-byte entry, recorded as 16
        ctx.pool.push_back({b, 16});
        ctx.pool_bytes += 16;
        {
            DevBufs m(&ctx);
            uint8_t *p = nullptr;
            CHECK(m.get_pooled(&p, 0) == hipSuccess);
            CHECK(p == b);
            CHECK(m.held().size() == 1 && m.held()[0].bytes == 16);
            CHECK(ctx.pool.size() == 1 && ctx.pool_bytes == 4096);
            m.drop(p);        // back to the pool now
            CHECK(p == nullptr && m.held().empty());
            CHECK(ctx.pool.size() == 2 && ctx.pool_bytes == 4096 + 16);
        }
        CHECK(ctx.pool.size() == 2 && ctx.pool[1].first == b && ctx.pool[1].second == 16);
        ctx.pool.clear();     // made-up addresses: nothing to free
    }
    {   // poison on (fpm_ctx_set_poison): without a device the fill of a pooled buffer fails, so
        // the buffer is not handed out and the pool keeps it at its own size
        fpm_ctx ctx;
        ctx.poison = 0xA5;
        CHECK(poison_fill(nullptr, a, 64) == hipSuccess);     // no context: nothing to do
        CHECK(poison_fill(&ctx, nullptr, 64) == hipSuccess);
        CHECK(poison_fill(&ctx, a, 0) == hipSuccess);
        CHECK(poison_fill(&ctx, a, 64) != hipSuccess);
        ctx.pool.push_back({a, 8192});
        ctx.pool.push_back({b, 4096});
        ctx.pool_bytes = 8192 + 4096;
        {
            DevBufs m(&ctx);
            uint8_t *p = reinterpret_cast<uint8_t *>(c);
            CHECK(m.get_pooled(&p, 4000) != hipSuccess);      // picks b (the smallest that fits)
            CHECK(p == nullptr && m.held().empty());
            CHECK(ctx.pool.size() == 2 && ctx.pool_bytes == 8192 + 4096);
            CHECK(ctx.pool[0].first == a && ctx.pool[0].second == 8192);
            CHECK(ctx.pool[1].first == b && ctx.pool[1].second == 4096);
            // past the pool and a plain get: hipMalloc fails before any fill
            CHECK(m.get_pooled(&p, 1u << 20) != hipSuccess);
            CHECK(m.get(&p, 64) != hipSuccess);
            CHECK(p == nullptr && m.held().empty() && ctx.pool.size() == 2);
        }
        // a slot that cannot grow stays empty
        fpm_ctx::Slot s;
        void *out = c;
        CHECK(grow_slot(&ctx, s, 64, &out) != hipSuccess);
        CHECK(s.p == nullptr && s.bytes == 0);
        // off again: the pool hands out as before
        ctx.poison = -1;
        {
            DevBufs m(&ctx);
            uint8_t *p = nullptr;
            CHECK(m.get_pooled(&p, 4000) == hipSuccess);
            CHECK(p == b && ctx.pool.size() == 1 && ctx.pool_bytes == 8192);
            CHECK(m.release(p) == p);
        }
        ctx.pool.clear();
    }
    puts("devmem ok");
    return 0;
}
