// screen_table.hpp — the lookup table of `screen` (screen.hip builds it, the count kernel in
// sketch.hip and the hash-list kernel in screen.hip read it): U, the sorted distinct union of
// every hash of the sketch database (u32 hashes zero-extended), one u32 counter per entry, and a
// bucket directory over U.  With U's largest entry shifted up to bit 63, bucket(v) = the top
// `dbits` bits of v shifted likewise (the scale of IdxGeom::kmax / contain_rows_kernel) and
// dir[b] = the first position of U whose bucket is >= b (dir[2^dbits] = n).  bucket() is
// monotone, so a key <= umax can only sit in [dir[bucket], dir[bucket + 1]).  Buckets may be of
// any length (clustered values): a long one is bisected, the result is exact for any U.
#pragma once

#include <stdint.h>

namespace fpm {

struct ScreenTable {
    const uint64_t *U = nullptr;
    const uint32_t *dir = nullptr;   // 2^dbits + 1 entries
    uint32_t *count = nullptr;       // count[u]: windows whose key is U[u] (hashSequence's
                                     // hashCounts, CommandScreen.cpp:366-369; wraps at 2^32)
    uint32_t n = 0;                  // |U|
    uint32_t dbits = 1, shift = 63;
    uint64_t umax = 0;               // U[n - 1]
};

constexpr uint32_t kScreenMiss = 0xFFFFFFFFu;

#if defined(__HIPCC__)
// the position of `key` in U, kScreenMiss when U does not hold it
__device__ __forceinline__ uint32_t screen_lookup(const ScreenTable &t, uint64_t key)
{
    if (t.n == 0 || key > t.umax) return kScreenMiss;
    const uint32_t b = (uint32_t)((key << t.shift) >> (64 - t.dbits));
    uint32_t lo = t.dir[b], hi = t.dir[b + 1];
    const uint32_t end = hi;
    // the first entry >= key lies in [lo, hi] throughout (hi itself when U[hi] was compared)
    while (hi - lo > 4) {
        const uint32_t mid = (lo + hi) >> 1;
        if (t.U[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    for (; lo < end; lo++) {
        const uint64_t x = t.U[lo];
        if (x >= key) return x == key ? lo : kScreenMiss;
    }
    return kScreenMiss;
}
#endif

}  // namespace fpm
