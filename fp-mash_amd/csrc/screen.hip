// screen.hip — the database side of `screen` for gfx950: the table build over the sketch
// database (the hashTable / hashCounts maps CommandScreen.cpp:87-102 fills hash by hash), the
// hash-list count kernel, the per-reference sums (shared count and median depth,
// CommandScreen.cpp:133-151, 208-211, 235) and the -w winner pass (:153-202).  The pool pass that
// hashes sequence windows into the counters (hashSequence, :280-384) is screen_count_kernel
// in sketch.hip, beside the tile staging it shares with the sketch kernels.
//
// Table build, once per database (rows strictly ascending, checked by launch_rows_ascending):
//   1. kmax = the largest last entry of a row (the bucket scale)
//   2. counting sort of every cell by the top `sbits` bits of key / kmax: histogram,
//      launch_exscan, scatter (key, cell)
//   3. each key's rank inside its bucket (ties by scatter position) -> sorted (key, cell)
//   4. heads of runs of equal keys, launch_exscan -> U, the postings' start per entry
//      (the cells of one entry are contiguous in the sort: its holders), the slot of every cell
//   5. the directory over U (screen_table.hpp)
// Step 3 reads a bucket once per key of the bucket: linear for hash-like rows (~2 keys per
// bucket), quadratic in the length of a bucket of clustered values (still exact).
#include "fpm_kernels.hpp"
#include "screen_table.hpp"

namespace fpm {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ uint32_t sort_bucket(uint64_t v, uint32_t shift, uint32_t sbits)
{
    return (uint32_t)((v << shift) >> (64 - sbits));
}

// kmax[0] = max over rows of their last entry (rows ascend); one thread per row
template <typename T>
__global__ __launch_bounds__(kThreads) void screen_kmax_kernel(
    const T *__restrict__ db, const uint32_t *__restrict__ len, uint64_t stride, uint32_t n_db,
    unsigned long long *__restrict__ kmax)
{
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_db) return;
    const uint32_t l = len[r];
    if (l) atomicMax(kmax, (unsigned long long)db[(uint64_t)r * stride + l - 1]);
}

// one workgroup per row.  SCATTER = false: hist[bucket]++; true: (key, cell) to
// start[bucket] + the bucket's fill count
template <typename T, bool SCATTER>
__global__ __launch_bounds__(kThreads) void screen_sort_kernel(
    const T *__restrict__ db, const uint32_t *__restrict__ len, uint64_t stride,
    const unsigned long long *__restrict__ kmax, uint32_t sbits, uint32_t *__restrict__ hist,
    const uint32_t *__restrict__ start, uint64_t *__restrict__ skey, uint32_t *__restrict__ scell)
{
    const uint32_t r = blockIdx.x;
    const uint32_t l = len[r];
    const uint64_t top = *kmax;
    const uint32_t shift = top ? (uint32_t)__clzll((long long)top) : 63u;
    const T *row = db + (uint64_t)r * stride;
    for (uint32_t i = threadIdx.x; i < l; i += kThreads) {
        const uint64_t v = (uint64_t)row[i];
        const uint32_t b = sort_bucket(v, shift, sbits);
        if (!SCATTER) atomicAdd(&hist[b], 1u);
        else {
            const uint32_t at = start[b] + atomicAdd(&hist[b], 1u);
            skey[at] = v;
            scell[at] = (uint32_t)((uint64_t)r * stride + i);
        }
    }
}

// sorted position of scattered element p: its bucket's start + the keys of the bucket below
// it (ties by scattered position)
__global__ __launch_bounds__(kThreads) void screen_rank_kernel(
    const uint64_t *__restrict__ skey, const uint32_t *__restrict__ scell, uint32_t E,
    const unsigned long long *__restrict__ kmax, uint32_t sbits,
    const uint32_t *__restrict__ start, const uint32_t *__restrict__ fill,
    uint64_t *__restrict__ okey, uint32_t *__restrict__ ocell)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= E) return;
    const uint64_t top = *kmax;
    const uint32_t shift = top ? (uint32_t)__clzll((long long)top) : 63u;
    const uint64_t key = skey[p];
    const uint32_t b = sort_bucket(key, shift, sbits);
    const uint32_t s0 = start[b], s1 = s0 + fill[b];
    uint32_t r = 0;
    for (uint32_t t = s0; t < s1; t++) {
        const uint64_t y = skey[t];
        r += (y < key) | ((y == key) & (t < p));
    }
    okey[s0 + r] = key;
    ocell[s0 + r] = scell[p];
}

__global__ __launch_bounds__(kThreads) void screen_heads_kernel(const uint64_t *__restrict__ okey,
                                                              uint32_t E, uint32_t *__restrict__ head)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= E) return;
    head[p] = (p == 0 || okey[p] != okey[p - 1]) ? 1u : 0u;
}

// hx = the exclusive scan of head: sorted element p belongs to entry u = hx[p] + head[p] - 1
__global__ __launch_bounds__(kThreads) void screen_compact_kernel(
    const uint64_t *__restrict__ okey, const uint32_t *__restrict__ ocell,
    const uint32_t *__restrict__ head, const uint32_t *__restrict__ hx, uint32_t E,
    uint64_t stride, uint64_t *__restrict__ U, uint32_t *__restrict__ ustart,
    uint32_t *__restrict__ slot, uint32_t *__restrict__ post)
{
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= E) return;
    const uint32_t h = head[p], u = hx[p] + h - 1;
    const uint32_t cell = ocell[p];
    if (h) {
        U[u] = okey[p];
        ustart[u] = p;
    }
    if (p == E - 1) ustart[u + 1] = E;
    slot[cell] = u;
    post[p] = (uint32_t)(cell / stride);
}

__global__ __launch_bounds__(kThreads) void screen_dir_kernel(const uint64_t *__restrict__ U,
                                                            uint32_t n, uint32_t dbits,
                                                            uint32_t shift, uint32_t *__restrict__ dir)
{
    const uint32_t b = blockIdx.x * kThreads + threadIdx.x;
    const uint32_t nb = 1u << dbits;
    if (b > nb) return;
    uint32_t lo = 0, hi = n;
    if (b == nb) lo = n;
    else {
        // the smallest value of bucket b: ceil((b << (64 - dbits)) / 2^shift)
        const uint64_t x = (uint64_t)b << (64 - dbits);
        const uint64_t tb = (x >> shift) + ((x & ((1ull << shift) - 1)) != 0);
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (U[mid] < tb) lo = mid + 1;
            else hi = mid;
        }
    }
    dir[b] = lo;
}

// one lane per key of a plain device array: the lookup of the count pass without the hashing
__global__ __launch_bounds__(kThreads) void screen_hashes_kernel(const uint64_t *__restrict__ keys,
                                                               uint64_t n, ScreenTable t)
{
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t u = screen_lookup(t, keys[i]);
    if (u != kScreenMiss) atomicAdd(&t.count[u], 1u);
}

// One workgroup per reference: shared = its cells whose counter is >= 1 (with `owner`, only
// the cells whose entry this row won), median = the depth at position shared / 2 of those
// counters in ascending order (depths[i].at(shared[i] / 2), CommandScreen.cpp:235), by a 4-pass
// 256-bin radix selection over the u32 counters, most significant byte first.  LDS: the row's
// counters are gathered once into LDS; otherwise every pass gathers them again from global
// memory.
template <bool LDS>
__global__ __launch_bounds__(kThreads) void screen_rows_kernel(
    const uint32_t *__restrict__ slot, const uint32_t *__restrict__ len, uint64_t stride,
    const uint32_t *__restrict__ count, const uint32_t *__restrict__ owner,
    uint32_t *__restrict__ out_shared, uint32_t *__restrict__ out_median)
{
    __shared__ uint32_t vals[LDS ? kScreenRowsLdsCap : 1];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t red[kWaves];
    __shared__ uint32_t s_prefix, s_rank;
    const uint32_t row = blockIdx.x, n = len[row], tid = threadIdx.x;
    const uint32_t *srow = slot + (uint64_t)row * stride;
    auto gather = [&](uint32_t i) -> uint32_t {
        const uint32_t u = srow[i];
        return (owner && owner[u] != row) ? 0u : count[u];
    };
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n; i += kThreads) {
        const uint32_t c = gather(i);
        if (LDS) vals[i] = c;
        mine += c ? 1u : 0u;
    }
    for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = mine;
    __syncthreads();
    uint32_t shared = 0;
    for (int w = 0; w < kWaves; w++) shared += red[w];
    if (shared == 0) {                                     // block-uniform
        if (tid == 0) { out_shared[row] = 0; out_median[row] = 0; }
        return;
    }
    if (tid == 0) { s_prefix = 0; s_rank = shared / 2; }
    uint32_t mask = 0;
    for (int pass = 3; pass >= 0; pass--) {
        hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        for (uint32_t i = tid; i < n; i += kThreads) {
            const uint32_t c = LDS ? vals[i] : gather(i);
            if (c && (c & mask) == prefix) atomicAdd(&hist[(c >> (8 * pass)) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t rank = s_rank, b = 0;
            while (b < 255 && rank >= hist[b]) rank -= hist[b++];
            s_rank = rank;
            s_prefix = prefix | (b << (8 * pass));
        }
        mask |= 0xffu << (8 * pass);
        __syncthreads();
    }
    if (tid == 0) { out_shared[row] = shared; out_median[row] = s_prefix; }
}

// -w: per entry of U seen in the pool, the one reference among its holders (post[ustart[u] ..
// ustart[u + 1])) that keeps it: the greatest score, then the greatest Reference::length
// (CommandScreen.cpp:182-195), then the lowest index (in place of the reference's
// unordered-set visiting order).  Scores are the host's doubles, only compared here.
__global__ __launch_bounds__(kThreads) void screen_winner_kernel(
    const uint32_t *__restrict__ count, const uint32_t *__restrict__ ustart,
    const uint32_t *__restrict__ post, uint32_t n, const double *__restrict__ scores,
    const uint64_t *__restrict__ lengths, uint32_t *__restrict__ owner)
{
    const uint32_t u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= n) return;
    uint32_t best = kScreenMiss;
    if (count[u]) {
        double bs = 0;
        uint64_t bl = 0;
        for (uint32_t p = ustart[u], e = ustart[u + 1]; p < e; p++) {
            const uint32_t r = post[p];
            const double sc = scores[r];
            const uint64_t l = lengths[r];
            if (best == kScreenMiss || sc > bs ||
                (sc == bs && (l > bl || (l == bl && r < best)))) {
                best = r;
                bs = sc;
                bl = l;
            }
        }
    }
    owner[u] = best;
}

inline dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + kThreads - 1) / kThreads)); }

}  // namespace

hipError_t launch_screen_sort(const void *d_db, const uint32_t *d_len, uint64_t stride,
                              uint32_t n_db, uint32_t hash_bytes, uint32_t E, uint32_t sbits,
                              unsigned long long *kmax, uint32_t *hist, uint32_t *start,
                              uint32_t *scan_s, uint64_t *skey, uint32_t *scell, uint64_t *okey,
                              uint32_t *ocell, hipStream_t st)
{
    if (!n_db || !E) return hipSuccess;
    if (hash_bytes != 4 && hash_bytes != 8) return hipErrorInvalidValue;
    const uint64_t nb = 1ull << sbits;
    hipError_t e;
    if ((e = hipMemsetAsync(kmax, 0, 8, st))) return e;
    if ((e = hipMemsetAsync(hist, 0, nb * 4, st))) return e;
#define FPM_SCREEN_T(T)                                                                          \
    do {                                                                                         \
        const T *db = (const T *)d_db;                                                           \
        hipLaunchKernelGGL(screen_kmax_kernel<T>, grid_for(n_db), dim3(kThreads), 0, st, db,     \
                           d_len, stride, n_db, kmax);                                           \
        hipLaunchKernelGGL((screen_sort_kernel<T, false>), dim3(n_db), dim3(kThreads), 0, st, db, \
                           d_len, stride, kmax, sbits, hist, nullptr, nullptr, nullptr);         \
        if ((e = launch_exscan(hist, start, nullptr, nb, scan_s, nullptr, st))) return e;        \
        if ((e = hipMemsetAsync(hist, 0, nb * 4, st))) return e;                                 \
        hipLaunchKernelGGL((screen_sort_kernel<T, true>), dim3(n_db), dim3(kThreads), 0, st, db, \
                           d_len, stride, kmax, sbits, hist, start, skey, scell);                \
    } while (0)
    if (hash_bytes == 8) FPM_SCREEN_T(uint64_t);
    else FPM_SCREEN_T(uint32_t);
#undef FPM_SCREEN_T
    hipLaunchKernelGGL(screen_rank_kernel, grid_for(E), dim3(kThreads), 0, st, skey, scell, E, kmax,
                       sbits, start, hist, okey, ocell);
    return hipGetLastError();
}

hipError_t launch_screen_heads(const uint64_t *okey, uint32_t E, uint32_t *head, uint32_t *hx,
                               uint32_t *scan_s, uint32_t *n_distinct, hipStream_t st)
{
    if (!E) return hipSuccess;
    hipLaunchKernelGGL(screen_heads_kernel, grid_for(E), dim3(kThreads), 0, st, okey, E, head);
    return launch_exscan(head, hx, nullptr, E, scan_s, n_distinct, st);
}

hipError_t launch_screen_compact(const uint64_t *okey, const uint32_t *ocell, const uint32_t *head,
                                 const uint32_t *hx, uint32_t E, uint64_t stride, uint32_t n,
                                 uint32_t dbits, uint32_t shift, uint64_t *U, uint32_t *ustart,
                                 uint32_t *slot, uint32_t *post, uint32_t *dir, hipStream_t st)
{
    if (!E) return hipSuccess;
    hipLaunchKernelGGL(screen_compact_kernel, grid_for(E), dim3(kThreads), 0, st, okey, ocell, head,
                       hx, E, stride, U, ustart, slot, post);
    hipLaunchKernelGGL(screen_dir_kernel, grid_for((1ull << dbits) + 1), dim3(kThreads), 0, st, U,
                       n, dbits, shift, dir);
    return hipGetLastError();
}

hipError_t launch_screen_hashes(const uint64_t *d_keys, uint64_t n, const ScreenTable &t,
                                hipStream_t st)
{
    if (!n || !t.n) return hipSuccess;
    if ((n + kThreads - 1) / kThreads > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(screen_hashes_kernel, grid_for(n), dim3(kThreads), 0, st, d_keys, n, t);
    return hipGetLastError();
}

hipError_t launch_screen_rows(const uint32_t *d_slot, const uint32_t *d_len, uint64_t stride,
                              uint32_t n_db, uint32_t max_len, const uint32_t *d_count,
                              const uint32_t *d_owner, uint32_t *d_shared, uint32_t *d_median,
                              hipStream_t st, bool *lds)
{
    if (lds) *lds = false;
    if (!n_db) return hipSuccess;
    const bool in_lds = max_len <= kScreenRowsLdsCap;
    if (lds) *lds = in_lds;
    if (in_lds)
        hipLaunchKernelGGL(screen_rows_kernel<true>, dim3(n_db), dim3(kThreads), 0, st, d_slot,
                           d_len, stride, d_count, d_owner, d_shared, d_median);
    else
        hipLaunchKernelGGL(screen_rows_kernel<false>, dim3(n_db), dim3(kThreads), 0, st, d_slot,
                           d_len, stride, d_count, d_owner, d_shared, d_median);
    return hipGetLastError();
}

hipError_t launch_screen_winner(const uint32_t *d_count, const uint32_t *d_ustart,
                                const uint32_t *d_post, uint32_t n, const double *d_scores,
                                const uint64_t *d_lengths, uint32_t *d_owner, hipStream_t st)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(screen_winner_kernel, grid_for(n), dim3(kThreads), 0, st, d_count, d_ustart,
                       d_post, n, d_scores, d_lengths, d_owner);
    return hipGetLastError();
}

}  // namespace fpm
