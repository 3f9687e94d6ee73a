// contain.hip — the per-pair walk of `contain` (containSketches, CommandContain.cpp:368-412)
// over the whole ref x query grid, for gfx950.
//
//     common = 0; denom = min(lr, lq); i = j = 0
//     for (steps = 0; steps < denom && i < lr; steps++)
//         if      R[i] < Q[j]  { i++; steps--; }
//         else if Q[j] < R[i]  { j++; }
//         else                 { i++; j++; common++; }
//     -> (common, j)
//
// steps == j throughout (a step that only advances i is taken back), so the loop is
// "while (j < denom && i < lr)" and Q[j] is never read at or past denom.
//
// For strictly ascending lists the result has an order-free form.  The walk leaves Q entries
// behind one by one, each either matched or passed by a larger R entry, and stops when j
// reaches denom or R is exhausted; R is exhausted exactly when the next Q entry is larger than
// R's maximum.  So with m = min(lr, lq): (0, 0) when m == 0, else
//     jf = min(m, #{q in Q : q <= R[lr - 1]}),  j = jf,  common = |Q[0..jf) n R|.
// contain_rows_kernel computes that with one wave per ref row; contain_literal_kernel is the
// walk as written, one lane per pair, for lists in any order (-fp sketches) and as the
// cross-check of the fast kernel; rows_ascending_kernel tells the host which one applies.
#include "fpm_device.hpp"
#include "fpm_kernels.hpp"
#include "../../include/fpmash.h"

#include <algorithm>
#include <atomic>

namespace fpm {

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kBlockRefs = FPM_CONTAIN_BLOCK_REFS;   // ref rows per workgroup
static_assert(kBlockRefs % kWaves == 0 && kBlockRefs <= kThreads, "one wave per ref row at a time");
constexpr uint32_t kMaxLds = 156 * 1024;    // dynamic LDS asked for (160 KB per CU on gfx950)
constexpr uint32_t kDefLds = 63 * 1024;     // without the attribute: 64 KB with the static part
// the staged row starts at its global 16-B residue (<= 12 B of padding before it) and is
// followed by two spare entries that the lookup may read (2 x 8 B)
constexpr uint32_t kLdsPad = 32;
// the staged row's bucket directory: 2^bbits + 1 u32, 2^bbits >= twice the longest row where
// kDirBitsMax allows; its largest size is always set aside, so the cap does not depend on it
constexpr uint32_t kDirBitsMin = 4, kDirBitsMax = 12;
__host__ __device__ constexpr uint32_t dir_bytes(uint32_t bbits)
{
    return (((1u << bbits) + 1) * 4 + 15) & ~15u;
}

// One block per row of either set: flag[0] = 1 when a row is not strictly ascending within its
// length (every thread that sees a break stores the same 1: plain vector stores), flag[1] = the
// longest query row.
template <typename T>
__global__ __launch_bounds__(kThreads) void rows_ascending_kernel(
    const T *__restrict__ ref, const uint32_t *__restrict__ ref_len, uint64_t ref_stride,
    uint32_t n_ref, const T *__restrict__ qry, const uint32_t *__restrict__ qry_len,
    uint64_t qry_stride, uint32_t *__restrict__ flag)
{
    const uint32_t b = blockIdx.x;
    const bool is_q = b >= n_ref;
    const uint32_t row = is_q ? b - n_ref : b;
    const uint32_t len = is_q ? qry_len[row] : ref_len[row];
    const T *p = is_q ? qry + (uint64_t)row * qry_stride : ref + (uint64_t)row * ref_stride;
    bool bad = false;
    for (uint32_t i = threadIdx.x + 1; i < len; i += kThreads) bad |= !(p[i - 1] < p[i]);
    if (bad) flag[0] = 1;
    if (is_q && threadIdx.x == 0 && len) atomicMax(flag + 1, len);
}

// The closed form.  Workgroup b: query row b % n_qry against the ref rows
// [kBlockRefs * (b / n_qry), + kBlockRefs): neighbouring workgroups share their ref rows (L2)
// and each stages its own query row.
// QInLds: the query row copied into LDS first, at the residue of its global address modulo
// 16 B, so that 16-B global loads land on 16-B LDS stores whatever the row's start (strides may
// be odd: rows are only element-aligned); the entries before the first and after the last
// aligned 16 B go one by one, and nothing at or past the row's length is read.  A directory
// over the row follows: with the row's largest entry shifted up to bit 63, bucket(v) = the top
// `bbits` bits of v shifted likewise, and dir[b] = the first position whose bucket is >= b
// (dir[2^bbits] = lq).  bucket() is monotone, so an entry v <= Q[lq - 1] can only sit in
// [dir[bucket(v)], dir[bucket(v) + 1]): one 8-byte directory read and, for hash-like rows with
// 2^bbits >= 2 lq, about one entry read per lookup instead of a log2(lq)-step search.  Any
// distribution stays exact: a long bucket is searched by bisection.
// Otherwise (the row exceeds the LDS cap) Q is searched by bisection in global memory.
template <typename T, bool QInLds>
__global__ __launch_bounds__(kThreads) void contain_rows_kernel(
    const T *__restrict__ ref, const uint32_t *__restrict__ ref_len, uint64_t ref_stride,
    uint32_t n_ref, const T *__restrict__ qry, const uint32_t *__restrict__ qry_len,
    uint64_t qry_stride, uint32_t n_qry, uint32_t bbits, uint32_t *__restrict__ common,
    uint32_t *__restrict__ steps)
{
    extern __shared__ uint4 lds_raw[];
    __shared__ uint32_t res[2][kBlockRefs];
    constexpr uint32_t V = 16 / sizeof(T);   // entries per 16 B
    const uint32_t q = blockIdx.x % n_qry, r0 = (blockIdx.x / n_qry) * kBlockRefs;
    const uint32_t lq = qry_len[q];
    const T *Qg = qry + (uint64_t)q * qry_stride;
    const uint32_t pad = (uint32_t)(((uintptr_t)Qg & 15) / sizeof(T));
    const uint32_t nb = 1u << bbits;
    uint32_t *dir = (uint32_t *)lds_raw;                          // nb + 1 entries
    T *Ql = (T *)((char *)lds_raw + dir_bytes(bbits)) + pad;
    uint32_t shift = 0;
    if (QInLds && lq) {
        const uint32_t head = min(lq, (V - pad) % V);
        const uint32_t nvec = (lq - head) / V;
        const uint32_t tail = head + nvec * V;
        if (threadIdx.x < head) Ql[threadIdx.x] = Qg[threadIdx.x];
        const uint4 *src = (const uint4 *)(Qg + head);
        uint4 *dst = (uint4 *)(Ql + head);
        for (uint32_t v = threadIdx.x; v < nvec; v += kThreads) dst[v] = src[v];
        if (threadIdx.x < lq - tail) Ql[tail + threadIdx.x] = Qg[tail + threadIdx.x];
        __syncthreads();
        const uint64_t top = (uint64_t)Ql[lq - 1];
        shift = top ? (uint32_t)__clzll((long long)top) : 63u;
        // dir[b] = the first position holding a value >= t_b, the smallest value of bucket b:
        // t_b = ceil((b << (64 - bbits)) / 2^shift)
        for (uint32_t b = threadIdx.x; b <= nb; b += kThreads) {
            uint32_t lo = 0, hi = lq;
            if (b == nb) lo = lq;
            else {
                const uint64_t x = (uint64_t)b << (64 - bbits);
                const uint64_t tb = (x >> shift) + ((x & ((1ull << shift) - 1)) != 0);
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((uint64_t)Ql[mid] < tb) lo = mid + 1;
                    else hi = mid;
                }
            }
            dir[b] = lo;
        }
        __syncthreads();
    }
    auto Q = [&](uint32_t i) -> T { return QInLds ? Ql[i] : Qg[i]; };
    // the first position in [lo, hi) whose entry is >= v (strict = false: > v), else hi
    auto bound = [&](uint32_t lo, uint32_t hi, T v, bool strict) -> uint32_t {
        while (hi - lo > 4) {
            const uint32_t mid = (lo + hi) >> 1;
            const T x = Q(mid);
            if (strict ? x < v : x <= v) lo = mid + 1;
            else hi = mid;
        }
        while (lo < hi) {
            const T x = Q(lo);
            if (strict ? x >= v : x > v) break;
            lo++;
        }
        return lo;
    };
    auto bucket = [&](T v) -> uint32_t {
        return (uint32_t)(((uint64_t)v << shift) >> (64 - bbits));
    };

    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    for (uint32_t t = wave; t < kBlockRefs; t += kWaves) {
        const uint32_t r = r0 + t;
        if (r >= n_ref) break;
        const uint32_t lr = ref_len[r];
        const T *R = ref + (uint64_t)r * ref_stride;
        const uint32_t m = min(lr, lq);
        uint32_t jf = 0, cnt = 0;
        if (m) {
            // jf = #{q in Q[0..m) : q <= maxR}: a tie with R's maximum counts
            const T maxR = R[lr - 1];
            if (!QInLds) jf = bound(0, m, maxR, false);
            else if (maxR >= Q(lq - 1)) jf = m;
            else {
                const uint32_t b = bucket(maxR);
                jf = min(m, bound(dir[b], dir[b + 1], maxR, false));
            }
        }
        // (the builtin returns int: each half goes back through uint32_t, unextended)
        auto first_lane = [](T v) -> T {
            const uint32_t f_lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v);
            const uint32_t f_hi =
                (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
            return (T)(((uint64_t)f_hi << 32) | f_lo);
        };
        // Only the entries of R in [Q[0], Q[jf - 1]] are looked up: a match of those lies in
        // Q[0..jf).  Once a chunk's first entry is past Q[jf - 1], so is the rest of R.
        if (jf && QInLds) {
            const T qmax = Ql[jf - 1];
            // kUnroll chunks of 64 entries at a time: their global loads, directory reads and
            // entry reads are issued together (one chunk at a time the wave waits out each
            // load's latency in turn: 169 ms against 125 ms on the 10,000 x 10,000 grid of
            // 1,000-hash rows; 8 chunks: 123 ms).  An entry above Q[jf - 1] could only match
            // at or past jf, so it is left out; one below Q[0], or above the whole row (its
            // bucket is then meaningless, yet below 2^bbits), finds no equal entry.  The first
            // two entries of a bucket are read whether or not they exist (the row is followed
            // by two spare entries; what they hold is never used): reading them only in the
            // lanes that need them put a branch between the reads of the unrolled chunks,
            // 160 ms against 121 ms.  Longer buckets, rare for hash-like rows, go on from the
            // third entry.
            constexpr uint32_t kUnroll = 4;
            for (uint32_t base = 0; base < lr; base += kUnroll * kWave) {
                T v[kUnroll];
                uint32_t lo[kUnroll], hi[kUnroll];
                bool act[kUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) {
                    const uint32_t i = base + u * kWave + lane;
                    v[u] = i < lr ? R[i] : (T)0;
                    act[u] = i < lr;
                }
                if (first_lane(v[0]) > qmax) break;
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) {
                    act[u] = act[u] && v[u] <= qmax;
                    const uint32_t b = bucket(v[u]);
                    lo[u] = dir[b];
                    hi[u] = dir[b + 1];
                }
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) {
                    const uint32_t n = hi[u] - lo[u];
                    const T x0 = Ql[lo[u]], x1 = Ql[lo[u] + 1];
                    bool hit = act[u] && ((n > 0 && x0 == v[u]) || (n > 1 && x1 == v[u]));
                    if (act[u] && n > 2 && x1 < v[u]) {
                        const uint32_t p = bound(lo[u] + 2, hi[u], v[u], true);
                        hit = p < hi[u] && Ql[p] == v[u];
                    }
                    cnt += (uint32_t)__popcll(__ballot(hit));
                }
            }
        } else if (jf) {
            const T qmin = Q(0), qmax = Q(jf - 1);
            // each lane's lower bound only moves up from chunk to chunk: R ascends
            uint32_t from = 0;
            for (uint32_t base = 0; base < lr; base += kWave) {
                const uint32_t i = base + lane;
                const T v = i < lr ? R[i] : (T)0;
                if (first_lane(v) > qmax) break;
                bool hit = false;
                if (i < lr && v >= qmin && v <= qmax) {
                    from = bound(from, jf, v, true);
                    hit = from < jf && Q(from) == v;
                }
                cnt += (uint32_t)__popcll(__ballot(hit));
            }
        }
        if (lane == 0) {
            res[0][t] = cnt;
            res[1][t] = jf;
        }
    }
    __syncthreads();
    if (threadIdx.x < kBlockRefs && r0 + threadIdx.x < n_ref) {
        const uint64_t cell = (uint64_t)q * n_ref + r0 + threadIdx.x;
        common[cell] = res[0][threadIdx.x];
        steps[cell] = res[1][threadIdx.x];
    }
}

// The walk as written, one lane per pair, lists read from global memory.
template <typename T>
__global__ __launch_bounds__(kThreads) void contain_literal_kernel(
    const T *__restrict__ ref, const uint32_t *__restrict__ ref_len, uint64_t ref_stride,
    uint32_t n_ref, const T *__restrict__ qry, const uint32_t *__restrict__ qry_len,
    uint64_t qry_stride, uint64_t n_pairs, uint32_t *__restrict__ common,
    uint32_t *__restrict__ steps)
{
    const uint64_t cell = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (cell >= n_pairs) return;
    const uint32_t q = (uint32_t)(cell / n_ref), r = (uint32_t)(cell % n_ref);
    const uint32_t lr = ref_len[r], lq = qry_len[q];
    const T *R = ref + (uint64_t)r * ref_stride, *Q = qry + (uint64_t)q * qry_stride;
    const uint32_t denom = min(lr, lq);
    uint32_t i = 0, j = 0, c = 0;
    while (j < denom && i < lr) {
        const T a = R[i], b = Q[j];
        if (a < b) i++;
        else if (b < a) j++;
        else { i++; j++; c++; }
    }
    common[cell] = c;
    steps[cell] = j;
}

// dynamic LDS a contain_rows_kernel<T, true> launch may ask for on the current device: the
// limit is a per-device attribute of each instance, raised once per device ordinal
uint32_t lds_granted()
{
    constexpr int kMaxDev = 64;
    static std::atomic<uint32_t> got[kMaxDev];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return kDefLds;
    const bool slot = dev >= 0 && dev < kMaxDev;
    if (slot) {
        const uint32_t g = got[dev].load(std::memory_order_acquire);
        if (g) return g;
    }
    uint32_t bytes = kMaxLds;
    for (const void *fn : {(const void *)contain_rows_kernel<uint64_t, true>,
                           (const void *)contain_rows_kernel<uint32_t, true>})
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds) !=
            hipSuccess) {
            (void)hipGetLastError();
            bytes = kDefLds;
        }
    if (slot) got[dev].store(bytes, std::memory_order_release);
    return bytes;
}

}  // namespace

uint32_t contain_lds_cap(uint32_t hash_bytes)
{
    return (lds_granted() - kLdsPad - dir_bytes(kDirBitsMax)) / hash_bytes;
}

hipError_t launch_rows_ascending(const RowSet &R, const RowSet &Q, uint32_t hash_bytes,
                                 uint32_t *flag, hipStream_t st)
{
    const uint64_t rows = (uint64_t)R.n + Q.n;
    if (!rows) return hipSuccess;
    if (rows > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return with_hash(hash_bytes, [&](auto h) {
        using T = decltype(h);
        hipLaunchKernelGGL(rows_ascending_kernel<T>, dim3((uint32_t)rows), dim3(kThreads), 0, st,
                           (const T *)R.rows, R.len, R.stride, R.n, (const T *)Q.rows, Q.len,
                           Q.stride, flag);
        return hipGetLastError();
    });
}

hipError_t launch_contain_rows(const RowSet &R, const RowSet &Q, uint32_t hash_bytes,
                               uint32_t max_qry_len, uint32_t *d_common, uint32_t *d_steps,
                               bool *lds, hipStream_t st)
{
    if (lds) *lds = false;
    if (!R.n || !Q.n) return hipSuccess;
    // the grid flattened into gridDim.x: n_qry may exceed the 65,535 of gridDim.y
    const uint64_t blocks = (uint64_t)Q.n * ((R.n + kBlockRefs - 1) / kBlockRefs);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return with_hash(hash_bytes, [&](auto h) {
        using T = decltype(h);
        const T *ref = (const T *)R.rows, *qry = (const T *)Q.rows;
        const bool in_lds = max_qry_len <= contain_lds_cap(sizeof(T));
        if (lds) *lds = in_lds;
        if (in_lds) {
            uint32_t bbits = kDirBitsMin;
            while (bbits < kDirBitsMax && (1u << bbits) < 2 * (uint64_t)max_qry_len) bbits++;
            const size_t bytes = dir_bytes(bbits) +
                                 (((size_t)max_qry_len * sizeof(T) + kLdsPad + 15) & ~(size_t)15);
            hipLaunchKernelGGL((contain_rows_kernel<T, true>), dim3((uint32_t)blocks),
                               dim3(kThreads), bytes, st, ref, R.len, R.stride, R.n, qry, Q.len,
                               Q.stride, Q.n, bbits, d_common, d_steps);
        } else {
            hipLaunchKernelGGL((contain_rows_kernel<T, false>), dim3((uint32_t)blocks),
                               dim3(kThreads), 0, st, ref, R.len, R.stride, R.n, qry, Q.len,
                               Q.stride, Q.n, kDirBitsMin, d_common, d_steps);
        }
        return hipGetLastError();
    });
}

hipError_t launch_contain_literal(const RowSet &R, const RowSet &Q, uint32_t hash_bytes,
                                  uint32_t *d_common, uint32_t *d_steps, hipStream_t st)
{
    const uint64_t n = (uint64_t)R.n * Q.n;
    if (!n) return hipSuccess;
    const uint64_t blocks = (n + kThreads - 1) / kThreads;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return with_hash(hash_bytes, [&](auto h) {
        using T = decltype(h);
        hipLaunchKernelGGL(contain_literal_kernel<T>, dim3((uint32_t)blocks), dim3(kThreads), 0, st,
                           (const T *)R.rows, R.len, R.stride, R.n, (const T *)Q.rows, Q.len,
                           Q.stride, n, d_common, d_steps);
        return hipGetLastError();
    });
}

}  // namespace fpm
