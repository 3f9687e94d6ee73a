// kfinger.hip — CFL k-fingers of sequence records: lyn2vec `--type basic --type_factorization CFL`
// (fingerprint_utils.py:95-110, 443-476: the cyclic windows and their lines; factorizations.py:
// 102-126: Duval) and the line hash of Sketch::initFromFingerprints (getHashFingerPrint,
// hash.cpp:45-73), from the sequence bytes, with no k-finger text in between.
//
// One lane per line.  A workgroup takes one KfDesc: either a run of up to kKfRun consecutive
// window starts of one record (n >= w: its run + w - 1 bytes, wrapping past the record's end,
// are staged upper-cased in LDS once, and every lane's window is a contiguous slice of them), or
// a pack of up to kKfRun records shorter than the window (one line each, staged back to back).
// Pass one (kf_hash_kernel) runs Duval over the lane's window in LDS and streams the factor
// lengths into Murmur as they come, two values a block; it keeps the value count and the bytes
// the line's text takes after its ID.  Pass two (kf_emit_kernel), after an exclusive scan of the
// per-line sizes, runs Duval again and writes the u16 lengths or the text line at the line's
// offset.  Nothing is stored per factor between the passes.
//
// ICFL and CFL_ICFL-T (lyn2vec `--type_factorization ICFL` / `CFL_ICFL-T`; factorizations.py:
// 143-169 ICFL_recursive, 172-189 find_pre, 212-232 find_bre, 235-248 border, 265-301 CFL_icfl)
// run in the same two passes through the same emit callbacks.  The inverse Lyndon factorization
// is not streaming: each lane keeps, per window position, one entry (the border array of the
// step under way; behind it the `last` of every finished step, at the step's start) and one bit
// (where a step's piece ends; the right-to-left merge clears the bits of glued pieces, and what
// is left are the factor boundaries, read left to right).  Windows up to kKfLdsWindow keep that
// in LDS, u8 entries, lane-interleaved; wider ones in a device buffer of u16 entries, one region
// per resident workgroup, which then walks the descriptors in a grid-stride loop.
//
// The combined forms (lyn2vec `--type_factorization CFL_COMB` / `ICFL_COMB` / `CFL_ICFL_COMB-T`;
// factorizations_comb.py:178-246, d_duval_) cut a window of n bytes where its own factorization
// does and where the factorization of its reverse complement does, mirrored: at n - c for a cut c
// of the other strand.  The reverse complement is not staged: the routines take a byte view, and
// the reverse view reads the lane's slice backwards (descending LDS addresses, the same
// ds_read_u8) through the complement.  A lane factorizes the reverse side first, then the forward
// one, marks the cuts of both in one more bit array (a cut both share is one bit), and reads it
// left to right into the same emit callbacks.  The reverse side of CFL_ICFL_COMB-T runs at
// threshold 30 whatever T is, as lyn2vec's does (d_duval_ calls it without k, :221, :164).
//
// Long reads (lyn2vec `--type generalized --split N`; factors_string, fingerprint_utils.py:114-130,
// compute_long_fingerprint_by_list, :480-518) cut a record into consecutive pieces of N bytes and
// factorize each on its own.  The pieces take the place of the records in rec_pos / rec_len and
// ride in pack descriptors, so every kernel above runs over them as it stands; piece_rec maps a
// piece to its record for the one text line per record, "<id>  <lengths> | <lengths> | \n"
// (kf_ext_size_kernel, kf_emit_ext_kernel).  The same two kernels write the factor text of
// lyn2vec's `--fact create` (:471-474, :509-511) for either kind of job: a factor's upper-cased
// bytes, copied from the stage, where the fingerprint has its length.
#include "fpm_device.hpp"
#include "fpm_kernels.hpp"

#include <algorithm>
#include <type_traits>

namespace fpm {

namespace {

// LDS bytes a workgroup stages: a full run at the widest window, rounded up to dwords
constexpr uint32_t kKfLds = (kKfStage + 3) / 4 * 4;

__device__ __forceinline__ uint8_t kf_upper(uint8_t c)
{
    // ASCII a-z only; every other byte (those >= 0x80 too) stays as it is
    return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
}

// the complement of an upper-cased byte (factorizations_comb.py:8-10): A <-> T, C <-> G; N and
// every byte lyn2vec has no complement for stay as they are
__device__ __forceinline__ uint8_t kf_comp(uint8_t c)
{
    const uint32_t at = (c == 'A') | (c == 'T'), cg = (c == 'C') | (c == 'G');
    return (uint8_t)(c ^ (at ? ('A' ^ 'T') : 0) ^ (cg ? ('C' ^ 'G') : 0));
}

// The byte view of the reverse complement of a slice: byte i is the complement of the i-th byte
// from the slice's end (p: its last byte).  The forward view of a slice is the pointer itself.
struct KfRc {
    const uint8_t *p;
    __device__ __forceinline__ uint8_t operator[](uint32_t i) const { return kf_comp(*(p - i)); }
    __device__ __forceinline__ KfRc operator+(uint32_t k) const { return KfRc{p - k}; }
};

// Duval (factorizations.py:102-126), bytes compared unsigned; emit(len) per Lyndon factor.
// S: the byte view, const uint8_t * or KfRc.
template <typename S, typename Emit>
__device__ __forceinline__ void kf_duval(S s, uint32_t n, Emit emit)
{
    uint32_t k = 0;
    while (k < n) {
        uint32_t i = k, j = k + 1;
        while (j < n) {
            const uint8_t a = s[i], b = s[j];
            if (a > b) break;
            i = a < b ? k : i + 1;
            j++;
        }
        const uint32_t len = j - i;
        while (k <= i) {
            emit(len);
            k += len;
        }
    }
}

__device__ __forceinline__ uint32_t kf_digits(uint32_t v)   // v <= kKfMaxWindow < 10000
{
    return 1 + (v >= 10) + (v >= 100) + (v >= 1000);
}

// where a lane's ICFL working memory is: entry e and bit word i of lane t lie kKfRun entries
// apart, at a[e * kKfRun] and bits[i * kKfRun] (both pointers already at the lane)
template <typename E>
struct KfWork {
    E *a;
    uint32_t *bits;
    __device__ __forceinline__ uint32_t get(uint32_t e) const { return a[(size_t)e * kKfRun]; }
    __device__ __forceinline__ void set(uint32_t e, uint32_t v) const
    {
        a[(size_t)e * kKfRun] = (E)v;
    }
    __device__ __forceinline__ uint32_t &word(uint32_t i) const
    {
        return bits[(size_t)i * kKfRun];
    }
};

// The inverse Lyndon factorization of s[0 .. n) (ICFL_recursive, factorizations.py:143-169, as a
// loop), bytes compared unsigned, the end of the word known from n; emit(len) per factor, left
// to right.  wk: n entries (values < n) and (n + 31) / 32 bit words.
// Forward: from step start st, scan while the bytes descend (find_pre); where the scan stops at
// j before the end, build the border array of s[st .. st + j) at entries st .. st + j - 1,
// walk its chain from the longest border down to 0 and keep as `last` the shortest border whose
// next byte is below s[st + j], the longest border when none is (find_bre); the step's piece
// is s[st .. st + j - last).  Every
// step takes at least one byte, so the entries of finished steps (one each, at the step's
// start) lie below st, and st + j < n.
// Backward: the piece of a step starts a new factor when the factor behind it is longer than
// the step's `last`, else it is glued onto that factor.
template <typename S, typename E, typename Emit>
__device__ __forceinline__ void kf_icfl(S s, uint32_t n, const KfWork<E> &wk, Emit emit)
{
    if (!n) return;
    const uint32_t nw = (n + 31) / 32;
    for (uint32_t i = 0; i < nw; i++) wk.word(i) = 0;
    uint32_t st = 0;
    for (;;) {
        const S w = s + st;
        const uint32_t m = n - st;
        uint32_t i = 0, j = 1;
        while (j < m) {
            const uint8_t a = w[i], b = w[j];
            if (b > a) break;
            i = b < a ? 0 : i + 1;
            j++;
        }
        if (j >= m) break;                       // the rest is the last factor
        wk.set(st, 0);
        uint32_t k = 0;
        for (uint32_t e = 1; e < j; e++) {
            const uint8_t c = w[e];
            while (k > 0 && w[k] != c) k = wk.get(st + k - 1);
            if (w[k] == c) k++;
            wk.set(st + e, k);
        }
        uint32_t b = wk.get(st + j - 1), last = b;
        const uint8_t c = w[j];
        for (;;) {
            if (w[b] < c) last = b;
            if (!b) break;
            b = wk.get(st + b - 1);
        }
        wk.set(st, last);
        st += j - last;                          // 1 <= j - last, st < n
        wk.word(st >> 5) |= 1u << (st & 31);
    }
    uint32_t cur = n - st, hi = st;
    while (hi) {
        // the start of the step whose piece ends at hi: the highest bit below hi, or 0
        const uint32_t q = hi - 1;
        uint32_t wd = q >> 5;
        uint32_t v = wk.word(wd) & (0xFFFFFFFFu >> (31 - (q & 31)));
        while (!v && wd) v = wk.word(--wd);
        const uint32_t lo = v ? wd * 32 + 31 - (uint32_t)__clz((int)v) : 0;
        if (cur > wk.get(lo)) {
            cur = hi - lo;
        } else {
            cur += hi - lo;
            wk.word(hi >> 5) &= ~(1u << (hi & 31));
        }
        hi = lo;
    }
    uint32_t prev = 0;
    for (uint32_t wd = 0; wd < nw; wd++) {
        uint32_t v = wk.word(wd);
        while (v) {
            const uint32_t p = wd * 32 + (uint32_t)__ffs((int)v) - 1;
            v &= v - 1;
            emit(p - prev);
            prev = p;
        }
    }
    emit(n - prev);
}

// how a kernel instance factorizes: Duval alone (the instances CFL has always had; combined, with
// its cut bits in LDS), or ICFL / CFL_ICFL with the working memory in LDS, or in the device
// buffer; kKfModeCflWide is the combined Duval with its cut bits in the device buffer
enum : int { kKfModeCfl = 0, kKfModeLds = 1, kKfModeWide = 2, kKfModeCflWide = 3 };

constexpr bool kf_mode_icfl(int mode) { return mode == kKfModeLds || mode == kKfModeWide; }
constexpr bool kf_mode_wide(int mode) { return mode == kKfModeWide || mode == kKfModeCflWide; }

template <int MODE>
using KfWorkOf = KfWork<typename std::conditional<MODE == kKfModeWide, uint16_t, uint8_t>::type>;

// the workgroup's region of the device buffer (wide modes; else nullptr)
template <int MODE, bool COMB>
__device__ __forceinline__ uint8_t *kf_region(uint32_t w, uint8_t *work, uint32_t group)
{
    if constexpr (kf_mode_wide(MODE))
        return work + (size_t)group * kf_region_bytes(kf_mode_icfl(MODE), COMB, w);
    return nullptr;
}

// the lane's working memory.  LDS (dynamic, kf_lds_work_bytes(w)): the bit words of all lanes,
// then the u8 entries.  Wide: the same with u16 entries, at the head of the workgroup's region.
template <int MODE>
__device__ __forceinline__ KfWorkOf<MODE> kf_work(uint32_t w, uint8_t *region)
{
    KfWorkOf<MODE> wk{nullptr, nullptr};
    const uint32_t nw = (w + 31) / 32;
    if constexpr (MODE == kKfModeLds) {
        extern __shared__ uint32_t s_work[];
        wk.bits = s_work + threadIdx.x;
        wk.a = reinterpret_cast<uint8_t *>(s_work + (size_t)nw * kKfRun) + threadIdx.x;
    } else if constexpr (MODE == kKfModeWide) {
        wk.bits = reinterpret_cast<uint32_t *>(region) + threadIdx.x;
        wk.a = reinterpret_cast<uint16_t *>(region + (size_t)nw * kKfRun * 4) + threadIdx.x;
    }
    return wk;
}

// the lane's cut bits of a combined factorization: (w + 31) / 32 words, kKfRun words apart like
// the ICFL bits, behind the ICFL working memory where the mode has one
template <int MODE, bool COMB>
__device__ __forceinline__ uint32_t *kf_cut_bits(uint32_t w, uint8_t *region)
{
    if constexpr (!COMB) {
        return nullptr;
    } else if constexpr (kf_mode_wide(MODE)) {
        return reinterpret_cast<uint32_t *>(region + kf_region_bytes(kf_mode_icfl(MODE), false, w)) +
               threadIdx.x;
    } else {
        extern __shared__ uint32_t s_work[];
        return s_work + kf_lds_bytes(kf_mode_icfl(MODE), false, w) / 4 + threadIdx.x;
    }
}

// the factor lengths of s[0 .. n): thr 0, ICFL; else CFL_ICFL-thr, a Lyndon factor longer than
// thr replaced by its own ICFL factors (CFL_icfl, factorizations.py:265-301)
template <int MODE, typename S, typename Emit>
__device__ __forceinline__ void kf_factorize(S s, uint32_t n, uint32_t thr,
                                             const KfWorkOf<MODE> &wk, Emit emit)
{
    if constexpr (!kf_mode_icfl(MODE)) {
        kf_duval(s, n, emit);
    } else if (!thr) {
        kf_icfl(s, n, wk, emit);
    } else {
        uint32_t at = 0;
        kf_duval(s, n, [&](uint32_t len) {
            if (len <= thr) emit(len);
            else kf_icfl(s + at, len, wk, emit);
            at += len;
        });
    }
}

// The lengths of a line, s[0 .. n): kf_factorize, or with COMB the gaps between the cuts of
// d_duval_ (factorizations_comb.py:213-246): every cut c < n of the reverse complement's
// factorization marked at n - c in `cuts`, every cut of the window's own marked where it is, and
// the marks read left to right.  The lane clears its (n + 31) / 32 words first, every line.  The
// reverse side's threshold is kKfCombRevThreshold where the forward one has any.
template <int MODE, bool COMB, typename Emit>
__device__ __forceinline__ void kf_line(const uint8_t *s, uint32_t n, uint32_t thr,
                                        const KfWorkOf<MODE> &wk, uint32_t *cuts, Emit emit)
{
    if constexpr (!COMB) {
        kf_factorize<MODE>(s, n, thr, wk, emit);
    } else {
        if (!n) return;
        const uint32_t nw = (n + 31) / 32;
        for (uint32_t i = 0; i < nw; i++) cuts[(size_t)i * kKfRun] = 0;
        uint32_t at = 0;
        kf_factorize<MODE>(KfRc{s + n - 1}, n, thr ? kKfCombRevThreshold : 0, wk,
                           [&](uint32_t len) {
                               at += len;
                               if (at < n) {
                                   const uint32_t p = n - at;
                                   cuts[(size_t)(p >> 5) * kKfRun] |= 1u << (p & 31);
                               }
                           });
        at = 0;
        kf_factorize<MODE>(s, n, thr, wk, [&](uint32_t len) {
            at += len;
            if (at < n) cuts[(size_t)(at >> 5) * kKfRun] |= 1u << (at & 31);
        });
        uint32_t prev = 0;
        for (uint32_t wd = 0; wd < nw; wd++) {
            uint32_t v = cuts[(size_t)wd * kKfRun];
            while (v) {
                const uint32_t p = wd * 32 + (uint32_t)__ffs((int)v) - 1;
                v &= v - 1;
                emit(p - prev);
                prev = p;
            }
        }
        emit(n - prev);
    }
}

// Stage the descriptor's bytes in s_seq.  On return the lane's window is s_seq[base .. base + n)
// and `rec` its record; false: the lane has no line.
__device__ __forceinline__ bool kf_stage(const uint8_t *__restrict__ seq,
                                         const uint64_t *__restrict__ rec_pos,
                                         const uint32_t *__restrict__ rec_len, const KfDesc &d,
                                         uint32_t w, uint8_t *s_seq, uint32_t *s_off,
                                         uint32_t &base, uint32_t &n, uint32_t &rec)
{
    const uint32_t tid = threadIdx.x;
    const bool active = tid < d.count;
    if (d.kind == 0) {
        // a run of window starts [start, start + count) of one record of length len >= w:
        // byte t of the stage is record byte (start + t) mod len, and start + t < 2 len
        rec = d.rec;
        const uint32_t len = rec_len[rec];
        const uint8_t *p = seq + rec_pos[rec];
        const uint32_t need = d.count + w - 1;
        for (uint32_t t = tid; t < need; t += kKfRun) {
            uint64_t at = (uint64_t)d.start + t;
            if (at >= len) at -= len;
            s_seq[t] = kf_upper(p[at]);
        }
        base = tid;
        n = w;
    } else {
        // records rec .. rec + count - 1, each shorter than the window and together at most
        // kKfStage bytes: lane t stages record rec + t behind the ones before it
        rec = d.rec + (active ? tid : 0);
        const uint32_t len = active ? rec_len[rec] : 0;
        s_off[tid] = len;
        __syncthreads();
        for (uint32_t step = 1; step < kKfRun; step <<= 1) {
            const uint32_t v = tid >= step ? s_off[tid - step] : 0;
            __syncthreads();
            s_off[tid] += v;
            __syncthreads();
        }
        base = s_off[tid] - len;
        n = len;
        if (active) {
            const uint8_t *p = seq + rec_pos[rec];
            for (uint32_t t = 0; t < len; t++) s_seq[base + t] = kf_upper(p[t]);
        }
    }
    __syncthreads();
    return active;
}

// sum of v over the workgroup, valid in thread 0 (s_red: kKfRun / 64 words)
__device__ __forceinline__ unsigned long long kf_block_sum(unsigned long long v,
                                                           unsigned long long *s_red)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    if (threadIdx.x == 0)
        for (uint32_t i = 0; i < kKfRun / 64; i++) t += s_red[i];
    return t;
}

}  // namespace

// Pass one.  hash: u32 or u64 per line; n_vals: factors per line; body: the text bytes of the
// line after its ID (" <len>" per factor and the '\n'); *val_total += the factors of all lines.
template <int MODE, bool COMB>
__device__ __forceinline__ void kf_hash_desc(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc &d, uint32_t w, uint32_t seed,
    uint32_t use64, void *__restrict__ hash, uint32_t *__restrict__ n_vals,
    uint32_t *__restrict__ body, unsigned long long *__restrict__ val_total, uint32_t thr,
    const KfWorkOf<MODE> &wk, uint32_t *cuts, uint8_t *s_seq, uint32_t *s_off,
    unsigned long long *s_red)
{
    uint32_t base, n, rec;
    const bool active = kf_stage(seq, rec_pos, rec_len, d, w, s_seq, s_off, base, n, rec);
    uint32_t cnt = 0;
    if (active) {
        uint32_t bytes = 1;
        uint64_t h1 = seed, h2 = seed, pend = 0;
        // Murmur over the lengths as little-endian u64 (hash.cpp:45-73): a 16-byte block per two
        // values, an odd last value as the 8-byte tail, 8 * count folded in at the end
        kf_line<MODE, COMB>(s_seq + base, n, thr, wk, cuts, [&](uint32_t len) {
            bytes += 1 + kf_digits(len);
            if (cnt & 1) mur_block(h1, h2, pend, len);
            else pend = len;
            cnt++;
        });
        if (cnt & 1) {
            uint64_t k1 = mul_opaque(pend, kC1);
            k1 = rotl64(k1, 31);
            k1 *= kC2;
            h1 ^= k1;
        }
        const uint64_t h = mur_final(h1, h2, (uint64_t)cnt * 8);
        const uint64_t line = d.line_base + threadIdx.x;
        if (use64) reinterpret_cast<uint64_t *>(hash)[line] = h;
        else reinterpret_cast<uint32_t *>(hash)[line] = (uint32_t)h;
        n_vals[line] = cnt;
        body[line] = bytes;
    }
    const unsigned long long t = kf_block_sum(cnt, s_red);
    if (threadIdx.x == 0 && t) atomicAdd(val_total, t);
}

// One descriptor per workgroup; the wide modes: workgroup g owns region g of `work` and takes the
// descriptors g, g + gridDim.x, ...
template <int MODE, bool COMB>
__global__ __launch_bounds__(kKfRun) void kf_hash_kernel(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc *__restrict__ descs, uint32_t n_desc,
    uint32_t w, uint32_t seed, uint32_t use64, void *__restrict__ hash,
    uint32_t *__restrict__ n_vals, uint32_t *__restrict__ body,
    unsigned long long *__restrict__ val_total, uint32_t thr, uint8_t *__restrict__ work)
{
    __shared__ uint8_t s_seq[kKfLds];
    __shared__ uint32_t s_off[kKfRun];
    __shared__ unsigned long long s_red[kKfRun / 64];
    uint8_t *region = kf_region<MODE, COMB>(w, work, blockIdx.x);
    const KfWorkOf<MODE> wk = kf_work<MODE>(w, region);
    uint32_t *cuts = kf_cut_bits<MODE, COMB>(w, region);
    if constexpr (kf_mode_wide(MODE)) {
        // (kf_block_sum's barrier stands between one descriptor's reads of the stage and the
        // next one's writes)
        for (uint32_t b = blockIdx.x; b < n_desc; b += gridDim.x)
            kf_hash_desc<MODE, COMB>(seq, rec_pos, rec_len, descs[b], w, seed, use64, hash, n_vals,
                                     body, val_total, thr, wk, cuts, s_seq, s_off, s_red);
    } else {
        kf_hash_desc<MODE, COMB>(seq, rec_pos, rec_len, descs[blockIdx.x], w, seed, use64, hash,
                                 n_vals, body, val_total, thr, wk, cuts, s_seq, s_off, s_red);
    }
}

// size[line] = the line's text bytes: its record's ID (id_len, per record) + body[line];
// *text_total += their sum
__global__ __launch_bounds__(kKfRun) void kf_text_size_kernel(
    const KfDesc *__restrict__ descs, const uint32_t *__restrict__ body,
    const uint32_t *__restrict__ id_len, uint32_t *__restrict__ size,
    unsigned long long *__restrict__ text_total)
{
    __shared__ unsigned long long s_red[kKfRun / 64];
    const KfDesc d = descs[blockIdx.x];
    uint32_t sz = 0;
    if (threadIdx.x < d.count) {
        const uint64_t line = d.line_base + threadIdx.x;
        const uint32_t rec = d.kind == 0 ? d.rec : d.rec + threadIdx.x;
        sz = body[line] + id_len[rec];
        size[line] = sz;
    }
    const unsigned long long t = kf_block_sum(sz, s_red);
    if (threadIdx.x == 0 && t) atomicAdd(text_total, t);
}

// Pass two.  TEXT: the line "<id> <len> <len> ...\n" at out + off[line], the ID copied from
// ids[id_off[rec] .. + id_len[rec]); else the lengths as u16 at vals + off[line].
template <bool TEXT, int MODE, bool COMB>
__device__ __forceinline__ void kf_emit_desc(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc &d, uint32_t w,
    const uint32_t *__restrict__ off, const uint8_t *__restrict__ ids,
    const uint64_t *__restrict__ id_off, const uint32_t *__restrict__ id_len,
    uint8_t *__restrict__ out, uint16_t *__restrict__ vals, uint32_t thr,
    const KfWorkOf<MODE> &wk, uint32_t *cuts, uint8_t *s_seq, uint32_t *s_off)
{
    uint32_t base, n, rec;
    if (!kf_stage(seq, rec_pos, rec_len, d, w, s_seq, s_off, base, n, rec)) return;
    const uint64_t line = d.line_base + threadIdx.x;
    if (TEXT) {
        uint8_t *o = out + off[line];
        const uint8_t *id = ids + id_off[rec];
        const uint32_t il = id_len[rec];
        for (uint32_t t = 0; t < il; t++) o[t] = id[t];
        o += il;
        kf_line<MODE, COMB>(s_seq + base, n, thr, wk, cuts, [&](uint32_t len) {
            const uint32_t nd = kf_digits(len);
            *o = ' ';
            uint32_t v = len;
            for (uint32_t t = nd; t > 0; t--) {
                o[t] = (uint8_t)('0' + v % 10);
                v /= 10;
            }
            o += 1 + nd;
        });
        *o = '\n';
    } else {
        uint16_t *o = vals + off[line];
        kf_line<MODE, COMB>(s_seq + base, n, thr, wk, cuts,
                            [&](uint32_t len) { *o++ = (uint16_t)len; });
    }
}

template <bool TEXT, int MODE, bool COMB>
__global__ __launch_bounds__(kKfRun) void kf_emit_kernel(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc *__restrict__ descs, uint32_t n_desc,
    uint32_t w, const uint32_t *__restrict__ off, const uint8_t *__restrict__ ids,
    const uint64_t *__restrict__ id_off, const uint32_t *__restrict__ id_len,
    uint8_t *__restrict__ out, uint16_t *__restrict__ vals, uint32_t thr,
    uint8_t *__restrict__ work)
{
    __shared__ uint8_t s_seq[kKfLds];
    __shared__ uint32_t s_off[kKfRun];
    uint8_t *region = kf_region<MODE, COMB>(w, work, blockIdx.x);
    const KfWorkOf<MODE> wk = kf_work<MODE>(w, region);
    uint32_t *cuts = kf_cut_bits<MODE, COMB>(w, region);
    if constexpr (kf_mode_wide(MODE)) {
        for (uint32_t b = blockIdx.x; b < n_desc; b += gridDim.x) {
            kf_emit_desc<TEXT, MODE, COMB>(seq, rec_pos, rec_len, descs[b], w, off, ids, id_off,
                                           id_len, out, vals, thr, wk, cuts, s_seq, s_off);
            __syncthreads();   // every lane is done with the stage before the next one fills it
        }
    } else {
        kf_emit_desc<TEXT, MODE, COMB>(seq, rec_pos, rec_len, descs[blockIdx.x], w, off, ids,
                                       id_off, id_len, out, vals, thr, wk, cuts, s_seq, s_off);
    }
}

// The record a unit (a line's record, or a split job's piece) belongs to, and whether the unit
// opens and closes that record's text line.  piece_rec null: a window job, whose every line is
// a text line of its own; else piece_rec[p] is the record of piece p of n_piece, ascending.
struct KfUnit {
    uint32_t rec;
    bool first, last;
};

__device__ __forceinline__ KfUnit kf_unit(const uint32_t *__restrict__ piece_rec,
                                          uint32_t n_piece, uint32_t unit)
{
    if (!piece_rec) return KfUnit{unit, true, true};
    const uint32_t rec = piece_rec[unit];
    return KfUnit{rec, unit == 0 || piece_rec[unit - 1] != rec,
                  unit + 1 == n_piece || piece_rec[unit + 1] != rec};
}

// The sizes of the layouts kf_emit_ext_kernel writes, from what pass one kept (body: 1 + per
// factor 1 + its digits; n_vals: the factors).  A line's tokens joined by single spaces take
// body - 2 bytes as lengths and n + factors - 1 as factor bytes (fact).  A window job's line
// (piece_rec null) is "<id> <tokens>\n"; a split job's unit is "<tokens> | ", behind
// "<id>  " where it opens its record's line and before "\n" where it closes it.
// *text_total += the sum.
__global__ __launch_bounds__(kKfRun) void kf_ext_size_kernel(
    const KfDesc *__restrict__ descs, const uint32_t *__restrict__ rec_len,
    const uint32_t *__restrict__ piece_rec, uint32_t n_piece, uint32_t w, uint32_t fact,
    const uint32_t *__restrict__ n_vals, const uint32_t *__restrict__ body,
    const uint32_t *__restrict__ id_len, uint32_t *__restrict__ size,
    unsigned long long *__restrict__ text_total)
{
    __shared__ unsigned long long s_red[kKfRun / 64];
    const KfDesc d = descs[blockIdx.x];
    uint32_t sz = 0;
    if (threadIdx.x < d.count) {
        const uint64_t line = d.line_base + threadIdx.x;
        const uint32_t unit = d.kind == 0 ? d.rec : d.rec + threadIdx.x;
        const uint32_t n = d.kind == 0 ? w : rec_len[unit];
        const KfUnit u = kf_unit(piece_rec, n_piece, unit);
        sz = fact ? n + n_vals[line] - 1 : body[line] - 2;
        if (piece_rec) sz += 3 + (u.first ? id_len[u.rec] + 2 : 0) + (u.last ? 1 : 0);
        else sz += id_len[u.rec] + 2;
        size[line] = sz;
    }
    const unsigned long long t = kf_block_sum(sz, s_red);
    if (threadIdx.x == 0 && t) atomicAdd(text_total, t);
}

// Pass two of the layouts above, at out + off[line]: the lane factorizes its line again and
// writes per factor its length in digits or, with FACT, its upper-cased bytes from the stage.
template <bool FACT, int MODE, bool COMB>
__device__ __forceinline__ void kf_emit_ext_desc(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc &d, uint32_t w,
    const uint32_t *__restrict__ off, const uint8_t *__restrict__ ids,
    const uint64_t *__restrict__ id_off, const uint32_t *__restrict__ id_len,
    const uint32_t *__restrict__ piece_rec, uint32_t n_piece, uint8_t *__restrict__ out,
    uint32_t thr, const KfWorkOf<MODE> &wk, uint32_t *cuts, uint8_t *s_seq, uint32_t *s_off)
{
    uint32_t base, n, unit;
    if (!kf_stage(seq, rec_pos, rec_len, d, w, s_seq, s_off, base, n, unit)) return;
    const uint64_t line = d.line_base + threadIdx.x;
    const bool split = piece_rec != nullptr;
    const KfUnit u = kf_unit(piece_rec, n_piece, unit);
    uint8_t *o = out + off[line];
    if (u.first) {
        const uint8_t *id = ids + id_off[u.rec];
        const uint32_t il = id_len[u.rec];
        for (uint32_t t = 0; t < il; t++) o[t] = id[t];
        o += il;
        if (split) {
            o[0] = o[1] = ' ';
            o += 2;
        }
    }
    bool lead = !split;                      // a space goes before this token
    const uint8_t *s = s_seq + base;
    kf_line<MODE, COMB>(s_seq + base, n, thr, wk, cuts, [&](uint32_t len) {
        if (lead) *o++ = ' ';
        lead = true;
        if (FACT) {
            for (uint32_t t = 0; t < len; t++) o[t] = s[t];
            s += len;
            o += len;
        } else {
            const uint32_t nd = kf_digits(len);
            uint32_t v = len;
            for (uint32_t t = nd; t > 0; t--) {
                o[t - 1] = (uint8_t)('0' + v % 10);
                v /= 10;
            }
            o += nd;
        }
    });
    if (split) {
        o[0] = ' ';
        o[1] = '|';
        o[2] = ' ';
        o += 3;
    }
    if (u.last) *o = '\n';
}

template <bool FACT, int MODE, bool COMB>
__global__ __launch_bounds__(kKfRun) void kf_emit_ext_kernel(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc *__restrict__ descs, uint32_t n_desc,
    uint32_t w, const uint32_t *__restrict__ off, const uint8_t *__restrict__ ids,
    const uint64_t *__restrict__ id_off, const uint32_t *__restrict__ id_len,
    const uint32_t *__restrict__ piece_rec, uint32_t n_piece, uint8_t *__restrict__ out,
    uint32_t thr, uint8_t *__restrict__ work)
{
    __shared__ uint8_t s_seq[kKfLds];
    __shared__ uint32_t s_off[kKfRun];
    uint8_t *region = kf_region<MODE, COMB>(w, work, blockIdx.x);
    const KfWorkOf<MODE> wk = kf_work<MODE>(w, region);
    uint32_t *cuts = kf_cut_bits<MODE, COMB>(w, region);
    if constexpr (kf_mode_wide(MODE)) {
        for (uint32_t b = blockIdx.x; b < n_desc; b += gridDim.x) {
            kf_emit_ext_desc<FACT, MODE, COMB>(seq, rec_pos, rec_len, descs[b], w, off, ids,
                                               id_off, id_len, piece_rec, n_piece, out, thr, wk,
                                               cuts, s_seq, s_off);
            __syncthreads();   // every lane is done with the stage before the next one fills it
        }
    } else {
        kf_emit_ext_desc<FACT, MODE, COMB>(seq, rec_pos, rec_len, descs[blockIdx.x], w, off, ids,
                                           id_off, id_len, piece_rec, n_piece, out, thr, wk, cuts,
                                           s_seq, s_off);
    }
}

namespace {

// What a launch with factorization f over window w takes: the instance, its grid, its dynamic
// LDS and the threshold the kernel sees (0: ICFL).  false: f is not a factorization, or a wide
// window has descriptors and no working memory (a job without lines needs none and launches
// nothing).
struct KfShape {
    int mode = kKfModeCfl;
    bool comb = false;
    uint32_t grid = 0, lds = 0, thr = 0;
};

bool kf_shape(const KfFact &f, uint32_t w, uint32_t n_desc, KfShape &sh)
{
    sh.grid = n_desc;
    if (f.comb > 1) return false;
    sh.comb = f.comb != 0;
    if (f.kind == kKfCflIcfl) {
        if (f.threshold < 1 || f.threshold > kKfMaxWindow) return false;
        sh.thr = f.threshold;
    } else if (f.kind != kKfIcfl && f.kind != kKfCfl) {
        return false;
    }
    const bool icfl = f.kind != kKfCfl;
    if (w <= kf_lds_window(f.kind, f.comb)) {
        sh.mode = icfl ? kKfModeLds : kKfModeCfl;
        sh.lds = kf_lds_bytes(icfl, sh.comb, w);
        return true;
    }
    if (n_desc && (!f.work || !f.work_groups)) return false;
    sh.mode = icfl ? kKfModeWide : kKfModeCflWide;
    sh.grid = std::min(n_desc, f.work_groups);
    return true;
}

// the instance of a kernel template K<MODE, COMB> that sh names (kKfModeCflWide exists combined
// only: plain Duval has no working memory)
#define KF_PICK(K, ...)                                                                          \
    (!sh.comb ? (sh.mode == kKfModeCfl   ? K<__VA_ARGS__ kKfModeCfl, false>                      \
                 : sh.mode == kKfModeLds ? K<__VA_ARGS__ kKfModeLds, false>                      \
                                         : K<__VA_ARGS__ kKfModeWide, false>)                    \
              : (sh.mode == kKfModeCfl    ? K<__VA_ARGS__ kKfModeCfl, true>                      \
                 : sh.mode == kKfModeLds  ? K<__VA_ARGS__ kKfModeLds, true>                      \
                 : sh.mode == kKfModeWide ? K<__VA_ARGS__ kKfModeWide, true>                     \
                                          : K<__VA_ARGS__ kKfModeCflWide, true>))

}  // namespace

hipError_t launch_kf_hash(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, uint32_t seed, uint32_t use64, void *d_hash,
                          uint32_t *d_n_vals, uint32_t *d_body, unsigned long long *d_val_total,
                          const KfFact &f, hipStream_t st)
{
    KfShape sh;
    if (w < 1 || w > kKfMaxWindow || !kf_shape(f, w, n_desc, sh)) return hipErrorInvalidValue;
    if (!n_desc) return hipSuccess;
    auto kernel = KF_PICK(kf_hash_kernel, );
    hipLaunchKernelGGL(kernel, dim3(sh.grid), dim3(kKfRun), sh.lds, st, d_seq, d_rec_pos, d_rec_len,
                       d_descs, n_desc, w, seed, use64, d_hash, d_n_vals, d_body, d_val_total,
                       sh.thr, (uint8_t *)f.work);
    return hipGetLastError();
}

hipError_t launch_kf_text_size(const KfDesc *d_descs, uint32_t n_desc, const uint32_t *d_body,
                               const uint32_t *d_id_len, uint32_t *d_size,
                               unsigned long long *d_text_total, hipStream_t st)
{
    if (!n_desc) return hipSuccess;
    hipLaunchKernelGGL(kf_text_size_kernel, dim3(n_desc), dim3(kKfRun), 0, st, d_descs, d_body,
                       d_id_len, d_size, d_text_total);
    return hipGetLastError();
}

namespace {

// pass two of either form: the instance the factorization and the window call for
template <bool TEXT>
hipError_t kf_launch_emit(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                          const uint64_t *d_id_off, const uint32_t *d_id_len, uint8_t *d_out,
                          uint16_t *d_vals, const KfFact &f, hipStream_t st)
{
    KfShape sh;
    if (w < 1 || w > kKfMaxWindow || !kf_shape(f, w, n_desc, sh)) return hipErrorInvalidValue;
    if (!n_desc) return hipSuccess;
    auto kernel = KF_PICK(kf_emit_kernel, TEXT, );
    hipLaunchKernelGGL(kernel, dim3(sh.grid), dim3(kKfRun), sh.lds, st, d_seq, d_rec_pos, d_rec_len,
                       d_descs, n_desc, w, d_off, d_ids, d_id_off, d_id_len, d_out, d_vals, sh.thr,
                       (uint8_t *)f.work);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_kf_values(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                            const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                            uint32_t w, const uint32_t *d_off, uint16_t *d_vals, const KfFact &f,
                            hipStream_t st)
{
    return kf_launch_emit<false>(d_seq, d_rec_pos, d_rec_len, d_descs, n_desc, w, d_off, nullptr,
                                 nullptr, nullptr, nullptr, d_vals, f, st);
}

hipError_t launch_kf_text(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                          const uint64_t *d_id_off, const uint32_t *d_id_len, uint8_t *d_out,
                          const KfFact &f, hipStream_t st)
{
    return kf_launch_emit<true>(d_seq, d_rec_pos, d_rec_len, d_descs, n_desc, w, d_off, d_ids,
                                d_id_off, d_id_len, d_out, nullptr, f, st);
}

hipError_t launch_kf_ext_size(const KfDesc *d_descs, uint32_t n_desc, const uint32_t *d_rec_len,
                              const uint32_t *d_piece_rec, uint32_t n_piece, uint32_t w,
                              bool fact, const uint32_t *d_n_vals, const uint32_t *d_body,
                              const uint32_t *d_id_len, uint32_t *d_size,
                              unsigned long long *d_text_total, hipStream_t st)
{
    if (!n_desc) return hipSuccess;
    hipLaunchKernelGGL(kf_ext_size_kernel, dim3(n_desc), dim3(kKfRun), 0, st, d_descs, d_rec_len,
                       d_piece_rec, n_piece, w, fact ? 1u : 0u, d_n_vals, d_body, d_id_len, d_size,
                       d_text_total);
    return hipGetLastError();
}

namespace {

template <bool FACT>
hipError_t kf_launch_ext(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                         const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                         uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                         const uint64_t *d_id_off, const uint32_t *d_id_len,
                         const uint32_t *d_piece_rec, uint32_t n_piece, uint8_t *d_out,
                         const KfFact &f, hipStream_t st)
{
    KfShape sh;
    if (w < 1 || w > kKfMaxWindow || !kf_shape(f, w, n_desc, sh)) return hipErrorInvalidValue;
    if (!n_desc) return hipSuccess;
    auto kernel = KF_PICK(kf_emit_ext_kernel, FACT, );
    hipLaunchKernelGGL(kernel, dim3(sh.grid), dim3(kKfRun), sh.lds, st, d_seq, d_rec_pos, d_rec_len,
                       d_descs, n_desc, w, d_off, d_ids, d_id_off, d_id_len, d_piece_rec, n_piece,
                       d_out, sh.thr, (uint8_t *)f.work);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_kf_ext_text(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                              const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                              uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                              const uint64_t *d_id_off, const uint32_t *d_id_len,
                              const uint32_t *d_piece_rec, uint32_t n_piece, bool fact,
                              uint8_t *d_out, const KfFact &f, hipStream_t st)
{
    return fact ? kf_launch_ext<true>(d_seq, d_rec_pos, d_rec_len, d_descs, n_desc, w, d_off,
                                      d_ids, d_id_off, d_id_len, d_piece_rec, n_piece, d_out, f, st)
                : kf_launch_ext<false>(d_seq, d_rec_pos, d_rec_len, d_descs, n_desc, w, d_off,
                                       d_ids, d_id_off, d_id_len, d_piece_rec, n_piece, d_out, f,
                                       st);
}

}  // namespace fpm
