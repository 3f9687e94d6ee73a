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
#include "fpm_device.hpp"
#include "fpm_kernels.hpp"

namespace fpm {

namespace {

// LDS bytes a workgroup stages: a full run at the widest window, rounded up to dwords
constexpr uint32_t kKfLds = (kKfStage + 3) / 4 * 4;

__device__ __forceinline__ uint8_t kf_upper(uint8_t c)
{
    // ASCII a-z only; every other byte (those >= 0x80 too) stays as it is
    return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
}

// Duval (factorizations.py:102-126), bytes compared unsigned; emit(len) per Lyndon factor
template <typename Emit>
__device__ __forceinline__ void kf_duval(const uint8_t *s, uint32_t n, Emit emit)
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
__global__ __launch_bounds__(kKfRun) void kf_hash_kernel(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc *__restrict__ descs, uint32_t w,
    uint32_t seed, uint32_t use64, void *__restrict__ hash, uint32_t *__restrict__ n_vals,
    uint32_t *__restrict__ body, unsigned long long *__restrict__ val_total)
{
    __shared__ uint8_t s_seq[kKfLds];
    __shared__ uint32_t s_off[kKfRun];
    __shared__ unsigned long long s_red[kKfRun / 64];
    const KfDesc d = descs[blockIdx.x];
    uint32_t base, n, rec;
    const bool active = kf_stage(seq, rec_pos, rec_len, d, w, s_seq, s_off, base, n, rec);
    uint32_t cnt = 0;
    if (active) {
        uint32_t bytes = 1;
        uint64_t h1 = seed, h2 = seed, pend = 0;
        // Murmur over the lengths as little-endian u64 (hash.cpp:45-73): a 16-byte block per two
        // values, an odd last value as the 8-byte tail, 8 * count folded in at the end
        kf_duval(s_seq + base, n, [&](uint32_t len) {
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
template <bool TEXT>
__global__ __launch_bounds__(kKfRun) void kf_emit_kernel(
    const uint8_t *__restrict__ seq, const uint64_t *__restrict__ rec_pos,
    const uint32_t *__restrict__ rec_len, const KfDesc *__restrict__ descs, uint32_t w,
    const uint32_t *__restrict__ off, const uint8_t *__restrict__ ids,
    const uint64_t *__restrict__ id_off, const uint32_t *__restrict__ id_len,
    uint8_t *__restrict__ out, uint16_t *__restrict__ vals)
{
    __shared__ uint8_t s_seq[kKfLds];
    __shared__ uint32_t s_off[kKfRun];
    const KfDesc d = descs[blockIdx.x];
    uint32_t base, n, rec;
    if (!kf_stage(seq, rec_pos, rec_len, d, w, s_seq, s_off, base, n, rec)) return;
    const uint64_t line = d.line_base + threadIdx.x;
    if (TEXT) {
        uint8_t *o = out + off[line];
        const uint8_t *id = ids + id_off[rec];
        const uint32_t il = id_len[rec];
        for (uint32_t t = 0; t < il; t++) o[t] = id[t];
        o += il;
        kf_duval(s_seq + base, n, [&](uint32_t len) {
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
        kf_duval(s_seq + base, n, [&](uint32_t len) { *o++ = (uint16_t)len; });
    }
}

hipError_t launch_kf_hash(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, uint32_t seed, uint32_t use64, void *d_hash,
                          uint32_t *d_n_vals, uint32_t *d_body, unsigned long long *d_val_total,
                          hipStream_t st)
{
    if (w < 1 || w > kKfMaxWindow) return hipErrorInvalidValue;
    if (!n_desc) return hipSuccess;
    hipLaunchKernelGGL(kf_hash_kernel, dim3(n_desc), dim3(kKfRun), 0, st, d_seq, d_rec_pos,
                       d_rec_len, d_descs, w, seed, use64, d_hash, d_n_vals, d_body, d_val_total);
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

hipError_t launch_kf_values(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                            const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                            uint32_t w, const uint32_t *d_off, uint16_t *d_vals, hipStream_t st)
{
    if (w < 1 || w > kKfMaxWindow) return hipErrorInvalidValue;
    if (!n_desc) return hipSuccess;
    hipLaunchKernelGGL(kf_emit_kernel<false>, dim3(n_desc), dim3(kKfRun), 0, st, d_seq, d_rec_pos,
                       d_rec_len, d_descs, w, d_off, (const uint8_t *)nullptr,
                       (const uint64_t *)nullptr, (const uint32_t *)nullptr, (uint8_t *)nullptr,
                       d_vals);
    return hipGetLastError();
}

hipError_t launch_kf_text(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                          const uint64_t *d_id_off, const uint32_t *d_id_len, uint8_t *d_out,
                          hipStream_t st)
{
    if (w < 1 || w > kKfMaxWindow) return hipErrorInvalidValue;
    if (!n_desc) return hipSuccess;
    hipLaunchKernelGGL(kf_emit_kernel<true>, dim3(n_desc), dim3(kKfRun), 0, st, d_seq, d_rec_pos,
                       d_rec_len, d_descs, w, d_off, d_ids, d_id_off, d_id_len, d_out,
                       (uint16_t *)nullptr);
    return hipGetLastError();
}

}  // namespace fpm
