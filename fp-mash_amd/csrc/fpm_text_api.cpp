// fpm_text_api.cpp — the text-input part of the C ABI declared in include/fpmash.h: -fp line
// hashing and -fp text parsing (fingerprint.hip), FASTA / FASTQ parsing on the device
// (seqparse.hip), and the staging of parsed records into a sketch job.
#include "fpm_internal.hpp"

#include <memory>

extern "C" {

// ----------------------------------------------------------------------------
// -fp line hashing
// ----------------------------------------------------------------------------

int fpm_fp_hash_lines_dev(fpm_ctx *ctx, const uint64_t *d_vals, const uint64_t *d_line_off,
                          uint64_t n_lines, uint32_t seed, uint32_t use64, void *d_out,
                          void *stream)
{
    if (int rc = set_device(ctx)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    TimedLaunch tl(ctx, FPM_K_FPHASH, st);
    HIP_TRY(launch_fp_hash(d_vals, d_line_off, n_lines, seed, use64, d_out, st));
    tl.done();
    return FPM_OK;
}

int fpm_fp_hash_lines(fpm_ctx *ctx, const uint64_t *vals, const uint64_t *line_off,
                      uint64_t n_lines, uint32_t seed, uint32_t use64, void *out)
{
    if (int rc = set_device(ctx)) return rc;
    if (!line_off || (n_lines && !out)) return fail(FPM_EINVAL, "null argument");
    if (n_lines == 0) return FPM_OK;
    const uint64_t nv = line_off[n_lines];
    const size_t ob = (use64 ? 8 : 4) * n_lines;
    DevBufs mem(ctx);
    uint64_t *dv, *doff;
    void *dout;
    hipError_t e = mem.get(&dv, std::max<uint64_t>(nv, 1) * 8);
    if (e == hipSuccess) e = mem.get(&doff, (n_lines + 1) * 8);
    if (e == hipSuccess) e = mem.get(&dout, ob);
    if (e == hipSuccess) e = copy_in(ctx, dv, vals, nv * 8);
    if (e == hipSuccess) e = copy_in(ctx, doff, line_off, (n_lines + 1) * 8);
    if (e != hipSuccess) return fail(FPM_EHIP, std::string("fp staging: ") + hipGetErrorString(e));
    if (int rc = fpm_fp_hash_lines_dev(ctx, dv, doff, n_lines, seed, use64, dout, nullptr)) return rc;
    e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = copy_out(ctx, out, dout, ob);
    if (e != hipSuccess) return fail(FPM_EHIP, std::string("fp fetch: ") + hipGetErrorString(e));
    return FPM_OK;
}

}  // extern "C"

// ----------------------------------------------------------------------------
// -fp text
// ----------------------------------------------------------------------------

struct fpm_fptext {
    fpm_ctx *ctx = nullptr;
    uint64_t n_lines = 0;
    uint32_t use64 = 0;
    uint8_t *d_text = nullptr;
    uint64_t *d_line_start = nullptr;
    uint32_t *d_blk = nullptr;
    uint64_t *d_id_off = nullptr;
    uint32_t *d_id_len = nullptr, *d_n_vals = nullptr;
    void *d_hash = nullptr;
    uint8_t *d_new_id = nullptr;
    // the file's References (fpm_fp_text_refs), computed on the first call
    bool refs_done = false;
    uint64_t n_refs = 0;
    uint64_t *d_first = nullptr, *d_length = nullptr, *d_ref_id_off = nullptr;
    uint32_t *d_ref_id_len = nullptr;
    DevBufs mem;                                   // owns every buffer above, all pooled
};

static void fptext_release(fpm_fptext *j)
{
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    // the job's kernels ran on the context stream: done before its buffers are handed out again
    (void)hipStreamSynchronize(j->ctx->stream);
}

extern "C" {

int fpm_fp_text_stage(fpm_ctx *ctx, const char *text, uint64_t text_len, uint64_t max_lines,
                      uint32_t seed, uint32_t use64, fpm_fptext **job, uint64_t *n_lines)
{
    if (!job || !n_lines) return fail(FPM_EINVAL, "fp_text_stage: null output");
    *job = nullptr;
    *n_lines = 0;
    if (int rc = set_device(ctx)) return rc;
    std::unique_ptr<fpm_fptext, void (*)(fpm_fptext *)> j(new fpm_fptext,
        [](fpm_fptext *p) { fptext_release(p); delete p; });
    j->ctx = j->mem.ctx = ctx;
    j->use64 = use64;
    hipStream_t st = ctx->stream;
    const uint32_t nb = text_blocks(text_len);
    const uint64_t scan_w = scan_scratch_words(nb ? nb : 1);
    HIP_TRY(j->mem.get_pooled(&j->d_text, text_len + 16));
    HIP_TRY(j->mem.get_pooled(&j->d_blk, ((size_t)2 * nb + 2 + scan_w) * 4));
    if (text_len) HIP_TRY(h2d_staged(ctx, j->d_text, text, text_len));
    uint32_t *blk_cnt = j->d_blk, *blk_off = j->d_blk + nb, *scan_s = j->d_blk + 2 * nb + 2;
    // newline count first: it sizes the line index
    uint64_t n_nl = 0;
    if (nb) {
        {
            TimedLaunch tl(ctx, FPM_K_FPTEXT, st);
            HIP_TRY(launch_fp_nl_count(j->d_text, text_len, blk_cnt, blk_off, scan_s, st));
            tl.done();
        }
        // the total (blk_off[nb], 8-B aligned: blk_off starts nb words into an aligned block)
        // through the mapped counter block: no copy + stream sync round trip
        if (int rc = read_counters(ctx, (const unsigned long long *)(blk_off + nb), 1, st)) return rc;
        n_nl = (uint32_t)ctx->host_counters[0];
    }
    HIP_TRY(j->mem.get_pooled(&j->d_line_start, (n_nl + 1) * 8));
    HIP_TRY(hipMemsetAsync(j->d_line_start, 0, 8, st));
    if (n_nl) {
        TimedLaunch tl(ctx, FPM_K_FPTEXT, st);
        HIP_TRY(launch_fp_nl_scatter(j->d_text, text_len, blk_off, j->d_line_start, st));
        tl.done();
    }
    const uint64_t total = n_nl + ((text_len && text[text_len - 1] != '\n') ? 1 : 0);
    const uint64_t nl = std::min(total, max_lines);
    j->n_lines = nl;
    if (nl) {
        HIP_TRY(j->mem.get_pooled(&j->d_id_off, nl * 8));
        HIP_TRY(j->mem.get_pooled(&j->d_id_len, nl * 4));
        HIP_TRY(j->mem.get_pooled(&j->d_n_vals, nl * 4));
        HIP_TRY(j->mem.get_pooled(&j->d_hash, nl * (use64 ? 8 : 4)));
        HIP_TRY(j->mem.get_pooled(&j->d_new_id, nl));
        TimedLaunch tl(ctx, FPM_K_FPTEXT, st);
        HIP_TRY(launch_fp_lines(j->d_text, text_len, j->d_line_start, n_nl, nl, seed, use64,
                                j->d_id_off, j->d_id_len, j->d_n_vals, j->d_hash, j->d_new_id, st));
        tl.done();
    }
    *n_lines = nl;
    *job = j.release();
    return FPM_OK;
}

int fpm_fp_text_fetch(fpm_fptext *j, uint64_t *id_off, uint32_t *id_len, uint32_t *n_vals,
                      void *hash, uint8_t *new_id)
{
    if (!j) return fail(FPM_EINVAL, "fp_text_fetch: null job");
    if (int rc = set_device(j->ctx)) return rc;
    hipStream_t st = j->ctx->stream;
    const uint64_t n = j->n_lines;
    HIP_TRY(hipStreamSynchronize(st));
    if (n) {
        fpm_ctx *ctx = j->ctx;
        if (id_off) HIP_TRY(copy_out(ctx, id_off, j->d_id_off, n * 8));
        if (id_len) HIP_TRY(copy_out(ctx, id_len, j->d_id_len, n * 4));
        if (n_vals) HIP_TRY(copy_out(ctx, n_vals, j->d_n_vals, n * 4));
        if (hash) HIP_TRY(copy_out(ctx, hash, j->d_hash, n * (j->use64 ? 8 : 4)));
        if (new_id) HIP_TRY(copy_out(ctx, new_id, j->d_new_id, n));
    }
    return FPM_OK;
}

int fpm_fp_text_refs(fpm_fptext *j, uint64_t cap, uint64_t *n_refs, uint64_t *first_line,
                     uint64_t *id_off, uint32_t *id_len, uint64_t *length)
{
    if (!j || !n_refs) return fail(FPM_EINVAL, "fp_text_refs: null argument");
    if (int rc = set_device(j->ctx)) return rc;
    fpm_ctx *ctx = j->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = j->n_lines;
    if (!j->refs_done && n) {
        const uint32_t nb = fp_head_blocks(n);
        uint32_t *blk;
        HIP_TRY(j->mem.get_pooled(&blk, ((size_t)2 * nb + 2 + scan_scratch_words(nb)) * 4));
        uint32_t *blk_cnt = blk, *blk_off = blk + nb, *scan_s = blk + 2 * nb + 2;
        {
            TimedLaunch tl(ctx, FPM_K_FPTEXT, st);
            HIP_TRY(launch_fp_heads(j->d_new_id, n, blk_cnt, blk_off, scan_s, st));
            tl.done();
        }
        // the total, as in fpm_fp_text_stage
        if (int rc = read_counters(ctx, (const unsigned long long *)(blk_off + nb), 1, st)) return rc;
        const uint32_t tot = (uint32_t)ctx->host_counters[0];
        j->n_refs = tot;
        uint64_t *blk4;
        HIP_TRY(j->mem.get_pooled(&blk4, (size_t)tot * 28 + 32));
        j->d_first = blk4;
        j->d_ref_id_off = blk4 + tot;
        j->d_length = blk4 + 2 * (size_t)tot;
        j->d_ref_id_len = reinterpret_cast<uint32_t *>(blk4 + 3 * (size_t)tot);
        TimedLaunch tl(ctx, FPM_K_FPTEXT, st);
        HIP_TRY(launch_fp_refs(j->d_new_id, n, blk_off, tot, j->d_n_vals, j->d_id_off,
                               j->d_id_len, j->d_first, j->d_length, j->d_ref_id_off,
                               j->d_ref_id_len, st));
        tl.done();
    }
    j->refs_done = true;
    *n_refs = j->n_refs;
    if (cap < j->n_refs || !j->n_refs) return FPM_OK;     // sized by this call
    const uint64_t m = j->n_refs;
    // the four arrays are one device block (first, ID offset, length: u64; ID length: u32):
    // one copy into the pinned ring and one wait, then spread into the caller's arrays
    const size_t bytes = m * 28;
    if (bytes <= fpm_ctx::kRingBytes) {
        HIP_TRY(ensure_ring(ctx));
        HIP_TRY(hipMemcpyAsync(ctx->ring[0], j->d_first, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const char *r = static_cast<const char *>(ctx->ring[0]);
        if (first_line) memcpy(first_line, r, m * 8);
        if (id_off) memcpy(id_off, r + m * 8, m * 8);
        if (length) memcpy(length, r + m * 16, m * 8);
        if (id_len) memcpy(id_len, r + m * 24, m * 4);
        return FPM_OK;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (first_line) HIP_TRY(copy_out(ctx, first_line, j->d_first, m * 8));
    if (id_off) HIP_TRY(copy_out(ctx, id_off, j->d_ref_id_off, m * 8));
    if (id_len) HIP_TRY(copy_out(ctx, id_len, j->d_ref_id_len, m * 4));
    if (length) HIP_TRY(copy_out(ctx, length, j->d_length, m * 8));
    return FPM_OK;
}

void fpm_fp_text_free(fpm_fptext *j)
{
    fptext_release(j);
    delete j;
}

void fpm_fp_text_limits(uint32_t *text_chunk, uint32_t *span_bytes, uint32_t *head_lines)
{
    if (text_chunk) *text_chunk = fp_text_chunk();
    if (span_bytes) *span_bytes = fp_span_bytes();
    if (head_lines) *head_lines = fp_head_lines();
}

}  // extern "C"

// ----------------------------------------------------------------------------
// FASTA text -> packed records on the device (seqparse.hip)
// ----------------------------------------------------------------------------

struct fpm_seqtext {
    fpm_ctx *ctx = nullptr;
    std::vector<uint64_t> seg_off, seg_len;     // each file's offset in the device text
    uint64_t n_rec = 0, total_kept = 0;
    uint8_t *d_text = nullptr, *d_reset = nullptr, *d_out = nullptr;
    void *d_xf = nullptr, *d_cin = nullptr;
    uint64_t *d_rec = nullptr;                  // hdr_pos | hdr_end | kept_at | seq_off | seq_len
    uint64_t *d_totals = nullptr;
    DevBufs mem;                                // owns every buffer above
};

static void seqtext_release(fpm_seqtext *j)
{
    if (j) (void)hipSetDevice(j->ctx->device);
}

// The FASTQ path of fpm_seq_parse (seqparse.hip: 4-line records verified against kseq_read):
// newline index, lines per file, record table + packed bases.  *ok = false when a record does
// not read the 4-line way (nothing of the job changed then).
static int fastq_parse(fpm_ctx *ctx, fpm_seqtext *j, uint64_t text_bytes, hipStream_t st, bool *ok)
{
    *ok = false;
    const uint32_t n_seg = (uint32_t)j->seg_off.size();
    DevBufs tmp(ctx);   // the scratch, and until the end the record table and the packed records
    const uint32_t nb = text_blocks(text_bytes);
    const uint64_t scan_w = scan_scratch_words(nb ? nb : 1);
    uint32_t *blk;
    HIP_TRY(tmp.get(&blk, ((size_t)2 * nb + 2 + scan_w) * 4));
    uint32_t *blk_cnt = blk, *blk_off = blk + nb, *scan_s = blk + 2 * nb + 2;
    TimedLaunch tl(ctx, FPM_K_SEQPARSE, st);
    HIP_TRY(launch_fp_nl_count(j->d_text, text_bytes, blk_cnt, blk_off, scan_s, st));
    uint32_t n_nl = 0;
    HIP_TRY(hipMemcpyAsync(&n_nl, blk_off + nb, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t *line_start, *d_seg, *file_lines;
    HIP_TRY(tmp.get(&line_start, ((size_t)n_nl + 1) * 8));
    HIP_TRY(hipMemsetAsync(line_start, 0, 8, st));
    HIP_TRY(launch_fp_nl_scatter(j->d_text, text_bytes, blk_off, line_start, st));
    std::vector<uint64_t> seg(2 * (size_t)n_seg), fl(2 * (size_t)n_seg);
    for (uint32_t f = 0; f < n_seg; f++) {
        seg[2 * f] = j->seg_off[f];
        seg[2 * f + 1] = j->seg_len[f];
    }
    HIP_TRY(tmp.get(&d_seg, seg.size() * 8));
    HIP_TRY(tmp.get(&file_lines, seg.size() * 8));
    if (n_seg) HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), seg.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_fq_files(line_start, (uint64_t)n_nl + 1, d_seg, n_seg, file_lines, st));
    if (n_seg) HIP_TRY(hipMemcpyAsync(fl.data(), file_lines, fl.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> base(n_seg ? n_seg : 1, 0);
    uint64_t n_rec = 0;
    for (uint32_t f = 0; f < n_seg; f++) {
        base[f] = n_rec;
        n_rec += fl[2 * f + 1] / 4;
    }
    uint64_t *d_base, *d_rec, *d_scan, *d_total;
    uint32_t *d_fail;
    HIP_TRY(tmp.get(&d_base, base.size() * 8));
    HIP_TRY(tmp.get(&d_rec, (size_t)(n_rec ? n_rec : 1) * 5 * 8));
    HIP_TRY(tmp.get(&d_scan, ((n_rec + 1023) / 1024 + 1) * 8));
    HIP_TRY(tmp.get(&d_total, 16));
    HIP_TRY(tmp.get(&d_fail, 4));
    HIP_TRY(hipMemcpyAsync(d_base, base.data(), base.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_fail, 0, 4, st));
    HIP_TRY(hipMemsetAsync(d_total, 0, 16, st));
    HIP_TRY(launch_fq_records(j->d_text, line_start, d_seg, file_lines, d_base, n_seg, n_rec, d_rec,
                              d_scan, d_total, d_fail, nullptr, st));
    uint64_t total = 0;
    uint32_t failed = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&failed, d_fail, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (failed) {
        tl.done();
        return FPM_OK;
    }
    uint8_t *d_out;
    HIP_TRY(tmp.get(&d_out, total + n_rec + 64));
    hipError_t e = launch_fq_emit(j->d_text, n_rec, d_rec, d_out, st);
    if (e == hipSuccess) {
        tl.done();
        e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return fail(FPM_EHIP, std::string("fastq emit: ") + hipGetErrorString(e));
    j->mem.adopt(j->d_rec = tmp.release(d_rec));   // the job keeps these two
    j->mem.adopt(j->d_out = tmp.release(d_out));
    j->n_rec = n_rec;
    j->total_kept = total;
    *ok = true;
    return FPM_OK;
}

extern "C" {

int fpm_seq_parse(fpm_ctx *ctx, const char *const *seg_text, const uint64_t *seg_len,
                  uint32_t n_seg, fpm_seqtext **job, uint64_t *n_records, int *quality_lines)
{
    if (!job || !n_records || (n_seg && (!seg_text || !seg_len)))
        return fail(FPM_EINVAL, "seq_parse: null argument");
    *job = nullptr;
    *n_records = 0;
    if (quality_lines) *quality_lines = 0;
    if (int rc = set_device(ctx)) return rc;
    std::unique_ptr<fpm_seqtext, void (*)(fpm_seqtext *)> j(new fpm_seqtext,
        [](fpm_seqtext *p) { seqtext_release(p); delete p; });
    j->ctx = j->mem.ctx = ctx;
    // each file from a chunk boundary, at least one '\n' after it
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_seg; i++) {
        j->seg_off.push_back(at);
        j->seg_len.push_back(seg_len[i]);
        at = (at + seg_len[i] + 1 + kSpChunk - 1) / kSpChunk * kSpChunk;
    }
    const uint64_t text_bytes = at;
    const uint64_t n_chunks64 = text_bytes / kSpChunk;
    if (n_chunks64 > 0xFFFFFFFFull) return fail(FPM_EINVAL, "seq_parse: input too large");
    const uint32_t n_chunks = (uint32_t)n_chunks64;
    hipStream_t st = ctx->stream;
    // 64 bytes of slack: the FASTQ emit reads whole 64-byte windows past a sequence line
    HIP_TRY(j->mem.get(&j->d_text, text_bytes + 64));
    HIP_TRY(j->mem.get(&j->d_reset, n_chunks ? n_chunks : 1));
    HIP_TRY(j->mem.get(&j->d_xf, (size_t)(n_chunks ? n_chunks : 1) * seq_xf_bytes()));
    HIP_TRY(j->mem.get(&j->d_cin, (size_t)(n_chunks ? n_chunks : 1) * seq_cin_bytes()));
    HIP_TRY(j->mem.get(&j->d_totals, 3 * sizeof(uint64_t)));
    std::vector<uint8_t> reset(n_chunks ? n_chunks : 1, 0);
    for (uint32_t i = 0; i < n_seg; i++)
        if (j->seg_off[i] / kSpChunk < n_chunks) reset[j->seg_off[i] / kSpChunk] = 1;
    HIP_TRY(hipMemsetAsync(j->d_text, '\n', text_bytes, st));
    HIP_TRY(hipMemcpyAsync(j->d_reset, reset.data(), n_chunks, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n_seg; i++)
        HIP_TRY(h2d_staged(ctx, j->d_text + j->seg_off[i], seg_text[i], seg_len[i]));
    // the records are emitted: the text image and scan scratch are not needed past that point
    auto finish = [&]() {
        j->mem.drop(j->d_text);
        j->mem.drop(j->d_xf);
        j->mem.drop(j->d_cin);
        *n_records = j->n_rec;
        *job = j.release();
        return FPM_OK;
    };
    uint64_t tot[3] = {0, 0, 0};
    if (n_chunks) {
        TimedLaunch tl(ctx, FPM_K_SEQPARSE, st);
        HIP_TRY(launch_seq_scan(j->d_text, j->d_reset, n_chunks, j->d_xf, j->d_cin, j->d_totals, st));
        tl.done();
        HIP_TRY(hipMemcpyAsync(tot, j->d_totals, sizeof(tot), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (tot[2]) {
        // a '+' in sequence text: FASTQ.  The 4-line layout is parsed on the device and every
        // record verified against kseq_read's quality rules; a file that does not read that way
        // leaves *quality_lines set and the caller walks the files on the host
        bool parsed = false;
        if (int rc = fastq_parse(ctx, j.get(), text_bytes, st, &parsed)) return rc;
        if (parsed) return finish();
    }
    j->n_rec = tot[0];
    j->total_kept = tot[1];
    if (quality_lines) *quality_lines = tot[2] ? 1 : 0;
    HIP_TRY(j->mem.get(&j->d_out, j->total_kept + j->n_rec + 64));
    HIP_TRY(j->mem.get(&j->d_rec, (size_t)(j->n_rec ? j->n_rec : 1) * 5 * sizeof(uint64_t)));
    if (n_chunks) {
        const uint64_t n = j->n_rec ? j->n_rec : 1;
        TimedLaunch tl(ctx, FPM_K_SEQPARSE, st);
        HIP_TRY(launch_seq_emit(j->d_text, n_chunks, j->d_cin, j->n_rec, j->total_kept, j->d_rec,
                                j->d_rec + n, j->d_rec + 2 * n, j->d_rec + 3 * n, j->d_rec + 4 * n,
                                j->d_out, st));
        tl.done();
    }
    HIP_TRY(hipStreamSynchronize(st));
    return finish();
}

int fpm_seq_records(fpm_seqtext *j, uint32_t *seg_of_rec, uint64_t *hdr_off, uint64_t *hdr_len,
                    uint64_t *seq_len)
{
    if (!j) return fail(FPM_EINVAL, "seq_records: null job");
    if (int rc = set_device(j->ctx)) return rc;
    const uint64_t n = j->n_rec;
    if (!n) return FPM_OK;
    std::vector<uint64_t> rec((size_t)n * 5);
    HIP_TRY(d2h_staged(j->ctx, rec.data(), j->d_rec, rec.size() * 8));
    const uint64_t *pos = rec.data(), *end = pos + n, *len = pos + 4 * n;
    for (uint64_t r = 0; r < n; r++) {
        // the file holding the header: the last segment starting at or before it
        const uint32_t sg = (uint32_t)(std::upper_bound(j->seg_off.begin(), j->seg_off.end(), pos[r]) -
                                       j->seg_off.begin()) - 1;
        const uint64_t o = pos[r] - j->seg_off[sg];
        // the header's '\n', or the end of its file (the '\n' bytes after a file are padding)
        const uint64_t e = std::min(end[r] - j->seg_off[sg], j->seg_len[sg]);
        if (seg_of_rec) seg_of_rec[r] = sg;
        if (hdr_off) hdr_off[r] = o;
        if (hdr_len) hdr_len[r] = e - o;
        if (seq_len) seq_len[r] = len[r];
    }
    return FPM_OK;
}

int fpm_seq_packed(fpm_seqtext *j, uint64_t *seq_off, uint8_t *out, uint64_t cap,
                   uint64_t *n_bytes)
{
    if (!j || !n_bytes) return fail(FPM_EINVAL, "seq_packed: null argument");
    if (int rc = set_device(j->ctx)) return rc;
    if (!j->d_out) return fail(FPM_EINVAL, "seq_packed: records already staged");
    const uint64_t n = j->n_rec, bytes = j->total_kept + n;
    *n_bytes = bytes;
    if (!out) return FPM_OK;                              // sized by this call
    if (cap < bytes) return fail(FPM_EINVAL, "seq_packed: buffer too small");
    // seq_off is the fourth of d_rec's five arrays in both layouts (the FASTA emit strides
    // them by max(n_rec, 1), the FASTQ emit by n_rec: the same wherever a record exists)
    if (seq_off) HIP_TRY(d2h_staged(j->ctx, seq_off, j->d_rec + 3 * n, n * 8));
    HIP_TRY(d2h_staged(j->ctx, out, j->d_out, bytes));
    return FPM_OK;
}

}  // extern "C"

int seqtext_records(fpm_ctx *ctx, fpm_seqtext *seq, uint64_t *n_rec, std::vector<uint64_t> *pos,
                    std::vector<uint64_t> *len, uint8_t **d_packed)
{
    if (seq->ctx != ctx) return fail(FPM_EINVAL, "records parsed on another context");
    if (!seq->d_out) return fail(FPM_EINVAL, "records already staged");
    const uint64_t n = seq->n_rec, nn = n ? n : 1;
    pos->resize(n);
    len->resize(n);
    HIP_TRY(d2h_staged(ctx, pos->data(), seq->d_rec + 3 * nn, n * 8));
    HIP_TRY(d2h_staged(ctx, len->data(), seq->d_rec + 4 * nn, n * 8));
    *n_rec = n;
    *d_packed = seq->mem.release(seq->d_out);
    seq->d_out = nullptr;
    return FPM_OK;
}

extern "C" {

void fpm_seq_free(fpm_seqtext *j)
{
    seqtext_release(j);
    delete j;
}

int fpm_sketch_stage_seq(fpm_ctx *ctx, const fpm_sketch_params *p, fpm_seqtext *seq,
                         const uint32_t *group_of_rec, uint32_t n_groups, fpm_sketch_job **job_out)
{
    if (int rc = set_device(ctx)) return rc;
    if (!p || !seq || !job_out || (seq->n_rec && !group_of_rec))
        return fail(FPM_EINVAL, "sketch_stage_seq: null argument");
    if (seq->ctx != ctx) return fail(FPM_EINVAL, "sketch_stage_seq: records parsed on another context");
    if (!seq->d_out) return fail(FPM_EINVAL, "sketch_stage_seq: records already staged");
    *job_out = nullptr;
    const uint64_t n = seq->n_rec;
    if (n > 0xFFFFFFFFull) return fail(FPM_EINVAL, "sketch_stage_seq: too many records");
    StageRecords R;
    R.n_groups = n_groups;
    R.pos.resize(n);
    R.len.resize(n);
    R.group.assign(group_of_rec, group_of_rec + n);
    const uint64_t nn = n ? n : 1;
    HIP_TRY(d2h_staged(ctx, R.pos.data(), seq->d_rec + 3 * nn, n * 8));
    HIP_TRY(d2h_staged(ctx, R.len.data(), seq->d_rec + 4 * nn, n * 8));
    for (uint64_t r = 0; r < n; r++) {
        if (group_of_rec[r] == FPM_NO_GROUP) continue;
        if (group_of_rec[r] >= n_groups) return fail(FPM_EINVAL, "group id out of range");
        R.order.push_back((uint32_t)r);
    }
    std::stable_sort(R.order.begin(), R.order.end(),
                     [&](uint32_t a, uint32_t b) { return R.group[a] < R.group[b]; });
    R.d_seq = seq->d_out;
    R.d_seq_bytes = seq->total_kept + seq->n_rec;
    if (int rc = stage_core(ctx, p, R, job_out)) return rc;
    seq->mem.release(seq->d_out);   // the job owns the packed records now
    seq->d_out = nullptr;
    return FPM_OK;
}

}  // extern "C"
