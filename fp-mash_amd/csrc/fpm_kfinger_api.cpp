// fpm_kfinger_api.cpp — the k-finger part of the C ABI declared in include/fpmash.h: CFL,
// ICFL or CFL_ICFL k-fingers of sequence records and their combined (_COMB) forms (kfinger.hip),
// their line hashes, and the lines as u16 values or as text; the long-read jobs, whose unit is one
// of a record's consecutive pieces (fpm_kfinger_stage_split), and the factor text of either.
#include "fpm_internal.hpp"

#include <memory>

struct fpm_kfinger {
    fpm_ctx *ctx = nullptr;
    uint32_t window = 0, use64 = 0, n_desc = 0;
    uint64_t n_in = 0;                       // input records (taken or not)
    uint64_t n_lines = 0;
    bool ran = false;
    KfFact fact;                             // CFL unless fpm_kfinger_set_factorization said else,
                                             // combined where fpm_kfinger_set_comb said so;
                                             // its work: the wide windows' working memory (pooled)
    hipStream_t stream = nullptr;            // the last run's
    std::vector<uint64_t> rec_first_line;    // n_in + 1
    std::vector<uint32_t> src;               // input record of each kept record
    uint8_t *d_seq = nullptr;                // the records' bytes (hipMalloc: own or adopted)
                                             // every other buffer below is pooled
    uint64_t *d_rec_pos = nullptr;           // per kept record
    uint32_t *d_rec_len = nullptr;
    KfDesc *d_desc = nullptr;
    void *d_hash = nullptr;
    uint32_t *d_n_vals = nullptr, *d_body = nullptr;
    uint32_t *d_size = nullptr, *d_off = nullptr, *d_scan = nullptr;   // pass two, per line
    unsigned long long *d_totals = nullptr;  // [0] values of all lines, [1] text bytes
    // a split job (fpm_kfinger_stage_split): d_rec_pos / d_rec_len are per piece, a line is a
    // piece, `window` is the split and d_piece_rec the kept record of each piece
    bool split = false;
    uint32_t *d_piece_rec = nullptr;
    // the last text call's IDs (packed per kept record), uploaded, and which text's size pass
    // ran over them (kSized*)
    bool ids_up = false;
    int sized = 0;
    std::string text_ids;
    std::vector<uint32_t> text_id_len;
    uint8_t *d_ids = nullptr;
    uint64_t *d_id_off = nullptr;
    uint32_t *d_id_len = nullptr;
    uint64_t text_total = 0;
    DevBufs mem;                             // owns every buffer above
};

static void kfinger_release(fpm_kfinger *j)
{
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    // the job's kernels are done before its buffers are handed out again
    (void)hipStreamSynchronize(j->stream ? j->stream : j->ctx->stream);
    (void)hipStreamSynchronize(j->ctx->stream);
}

namespace {

using JobPtr = std::unique_ptr<fpm_kfinger, void (*)(fpm_kfinger *)>;

JobPtr new_job(fpm_ctx *ctx)
{
    JobPtr j(new fpm_kfinger, [](fpm_kfinger *p) { kfinger_release(p); delete p; });
    j->ctx = j->mem.ctx = ctx;
    return j;
}

// The descriptors of the taken records (pos / len per input record, in the job's d_seq), cut at
// max_lines, and the per-record arrays on the device.
int plan(fpm_kfinger *j, const std::vector<uint64_t> &pos, const std::vector<uint64_t> &len,
         const uint8_t *take, uint32_t window, uint64_t max_lines)
{
    fpm_ctx *ctx = j->ctx;
    const uint64_t n = pos.size();
    j->n_in = n;
    j->window = window;
    j->rec_first_line.assign(n + 1, 0);
    std::vector<uint64_t> kpos;
    std::vector<uint32_t> klen;
    std::vector<KfDesc> descs;
    uint64_t line = 0;
    // the open pack of short records: its first kept record, records and bytes
    uint32_t pack_first = 0, pack_n = 0, pack_bytes = 0;
    uint64_t pack_line = 0;
    auto flush = [&] {
        if (pack_n) descs.push_back(KfDesc{pack_line, pack_first, 0, pack_n, 1});
        pack_n = pack_bytes = 0;
    };
    for (uint64_t r = 0; r < n; r++) {
        j->rec_first_line[r] = line;
        if ((take && !take[r]) || len[r] == 0 || line >= max_lines) continue;
        if (len[r] > 0xFFFFFFFFull) return fail(FPM_EINVAL, "kfinger: a record of 2^32 bytes or more");
        const uint32_t k = (uint32_t)kpos.size();
        if (k == 0xFFFFFFFFu) return fail(FPM_EINVAL, "kfinger: too many records");
        kpos.push_back(pos[r]);
        klen.push_back((uint32_t)len[r]);
        j->src.push_back((uint32_t)r);
        if (len[r] < window) {
            if (pack_n == kKfRun || pack_bytes + len[r] > kKfStage) flush();
            if (!pack_n) { pack_first = k; pack_line = line; }
            pack_n++;
            pack_bytes += (uint32_t)len[r];
            line++;
            continue;
        }
        flush();
        const uint64_t lines = std::min<uint64_t>(len[r], max_lines - line);
        for (uint64_t s = 0; s < lines; s += kKfRun)
            descs.push_back(KfDesc{line + s, k, (uint32_t)s,
                                   (uint32_t)std::min<uint64_t>(kKfRun, lines - s), 0});
        line += lines;
    }
    flush();
    j->rec_first_line[n] = line;
    j->n_lines = line;
    if (descs.size() > 0x7FFFFFFFull) return fail(FPM_EINVAL, "kfinger: too many lines for one job");
    j->n_desc = (uint32_t)descs.size();
    HIP_TRY(j->mem.get_pooled(&j->d_rec_pos, kpos.size() * 8));
    HIP_TRY(j->mem.get_pooled(&j->d_rec_len, klen.size() * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_desc, descs.size() * sizeof(KfDesc)));
    if (!kpos.empty()) {
        HIP_TRY(h2d_staged(ctx, j->d_rec_pos, kpos.data(), kpos.size() * 8));
        HIP_TRY(h2d_staged(ctx, j->d_rec_len, klen.data(), klen.size() * 4));
    }
    if (!descs.empty()) HIP_TRY(h2d_staged(ctx, j->d_desc, descs.data(), descs.size() * sizeof(KfDesc)));
    HIP_TRY(j->mem.get_pooled(&j->d_hash, line * 8));
    HIP_TRY(j->mem.get_pooled(&j->d_n_vals, line * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_body, line * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_totals, 16));
    return FPM_OK;
}

// The split job's plan (factors_string, fingerprint_utils.py:114-130): every taken record of
// n > 0 bytes is one piece when n < split, else the pieces [0, split) [split, 2 split) ... with
// a last one of n mod split bytes where that is not 0.  The pieces stand where plan() has its
// kept records, and consecutive ones share pack descriptors of at most kKfRun pieces and
// kKfStage bytes (a piece has at most split <= kKfMaxWindow < kKfStage), across records.
int plan_split(fpm_kfinger *j, const std::vector<uint64_t> &pos, const std::vector<uint64_t> &len,
               const uint8_t *take, uint32_t split)
{
    fpm_ctx *ctx = j->ctx;
    const uint64_t n = pos.size();
    j->n_in = n;
    j->window = split;
    j->split = true;
    j->rec_first_line.assign(n + 1, 0);
    std::vector<uint64_t> ppos;
    std::vector<uint32_t> plen, prec;
    std::vector<KfDesc> descs;
    uint32_t pack_first = 0, pack_n = 0, pack_bytes = 0;
    auto flush = [&] {
        if (pack_n) descs.push_back(KfDesc{pack_first, pack_first, 0, pack_n, 1});
        pack_n = pack_bytes = 0;
    };
    for (uint64_t r = 0; r < n; r++) {
        j->rec_first_line[r] = ppos.size();
        if ((take && !take[r]) || len[r] == 0) continue;
        if (len[r] > 0xFFFFFFFFull) return fail(FPM_EINVAL, "kfinger: a record of 2^32 bytes or more");
        const uint32_t k = (uint32_t)j->src.size();
        const uint64_t step = len[r] < split ? len[r] : split;
        if (ppos.size() + (len[r] + step - 1) / step > 0xFFFFFFFEull)
            return fail(FPM_EINVAL, "kfinger: too many pieces for one job");
        j->src.push_back((uint32_t)r);
        for (uint64_t o = 0; o < len[r]; o += step) {
            const uint32_t pl = (uint32_t)std::min<uint64_t>(step, len[r] - o);
            if (pack_n == kKfRun || pack_bytes + pl > kKfStage) flush();
            if (!pack_n) pack_first = (uint32_t)ppos.size();
            pack_n++;
            pack_bytes += pl;
            ppos.push_back(pos[r] + o);
            plen.push_back(pl);
            prec.push_back(k);
        }
    }
    flush();
    const uint64_t pieces = ppos.size();
    j->rec_first_line[n] = pieces;
    j->n_lines = pieces;
    j->n_desc = (uint32_t)descs.size();
    HIP_TRY(j->mem.get_pooled(&j->d_rec_pos, pieces * 8));
    HIP_TRY(j->mem.get_pooled(&j->d_rec_len, pieces * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_piece_rec, pieces * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_desc, descs.size() * sizeof(KfDesc)));
    if (pieces) {
        HIP_TRY(h2d_staged(ctx, j->d_rec_pos, ppos.data(), pieces * 8));
        HIP_TRY(h2d_staged(ctx, j->d_rec_len, plen.data(), pieces * 4));
        HIP_TRY(h2d_staged(ctx, j->d_piece_rec, prec.data(), pieces * 4));
        HIP_TRY(h2d_staged(ctx, j->d_desc, descs.data(), descs.size() * sizeof(KfDesc)));
    }
    HIP_TRY(j->mem.get_pooled(&j->d_hash, pieces * 8));
    HIP_TRY(j->mem.get_pooled(&j->d_n_vals, pieces * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_body, pieces * 4));
    HIP_TRY(j->mem.get_pooled(&j->d_totals, 16));
    return FPM_OK;
}

bool window_ok(uint32_t w) { return w >= 1 && w <= kKfMaxWindow; }

// The working memory for windows past kf_lds_window of the job's factorization: one region per
// workgroup of a grid of two workgroups per compute unit, whatever the job's line count
int wide_work(fpm_kfinger *j)
{
    if (j->window <= kf_lds_window(j->fact.kind, j->fact.comb) || j->fact.work || !j->n_desc)
        return FPM_OK;
    int n_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, j->ctx->device));
    const uint32_t groups = kf_wide_groups(j->n_desc, (uint32_t)std::max(n_cu, 1));
    uint8_t *work = nullptr;
    HIP_TRY(j->mem.get_pooled(&work, groups * kf_region_bytes(j->fact.kind != kKfCfl,
                                                               j->fact.comb != 0, j->window)));
    j->fact.work = work;
    j->fact.work_groups = groups;
    return FPM_OK;
}

// the exclusive scan of d_size into d_off (both per line), on the job's stream
int scan_sizes(fpm_kfinger *j, hipStream_t st)
{
    if (!j->d_off) {
        HIP_TRY(j->mem.get_pooled(&j->d_off, j->n_lines * 4));
        HIP_TRY(j->mem.get_pooled(&j->d_scan, scan_scratch_words(j->n_lines ? j->n_lines : 1) * 4));
    }
    HIP_TRY(launch_exscan(j->d_size, j->d_off, nullptr, j->n_lines, j->d_scan, nullptr, st));
    return FPM_OK;
}

// what the job's d_size / text_total hold: nothing, the k-finger text, or the factor text
enum : int { kSizedNone = 0, kSizedText = 1, kSizedFact = 2 };

// fpm_kfinger_text and fpm_kfinger_fact_text (fact): size, scan, emit.  A window job's k-finger
// text runs the kernels it always has; a split job's text and every factor text run
// kf_ext_size_kernel / kf_emit_ext_kernel.
int text_out(fpm_kfinger *j, const char *ids, const uint64_t *id_off, char *out, uint64_t cap,
             uint64_t *n_bytes, bool fact, const char *who)
{
    const std::string name = std::string(who);
    if (!j || !n_bytes) return fail(FPM_EINVAL, name + ": null argument");
    fpm_ctx *ctx = j->ctx;
    if (int rc = set_device(ctx)) return rc;
    if (!j->ran) return fail(FPM_EINVAL, name + ": the job has not run");
    *n_bytes = 0;
    const uint64_t n = j->n_lines;
    if (!n) return FPM_OK;
    if (!ids || !id_off) return fail(FPM_EINVAL, name + ": null ids");
    hipStream_t st = j->stream;
    const bool ext = fact || j->split;
    // the IDs of the kept records, packed in their order
    const size_t nk = j->src.size();
    std::vector<uint64_t> koff(nk);
    std::vector<uint32_t> klen(nk);
    std::string kid;
    for (size_t k = 0; k < nk; k++) {
        const uint64_t a = id_off[j->src[k]], b = id_off[j->src[k] + 1];
        if (b < a || b - a > 0xFFFFFFFFull) return fail(FPM_EINVAL, name + ": bad ID offsets");
        koff[k] = kid.size();
        klen[k] = (uint32_t)(b - a);
        kid.append(ids + a, b - a);
    }
    // a call that sized a text is usually followed by one that fetches it with the same IDs:
    // their upload and the size pass are kept
    const bool same_ids = j->ids_up && kid == j->text_ids && klen == j->text_id_len;
    const int want = fact ? kSizedFact : kSizedText;
    if (!same_ids || j->sized != want) {
        j->sized = kSizedNone;
        if (!same_ids) {
            j->ids_up = false;
            HIP_TRY(j->mem.get_pooled(&j->d_ids, kid.size()));
            HIP_TRY(j->mem.get_pooled(&j->d_id_off, nk * 8));
            HIP_TRY(j->mem.get_pooled(&j->d_id_len, nk * 4));
            if (!kid.empty()) HIP_TRY(h2d_staged(ctx, j->d_ids, kid.data(), kid.size()));
            HIP_TRY(h2d_staged(ctx, j->d_id_off, koff.data(), nk * 8));
            HIP_TRY(h2d_staged(ctx, j->d_id_len, klen.data(), nk * 4));
            j->text_ids = kid;
            j->text_id_len = klen;
            j->ids_up = true;
        }
        if (!j->d_size) HIP_TRY(j->mem.get_pooled(&j->d_size, n * 4));
        HIP_TRY(hipMemsetAsync(j->d_totals + 1, 0, 8, st));
        {
            TimedLaunch tl(ctx, FPM_K_KFINGER_OUT, st);
            if (ext)
                HIP_TRY(launch_kf_ext_size(j->d_desc, j->n_desc, j->d_rec_len, j->d_piece_rec,
                                           (uint32_t)n, j->window, fact, j->d_n_vals, j->d_body,
                                           j->d_id_len, j->d_size, j->d_totals + 1, st));
            else
                HIP_TRY(launch_kf_text_size(j->d_desc, j->n_desc, j->d_body, j->d_id_len,
                                            j->d_size, j->d_totals + 1, st));
            tl.done();
        }
        unsigned long long t = 0;
        HIP_TRY(hipMemcpyAsync(&t, j->d_totals + 1, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        j->text_total = t;
        j->sized = want;
    }
    const uint64_t tot = j->text_total;
    *n_bytes = tot;
    if (tot > 0xFFFFFFFFull)
        return fail(FPM_EINVAL, name + ": 2^32 bytes of text or more in one job");
    if (!out) return FPM_OK;                              // sized by this call
    if (cap < tot) return fail(FPM_EINVAL, name + ": buffer too small");
    uint8_t *d_out = nullptr;
    HIP_TRY(j->mem.get_pooled(&d_out, tot));
    TimedLaunch tl(ctx, FPM_K_KFINGER_OUT, st);
    if (int rc = scan_sizes(j, st)) return rc;
    if (ext)
        HIP_TRY(launch_kf_ext_text(j->d_seq, j->d_rec_pos, j->d_rec_len, j->d_desc, j->n_desc,
                                   j->window, j->d_off, j->d_ids, j->d_id_off, j->d_id_len,
                                   j->d_piece_rec, (uint32_t)n, fact, d_out, j->fact, st));
    else
        HIP_TRY(launch_kf_text(j->d_seq, j->d_rec_pos, j->d_rec_len, j->d_desc, j->n_desc,
                               j->window, j->d_off, j->d_ids, j->d_id_off, j->d_id_len, d_out,
                               j->fact, st));
    tl.done();
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(d2h_staged(ctx, out, d_out, tot));
    return FPM_OK;
}

}  // namespace

extern "C" {

int fpm_kfinger_stage(fpm_ctx *ctx, const char *seq, const uint64_t *rec_off, uint32_t n_rec,
                      uint32_t window, uint64_t max_lines, fpm_kfinger **job, uint64_t *n_lines)
{
    if (!job || !n_lines) return fail(FPM_EINVAL, "kfinger_stage: null output");
    *job = nullptr;
    *n_lines = 0;
    if (int rc = set_device(ctx)) return rc;
    if (n_rec && (!seq || !rec_off)) return fail(FPM_EINVAL, "kfinger_stage: null argument");
    if (!window_ok(window)) return fail(FPM_EINVAL, "kfinger_stage: window out of range");
    JobPtr j = new_job(ctx);
    std::vector<uint64_t> pos(n_rec), len(n_rec);
    for (uint32_t r = 0; r < n_rec; r++) {
        if (rec_off[r + 1] < rec_off[r]) return fail(FPM_EINVAL, "kfinger_stage: record offsets descend");
        pos[r] = rec_off[r] - rec_off[0];
        len[r] = rec_off[r + 1] - rec_off[r];
    }
    const uint64_t bytes = n_rec ? rec_off[n_rec] - rec_off[0] : 0;
    HIP_TRY(j->mem.get(&j->d_seq, bytes));
    if (bytes) HIP_TRY(h2d_staged(ctx, j->d_seq, seq + rec_off[0], bytes));
    if (int rc = plan(j.get(), pos, len, nullptr, window, max_lines)) return rc;
    *n_lines = j->n_lines;
    *job = j.release();
    return FPM_OK;
}

int fpm_kfinger_stage_seq(fpm_ctx *ctx, fpm_seqtext *seq, const uint8_t *take, uint32_t window,
                          uint64_t max_lines, fpm_kfinger **job, uint64_t *n_lines)
{
    if (!job || !n_lines) return fail(FPM_EINVAL, "kfinger_stage_seq: null output");
    *job = nullptr;
    *n_lines = 0;
    if (int rc = set_device(ctx)) return rc;
    if (!seq) return fail(FPM_EINVAL, "kfinger_stage_seq: null argument");
    if (!window_ok(window)) return fail(FPM_EINVAL, "kfinger_stage_seq: window out of range");
    uint64_t n = 0;
    uint8_t *d_packed = nullptr;
    std::vector<uint64_t> pos, len;
    if (int rc = seqtext_records(ctx, seq, &n, &pos, &len, &d_packed)) return rc;
    JobPtr j = new_job(ctx);
    j->mem.adopt(j->d_seq = d_packed);   // the job owns the packed records now
    if (int rc = plan(j.get(), pos, len, take, window, max_lines)) return rc;
    *n_lines = j->n_lines;
    *job = j.release();
    return FPM_OK;
}

int fpm_kfinger_stage_split(fpm_ctx *ctx, const char *seq, const uint64_t *rec_off, uint32_t n_rec,
                            uint32_t split, fpm_kfinger **job, uint64_t *n_pieces)
{
    if (!job || !n_pieces) return fail(FPM_EINVAL, "kfinger_stage_split: null output");
    *job = nullptr;
    *n_pieces = 0;
    if (int rc = set_device(ctx)) return rc;
    if (n_rec && (!seq || !rec_off)) return fail(FPM_EINVAL, "kfinger_stage_split: null argument");
    if (!window_ok(split)) return fail(FPM_EINVAL, "kfinger_stage_split: split out of range");
    JobPtr j = new_job(ctx);
    std::vector<uint64_t> pos(n_rec), len(n_rec);
    for (uint32_t r = 0; r < n_rec; r++) {
        if (rec_off[r + 1] < rec_off[r])
            return fail(FPM_EINVAL, "kfinger_stage_split: record offsets descend");
        pos[r] = rec_off[r] - rec_off[0];
        len[r] = rec_off[r + 1] - rec_off[r];
    }
    const uint64_t bytes = n_rec ? rec_off[n_rec] - rec_off[0] : 0;
    HIP_TRY(j->mem.get(&j->d_seq, bytes));
    if (bytes) HIP_TRY(h2d_staged(ctx, j->d_seq, seq + rec_off[0], bytes));
    if (int rc = plan_split(j.get(), pos, len, nullptr, split)) return rc;
    *n_pieces = j->n_lines;
    *job = j.release();
    return FPM_OK;
}

int fpm_kfinger_stage_split_seq(fpm_ctx *ctx, fpm_seqtext *seq, const uint8_t *take,
                                uint32_t split, fpm_kfinger **job, uint64_t *n_pieces)
{
    if (!job || !n_pieces) return fail(FPM_EINVAL, "kfinger_stage_split_seq: null output");
    *job = nullptr;
    *n_pieces = 0;
    if (int rc = set_device(ctx)) return rc;
    if (!seq) return fail(FPM_EINVAL, "kfinger_stage_split_seq: null argument");
    if (!window_ok(split)) return fail(FPM_EINVAL, "kfinger_stage_split_seq: split out of range");
    uint64_t n = 0;
    uint8_t *d_packed = nullptr;
    std::vector<uint64_t> pos, len;
    if (int rc = seqtext_records(ctx, seq, &n, &pos, &len, &d_packed)) return rc;
    JobPtr j = new_job(ctx);
    j->mem.adopt(j->d_seq = d_packed);   // the job owns the packed records now
    if (int rc = plan_split(j.get(), pos, len, take, split)) return rc;
    *n_pieces = j->n_lines;
    *job = j.release();
    return FPM_OK;
}

int fpm_kfinger_set_factorization(fpm_kfinger *j, uint32_t kind, uint32_t threshold)
{
    static_assert(FPM_KF_CFL == kKfCfl && FPM_KF_ICFL == kKfIcfl && FPM_KF_CFL_ICFL == kKfCflIcfl,
                  "fpmash.h states the factorization kinds");
    if (!j) return fail(FPM_EINVAL, "kfinger_set_factorization: null job");
    if (j->ran) return fail(FPM_EINVAL, "kfinger_set_factorization: the job has run");
    if (kind != FPM_KF_CFL && kind != FPM_KF_ICFL && kind != FPM_KF_CFL_ICFL)
        return fail(FPM_EINVAL, "kfinger_set_factorization: unknown kind");
    if (kind == FPM_KF_CFL_ICFL && !window_ok(threshold))
        return fail(FPM_EINVAL, "kfinger_set_factorization: threshold out of range");
    j->fact.kind = kind;
    j->fact.threshold = kind == FPM_KF_CFL_ICFL ? threshold : 0;
    return FPM_OK;
}

int fpm_kfinger_set_comb(fpm_kfinger *j, uint32_t on)
{
    if (!j) return fail(FPM_EINVAL, "kfinger_set_comb: null job");
    if (j->ran) return fail(FPM_EINVAL, "kfinger_set_comb: the job has run");
    if (on > 1) return fail(FPM_EINVAL, "kfinger_set_comb: on is 0 or 1");
    j->fact.comb = on;
    return FPM_OK;
}

int fpm_kfinger_run(fpm_kfinger *j, uint32_t seed, uint32_t use64, void *stream)
{
    if (!j) return fail(FPM_EINVAL, "kfinger_run: null job");
    fpm_ctx *ctx = j->ctx;
    if (int rc = set_device(ctx)) return rc;
    if (int rc = wide_work(j)) return rc;
    hipStream_t st = pick_stream(ctx, stream);
    j->stream = st;
    j->use64 = use64 ? 1 : 0;
    HIP_TRY(hipMemsetAsync(j->d_totals, 0, 16, st));
    TimedLaunch tl(ctx, FPM_K_KFINGER, st);
    HIP_TRY(launch_kf_hash(j->d_seq, j->d_rec_pos, j->d_rec_len, j->d_desc, j->n_desc, j->window,
                           seed, j->use64, j->d_hash, j->d_n_vals, j->d_body, j->d_totals, j->fact,
                           st));
    tl.done();
    j->ran = true;
    return FPM_OK;
}

int fpm_kfinger_fetch(fpm_kfinger *j, uint64_t *rec_first_line, void *hash, uint32_t *n_vals)
{
    if (!j) return fail(FPM_EINVAL, "kfinger_fetch: null job");
    fpm_ctx *ctx = j->ctx;
    if (int rc = set_device(ctx)) return rc;
    if (rec_first_line)
        memcpy(rec_first_line, j->rec_first_line.data(), j->rec_first_line.size() * 8);
    if (!hash && !n_vals) return FPM_OK;
    if (!j->ran) return fail(FPM_EINVAL, "kfinger_fetch: the job has not run");
    HIP_TRY(hipStreamSynchronize(j->stream));
    const uint64_t n = j->n_lines;
    if (n && hash) HIP_TRY(copy_out(ctx, hash, j->d_hash, n * (j->use64 ? 8 : 4)));
    if (n && n_vals) HIP_TRY(copy_out(ctx, n_vals, j->d_n_vals, n * 4));
    return FPM_OK;
}

int fpm_kfinger_device_output(fpm_kfinger *j, void **d_hash, uint32_t **d_n_vals,
                              uint64_t *n_lines, uint32_t *hash_bytes)
{
    if (!j) return fail(FPM_EINVAL, "kfinger_device_output: null job");
    if (!j->ran) return fail(FPM_EINVAL, "kfinger_device_output: the job has not run");
    if (d_hash) *d_hash = j->d_hash;
    if (d_n_vals) *d_n_vals = j->d_n_vals;
    if (n_lines) *n_lines = j->n_lines;
    if (hash_bytes) *hash_bytes = j->use64 ? 8 : 4;
    return FPM_OK;
}

int fpm_kfinger_values(fpm_kfinger *j, uint64_t *val_off, uint16_t *vals, uint64_t cap,
                       uint64_t *total)
{
    if (!j || !total) return fail(FPM_EINVAL, "kfinger_values: null argument");
    fpm_ctx *ctx = j->ctx;
    if (int rc = set_device(ctx)) return rc;
    if (!j->ran) return fail(FPM_EINVAL, "kfinger_values: the job has not run");
    hipStream_t st = j->stream;
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, j->d_totals, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *total = tot;
    if (tot > 0xFFFFFFFFull) return fail(FPM_EINVAL, "kfinger_values: 2^32 values or more in one job");
    if (!vals) return FPM_OK;                             // sized by this call
    if (cap < tot) return fail(FPM_EINVAL, "kfinger_values: buffer too small");
    const uint64_t n = j->n_lines;
    if (!n) {
        if (val_off) val_off[0] = 0;
        return FPM_OK;
    }
    uint16_t *d_vals = nullptr;
    HIP_TRY(j->mem.get_pooled(&d_vals, tot * 2));
    {
        TimedLaunch tl(ctx, FPM_K_KFINGER_OUT, st);
        // the sizes are the value counts themselves
        uint32_t *keep = j->d_size;
        j->d_size = j->d_n_vals;
        const int rc = scan_sizes(j, st);
        j->d_size = keep;
        if (rc) return rc;
        HIP_TRY(launch_kf_values(j->d_seq, j->d_rec_pos, j->d_rec_len, j->d_desc, j->n_desc,
                                 j->window, j->d_off, d_vals, j->fact, st));
        tl.done();
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (val_off) {
        std::vector<uint32_t> off(n);
        HIP_TRY(copy_out(ctx, off.data(), j->d_off, n * 4));
        for (uint64_t i = 0; i < n; i++) val_off[i] = off[i];
        val_off[n] = tot;
    }
    if (tot) HIP_TRY(d2h_staged(ctx, vals, d_vals, tot * 2));
    return FPM_OK;
}

int fpm_kfinger_text(fpm_kfinger *j, const char *ids, const uint64_t *id_off, char *out,
                     uint64_t cap, uint64_t *n_bytes)
{
    return text_out(j, ids, id_off, out, cap, n_bytes, false, "kfinger_text");
}

int fpm_kfinger_fact_text(fpm_kfinger *j, const char *ids, const uint64_t *id_off, char *out,
                          uint64_t cap, uint64_t *n_bytes)
{
    return text_out(j, ids, id_off, out, cap, n_bytes, true, "kfinger_fact_text");
}

void fpm_kfinger_free(fpm_kfinger *j)
{
    kfinger_release(j);
    delete j;
}

int fpm_kfinger_wide_groups(fpm_kfinger *j, uint32_t *groups)
{
    if (!j || !groups) return fail(FPM_EINVAL, "kfinger_wide_groups: null argument");
    *groups = j->ran ? j->fact.work_groups : 0;
    return FPM_OK;
}

void fpm_kfinger_limits(uint32_t *max_window, uint32_t *run_length)
{
    if (max_window) *max_window = kKfMaxWindow;
    if (run_length) *run_length = kKfRun;
}

int fpm_kfinger_lds_window(uint32_t kind, uint32_t comb, uint32_t *window)
{
    if (!window) return fail(FPM_EINVAL, "kfinger_lds_window: null output");
    if ((kind != FPM_KF_CFL && kind != FPM_KF_ICFL && kind != FPM_KF_CFL_ICFL) || comb > 1)
        return fail(FPM_EINVAL, "kfinger_lds_window: unknown factorization");
    *window = kf_lds_window(kind, comb);
    return FPM_OK;
}

}  // extern "C"
