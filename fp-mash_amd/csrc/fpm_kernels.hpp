// fpm_kernels.hpp — launch interface between the C-ABI (fpm_*_api.cpp) and the
// gfx950 kernels (sketch.hip, dist.hip, dist_index.hip, fingerprint.hip, seqparse.hip,
// contain.hip, screen.hip, taxscreen.hip, kfinger.hip).  Host-only types.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fpm {

// One tile = a contiguous byte range of the packed, separator-delimited sequence
// buffer, all of it from one sketch group.  Every k-mer start of the tile lies
// in [byte_off, byte_off + n_bytes - k]; windows that cross a 0x00 separator are
// invalid by construction (0x00 is never in an alphabet).
struct TileDesc {
    uint64_t byte_off;
    uint32_t n_bytes;
    uint32_t out_row;   // row of the output (or temp) matrix this tile writes
    uint32_t thr_slot;  // 0: keep every hash; i > 0: keep hashes <= thr[i - 1] (long groups)
    uint32_t pad;       // the tile's group (read by the -M multiplicity pass only)
};

struct SketchKParams {
    uint32_t k;
    uint32_t s;             // sketch size (row stride of the output matrix)
    uint32_t seed;
    uint32_t use64;
    uint32_t canonical;
    uint32_t preserve_case;
    uint32_t compl_acgt;    // every alphabet byte is one of A C G T: complement by bit ops
    uint8_t alphabet[256];  // 1 = valid (after uppercasing)
    uint8_t complement[256];
};

// Pairwise merge of two ascending distinct lists into the first s distinct of
// their union (bottom-s of a union = bottom-s of the union of bottom-s sets).
struct MergeDesc {
    const uint64_t *a; const uint32_t *alen;
    const uint64_t *b; const uint32_t *blen;   // b == nullptr: copy a
    uint64_t *c; uint32_t *clen;
};

// numer / denom output cells of the dist grid: u32, or u16 (c16) when the sketch size fits
// (fpm_dist_dev16: counts <= s <= 65535, 4 bytes per pair instead of 8)
struct Counts {
    void *numer = nullptr, *denom = nullptr;
    bool c16 = false;
};

// A set of sketch rows on the device: n rows of `stride` hashes, each row's entry count and
// (for the distances) each sequence's length, null where a launcher has no use for it.  The two
// sides of a launch are two of these, ref first: a swap (the transposed fill) shows as one.
struct RowSet {
    const void *rows = nullptr;
    const uint32_t *len = nullptr;
    const uint64_t *length = nullptr;
    uint64_t stride = 0;
    uint32_t n = 0;
};

// what turns a pair's counts into a distance, a p-value and a pass flag (max_dist / max_pvalue
// < 0: no -d / -v filter)
struct DistParams {
    uint32_t kmer_size = 0;
    double kmer_space = 0, max_dist = -1, max_pvalue = -1;
};

// the full per-cell outputs of a grid beside its counts (pass may be null)
struct CellOut {
    double *dist = nullptr, *pval = nullptr;
    uint8_t *pass = nullptr;
};

// The probe's candidate cells (cell index q * n_ref + r): cand[0 .. *n), at most cap.  cnum /
// cden non-null: the rank kernel's (numer, denom) of candidate c go to slot c instead of the grid
// cells, and the candidate finalize / list scatters them; null: the counts are in the grid.
struct CandList {
    uint64_t *cand = nullptr;
    unsigned long long *n = nullptr;
    uint64_t cap = 0;
    uint32_t *cnum = nullptr, *cden = nullptr;
};

// Tile capacity classes (k-mer starts per tile).
constexpr int kTileClasses = 6;
constexpr uint32_t kTileCap[kTileClasses] = {256, 512, 1024, 2048, 4096, 8192};

// class-4 (4096-window) tiles that all carry a bound (thr_slot != 0): survivors only; tiles
// with more than the kernel holds are appended to d_redo (count *d_redo_n, zeroed by the
// caller) for launch_sketch_tiles
hipError_t launch_sketch_tiles_thr(const uint8_t *d_seq, const TileDesc *d_tiles, uint32_t n_tiles,
                                   const SketchKParams &p, const uint64_t *d_thr, uint64_t *d_out,
                                   uint32_t *d_count, TileDesc *d_redo, uint32_t *d_redo_n,
                                   hipStream_t st);
// the tiles a launch_sketch_tiles_thr pass listed (d_redo[0 .. *d_redo_n), at most max_tiles),
// through the plain P = 4096 kernel, the count read on the device
hipError_t launch_sketch_redo(const uint8_t *d_seq, const TileDesc *d_redo, const uint32_t *d_redo_n,
                              uint32_t max_tiles, const SketchKParams &p, const uint64_t *d_thr,
                              uint64_t *d_out, uint32_t *d_count, hipStream_t st);
// survivors one THR tile holds (kBlock * kSurv + kSurvShared, sketch.hip)
constexpr uint32_t kThrTileKeys = 1024;
hipError_t launch_sketch_tiles(int cls, const uint8_t *d_seq, const TileDesc *d_tiles,
                               uint32_t n_tiles, const SketchKParams &p, const uint64_t *d_thr,
                               uint64_t *d_out, uint32_t *d_count, hipStream_t st);
// -M: pass 0 counts / first positions of the final hashes, pass 1 the final maximum up to T_top
hipError_t launch_sketch_mult(int cls, int pass, const uint8_t *d_seq, const TileDesc *d_tiles,
                              uint32_t n_tiles, const SketchKParams &p, const uint64_t *d_rows,
                              const uint32_t *d_count, uint32_t *d_mult,
                              unsigned long long *d_first, const uint64_t *d_ttop, hipStream_t st);
hipError_t launch_mult_ttop(const uint32_t *d_count, uint32_t n_groups, uint32_t s,
                            const unsigned long long *d_first, uint64_t *d_ttop, hipStream_t st);
// reads mode (min-copies m): counts and the m smallest positions (d_slots: m u64 per entry,
// all-ones before) of the entries of the wide rows d_rows (stride p.s); then per group not
// yet done the first s entries with count >= m into the output row (d_done[g] = round when
// that is final); then the count of a full sketch's maximum up to T (d_ttop)
hipError_t launch_reads_count(int cls, const uint8_t *d_seq, const TileDesc *d_tiles,
                              uint32_t n_tiles, const SketchKParams &p, const uint64_t *d_rows,
                              const uint32_t *d_count, uint32_t m, uint32_t *d_wcnt,
                              unsigned long long *d_slots, hipStream_t st);
hipError_t launch_reads_filter(const uint64_t *d_rows, const uint32_t *d_count, uint32_t wide,
                               uint32_t n_groups, const uint32_t *d_wcnt,
                               const unsigned long long *d_slots, uint32_t m, uint32_t s,
                               uint32_t round, uint32_t *d_done, uint64_t *d_out_rows,
                               uint32_t *d_out_count, uint32_t *d_out_mult, uint64_t *d_ttop,
                               hipStream_t st);
hipError_t launch_reads_maxcount(int cls, const uint8_t *d_seq, const TileDesc *d_tiles,
                                 uint32_t n_tiles, const SketchKParams &p, uint32_t s,
                                 uint32_t round, const uint32_t *d_done, const uint64_t *d_out_rows,
                                 const uint32_t *d_out_count, uint32_t *d_out_mult,
                                 const uint64_t *d_ttop, hipStream_t st);
// thr_safe[i] = s-th smallest of sample row srow[i] when it holds s hashes, else no bound;
// thr[i] = its kt[i]-th smallest (d_kt null: thr = thr_safe)
hipError_t launch_sketch_threshold(const uint32_t *d_srow, uint32_t n_slots, const uint64_t *d_rows,
                                   const uint32_t *d_count, uint32_t s, const uint32_t *d_kt,
                                   uint64_t *d_thr, uint64_t *d_thr_safe, hipStream_t st);
// slots whose group (slot_group[i]) ended with fewer than s hashes under thr < thr_safe:
// listed (d_short_slots, count *d_n_short, zeroed by the caller), with `raise` thr raised to
// thr_safe
// samples (sample row srow[i]) left with fewer than s hashes under their a-priori bound
// d_sbound[i] (< ~0): listed (count *d_n_short, zeroed by the caller), with `raise` the bound
// lifted to ~0
hipError_t launch_sketch_sample_short(const uint32_t *d_srow, uint32_t n_slots,
                                      const uint32_t *d_count, uint32_t s, uint64_t *d_sbound,
                                      uint32_t *d_n_short, uint32_t *d_short_slots, bool raise,
                                      hipStream_t st);
hipError_t launch_sketch_short(const uint32_t *d_slot_group, uint32_t n_slots,
                               const uint32_t *d_count, uint32_t s, uint64_t *d_thr,
                               const uint64_t *d_thr_safe, uint32_t *d_n_short,
                               uint32_t *d_short_slots, bool raise, hipStream_t st);
// list length merge_small_kernel stages in LDS (kSCap, sketch.hip)
constexpr uint32_t kMergeSmallCap = 2048;
// one long group's sketch selected from its bounded tile lists (rows row_ids[row_begin ..
// row_begin + n_rows)) into out_row; slot: its bound thr[slot] (0xFFFFFFFF: none, the
// sample pass of long groups)
struct SelDesc { uint32_t row_begin, n_rows, out_row, slot; };
// keys one selection stages in LDS (kSelCap, sketch.hip; sketch sizes up to ~0.85 x)
constexpr uint32_t kGroupSelectCap = 15360;
// *failed |= 1 when a group's keys below the cut do not fit (the caller merges instead)
hipError_t launch_group_select(const SelDesc *d_desc, uint32_t n, const uint32_t *d_row_ids,
                               uint64_t *d_rows, uint32_t *d_count, uint32_t s,
                               const uint64_t *d_thr, uint32_t *d_failed, hipStream_t st);
// small: the round's lists are estimated short (merge_small_kernel; exact for any length)
// merge_small_kernel launches whose lists overflowed its LDS cap since the last call (reset)
hipError_t merge_small_spills(uint64_t *count);
// sketch sizes up to which the other rounds stage a list in LDS (128 KiB; merge_lds_kernel),
// beyond it they search in global memory (merge_kernel)
constexpr uint32_t kMergeLdsKeys = 16384;
hipError_t launch_merge(const MergeDesc *d_desc, uint32_t n, uint32_t s, bool small,
                        hipStream_t st);

hipError_t launch_fp_hash(const uint64_t *d_vals, const uint64_t *d_line_off, uint64_t n_lines,
                          uint32_t seed, uint32_t use64, void *d_out, hipStream_t st);

// (*lds, may be null: whether the LDS-staged walk was launched, else the walk from global memory)
hipError_t launch_compare_grid(const RowSet &ref, const RowSet &qry, uint32_t hash_bytes,
                               uint32_t sketch_size, Counts cnt, bool *lds, hipStream_t st);

// dense walk of u32 lists on 16-bit rank images (dist.hip), for 64 <= min(S, stride) <= 1023;
// scratch from compare_grid_img_scratch
bool compare_grid_img_ok(uint32_t hash_bytes, uint32_t sketch_size, uint64_t ref_stride,
                         uint64_t qry_stride);
void compare_grid_img_scratch(uint32_t n_qry, uint32_t sketch_size, uint64_t ref_stride,
                              uint64_t qry_stride, size_t *ublk_bytes, size_t *bimg_bytes);
hipError_t launch_compare_grid_img(const RowSet &ref, const RowSet &qry, uint32_t sketch_size,
                                   void *ublk, void *bimg, Counts cnt, hipStream_t st);
// the record rows of one side of a candidate walk (launch_record_rows): values, positions,
// counts, row stride; val == nullptr: none (the walk starts at (0, 0))
struct RecRows {
    const void *val = nullptr;
    const uint32_t *pos = nullptr, *len = nullptr;
    uint64_t stride = 0;
};
// the literal walk of each candidate pair; with record rows of both sides (unsorted lists),
// only the stretches where both running maxima equal a shared record are walked
hipError_t launch_walk_candidates(const CandList &cl, const RowSet &ref, const RowSet &qry,
                                  uint32_t hash_bytes, uint32_t S, Counts cnt, RecRows rec_ref,
                                  RecRows rec_qry, hipStream_t st);

// bucket index over ref hashes (dist_index.hip)
constexpr uint32_t kIdxL1 = 10;        // level-1 partition bits
constexpr uint32_t kIdxTile = 16384;   // the most matrix cells per level-1 tile (~16 entries per partition)
struct IdxGeom {
    uint32_t l2;       // level-2 bits (1..14)
    uint32_t nbits;    // bucket bits = kIdxL1 + l2
    uint32_t rbits;    // ref-id bits in a u32 entry
    uint32_t fbits;    // key-fingerprint bits in a u32 entry (31 - rbits, >= 7); bit 31: the flag
    uint32_t ntiles;   // level-1 tiles
    uint32_t tile;     // matrix cells per level-1 tile (<= kIdxTile, a multiple of 1024)
    // device pointer: the largest indexed key (idx_kmax_kernel), from which every kernel
    // derives the bucket scale (bucket_of / key_fp in dist_index.hip)
    const unsigned long long *kmax;
    // level-1 partition capacity of the one-pass scatter (tent holds kParts x cap entries,
    // each tile appends to its partitions by one atomic per partition); 0 = the exact
    // two-pass build (histogram + scan, tent holds E entries)
    uint32_t cap;
    // the sketch size S of the half probe's cut: an entry's flag (bit 31) says that its
    // position is inside its own row's visited prefix, pos < (len >= S ? (S + 1) / 2 : len);
    // 0 = no cut, every entry flagged (record-row indexes)
    uint32_t cut;
    // value cut (needs cut != 0; an index probed by the half form only): *kmax is V*, the
    // largest value any row's visited prefix holds, max over rows of row[H_r - 1], and cells
    // whose key exceeds it are left out of the index (no probed hash can equal them).  0 = every
    // entry indexed, *kmax from the rows' last entries
    uint32_t vcut;
};
// entries of the level-1 staging buffer `tent` the build needs
uint64_t idx_tent_words(const IdxGeom &g, uint64_t E);
struct IdxBuild {
    RowSet rows;                  // the rows indexed
    uint32_t hash_bytes = 8;
    IdxGeom g{};
    // scratch: 2^kIdxL1 x g.ntiles u32, one more, scan_scratch_words of that, idx_tent_words u64
    uint32_t *tile_hist = nullptr, *tile_off = nullptr, *scan_s = nullptr;
    uint64_t *tent = nullptr;
    // the index: 2^g.nbits + 1 directory words and one u32 entry per cell of the rows
    uint32_t *dir = nullptr, *entries = nullptr;
    uint32_t *unsorted = nullptr;               // set to 1 when some row is not strictly increasing
    unsigned long long *self_events = nullptr;  // null, or += sum_b |b|^2 over the buckets
    // zero[0..nzero) (and *zero_x when given) is cleared first
    unsigned long long *zero = nullptr, *zero_x = nullptr;
    uint32_t nzero = 0;
    unsigned long long *acc = nullptr;   // acc[0..2]: three words that start and are left at zero
    // One-pass build (g.cap != 0): part_fill holds 2^kIdxL1 u32 (cleared by the build), *overflow
    // (inside zero[]) is set when a partition exceeded cap: the index is then unusable and the
    // caller rebuilds with g.cap = 0
    uint32_t *part_fill = nullptr, *overflow = nullptr;
    // may be null, may lie inside zero[]: [0] = the entries indexed (fewer than the rows hold
    // with g.vcut), [1] = the entries the rows hold (sum of the lengths)
    unsigned long long *n_entries = nullptr;
};
hipError_t launch_idx_build(const IdxBuild &a, hipStream_t st);

// launch_exscan's shapes: blocks of kScanBlock elements; up to kScanFoldBlocks of them the block
// totals are folded inside the add kernel (two launches), past that a single workgroup scans
// them between the two (three launches)
constexpr int kScanBlock = 1024;            // elements per block (256 threads x 4)
constexpr uint32_t kScanFoldBlocks = 4096;
uint64_t scan_scratch_words(uint64_t n);
// copy n (<= kPubWords - 1) u64 counters into host-mapped memory, then write `seq` into its
// last word (system-scope fence between): the host spins on that word
constexpr uint32_t kPubWords = 128;
hipError_t launch_publish(const unsigned long long *d_src, uint32_t n, unsigned long long *h_dst,
                          unsigned long long seq, hipStream_t st);
// each row's records among its first min(len, S, out_stride) entries (the strict increases of
// its running maximum: sorted and distinct; dist_index.hip), the index / probe input for
// unsorted lists: only pairs sharing a record value can count anything in the literal walk
// (pos_out, may be null: each record's position in its row, at the same offsets; unsorted,
// may be null: set to 1 when some row is not strictly increasing, the index build's test)
hipError_t launch_record_rows(const RowSet &in, uint32_t hash_bytes, uint32_t S, void *out,
                              uint32_t *pos_out, uint32_t *out_len, uint64_t out_stride,
                              uint32_t *unsorted, hipStream_t st);
hipError_t launch_exscan(const uint32_t *in, uint32_t *out, uint32_t *out2, uint64_t n,
                         uint32_t *scratch, uint32_t *total, hipStream_t st);
hipError_t launch_probe_count(const RowSet &qry, uint32_t hash_bytes, IdxGeom g,
                              const uint32_t *dir, unsigned long long *events, uint32_t *unsorted,
                              hipStream_t st);
// The final values of a pair that shares no hash: (0, min(S, la+lb)), distance 1 (0 when
// both lists are empty, numer == denom), p-value 1 and the -d / -v filters
// (CommandDistance.cpp:404-419 at numer = 0).  launch_dist_fill writes them to every cell
// of the grid; the candidate cells are then rewritten by the candidate compare and
// launch_dist_cand_finalize.
struct PairFill {
    CellOut out;
    double max_dist = -1, max_pvalue = -1;
};
// flat: the fill over the flattened grid (line-aligned wave stores, ~6.5 TB/s alone), else
// row-aligned workgroups (~4.8 TB/s alone, gentler on a latency-bound kernel beside it).
// fill.out.dist == nullptr: the numer / denom defaults only (the compact output)
hipError_t launch_dist_fill(const RowSet &ref, const RowSet &qry, uint32_t S, Counts cnt,
                            const PairFill &fill, bool flat, hipStream_t st);
// A compact grid's counts written ahead of its dist call (fpm_dist_list_prefill): (0, S) in
// every cell; then, once the lists are known, denom = la + lb where la + lb < S
hipError_t launch_dist_counts_const(uint16_t *numer, uint16_t *denom, uint64_t cells, uint32_t S,
                                    hipStream_t st);
hipError_t launch_dist_counts_fixup(const RowSet &ref, const RowSet &qry, uint32_t S,
                                    uint16_t *denom, hipStream_t st);
// The compacted candidate rows of one sorted u64 set against itself: the half probe
// writes them, the rank kernel streams them in place of the ref rows.  Row r's block of
// cmp_row_bytes(stride) bytes starts at rows + r * that: first its kept values (u64, ascending:
// the values of its probed prefix that another row holds too, then its whole tail), and at byte
// stride * 8 their positions in the original row, u16, interleaved by rank-kernel chunk (entry d
// at u16 index (d / 128) * 128 + (d % 64) * 2 + (d / 64) % 2: one dword holds the positions of
// a lane's two values of a chunk).  len[r] = the kept entries, len[n + r] = the row's own length.
struct CmpRows {
    void *rows = nullptr;
    uint32_t *len = nullptr;
};
constexpr uint64_t cmp_row_bytes(uint64_t stride) { return stride * 8 + (stride + 127) / 128 * 256; }
constexpr uint32_t kCmpMaxRow = 2048;   // the longest row the probe's kept bits cover

struct ProbeRows {
    // the query rows [q_lo, q_lo + qry.n) of the grid; qry.len stays the original list lengths
    // (the default cells) when the probed rows are record copies
    RowSet qry;
    uint32_t q_lo = 0;
    RowSet ref;                   // the indexed set: its lengths and n (the rows are not read)
    uint32_t hash_bytes = 8, S = 0;
    IdxGeom g{};
    const uint32_t *dir = nullptr, *entries = nullptr;
    bool sym = false;
    // also write (0, min(S, la+lb)) to every numer / denom cell of the row (off when
    // launch_dist_fill already did)
    bool defaults = false;
    // the query set is the indexed ref set, same buffers: buckets of one entry are the row's
    // own hash and are not read
    bool self_set = false;
    // the symmetric probe of one sorted set against itself over an index cut at this S (g.cut
    // == S): each row probes only its visited prefix and a pair is taken by its parity owner
    // when that row sees it, else by the other row; dist_index.hip step 2.  Needs sym and
    // self_set, and none of qry_it_len / q_unsorted / events: hipErrorInvalidValue otherwise
    bool half = false;
    Counts cnt;
    CandList out;                 // cand, n and cap (the slots are the rank kernel's)
    uint64_t *row_seg = nullptr;
    // non-null: the probed query rows are launch_record_rows copies of length qry_it_len[q]
    const uint32_t *qry_it_len = nullptr;
    uint32_t *q_unsorted = nullptr;
    unsigned long long *events = nullptr;
    uint32_t *cand_over = nullptr;
    // rows non-null: the half probe also writes each row's compacted copy.  Needs the half
    // form, u64 rows of stride <= kCmpMaxRow and every ref in one workgroup (n_ref <= 2^19):
    // hipErrorInvalidValue otherwise
    CmpRows cmp;
};
hipError_t launch_probe_rows(const ProbeRows &a, hipStream_t st);
// sorted-distinct candidates: one workgroup per query row, one wave per pair
// (cmp.rows non-null: one set against itself (sym, same ref and query rows) whose probe wrote the
// compacted rows: the candidates are streamed from those, the diagonal answered in closed form)
// (cl.cnum, cl.cden non-null: results go to candidate slot c instead of the grid cells;
// every query row's probe has run; *rank_cap, may be null: the CAP of the rank_rows_kernel
// instance launched, 1024 or 2048)
hipError_t launch_merge_rows(const CandList &cl, const uint64_t *row_seg, const RowSet &ref,
                             const RowSet &qry, uint32_t S, bool sym, Counts cnt, CmpRows cmp,
                             uint32_t *rank_cap, hipStream_t st);

// -fp CFL text: newline index, then one lane per line (fingerprint.hip)
uint32_t text_blocks(uint64_t len);
uint32_t fp_text_chunk();   // text bytes per newline-index workgroup
uint32_t fp_span_bytes();   // largest wave span fp_line_kernel stages in LDS
uint32_t fp_head_lines();   // lines per head-count workgroup
hipError_t launch_fp_nl_count(const uint8_t *d_text, uint64_t len, uint32_t *blk_cnt,
                              uint32_t *blk_off, uint32_t *scan_s, hipStream_t st);
hipError_t launch_fp_nl_scatter(const uint8_t *d_text, uint64_t len, const uint32_t *blk_off,
                                uint64_t *d_line_start, hipStream_t st);
// the References of a parsed -fp file (heads: line 0 and new_id == 1): per-block head counts +
// their exclusive scan (blk_off[nb] = the total), then the ordered heads, each Reference's
// length (the first line's count twice, Sketch.cpp:117, 134) and its ID bounds
uint32_t fp_head_blocks(uint64_t n_lines);
hipError_t launch_fp_heads(const uint8_t *d_new_id, uint64_t n_lines, uint32_t *blk_cnt,
                           uint32_t *blk_off, uint32_t *scan_s, hipStream_t st);
hipError_t launch_fp_refs(const uint8_t *d_new_id, uint64_t n_lines, const uint32_t *blk_off,
                          uint64_t n_refs, const uint32_t *d_n_vals, const uint64_t *d_id_off,
                          const uint32_t *d_id_len, uint64_t *d_first, uint64_t *d_length,
                          uint64_t *d_ref_id_off, uint32_t *d_ref_id_len, hipStream_t st);
hipError_t launch_fp_lines(const uint8_t *d_text, uint64_t len, const uint64_t *d_line_start,
                           uint64_t n_nl, uint64_t n_lines, uint32_t seed, uint32_t use64,
                           uint64_t *id_off, uint32_t *id_len, uint32_t *n_vals, void *hash,
                           uint8_t *new_id, hipStream_t st);

// FASTA text -> packed records (seqparse.hip).  The text buffer holds each file from a
// kSpChunk-aligned offset, '\n' bytes after it; reset[c] = 1 on a file's first chunk.
constexpr uint32_t kSpChunk = 4096;
size_t seq_xf_bytes();    // per-chunk summary
size_t seq_cin_bytes();   // per-chunk input state / counts
// summaries + chunk scan; d_totals = {records, sequence bytes, '+' in sequence text}
hipError_t launch_seq_scan(const uint8_t *d_text, const uint8_t *d_reset, uint32_t n_chunks,
                           void *d_xf, void *d_cin, uint64_t *d_totals, hipStream_t st);
// record table (header '>' position, header '\n' position, packed offset, length) and the
// packed records (sequence bytes + 0x00 each) in d_out
hipError_t launch_seq_emit(const uint8_t *d_text, uint32_t n_chunks, const void *d_cin,
                           uint64_t n_rec, uint64_t total_kept, uint64_t *d_hdr_pos,
                           uint64_t *d_hdr_end, uint64_t *d_kept_at, uint64_t *d_seq_off,
                           uint64_t *d_seq_len, uint8_t *d_out, hipStream_t st);

// FASTQ, 4-line records verified against kseq_read's quality rules (seqparse.hip).
// d_seg = (offset, length) per file in the text; d_file_lines = (first line, lines) per file
hipError_t launch_fq_files(const uint64_t *d_line_start, uint64_t n_starts, const uint64_t *d_seg,
                           uint32_t n_seg, uint64_t *d_file_lines, hipStream_t st);
// record table in d_rec (hdr_pos | hdr_end | kept_at | seq_off | seq_len), *d_fail != 0 when a
// record does not read the 4-line way; d_scan holds (n_rec + 1023) / 1024 u64, *d_total = bases
hipError_t launch_fq_records(const uint8_t *d_text, const uint64_t *d_line_start,
                             const uint64_t *d_seg, const uint64_t *d_file_lines,
                             const uint64_t *d_rec_base, uint32_t n_seg, uint64_t n_rec,
                             uint64_t *d_rec, uint64_t *d_scan, uint64_t *d_total, uint32_t *d_fail,
                             uint8_t *d_out, hipStream_t st);
hipError_t launch_fq_emit(const uint8_t *d_text, uint64_t n_rec, uint64_t *d_rec, uint8_t *d_out,
                          hipStream_t st);

// triangle -fp positional compare (dist.hip)
hipError_t launch_positional_grid(const RowSet &ref, const RowSet &qry, uint32_t hash_bytes,
                                  double max_dist, double max_pvalue, uint32_t *d_numer,
                                  uint32_t *d_denom, const CellOut &out, hipStream_t st);

// contain (contain.hip): per pair the (common, steps) of containSketches
// (CommandContain.cpp:368-412), query-major cells q * n_ref + r.
// flag[0..1] (zeroed by the caller): flag[0] = 1 when some row of either set is not strictly
// ascending within its length (plain stores), flag[1] = the longest query row (atomic max);
// the caller reads them back (one stream synchronisation)
hipError_t launch_rows_ascending(const RowSet &ref, const RowSet &qry, uint32_t hash_bytes,
                                 uint32_t *flag, hipStream_t st);
// the longest query row contain_rows_kernel stages in LDS on the current device (the dynamic
// LDS limit is raised above 64 KB when the device grants it)
uint32_t contain_lds_cap(uint32_t hash_bytes);
// closed form, for strictly ascending rows only; max_qry_len = the longest query row, which
// picks the LDS-staged or the global-memory instance (*lds)
hipError_t launch_contain_rows(const RowSet &ref, const RowSet &qry, uint32_t hash_bytes,
                               uint32_t max_qry_len, uint32_t *d_common, uint32_t *d_steps,
                               bool *lds, hipStream_t st);
// the literal walk, one lane per pair: exact for any lists
hipError_t launch_contain_literal(const RowSet &ref, const RowSet &qry, uint32_t hash_bytes,
                                  uint32_t *d_common, uint32_t *d_steps, hipStream_t st);

// screen (screen.hip, screen_table.hpp; the pool pass in sketch.hip; the p-values in dist.hip)
struct ScreenTable;
// longest reference row (cells) screen_rows_kernel holds in LDS (48 KB of u32 counters)
constexpr uint32_t kScreenRowsLdsCap = 12288;
// table build, part 1: every cell of the database (rows strictly ascending, E cells in all,
// cell index row * stride + i < 2^32) sorted by key into okey / ocell (E entries each; skey /
// scell: E entries of staging).  kmax: one u64; hist, start: 2^sbits u32; scan_s:
// scan_scratch_words(max(2^sbits, E)) u32
hipError_t launch_screen_sort(const void *d_db, const uint32_t *d_len, uint64_t stride,
                              uint32_t n_db, uint32_t hash_bytes, uint32_t E, uint32_t sbits,
                              unsigned long long *kmax, uint32_t *hist, uint32_t *start,
                              uint32_t *scan_s, uint64_t *skey, uint32_t *scell, uint64_t *okey,
                              uint32_t *ocell, hipStream_t st);
// part 2: head[p] = 1 where sorted key p starts a run of equal keys, hx = its exclusive scan,
// *n_distinct (device) = |U|; the caller reads it and kmax back to size part 3
hipError_t launch_screen_heads(const uint64_t *okey, uint32_t E, uint32_t *head, uint32_t *hx,
                               uint32_t *scan_s, uint32_t *n_distinct, hipStream_t st);
// part 3: U (n entries), ustart (n + 1: the sorted cells [ustart[u], ustart[u + 1]) hold U[u]),
// slot (per database cell, the layout of the rows: its entry of U), post (per sorted cell: its
// row) and the directory (2^dbits + 1 entries, shift = clz of the largest key)
hipError_t launch_screen_compact(const uint64_t *okey, const uint32_t *ocell, const uint32_t *head,
                                 const uint32_t *hx, uint32_t E, uint64_t stride, uint32_t n,
                                 uint32_t dbits, uint32_t shift, uint64_t *U, uint32_t *ustart,
                                 uint32_t *slot, uint32_t *post, uint32_t *dir, hipStream_t st);
// pool pass: every valid window of the tiles adds 1 to the counter of its key's entry of U
// (hashSequence, CommandScreen.cpp:280-384); sketch.hip
hipError_t launch_screen_count(int cls, const uint8_t *d_seq, const TileDesc *d_tiles,
                               uint32_t n_tiles, const SketchKParams &p, const ScreenTable &t,
                               hipStream_t st);
// the same for a plain device array of n keys (no hashing)
hipError_t launch_screen_hashes(const uint64_t *d_keys, uint64_t n, const ScreenTable &t,
                                hipStream_t st);
// per reference: shared and median (d_owner null: every cell; else the cells whose entry the
// row owns); *lds: the LDS-held instance ran (max_len <= kScreenRowsLdsCap)
hipError_t launch_screen_rows(const uint32_t *d_slot, const uint32_t *d_len, uint64_t stride,
                              uint32_t n_db, uint32_t max_len, const uint32_t *d_count,
                              const uint32_t *d_owner, uint32_t *d_shared, uint32_t *d_median,
                              hipStream_t st, bool *lds);
// -w: owner[u] = the holder of entry u that keeps it (0xFFFFFFFF when its counter is 0)
hipError_t launch_screen_winner(const uint32_t *d_count, const uint32_t *d_ustart,
                                const uint32_t *d_post, uint32_t n, const double *d_scores,
                                const uint64_t *d_lengths, uint32_t *d_owner, hipStream_t st);
// pValueWithin (CommandScreen.cpp:386-406) of n references: 1 when shared is 0, else
// gsl_cdf_binomial_Q(shared - 1, r, size) by dist.hip's binomial tail
hipError_t launch_screen_pvalues(const uint32_t *d_shared, const uint32_t *d_size, uint32_t n,
                                 double r, double *d_p, hipStream_t st);

// taxscreen (taxscreen.hip): the LCA fold per entry of U and the clade sums.  Nodes are dense
// indices; parent[v] is an index or kTaxRoot, depth[v] the links from v to its root (the host
// computes it while it checks for cycles: every walk in the kernels is counted by it); top is
// the node of taxID 1, or kTaxUnknown.  ref_node[i]: kTaxNone, kTaxUnknown or a node.
constexpr uint32_t kTaxRoot = 0xFFFFFFFFu, kTaxNone = 0xFFFFFFFFu, kTaxUnknown = 0xFFFFFFFEu;
// posting lists of this many holders and more are folded by a wave, shorter ones by one lane
constexpr uint32_t kTaxWaveCut = 64;
struct TaxTree {
    const uint32_t *parent = nullptr, *depth = nullptr;
    uint32_t n_nodes = 0, top = kTaxUnknown;
};
// lca: n entries; tax_hashes / tax_count: n_nodes counters, zeroed by the caller; totals[0] +=
// the entries with count >= 1; *wave_entries += the entries folded by a wave
hipError_t launch_tax_lca(const uint32_t *d_count, const uint32_t *d_ustart, const uint32_t *d_post,
                          uint32_t n, const uint32_t *d_ref_node, const TaxTree &t, uint32_t *d_lca,
                          uint32_t *d_tax_hashes, uint32_t *d_tax_count,
                          unsigned long long *d_totals, uint32_t *d_wave_entries, hipStream_t st);
// clade_hashes / clade_count: n_nodes counters, zeroed by the caller
hipError_t launch_tax_clade(const TaxTree &t, const uint32_t *d_tax_hashes,
                            const uint32_t *d_tax_count, uint32_t *d_clade_hashes,
                            uint32_t *d_clade_count, hipStream_t st);

// kfinger (kfinger.hip): CFL / ICFL / CFL_ICFL k-fingers of sequence records and their combined
// (_COMB) forms, one lane per line.  A workgroup
// takes one descriptor: kind 0, the window starts [start, start + count) of record rec (its
// length >= the window); kind 1, the records rec .. rec + count - 1, each shorter than the window
// (one line each) and together at most kKfStage bytes.  count <= kKfRun; the descriptor's lines
// are line_base .. line_base + count - 1.  Records are indexed by rec_pos / rec_len (offset in
// the sequence buffer, length).
constexpr uint32_t kKfMaxWindow = 4096;   // the widest window: lengths fit u16, the stage 4.3 KB
constexpr uint32_t kKfRun = 256;          // window starts (lanes) per workgroup
constexpr uint32_t kKfStage = kKfRun + kKfMaxWindow - 1;   // bytes a workgroup stages at most
struct KfDesc {
    uint64_t line_base;
    uint32_t rec, start, count, kind;
};
// The factorization of a window (FPM_KF_* of fpmash.h): Duval's Lyndon factors; the inverse
// Lyndon factors (ICFL); or the Lyndon factors with every one longer than `threshold` (1 ..
// kKfMaxWindow) replaced by its own inverse Lyndon factors (CFL_ICFL).  ICFL keeps, per lane,
// one entry and one bit per window position: in LDS, u8 entries, for windows up to kKfLdsWindow
// (kf_lds_work_bytes per workgroup, 54 KB at the bound; 29 KB at w = 100), and beyond it in
// `work`, u16 entries, work_groups regions of kf_wide_work_bytes(w), one per workgroup of a
// grid that is no larger (the caller sizes it: kf_wide_groups).  A kind or threshold outside
// these, or a wide window without `work`, is hipErrorInvalidValue from every launch below.
// comb (fpm_kfinger_set_comb; lyn2vec's CFL_COMB / ICFL_COMB / CFL_ICFL_COMB-T,
// factorizations_comb.py:178-246): the cuts of the window's factorization together with the
// mirrored cuts of its reverse complement's, the reverse side of CFL_ICFL at threshold
// kKfCombRevThreshold whatever `threshold` is (lyn2vec's d_duval_ calls it without one).  A
// combined line keeps one more bit per window position, behind the ICFL memory: kf_bits_bytes
// per workgroup.  Where that no longer fits the workgroup's 64 KB of LDS beside the kernels'
// static kKfStaticLds, past kf_lds_window(kind, comb), the whole working memory is a region of
// kf_region_bytes in `work` (CFL_COMB too, which has nothing but those bits).
constexpr uint32_t kKfCfl = 0, kKfIcfl = 1, kKfCflIcfl = 2;
constexpr uint32_t kKfLdsWindow = 192;    // entries < 256 fit u8 and the workgroup's LDS 64 KB
constexpr uint32_t kKfCombRevThreshold = 30;   // cfl_icfl_'s default cfl_max
struct KfFact {
    uint32_t kind = kKfCfl, threshold = 0;
    void *work = nullptr;
    uint32_t work_groups = 0;
    uint32_t comb = 0;
};
constexpr uint32_t kf_lds_work_bytes(uint32_t w) { return kKfRun * ((w + 31) / 32 * 4 + w); }
constexpr size_t kf_wide_work_bytes(uint32_t w)
{
    return (size_t)kKfRun * ((w + 31) / 32 * 4 + (size_t)w * 2);
}
constexpr uint32_t kf_bits_bytes(uint32_t w) { return kKfRun * ((w + 31) / 32 * 4); }
// the dynamic LDS of a workgroup, and its region of `work` in the wide modes (icfl: the kind is
// ICFL or CFL_ICFL)
constexpr uint32_t kf_lds_bytes(bool icfl, bool comb, uint32_t w)
{
    return (icfl ? kf_lds_work_bytes(w) : 0) + (comb ? kf_bits_bytes(w) : 0);
}
constexpr size_t kf_region_bytes(bool icfl, bool comb, uint32_t w)
{
    return (icfl ? kf_wide_work_bytes(w) : 0) + (comb ? kf_bits_bytes(w) : 0);
}
// what the kernels hold statically: the stage, the short-record offsets, the block sum
constexpr uint32_t kKfStaticLds = (kKfStage + 3) / 4 * 4 + kKfRun * 4 + kKfRun / 64 * 8;
constexpr uint32_t kKfGroupLds = 64 * 1024;
// The widest window whose working memory stays in LDS.  Combined ICFL kinds: 256 x (w + 2 x 4 x
// ceil(w / 32)) + 5,392 <= 65,536 holds up to w = 186 (65,296 B; 187 takes 65,552).  CFL_COMB:
// 1,024 x ceil(w / 32) + 5,392 <= 65,536 holds up to 58 words, w = 1,856 (64,784 B).
constexpr uint32_t kKfCombLdsWindow = 186, kKfCombCflLdsWindow = 1856;
constexpr uint32_t kf_lds_window(uint32_t kind, uint32_t comb)
{
    return kind == kKfCfl ? (comb ? kKfCombCflLdsWindow : kKfMaxWindow)
                          : (comb ? kKfCombLdsWindow : kKfLdsWindow);
}
static_assert(kf_lds_bytes(true, false, kKfLdsWindow) + kKfStaticLds <= kKfGroupLds, "ICFL LDS");
static_assert(kf_lds_bytes(true, true, kKfCombLdsWindow) + kKfStaticLds <= kKfGroupLds &&
              kf_lds_bytes(true, true, kKfCombLdsWindow + 1) + kKfStaticLds > kKfGroupLds,
              "combined ICFL LDS");
static_assert(kf_lds_bytes(false, true, kKfCombCflLdsWindow) + kKfStaticLds <= kKfGroupLds &&
              kf_lds_bytes(false, true, kKfCombCflLdsWindow + 1) + kKfStaticLds > kKfGroupLds,
              "combined CFL LDS");
// workgroups of a wide-window grid: two per compute unit, no more than there are descriptors
constexpr uint32_t kf_wide_groups(uint32_t n_desc, uint32_t n_cu)
{
    return n_desc < 2 * n_cu ? n_desc : 2 * n_cu;
}
// pass one: per line its hash (u32, or u64 with use64), factor count and the text bytes after
// its ID; *d_val_total (zeroed by the caller) += the factors of all lines
hipError_t launch_kf_hash(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, uint32_t seed, uint32_t use64, void *d_hash,
                          uint32_t *d_n_vals, uint32_t *d_body, unsigned long long *d_val_total,
                          const KfFact &f, hipStream_t st);
// size[line] = body[line] + id_len[its record]; *d_text_total (zeroed by the caller) += the sum
hipError_t launch_kf_text_size(const KfDesc *d_descs, uint32_t n_desc, const uint32_t *d_body,
                               const uint32_t *d_id_len, uint32_t *d_size,
                               unsigned long long *d_text_total, hipStream_t st);
// pass two, at the offsets an exclusive scan of the sizes gave (d_off, per line): the factor
// lengths as u16, or the text lines (record r's ID: d_ids[d_id_off[r] .. + d_id_len[r]))
hipError_t launch_kf_values(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                            const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                            uint32_t w, const uint32_t *d_off, uint16_t *d_vals, const KfFact &f,
                            hipStream_t st);
hipError_t launch_kf_text(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                          const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                          uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                          const uint64_t *d_id_off, const uint32_t *d_id_len, uint8_t *d_out,
                          const KfFact &f, hipStream_t st);
// Split jobs (lyn2vec --type generalized): the units of rec_pos / rec_len are a record's
// consecutive pieces, all in kind-1 descriptors, and d_piece_rec[p] (ascending, n_piece entries)
// is the record of piece p, which indexes the IDs.  d_piece_rec null: a window job.
// The sizes of the text below per line / piece (fact: of the factor text), from pass one's
// d_n_vals and d_body; *d_text_total (zeroed by the caller) += the sum
hipError_t launch_kf_ext_size(const KfDesc *d_descs, uint32_t n_desc, const uint32_t *d_rec_len,
                              const uint32_t *d_piece_rec, uint32_t n_piece, uint32_t w,
                              bool fact, const uint32_t *d_n_vals, const uint32_t *d_body,
                              const uint32_t *d_id_len, uint32_t *d_size,
                              unsigned long long *d_text_total, hipStream_t st);
// pass two of a split job's text, "<id>  <len> <len> | <len> | \n" per record, or with fact the
// factor text of either kind of job: the same line with each factor's upper-cased bytes for its
// length (a window job's line: "<id> <factor> <factor>\n")
hipError_t launch_kf_ext_text(const uint8_t *d_seq, const uint64_t *d_rec_pos,
                              const uint32_t *d_rec_len, const KfDesc *d_descs, uint32_t n_desc,
                              uint32_t w, const uint32_t *d_off, const uint8_t *d_ids,
                              const uint64_t *d_id_off, const uint32_t *d_id_len,
                              const uint32_t *d_piece_rec, uint32_t n_piece, bool fact,
                              uint8_t *d_out, const KfFact &f, hipStream_t st);

// The transposed grid of a rectangular compare (fpm_refset_dist_mirror_dev): cell (r, q) at
// r * n_qry + q holds the pair "query r of the ref set against ref q of the query set".  For
// sorted distinct lists (numer, denom) is symmetric, and so are distance and p-value.
struct MirrorOut {
    Counts cnt;
    CellOut out;
    uint32_t n_qry = 0;
};
// distance / p-value / pass of the candidate cells only (after the candidate compare), and
// of each mirror cell (r, q) when `sym`, or of its cell in the transposed grid `mir` (when
// mir.out.dist is set); the other cells hold the probe's PairFill values
hipError_t launch_dist_cand_finalize(const CandList &cl, bool sym, Counts cnt, const RowSet &ref,
                                     const RowSet &qry, const DistParams &par, const CellOut &out,
                                     const MirrorOut &mir, hipStream_t st);
// distance and p-value of n cells from their u16 / u32 counts and per-cell genome lengths
hipError_t launch_pvalue_batch(Counts cnt, const uint64_t *len_ref, const uint64_t *len_qry,
                               uint64_t n, const DistParams &par, double *dist, double *pvalue,
                               hipStream_t st);
hipError_t launch_dist_finalize(Counts cnt, const RowSet &ref, const RowSet &qry,
                                const DistParams &par, const CellOut &out, hipStream_t st);

// The compact dist output's list of cells with numer > 0 (fpm_dist_list_dev): entry i =
// (qry[i], ref[i]) with its distance / p-value / pass; *count (device) counts every entry,
// those at index >= cap are not written.
struct CellList {
    uint32_t *qry = nullptr, *ref = nullptr;
    double *dist = nullptr, *pval = nullptr;
    uint8_t *pass = nullptr;
    unsigned long long *count = nullptr;
    uint64_t cap = 0;
};
// candidates: scatter (numer, denom) (mirror cell with `sym`; transposed grid mcnt with its own
// list mlist) and list the cells with numer > 0; cl.cnum == nullptr: counts read from the grid
hipError_t launch_dist_cand_list(const CandList &cl, bool sym, Counts cnt, const RowSet &ref,
                                 const RowSet &qry, const DistParams &par, const CellList &list,
                                 Counts mcnt, const CellList &mlist, hipStream_t st);
// every cell of a computed grid with numer > 0 into the list
hipError_t launch_dist_grid_list(Counts cnt, const RowSet &ref, const RowSet &qry,
                                 const DistParams &par, const CellList &list, hipStream_t st);

}  // namespace fpm
