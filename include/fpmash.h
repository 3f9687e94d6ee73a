/*
 * fpmash.h — the drop-in C ABI of the MI355X (gfx950) sketch + dist hot path.
 *
 * Plain C: pointers, sizes and int status codes; no C++ or torch types.  Every
 * entry point names the fp-mash interface (file:line under
 * /root/reference/mash/src/mash) whose work it takes over.  The host side
 * (fp-mash_amd/host: the Command/Sketch/-fp surface) and the Python binding
 * (fp-mash_amd/fpmash) call only these symbols; INTEGRATION.md shows the binding
 * a maintainer adds to the reference.
 *
 * Conventions
 *  - Return FPM_OK (0) on success, a negative FPM_E* code otherwise; the message
 *    is in fpm_last_error() (thread-local).  The reference has no status codes on
 *    this path (it prints and exit(1)s: Sketch.cpp:75-76, 1446-1463); the host
 *    maps a non-zero status to that behaviour.
 *  - `*_dev` entry points take DEVICE pointers and a hipStream_t passed as
 *    void* (NULL = the context's stream) and never synchronise; the others take
 *    host buffers, stage them, run, copy back and synchronise.
 *  - Hashes are returned as uint64_t; with use64 == 0 the value is the low 32
 *    bits of h1, zero-extended (hash_u.hash32, hash.h:17-21).
 *  - There is no CPU fallback: with no usable gfx950 device every compute call
 *    fails with FPM_ENODEV.
 *  - A context is bound to one device; contexts are independent and may be used
 *    from different threads (one thread per context at a time).
 */
#ifndef FPMASH_H
#define FPMASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPM_OK 0
#define FPM_EINVAL (-1)
#define FPM_ENODEV (-2)
#define FPM_EHIP (-3)
#define FPM_ENOMEM (-4)

#define FPM_ABI_VERSION 1

typedef struct fpm_ctx fpm_ctx;
typedef struct fpm_sketch_job fpm_sketch_job;

/* Sketch::Parameters (Sketch.h:40-113) as filled by sketchParameterSetup
 * (sketchParameterSetup.cpp:9-126) and setAlphabetFromString (Sketch.cpp:1260-1289). */
typedef struct fpm_sketch_params {
    uint32_t kmer_size;      /* 1..32 (Command.cpp:183-185) */
    uint32_t sketch_size;    /* minHashesPerWindow, s */
    uint32_t seed;           /* hash seed (default 42) */
    uint32_t use64;          /* alphabetSize^k > 2^32 */
    uint32_t noncanonical;   /* -n / -a / -z / -fp */
    uint32_t preserve_case;  /* -Z */
    uint8_t alphabet[256];   /* parameters.alphabet[] (1 = in alphabet) */
} fpm_sketch_params;

/* ---- context / device --------------------------------------------------- */
int fpm_abi_version(void);
/* The build id of this libfpmash.so: the first 16 hex digits of a SHA-256 over the sources it
 * was compiled from (csrc/, include/fpmash.h, the Makefile), also embedded in the file as the
 * text "fpm-build-id:<id>" so a profile can be stamped with the build it measured without
 * loading the library (tools/pmc_traffic.py, bench.py's roofline check). */
const char *fpm_build_id(void);
const char *fpm_last_error(void);
int fpm_device_count(int *count);
int fpm_ctx_create(int device, fpm_ctx **out);
void fpm_ctx_destroy(fpm_ctx *ctx);
void *fpm_ctx_stream(fpm_ctx *ctx);          /* the context's hipStream_t */
int fpm_ctx_synchronize(fpm_ctx *ctx);
/* Extra streams and events on the context's device, for callers that overlap independent
 * batches (e.g. the sketch of batch i+1 beside the dist of batch i): every call above takes
 * a stream argument.  Handles are the library's own hipStream_t / hipEvent_t (the HIP runtime
 * libfpmash links, which need not be the one another framework in the process bundles). */
int fpm_stream_create(fpm_ctx *ctx, void **stream);
int fpm_stream_destroy(fpm_ctx *ctx, void *stream);
int fpm_event_create(fpm_ctx *ctx, void **event);
int fpm_event_destroy(fpm_ctx *ctx, void *event);
int fpm_event_record(fpm_ctx *ctx, void *event, void *stream);
int fpm_stream_wait_event(fpm_ctx *ctx, void *stream, void *event);
/* first-use costs of a process up front: the pinned staging ring and one small DMA each way
 * (~15-25 ms in a fresh process, paid by the first staged upload otherwise).  Optional; for a caller that can run it beside other start-up work (the CLI's
 * device warm-up thread). */
int fpm_ctx_warm(fpm_ctx *ctx);

/* device memory helpers (for bindings that own no allocator) */
int fpm_malloc(fpm_ctx *ctx, void **dptr, size_t bytes);
int fpm_free(fpm_ctx *ctx, void *dptr);
int fpm_memcpy_h2d(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
int fpm_memcpy_d2h(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
/* device-to-device copy, ordered on the context stream (e.g. sketch rows into a buffer
 * handed to a collective) */
int fpm_memcpy_d2d(fpm_ctx *ctx, void *dst, const void *src, size_t bytes);
int fpm_memset(fpm_ctx *ctx, void *dptr, int value, size_t bytes);
/* Poisoned device memory (test hooks; off by default).  The library reads device memory from
 * four places: its pool of released buffers, its grow-only scratch slots (the context's and a
 * resident set's), plain allocations of its handles, and fpm_malloc.  A fresh allocation is
 * usually zero and a reused one holds the last call's data, so a kernel that relies on a value
 * nobody wrote can pass by luck.
 * set_poison: byte 0..255 turns it on, -1 off (anything else is FPM_EINVAL); a context created
 * with FPM_POISON=<0..255> in the environment starts with it on.  While on, every buffer from
 * those four places is filled with the byte before it is handed out (a scratch slot when it
 * grows), and the context stream is synchronised before the call returns.  Scratch slots of
 * 4096 bytes or less are still zeroed after they grow: that is the counter block's contract.
 * poison_now: synchronises the device, then fills the whole of every scratch slot of the
 * context and every buffer lying free in its pool with the byte.  Only three words of the
 * counter block are left as they are: the accumulators the index build keeps at zero from one
 * call to the next.  Before it overwrites anything it reads what the fpm_ctx_last_dist_stats
 * and fpm_ctx_last_rank_compact queries fetch lazily from scratch, so a later query returns
 * the values of the last compare and reads no poisoned memory.  Buffers in use (handles,
 * resident sets, caller memory, a pending fpm_dist_list_prefill) are not touched.  FPM_EINVAL
 * while poison is off. */
int fpm_ctx_set_poison(fpm_ctx *ctx, int byte);
int fpm_ctx_poison_now(fpm_ctx *ctx);

/* Per-kernel timing with HIP events recorded on the launch stream.
 * kernel ids: sketch tiles, sketch merge, fp hash, compare walk, finalize,
 * dist index build (insert + scan + scatter + probe count), dist row probe, ...; the two
 * passes of the k-finger generator last. */
#define FPM_K_SKETCH 0
#define FPM_K_MERGE 1
#define FPM_K_FPHASH 2
#define FPM_K_COMPARE 3
#define FPM_K_FINALIZE 4
#define FPM_K_INDEX 5
#define FPM_K_PROBE 6
#define FPM_K_FPTEXT 7
#define FPM_K_FILL 8
#define FPM_K_SEQPARSE 9
#define FPM_K_SCREEN 10   /* screen: the pool count pass (screen_count_kernel) */
#define FPM_K_KFINGER 11      /* kfinger pass one: Duval + line hash (kf_hash_kernel) */
#define FPM_K_KFINGER_OUT 12  /* kfinger pass two: sizes, scan, values / text (kf_emit_kernel) */
#define FPM_K_COUNT 13
/* one-pass bucket-index builds (dist_index.hip) that overflowed a level-1 slot and were
 * redone by the exact two-pass build, since the context was created */
int fpm_ctx_index_rebuilds(fpm_ctx *ctx, uint64_t *count);
/* dist calls whose probe was enqueued behind the index build before the host read the
 * build's counters (a call of the previous sparse call's shape): kept (hits) or dropped and
 * redone on the path the counters chose (misses), since the context was created */
int fpm_ctx_spec_stats(fpm_ctx *ctx, uint64_t *hits, uint64_t *misses);
int fpm_ctx_set_timing(fpm_ctx *ctx, int enable);
int fpm_ctx_reset_timing(fpm_ctx *ctx);
/* total milliseconds and launch count since the last reset (synchronises) */
int fpm_ctx_kernel_time(fpm_ctx *ctx, int kernel, double *total_ms, uint64_t *launches);
/* merges routed to the small-list kernel whose lists overflowed its LDS cap (searched in global
 * memory instead: same results, slower) since the last call on this device; resets it */
int fpm_merge_small_spills(fpm_ctx *ctx, uint64_t *count);
/* The exclusive scan of u32 counts every table build, index build and text pass of the library
 * goes through (dist_index.hip: launch_exscan), by itself, as test hooks.
 * fpm_scan_limits (no device needed; any output may be NULL): *block the elements one workgroup
 * scans, *fold_blocks the most blocks whose totals the add kernel folds itself (two launches);
 * past block x fold_blocks elements one workgroup scans the block totals between the two (three
 * launches).
 * fpm_exscan_dev: d_out[i] = d_in[0] + ... + d_in[i - 1] (mod 2^32) for i < n, the same into
 * d_out2 and the sum of all n into *d_total where those are not NULL; device pointers, n at most
 * 2^31.  It takes the scan's scratch from the context's pool, launches the scan on the context's
 * stream as the callers inside the library do, and synchronises.  Nothing past element n - 1 is
 * written; n = 0 writes only *d_total = 0. */
void fpm_scan_limits(uint32_t *block, uint32_t *fold_blocks);
int fpm_exscan_dev(fpm_ctx *ctx, const uint32_t *d_in, uint64_t n, uint32_t *d_out,
                   uint32_t *d_out2, uint32_t *d_total);

/* dist strategy: FPM_DIST_AUTO picks the inverted-index path unless the shared-hash
 * events exceed pairs*S/4; DENSE walks every pair; SPARSE always uses the index.
 * All three give identical results. */
#define FPM_DIST_AUTO 0
#define FPM_DIST_DENSE 1
#define FPM_DIST_SPARSE 2
int fpm_ctx_set_dist_mode(fpm_ctx *ctx, int mode);
/* statistics of the last compare: path (0 dense walk, 1 index + literal walk of the
 * candidates, 2 index + sorted-set merge of the candidates), posting events, candidates */
int fpm_ctx_last_dist_stats(fpm_ctx *ctx, int *sparse, uint64_t *events, uint64_t *candidates);
/* The compare kernel the last compare launched (a test hook, the result does not depend on
 * it): the dense grid walk from global memory, staged in LDS or on the u32 lists' 16-bit rank
 * images; or, on the index path, the literal walk of the candidates or their rank kernel with
 * 1024 / 2048 staged query hashes.  NONE: no pairs.  When a transposed grid was computed by a
 * swapped call (fpm_refset_dist_mirror_dev*), the kernel of that call.  Decided on the host:
 * no synchronisation. */
#define FPM_DK_NONE 0
#define FPM_DK_GRID_GLOBAL 1
#define FPM_DK_GRID_LDS 2
#define FPM_DK_GRID_IMG 3
#define FPM_DK_CAND_WALK 4
#define FPM_DK_CAND_RANK_1024 5
#define FPM_DK_CAND_RANK_2048 6
int fpm_ctx_last_dist_kernel(fpm_ctx *ctx, int *kernel);
/* The symmetric probe of one sorted set against itself (index path, rank kernel) reads only
 * the first half of each row: a pair's smallest shared hash can count only from the first
 * ceil(S / 2) positions of one of its rows.  On by default; a context created with
 * FPM_PROBE_HALF=0 in the environment starts with it off.  Same results either way. */
int fpm_ctx_set_probe_half(fpm_ctx *ctx, int on);
/* The form of the last compare's row probe (a test hook): NONE without a probe (dense walk, no
 * pairs), else FULL or HALF.  When a transposed grid was computed by a swapped call, the form
 * of that call.  Decided on the host: no synchronisation. */
#define FPM_PROBE_NONE 0
#define FPM_PROBE_FULL 1
#define FPM_PROBE_HALF 2
int fpm_ctx_last_dist_probe(fpm_ctx *ctx, int *form);
/* The index a compare builds for one sorted set against itself, when the half probe will read
 * it, leaves out every hash above the largest value any row's probed half holds: no probed
 * hash can equal one.  Resident sets and the record index of unsorted lists are never cut.  On
 * by default; a context created with FPM_INDEX_CUT=0 in the environment starts with it off.
 * Same results either way. */
int fpm_ctx_set_index_cut(fpm_ctx *ctx, int on);
/* The index of the last compare (a test hook): *cut whether it was cut, *indexed the entries
 * it holds, *entries the entries its rows hold (equal without a cut; both 0 when the compare
 * used no index).  Any pointer may be NULL.  From counters the compare already read: no
 * synchronisation. */
int fpm_ctx_last_index_cut(fpm_ctx *ctx, int *cut, uint64_t *indexed, uint64_t *entries);
/* One sorted u64 set against itself, half probe and rank kernel: the probe writes each row once
 * more without the hashes of its probed half that no other row holds, and the candidates are
 * ranked on those compacted rows (a hash of one row alone shares nothing; the kept hashes carry
 * their positions).  The diagonal is answered without ranking.  On by default; a context
 * created with FPM_RANK_COMPACT=0 in the environment starts with it off.  Same results either
 * way. */
int fpm_ctx_set_rank_compact(fpm_ctx *ctx, int on);
/* The candidate rows of the last compare (a test hook): *compact whether they were ranked
 * compacted, *kept the entries the compacted rows hold, *entries the entries of the rows
 * themselves (both 0 when not compacted).  Any pointer may be NULL.  Reads the probe's per-row
 * lengths: synchronises with the compare's stream. */
int fpm_ctx_last_rank_compact(fpm_ctx *ctx, int *compact, uint64_t *kept, uint64_t *entries);

/* ---- k-mer sketch ------------------------------------------------------------
 * Replaces addMinHashes (Sketch.cpp:664-735) + MinHashHeap::tryInsert
 * (MinHashHeap.cpp:68-146) + setMinHashesForReference/HashSet::toHashList
 * (Sketch.cpp:1291-1297, HashSet.cpp:78-118), as driven by sketchSequence
 * (Sketch.cpp:1490-1517, -i: one sketch per record) and sketchFile
 * (Sketch.cpp:1299-1488, default: one sketch per file = group of records).
 *
 * Records: seq[rec_off[r] .. rec_off[r+1]).  Records shorter than k are skipped
 * (Sketch.cpp:488-492, 1373-1377).  group_of_rec == NULL: record r is sketch r
 * (n_groups is ignored); else record r belongs to sketch group_of_rec[r] and
 * records of a group are streamed in record order.
 * Output: sketch g's ascending distinct hashes at out_hashes[g*sketch_size ..],
 * out_count[g] of them (= min(s, distinct k-mers)).
 */
int fpm_sketch_batch(fpm_ctx *ctx, const fpm_sketch_params *p, const char *seq,
                     const uint64_t *rec_off, uint32_t n_rec, const uint32_t *group_of_rec,
                     uint32_t n_groups, uint64_t *out_hashes, uint32_t *out_count);

/* Staged form for device-resident pipelines: stage() packs and uploads the
 * sequence and the tile plan (H2D), run() launches the kernels only (inputs
 * already in HBM), device_output() exposes the [n_groups][s] u64 result matrix
 * and the u32 counts on the device, fetch() copies them back. */
int fpm_sketch_stage(fpm_ctx *ctx, const fpm_sketch_params *p, const char *seq,
                     const uint64_t *rec_off, uint32_t n_rec, const uint32_t *group_of_rec,
                     uint32_t n_groups, fpm_sketch_job **job);
int fpm_sketch_run(fpm_sketch_job *job, void *stream);
int fpm_sketch_device_output(fpm_sketch_job *job, uint64_t **d_hashes, uint32_t **d_count,
                             uint32_t *n_groups, uint32_t *row_stride);
int fpm_sketch_fetch(fpm_sketch_job *job, uint64_t *out_hashes, uint32_t *out_count);
/* -M: the multiplicity of every hash of the final sketches, as MinHashHeap counts them
 * (MinHashHeap.cpp:68-146 with multiplicityMinimum 1: occurrences from a hash's first one on;
 * the final maximum of a full sketch stops counting once the heap holds the final set), the
 * counts32 that sketch -M writes (Sketch.cpp:584-596).  After run() on the same stream;
 * out_mult: n_groups x sketch_size u32, row g's first out_count[g] entries in hash order. */
int fpm_sketch_mult(fpm_sketch_job *job, void *stream, uint32_t *out_mult);
/* ---- reads mode (sketch -r / -m N) ----
 * MinHashHeap::tryInsert with multiplicityMinimum = min_copies and no Bloom filter
 * (MinHashHeap.cpp:68-146), as sketchFile drives it for a read set (Sketch.cpp:1299-1488, the
 * reads branches at :1308, :1403, :1424-1434, :1471-1480): only hashes seen at least
 * min_copies times enter the sketch.  The heap's threshold only falls, so sketch g is the
 * sketch_size smallest hashes with >= min_copies occurrences in group g, each with its full
 * number of occurrences; only the maximum of a full sketch stops counting once the heap holds
 * the final set (`hash < top` fails at :73), i.e. after the last of the final hashes'
 * min_copies-th occurrences in stream order.
 * set_min_copies: on a staged job (fpm_sketch_stage / fpm_sketch_stage_seq), before
 * reads_run; 0 is FPM_EINVAL; the default 1 is sketch -r without -m.
 * reads_run: in place of fpm_sketch_run (which it calls; the job's plain output is then
 * unspecified).  It widens the exact bottom-s' sketch (s' > s) until every group holds s
 * qualifying hashes or all of its hashes, reading one flag per group per round, so it
 * synchronises `stream`.  One device: counts of parts would have to be summed, not merged.
 * reads_fetch: row g's hashes (stride sketch_size), out_count[g] of them, their counts (the
 * counts32 of the .msh, Sketch.cpp:584-596; reads mode implies them,
 * sketchParameterSetup.cpp:56-59) and MinHashHeap::estimateSetSize (MinHashHeap.h:45: 2^64, or
 * 2^32 for u32 hashes, x count / maximum, in double, truncated; 0 for an empty sketch), the
 * Reference::length of a read set without -g (Sketch.cpp:1424-1434).  Any output may be NULL.
 * With min_copies 1 hashes and counts are those of fpm_sketch_run + fpm_sketch_mult.
 * Device memory per round: the wide job's rows ((groups + tiles of the open groups) x s' x
 * 8 B, s' = 8 s, then x 4 per round up to the open groups' window count) and (4 + 8 min_copies)
 * B per group x s' entry; FPM_ENOMEM / FPM_EHIP when the device cannot hold them.
 * reads_rounds: widening rounds of the last reads_run (-1 before any; a test hook, the result
 * does not depend on it) and, when group_round is given, the round that completed each group. */
int fpm_sketch_job_set_min_copies(fpm_sketch_job *job, uint32_t min_copies);
int fpm_sketch_reads_run(fpm_sketch_job *job, void *stream);
int fpm_sketch_reads_fetch(fpm_sketch_job *job, uint64_t *out_hashes, uint32_t *out_count,
                           uint32_t *out_mult, uint64_t *out_estimate);
int fpm_sketch_job_reads_rounds(fpm_sketch_job *job, int32_t *n_rounds, uint32_t *group_round);
/* Long groups whose wide sketch in the last round of the last reads_run took the sampled
 * long-group path of fpm_sketch_run (a sample of their tiles bounds what every tile keeps), -1
 * before any run: a test hook beside the MinHashHeap restatement (MinHashHeap.cpp:68-146), the
 * result does not depend on it. */
int fpm_sketch_job_reads_sampled(fpm_sketch_job *job, int32_t *n_sampled);
/* bytes the run() kernels read + write by algorithm (for roofline accounting) */
int fpm_sketch_job_info(fpm_sketch_job *job, uint64_t *seq_bytes, uint64_t *n_tiles,
                        uint64_t *n_kmers);
/* Tiles of the last run() that the survivors-only tile kernel could not keep and the plain
 * kernel redid (a test hook beside the MinHashHeap restatement, MinHashHeap.cpp:68-146, the
 * result does not depend on it): -1 when the job does not use that kernel (no long groups, or
 * s too large for their bound to leave few survivors per tile).  Waits for the device. */
int fpm_sketch_job_redo_tiles(fpm_sketch_job *job, int32_t *n_redo);
/* Long groups of the last run() that their tight bound (the sample's kt-th smallest hash,
 * kt ~ f s + 8 sqrt(f s) + 32 for a sampled share f of the group's tiles) left with fewer
 * than s hashes, so their tiles and selection ran again under the sample's s-th smallest
 * (values repeated across the group's tiles): a test hook; the sketches are MinHashHeap's
 * either way (MinHashHeap.cpp:68-146).  -1 when the job has no tight bounds (no long
 * groups, or s beyond the one-workgroup selection). */
int fpm_sketch_job_short_groups(fpm_sketch_job *job, int32_t *n_short);
/* Samples of the last fpm_sketch_run that the a-priori sample bound (~1.25 s + 16 sqrt s of
 * the sample's windows below it) left with fewer than s distinct hashes and that were redone
 * unbounded (a test hook, like the two above; every run starts from the staged bounds).  -1
 * when the job's samples carry no a-priori bound. */
int fpm_sketch_job_sample_short(fpm_sketch_job *job, int32_t *n_short);
/* The routes staging chose for a job (a test hook like fpm_ctx_last_dist_kernel, the result
 * does not depend on it): what fpm_sketch_run will launch, as decided on the host when the job
 * was staged: no synchronisation.  Tile class c holds the tiles of at most 256 << c k-mer
 * starts (one sketch_tiles_kernel instance per class).  A merge plan's rounds are one launch
 * each: `small` of them go to the small-list kernel (merge_small_kernel, by the estimated list
 * lengths and FPM_MERGE_SMALL), the others to `merge_kernel`, which depends on sketch_size
 * only (lists staged in LDS up to 16,384 hashes, searched in global memory beyond). */
#define FPM_TILE_CLASSES 6
#define FPM_MK_LDS 0
#define FPM_MK_GLOBAL 1
typedef struct fpm_sketch_plan {
    uint32_t tiles[FPM_TILE_CLASSES];         /* main pass: tiles per class */
    uint32_t sample_tiles[FPM_TILE_CLASSES];  /* sample pass of the long groups */
    uint32_t thr4;            /* the class-4 tiles take the survivors-only kernel (+ its redo) */
    uint32_t n_slots;         /* sampled (long) groups */
    uint32_t tight;           /* their bounds are the tight ones (short_groups() >= 0) */
    uint32_t n_ssel, n_sel;   /* one-workgroup selections: of the samples, of the groups */
    uint32_t rounds, rounds_small;                /* main merge plan */
    uint32_t sample_rounds, sample_rounds_small;  /* sample merge plan */
    uint32_t merge_kernel;    /* FPM_MK_*: the kernel of the rounds that are not small */
} fpm_sketch_plan;
int fpm_sketch_job_plan(fpm_sketch_job *job, fpm_sketch_plan *out);
/* The same for reads mode, whose wide jobs are staged and freed inside fpm_sketch_reads_run: the
 * plan of the wide job of the last round of the last reads_run (the job itself at min_copies 1,
 * else a job over the groups still open in that round) and that round's width s' (a test hook
 * like fpm_sketch_job_reads_sampled, which is this plan's n_slots).  Recorded when the round
 * begins, so a round that fails with FPM_ENOMEM still reports its plan.  FPM_EINVAL before any
 * round of a reads_run; it launches nothing. */
int fpm_sketch_job_reads_plan(fpm_sketch_job *job, fpm_sketch_plan *out, uint32_t *width);
void fpm_sketch_job_free(fpm_sketch_job *job);

/* Bottom-s of the union of n_lists sketches (device rows of stride s, ascending and
 * distinct, counts[i] entries each) into d_out / d_out_count: the final min-merge when one
 * sketch is computed in parts (a genome or read set split over GPUs, then all-gathered).
 * MinHashHeap keeps the s smallest distinct hashes of one stream (MinHashHeap.cpp:68-146);
 * the s smallest of a union are the s smallest of the union of the parts' s smallest. */
int fpm_sketch_merge_dev(fpm_ctx *ctx, const uint64_t *d_lists, const uint32_t *d_counts,
                         uint32_t n_lists, uint32_t s, uint64_t *d_out, uint32_t *d_out_count,
                         void *stream);

/* ---- FASTA text on the device ------------------------------------------------------
 * Replaces the main-thread kseq loop that feeds sketching (kseq_read, kseq.h:170-208, in
 * sketchFileBySequence / sketchFile, Sketch.cpp:478-522, 1299-1488): the n_seg file images
 * (one per input file, already inflated) go to the device, where records are found (a '>'
 * or '@' that is the first such byte of its line starts one; the header runs to the next
 * '\n'; the sequence is every isgraph byte up to the next record) and their sequence bytes
 * are packed for the sketch kernels without returning to the host.
 * quality_lines = 1 when a '+' occurs in sequence text (FASTQ: kseq then reads quality
 * lines, which this parser does not restate): the caller parses such input on the host.
 * fpm_seq_records: per record, its file, the header's byte offset ('>' / '@') in that file,
 * the header line's length (to its '\n' or the end of the file) and the sequence length.
 * fpm_sketch_stage_seq: a sketch job over the parsed records (group_of_rec[r] as in
 * fpm_sketch_stage, FPM_NO_GROUP = not sketched, e.g. records shorter than k); the job
 * takes over the packed records (stage once per parse).
 * fpm_seq_packed: the packed records themselves, read back (a test hook like
 * fpm_sketch_job_plan: it launches nothing and leaves the job as it was).  The buffer holds
 * each record's sequence bytes followed by one 0x00, *n_bytes = the sequence lengths' sum +
 * the record count in all; seq_off[r] = record r's offset in it.  out == NULL only reports
 * *n_bytes; FPM_EINVAL where cap < *n_bytes or the job's records were staged already. */
typedef struct fpm_seqtext fpm_seqtext;
#define FPM_NO_GROUP 0xFFFFFFFFu
int fpm_seq_parse(fpm_ctx *ctx, const char *const *seg_text, const uint64_t *seg_len,
                  uint32_t n_seg, fpm_seqtext **job, uint64_t *n_records, int *quality_lines);
int fpm_seq_records(fpm_seqtext *job, uint32_t *seg_of_rec, uint64_t *hdr_off, uint64_t *hdr_len,
                    uint64_t *seq_len);
int fpm_seq_packed(fpm_seqtext *job, uint64_t *seq_off, uint8_t *out, uint64_t cap,
                   uint64_t *n_bytes);
int fpm_sketch_stage_seq(fpm_ctx *ctx, const fpm_sketch_params *p, fpm_seqtext *seq,
                         const uint32_t *group_of_rec, uint32_t n_groups, fpm_sketch_job **job);
void fpm_seq_free(fpm_seqtext *job);

/* ---- -fp k-finger lines ------------------------------------------------------
 * Replaces the per-line getHashFingerPrint of Sketch::initFromFingerprints
 * (Sketch.cpp:131 -> hash.cpp:45-73): line l hashes the 8*n little-endian bytes
 * of vals[line_off[l] .. line_off[l+1]).  use64 == 0 (the -fp setting) writes
 * uint32_t, else uint64_t, into out. */
int fpm_fp_hash_lines(fpm_ctx *ctx, const uint64_t *vals, const uint64_t *line_off,
                      uint64_t n_lines, uint32_t seed, uint32_t use64, void *out);
int fpm_fp_hash_lines_dev(fpm_ctx *ctx, const uint64_t *d_vals, const uint64_t *d_line_off,
                          uint64_t n_lines, uint32_t seed, uint32_t use64, void *d_out,
                          void *stream);

/* ---- -fp text ------------------------------------------------------------------
 * Replaces the parse loop of Sketch::initFromFingerprints (Sketch.cpp:82-101: getline,
 * `iss >> id`, `while (iss >> v)` over u64 values) and its per-line getHashFingerPrint
 * (:131): the whole file image goes to the device, lines are split on '\n' (a last line
 * without '\n' counts), at most max_lines are parsed (the caller passes what is left of
 * the 1,000,000-line budget, :37, :82).  Per line: the ID token (byte offset, length),
 * the number of values, the line hash (u32, or u64 when use64), and new_id = 1 when the
 * ID differs from the previous line's, 0 when equal, 2 on line 0 (the caller compares
 * it with the previous file's last ID).  Grouping lines into References stays with the
 * caller (it owns names/comments).  fetch may be given NULL for outputs it does not need. */
typedef struct fpm_fptext fpm_fptext;
int fpm_fp_text_stage(fpm_ctx *ctx, const char *text, uint64_t text_len, uint64_t max_lines,
                      uint32_t seed, uint32_t use64, fpm_fptext **job, uint64_t *n_lines);
int fpm_fp_text_fetch(fpm_fptext *job, uint64_t *id_off, uint32_t *id_len, uint32_t *n_vals,
                      void *hash, uint8_t *new_id);
/* The References the staged file's lines make (Sketch.cpp:104-145, the grouping of
 * initFromFingerprints): one at line 0 (the caller checks its ID against the previous file's
 * last ID: equal IDs across files crash the reference, :131) and one wherever the ID changes.
 * Per Reference: its first line, its ID (byte offset, length in the text) and its length (the
 * first line's value count, :117, plus every line's, :134).  Computed on the device on the
 * first call; *n_refs is always set, the arrays are filled when cap >= *n_refs (a first call
 * with cap 0 sizes them).  With it a caller fetches only the hashes (fpm_fp_text_fetch with
 * the other outputs NULL): 4 B per line instead of 21. */
int fpm_fp_text_refs(fpm_fptext *job, uint64_t cap, uint64_t *n_refs, uint64_t *first_line,
                     uint64_t *id_off, uint32_t *id_len, uint64_t *length);
void fpm_fp_text_free(fpm_fptext *job);
/* The sizes the -fp text kernels switch paths at, for tests that build inputs on them (no
 * device needed; any output may be NULL): text bytes per newline-index workgroup, the largest
 * wave span (64 lines, from the 16-byte block of the line before them) the line kernel stages
 * in LDS before it reads global memory instead, and lines per head-count workgroup. */
void fpm_fp_text_limits(uint32_t *text_chunk, uint32_t *span_bytes, uint32_t *head_lines);

/* ---- k-fingers from sequence --------------------------------------------------------
 * Replaces lyn2vec `--type basic --type_factorization CFL` (the cyclic windows and their lines,
 * fingerprint_utils.py:95-110, 443-476; Duval's factorization, factorizations.py:102-126) and
 * the per-line getHashFingerPrint that follows it in Sketch::initFromFingerprints (hash.cpp:
 * 45-73): the k-finger lines of sequence records and their hashes, with no text in between.
 * A record of n bytes (ASCII a-z upper-cased, every other byte as it is) and a window w gives
 * one line, the Lyndon factor lengths of the record, when n < w; n lines when n >= w, line i the
 * factor lengths of the cyclic window (s + s[:w])[i : i + w]; none when n == 0.  Bytes compare
 * unsigned.  Lines are numbered in record order, then window-start order; only the first
 * max_lines exist (a cut may fall inside a record) and *n_lines is their number.
 * fpm_kfinger_stage (fingerprint_utils.py:95-110: the windows of the records read): host records
 * laid out as for fpm_sketch_stage, record r = seq[rec_off[r] .. rec_off[r+1]), bytes 0x01-0xFF.
 * fpm_kfinger_stage_seq (the same, over kseq records): the records of a device parse; take[r]
 * == 0 leaves record r out (take == NULL: every record); the job takes over the packed records
 * as fpm_sketch_stage_seq does (stage once per parse).
 * window outside 1 .. the limit of fpm_kfinger_limits, or a record of 2^32 bytes or more, is
 * FPM_EINVAL.
 * fpm_kfinger_set_factorization (lyn2vec --type_factorization ICFL / CFL_ICFL-T: ICFL_recursive
 * with find_pre, find_bre and border, factorizations.py:143-248, and CFL_icfl, :265-301, with the
 * << >> markers dropped as fingerprint_utils.py:443-476 drops them), between stage and run: what
 * a line's lengths are.  FPM_KF_CFL, the Lyndon factors, is what a job that never calls it
 * makes; FPM_KF_ICFL, the inverse Lyndon factors of the window; FPM_KF_CFL_ICFL, the Lyndon
 * factors with every one longer than `threshold` replaced by its own inverse Lyndon factors
 * (threshold 1 .. the widest window; ignored for the other kinds).  The end of the window is
 * known out of band: a 0x24 byte is a byte like any other, where lyn2vec's in-band '$' is not.
 * Another kind, a threshold out of range, or a call after fpm_kfinger_run is FPM_EINVAL and
 * leaves the job as it was.
 * fpm_kfinger_set_comb (lyn2vec --type_factorization CFL_COMB / ICFL_COMB / CFL_ICFL_COMB-T:
 * d_cfl, d_icfl, d_cfl_icfl and d_duval_, factorizations_comb.py:178-246), between stage and run:
 * with on = 1 a line of n bytes is cut where the job's factorization cuts it and at n - c for
 * every cut c of the same factorization of its reverse complement (A <-> T, C <-> G, every other
 * byte itself, after the upper-casing), and its lengths are the gaps between those cuts; a cut
 * both sides share is one cut.  The reverse side of FPM_KF_CFL_ICFL runs at threshold 30
 * whatever the job's threshold is: lyn2vec's d_duval_ calls cfl_icfl on the reverse complement
 * without it (:221), so its default cfl_max = 30 (:164) holds there, and the lines are lyn2vec's
 * byte for byte.  lyn2vec's reverse_complement raises KeyError on a byte outside ACGTN; here
 * such a byte is its own complement.  on = 0 is what a job that never calls it makes.  on > 1, a
 * NULL job or a call after fpm_kfinger_run is FPM_EINVAL and leaves the job as it was.
 * fpm_kfinger_run (factorizations.py:102-126 + hash.cpp:45-73): pass one on `stream` (NULL: the
 * context's): per line the hash of its 8 x count little-endian bytes (u32, or u64 with use64:
 * what fpm_fp_hash_lines gives for the same values) and its value count.
 * fpm_kfinger_fetch: rec_first_line[r] = the first line of input record r (n_rec + 1 entries,
 * the last one *n_lines; a record without lines repeats the next one's), the hashes and the value
 * counts, copied back; any output may be NULL.  fpm_kfinger_device_output: the hashes and counts
 * on the device (valid until the job is freed or run again).
 * Pass two, after run (fingerprint_utils.py:443-476: the lines written): fpm_kfinger_values, the
 * factor lengths as u16, line l's at vals[val_off[l] .. val_off[l+1]) (val_off: n_lines + 1
 * entries, may be NULL); fpm_kfinger_text, the text, one line "<id> <len> <len> ...\n" per
 * line, formatted on the device; ids holds each input record's full ID bytes (lyn2vec's
 * "<id>_0"), record r's at ids[id_off[r] .. id_off[r+1]).  Both follow fpm_seq_packed's sizing:
 * out == NULL only reports *total / *n_bytes, else FPM_EINVAL where cap is smaller.  A job whose
 * text would reach 2^32 bytes (or whose values 2^32) is FPM_EINVAL: split the records over jobs.
 * fpm_kfinger_limits (no device needed; any output may be NULL): the widest window and the run
 * length, the window starts one workgroup takes, for tests that build inputs on them. */
typedef struct fpm_kfinger fpm_kfinger;
int fpm_kfinger_stage(fpm_ctx *ctx, const char *seq, const uint64_t *rec_off, uint32_t n_rec,
                      uint32_t window, uint64_t max_lines, fpm_kfinger **job, uint64_t *n_lines);
int fpm_kfinger_stage_seq(fpm_ctx *ctx, fpm_seqtext *seq, const uint8_t *take, uint32_t window,
                          uint64_t max_lines, fpm_kfinger **job, uint64_t *n_lines);
#define FPM_KF_CFL 0
#define FPM_KF_ICFL 1
#define FPM_KF_CFL_ICFL 2
int fpm_kfinger_set_factorization(fpm_kfinger *job, uint32_t kind, uint32_t threshold);
/* lyn2vec --type_factorization CFL_COMB / ICFL_COMB / CFL_ICFL_COMB-T (factorizations_comb.py:178-246) */
int fpm_kfinger_set_comb(fpm_kfinger *job, uint32_t on);   /* before fpm_kfinger_run; else FPM_EINVAL */
int fpm_kfinger_run(fpm_kfinger *job, uint32_t seed, uint32_t use64, void *stream);
int fpm_kfinger_fetch(fpm_kfinger *job, uint64_t *rec_first_line, void *hash, uint32_t *n_vals);
int fpm_kfinger_device_output(fpm_kfinger *job, void **d_hash, uint32_t **d_n_vals,
                              uint64_t *n_lines, uint32_t *hash_bytes);
int fpm_kfinger_values(fpm_kfinger *job, uint64_t *val_off, uint16_t *vals, uint64_t cap,
                       uint64_t *total);
int fpm_kfinger_text(fpm_kfinger *job, const char *ids, const uint64_t *id_off, char *out,
                     uint64_t cap, uint64_t *n_bytes);
void fpm_kfinger_free(fpm_kfinger *job);
void fpm_kfinger_limits(uint32_t *max_window, uint32_t *run_length);
/* The workgroups of the grid the job's run used for a window whose working memory (ICFL's, a
 * combined form's cut bits) lies in device memory (a test hook like fpm_sketch_job_plan, the
 * result does not depend on it): at most two per compute unit and no more than the job has
 * descriptors, each taking every *groups-th descriptor.  0 for CFL, for a window that keeps that
 * memory in LDS, for a job without lines, and before fpm_kfinger_run. */
int fpm_kfinger_wide_groups(fpm_kfinger *job, uint32_t *groups);
/* The widest window whose working memory stays in LDS under factorization `kind` (FPM_KF_*),
 * combined (comb = 1) or not; the next window is the first to keep it in device memory.  The
 * widest window of fpm_kfinger_limits for plain FPM_KF_CFL, which has no working memory.  No
 * device needed; an unknown kind or comb > 1 is FPM_EINVAL. */
int fpm_kfinger_lds_window(uint32_t kind, uint32_t comb, uint32_t *window);
/* Long reads: lyn2vec --type generalized --split N (factors_string, fingerprint_utils.py:114-130;
 * compute_long_fingerprint_by_list, :480-518).  A record of n > 0 bytes and a split N is cut
 * into pieces: the whole record when n < N, else [0, N) [N, 2N) ... with a last piece of n mod N
 * bytes where that is not 0.  Each piece is factorized on its own (no window, no cyclic wrap)
 * under the job's factorization, by the byte rules above.  The job's unit, the "line" of every
 * call above, is a piece: fpm_kfinger_set_factorization, _set_comb, _run, _fetch
 * (rec_first_line[r]: record r's first piece), _device_output, _values and _wide_groups work
 * per piece with no other change of meaning.  split runs from 1 to the widest window of
 * fpm_kfinger_limits, else FPM_EINVAL; the working memory of a split leaves LDS where that of
 * the same window does (fpm_kfinger_lds_window).  There is no max_lines.  Pieces share
 * workgroups in packs of at most run_length pieces and run_length + widest window - 1 bytes
 * (fpm_kfinger_limits), across records.
 * fpm_kfinger_text of a split job writes one line per record with a piece, "<id>" + two spaces,
 * then per piece its lengths joined by single spaces and " | ", then "\n"; ids holds the
 * record's ID as it is to appear (lyn2vec's, without "_0").
 * fpm_kfinger_fact_text (lyn2vec --fact create, :471-474 and :509-511), after run, for window
 * and split jobs: the same lines with each factor's upper-cased bytes in place of its length; a
 * window job's line is "<id> <factor> <factor> ...\n".  Sizing, errors and the 2^32 bound are
 * those of fpm_kfinger_text. */
int fpm_kfinger_stage_split(fpm_ctx *ctx, const char *seq, const uint64_t *rec_off,
                            uint32_t n_rec, uint32_t split, fpm_kfinger **job,
                            uint64_t *n_pieces);
int fpm_kfinger_stage_split_seq(fpm_ctx *ctx, fpm_seqtext *seq, const uint8_t *take,
                                uint32_t split, fpm_kfinger **job, uint64_t *n_pieces);
int fpm_kfinger_fact_text(fpm_kfinger *job, const char *ids, const uint64_t *id_off, char *out,
                          uint64_t cap, uint64_t *n_bytes);

/* ---- dist ---------------------------------------------------------------------
 * Replaces compare()/compareSketches()/pValue() (CommandDistance.cpp:335-450) over
 * the whole ref x query grid that CommandDistance::run chunks (:224-261).
 * Sketch lists are rows of dense matrices (row stride in elements) holding
 * hash_bytes = 8 (u64) or 4 (u32) values; lists may be unsorted and carry
 * duplicates (-fp), the walk is the reference's literal one.  sketch_size =
 * min(s_ref, s_query) (:342-344).  Outputs are query-major: index q*n_ref + r. */
int fpm_compare_grid(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len,
                     uint64_t ref_stride, uint32_t n_ref, const void *qry,
                     const uint32_t *qry_len, uint64_t qry_stride, uint32_t n_qry,
                     uint32_t hash_bytes, uint32_t sketch_size, uint32_t *out_numer,
                     uint32_t *out_denom);
int fpm_compare_grid_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                         uint64_t ref_stride, uint32_t n_ref, const void *d_qry,
                         const uint32_t *d_qry_len, uint64_t qry_stride, uint32_t n_qry,
                         uint32_t hash_bytes, uint32_t sketch_size, uint32_t *d_numer,
                         uint32_t *d_denom, void *stream);
/* distance (:404-419), p-value (:433-450, FP64) and the -d/-v filter (:421-429);
 * ref_length/qry_length are Reference::length (k-mer space scaling of pValue).
 * max_dist / max_pvalue < 0 disable the filter.  pass may be NULL. */
int fpm_dist_finalize_dev(fpm_ctx *ctx, const uint32_t *d_numer, const uint32_t *d_denom,
                          const uint64_t *d_ref_length, const uint64_t *d_qry_length,
                          uint32_t n_ref, uint32_t n_qry, uint32_t kmer_size,
                          double kmer_space, double max_dist, double max_pvalue,
                          double *d_dist, double *d_pvalue, uint8_t *d_pass, void *stream);
/* Distance and p-value of n independent cells from their counts (u16 when count_bytes = 2,
 * u32 when 4) and per-cell genome lengths, device pointers, stream-ordered, no -d / -v
 * filters: the values the compact output (fpm_dist_list_dev) leaves out, for the cells a
 * caller wants.  Replaces the per-pair distance + pValue of CommandDistance.cpp:404-419,
 * 433-450 (SURVEY §8(b)'s optional fpm_pvalue_batch).  d_dist / d_pvalue may each be NULL. */
int fpm_pvalue_batch_dev(fpm_ctx *ctx, const void *d_numer, const void *d_denom,
                         uint32_t count_bytes, const uint64_t *d_len_ref,
                         const uint64_t *d_len_qry, uint64_t n, uint32_t kmer_size,
                         double kmer_space, double *d_dist, double *d_pvalue, void *stream);
/* compare + finalize in one call on device buffers (= fpm_compare_grid_dev followed by
 * fpm_dist_finalize_dev on the same stream). */
int fpm_dist_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                 const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                 const void *d_qry, const uint32_t *d_qry_len, const uint64_t *d_qry_length,
                 uint64_t qry_stride, uint32_t n_qry, uint32_t hash_bytes, uint32_t sketch_size,
                 uint32_t kmer_size, double kmer_space, double max_dist, double max_pvalue,
                 uint32_t *d_numer, uint32_t *d_denom, double *d_dist, double *d_pvalue,
                 uint8_t *d_pass, void *stream);
/* fpm_dist_dev with u16 numer / denom cells (every count is <= sketch_size <= 65535): the
 * same results in 4 bytes per pair instead of 8 (the grid's counts as SURVEY.md §8(b)
 * sizes them); FPM_EINVAL when sketch_size > 65535. */
int fpm_dist_dev16(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                   const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                   const void *d_qry, const uint32_t *d_qry_len, const uint64_t *d_qry_length,
                   uint64_t qry_stride, uint32_t n_qry, uint32_t hash_bytes, uint32_t sketch_size,
                   uint32_t kmer_size, double kmer_space, double max_dist, double max_pvalue,
                   uint16_t *d_numer, uint16_t *d_denom, double *d_dist, double *d_pvalue,
                   uint8_t *d_pass, void *stream);
/* ---- compact dist output (the grid as u16 numer / denom) ----------
 * compareSketches' (numer, denom) for every cell of the n_qry x n_ref grid as u16 cells (4 B
 * per pair, query-major), and distance / p-value / pass only for the cells that share hashes
 * (numer > 0): an unordered list, each such cell exactly once.  A cell not in the list has
 * numer 0, and compareSketches / pValue give it closed-form values (CommandDistance.cpp:
 * 404-408 and 435-437 at common = 0): distance 0 when denom == 0 (two empty lists), else 1;
 * p-value 1; pass = (max_dist < 0 || distance <= max_dist) && (max_pvalue < 0 || 1 <=
 * max_pvalue).  Listed cells hold what fpm_dist_dev16 writes for them.
 * The list lives in caller device memory: entry i is (qry[i], ref[i], dist[i], pvalue[i],
 * pass[i]) (pass may be NULL).  *count is a DEVICE u64 the call resets and then sets to the
 * number of cells with numer > 0; entries at index >= cap are not written, so a caller that
 * reads *count > cap after the stream work repeats the call with cap >= *count. */
typedef struct fpm_cell_list {
    uint32_t *qry, *ref;
    double *dist, *pvalue;
    uint8_t *pass;
    uint64_t cap;
    uint64_t *count;
} fpm_cell_list;
int fpm_dist_list_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                      const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                      const void *d_qry, const uint32_t *d_qry_len, const uint64_t *d_qry_length,
                      uint64_t qry_stride, uint32_t n_qry, uint32_t hash_bytes,
                      uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
                      double max_dist, double max_pvalue, uint16_t *d_numer, uint16_t *d_denom,
                      const fpm_cell_list *list, void *stream);
/* The compact grid's counts ahead of the call that computes them, e.g. before the sketches
 * exist: numer 0 and denom sketch_size in all n_qry x n_ref u16 cells, on the context's side
 * stream after the work already on `stream` (a pure write stream beside the sketch kernels).
 * The next fpm_dist_list_dev on this context whose numer / denom / n_ref / n_qry /
 * sketch_size are these takes it over: it writes no no-shared-hash counts of
 * its own, sets denom = la + lb where la + lb < sketch_size (compareSketches' min(S, la + lb)
 * at common = 0, CommandDistance.cpp:416-418) and writes its cells after the prefill.  Any
 * other dist call on the context waits for it first.  Until then only that call (or
 * fpm_ctx_synchronize) orders the grid against the prefill.  No reference counterpart: its
 * compare writes every pair (CommandDistance.cpp:365-430). */
int fpm_dist_list_prefill(fpm_ctx *ctx, uint16_t *d_numer, uint16_t *d_denom, uint32_t n_ref,
                          uint32_t n_qry, uint32_t sketch_size, void *stream);
/* host-buffer convenience: compare + finalize */
int fpm_dist(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len, const uint64_t *ref_length,
             uint64_t ref_stride, uint32_t n_ref, const void *qry, const uint32_t *qry_len,
             const uint64_t *qry_length, uint64_t qry_stride, uint32_t n_qry,
             uint32_t hash_bytes, uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
             double max_dist, double max_pvalue, uint32_t *out_numer, uint32_t *out_denom,
             double *out_dist, double *out_pvalue, uint8_t *out_pass);

/* ---- resident reference set -------------------------------------------------------
 * CommandDistance::run compares every query against the same reference sketch
 * (CommandDistance.cpp:191-261: the pool's CompareInput holds `const Sketch & sketchRef`
 * for all query chunks).  A refset keeps the reference rows on the device and builds their
 * bucket index ONCE; each query block then only uploads its own rows, probes the resident
 * index and runs the exact candidate compare + distance / p-value (the same results as
 * fpm_dist_dev).  sketch_size (min of the two sketches' s, :342-344) is fixed per set when
 * its rows are unsorted (-fp lists: FPM_EINVAL for another); a set of sorted rows may be
 * compared at another sketch_size, at the cost of the half probe when it is its own query.
 * _create copies host rows to the device (owned); _create_dev borrows device rows, which
 * must outlive the set.  count_bytes selects u16 (2, sketch_size <= 65535) or u32 (4)
 * numer / denom cells.  fpm_refset_dist takes host query rows and host outputs (pinned
 * buffers from fpm_host_alloc copy at full PCIe rate). */
typedef struct fpm_refset fpm_refset;
int fpm_refset_create(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len,
                      const uint64_t *ref_length, uint64_t ref_stride, uint32_t n_ref,
                      uint32_t hash_bytes, uint32_t sketch_size, fpm_refset **out);
int fpm_refset_create_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                          const uint64_t *d_ref_length, uint64_t ref_stride, uint32_t n_ref,
                          uint32_t hash_bytes, uint32_t sketch_size, fpm_refset **out);
int fpm_refset_dist_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                        const uint64_t *d_qry_length, uint64_t qry_stride, uint32_t n_qry,
                        uint32_t sketch_size, uint32_t count_bytes, uint32_t kmer_size,
                        double kmer_space, double max_dist, double max_pvalue, void *d_numer,
                        void *d_denom, double *d_dist, double *d_pvalue, uint8_t *d_pass,
                        void *stream);
/* The same compare, plus its transposed grid: m_* cell (r, q) at r * n_qry + q holds what
 * fpm_refset_dist_dev would give for query r of the reference set against reference q of the
 * query rows (the pair seen from the other side, CommandDistance.cpp:224-261 with the two
 * sketches exchanged).  For the sorted distinct lists of the k-mer path the candidate
 * results are scattered to both grids (compareSketches' counts are symmetric there, and so
 * are distance and p-value); otherwise (unsorted -fp lists, dense path) the transposed grid
 * is computed by the swapped call.  Multi-GPU all-vs-all dist deals unordered block pairs
 * to the ranks with this call (fpmash/shard.py: pair_block_jobs).  The query rows must not
 * be the set's own rows (that grid is its own transpose: fpm_refset_dist_dev). */
int fpm_refset_dist_mirror_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                               const uint64_t *d_qry_length, uint64_t qry_stride, uint32_t n_qry,
                               uint32_t sketch_size, uint32_t count_bytes, uint32_t kmer_size,
                               double kmer_space, double max_dist, double max_pvalue,
                               void *d_numer, void *d_denom, double *d_dist, double *d_pvalue,
                               uint8_t *d_pass, void *m_numer, void *m_denom, double *m_dist,
                               double *m_pvalue, uint8_t *m_pass, void *stream);
/* The compact output (fpm_dist_list_dev) against a resident set, and with its transposed grid
 * (m_numer / m_denom cell (r, q) at r * n_qry + q, m_list its own list of cells). */
int fpm_refset_dist_list_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                             const uint64_t *d_qry_length, uint64_t qry_stride, uint32_t n_qry,
                             uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
                             double max_dist, double max_pvalue, uint16_t *d_numer,
                             uint16_t *d_denom, const fpm_cell_list *list, void *stream);
int fpm_refset_dist_mirror_list_dev(fpm_refset *rs, const void *d_qry, const uint32_t *d_qry_len,
                                    const uint64_t *d_qry_length, uint64_t qry_stride,
                                    uint32_t n_qry, uint32_t sketch_size, uint32_t kmer_size,
                                    double kmer_space, double max_dist, double max_pvalue,
                                    uint16_t *d_numer, uint16_t *d_denom,
                                    const fpm_cell_list *list, uint16_t *m_numer,
                                    uint16_t *m_denom, const fpm_cell_list *m_list, void *stream);
/* Rebuild the set's bucket index from its (device, borrowed) rows in place, e.g. after the
 * rows were rewritten by a new sketch run; no reallocation when the geometry is unchanged. */
int fpm_refset_reindex(fpm_refset *rs, void *stream);
int fpm_refset_dist(fpm_refset *rs, const void *qry, const uint32_t *qry_len,
                    const uint64_t *qry_length, uint64_t qry_stride, uint32_t n_qry,
                    uint32_t sketch_size, uint32_t kmer_size, double kmer_space, double max_dist,
                    double max_pvalue, uint32_t *out_numer, uint32_t *out_denom, double *out_dist,
                    double *out_pvalue, uint8_t *out_pass);
/* The compact output of one host query block (fpm_refset_dist_list_dev with host buffers):
 * out_numer / out_denom (n_qry x n_ref cells of count_bytes = 2 (u16, sketch_size <= 65535)
 * or 4 (u32), query-major, may be NULL) and the cells with numer > 0 (l_* arrays of cap
 * entries, any may be NULL).  *n_listed = the number of such cells; only the first
 * min(*n_listed, cap) are copied (the device list grows as needed). */
int fpm_refset_dist_list(fpm_refset *rs, const void *qry, const uint32_t *qry_len,
                         const uint64_t *qry_length, uint64_t qry_stride, uint32_t n_qry,
                         uint32_t sketch_size, uint32_t kmer_size, double kmer_space,
                         double max_dist, double max_pvalue, uint32_t count_bytes,
                         void *out_numer, void *out_denom, uint32_t *l_qry, uint32_t *l_ref,
                         double *l_dist, double *l_pvalue, uint8_t *l_pass, uint64_t cap,
                         uint64_t *n_listed);
void fpm_refset_free(fpm_refset *rs);

/* pinned (page-locked) host memory for staging buffers of the host-buffer calls */
int fpm_host_alloc(fpm_ctx *ctx, void **p, size_t bytes);
int fpm_host_free(fpm_ctx *ctx, void *p);

/* ---- triangle -fp ---------------------------------------------------------------
 * Replaces compareFingerprints (CommandTriangle.cpp:255-302): positional compare of
 * two lists over min(len) entries, matches = equal values at the same position (the
 * fork reads an uninitialised union half, :279; u32 values are zero-extended here).
 * distance = 1 - matches/min(len), p-value = gsl_cdf_chisq_Q(matches, 1) =
 * erfc(sqrt(matches/2)), pass = distance <= max_dist && p <= max_pvalue.
 * Host buffers, query-major output (q*n_ref + r); n_qry <= 65535 per call. */
int fpm_fp_positional_grid(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len,
                           uint64_t ref_stride, uint32_t n_ref, const void *qry,
                           const uint32_t *qry_len, uint64_t qry_stride, uint32_t n_qry,
                           uint32_t hash_bytes, double max_dist, double max_pvalue,
                           uint32_t *out_numer, uint32_t *out_denom, double *out_dist,
                           double *out_pvalue, uint8_t *out_pass);

/* ---- contain ------------------------------------------------------------------------
 * Replaces contain()/containSketches() (CommandContain.cpp:314-412) over the whole ref x query
 * grid.  Per pair, with R / Q the lists as stored (lengths lr / lq, no cut to a sketch size):
 *     common = 0; denom = min(lr, lq); i = j = 0
 *     for (steps = 0; steps < denom && i < lr; steps++)
 *         if      R[i] < Q[j]  { i++; steps--; }
 *         else if Q[j] < R[i]  { j++; }
 *         else                 { i++; j++; common++; }
 * and the cell gets (common, j); compares are unsigned at hash_bytes.  The caller computes
 * score = common / j and error = 1 / sqrt(j) in double (:408-411), so the device holds integers
 * only.  Rows, strides, lengths and the query-major output (index q*n_ref + r) are those of
 * fpm_compare_grid.
 * When every row of both sets is strictly ascending the walk has an order-free form
 * (jf = min(lr, lq, #{q in Q : q <= R[lr-1]}), common = |Q[0..jf) n R|, (0, 0) when a list is
 * empty), which contain_rows_kernel computes with the query row staged in LDS, or read from
 * global memory when the longest query row exceeds fpm_contain_lds_cap entries.  Otherwise,
 * or in FPM_CONTAIN_LITERAL mode, contain_literal_kernel walks each pair as written above.
 * The rows are tested on the device and the host reads the one flag: both calls synchronise
 * `stream` once before the compare is launched (LITERAL mode skips the test and does not).
 * No CPU fallback. */
int fpm_contain_dev(fpm_ctx *ctx, const void *d_ref, const uint32_t *d_ref_len,
                    uint64_t ref_stride, uint32_t n_ref, const void *d_qry,
                    const uint32_t *d_qry_len, uint64_t qry_stride, uint32_t n_qry,
                    uint32_t hash_bytes, uint32_t *d_common, uint32_t *d_steps, void *stream);
/* host buffers, copied through the pinned staging ring */
int fpm_contain(fpm_ctx *ctx, const void *ref, const uint32_t *ref_len, uint64_t ref_stride,
                uint32_t n_ref, const void *qry, const uint32_t *qry_len, uint64_t qry_stride,
                uint32_t n_qry, uint32_t hash_bytes, uint32_t *out_common, uint32_t *out_steps);
#define FPM_CONTAIN_AUTO 0
#define FPM_CONTAIN_LITERAL 1
int fpm_ctx_set_contain_mode(fpm_ctx *ctx, int mode);
/* The kernel the last contain call launched (a test hook like fpm_ctx_last_dist_kernel).
 * NONE: an empty grid. */
#define FPM_CK_NONE 0
#define FPM_CK_ROWS_LDS 1
#define FPM_CK_ROWS_GLOBAL 2
#define FPM_CK_LITERAL 3
int fpm_ctx_last_contain_kernel(fpm_ctx *ctx, int *kernel);
/* the longest query row (entries of hash_bytes) contain_rows_kernel stages in LDS on this
 * context's device */
int fpm_contain_lds_cap(fpm_ctx *ctx, uint32_t hash_bytes, uint32_t *cap);
/* ref rows one contain_rows_kernel workgroup takes (one wave per row at a time) */
#define FPM_CONTAIN_BLOCK_REFS 64

/* ---- screen -------------------------------------------------------------------------
 * The documented `mash screen` (doc/man/mash-screen.1): how much of each sketch of a database
 * is in a pool of sequences, and at what depth.  The fork's CommandScreen::run no longer
 * streams the pool; these calls replace the parts of the verb that are intact in the tree:
 *   the hashTable / hashCounts maps over the database    CommandScreen.cpp:87-102
 *   hashSequence, every window's key counted             CommandScreen.cpp:280-384
 *   the pool's one MinHashHeap and its set size          CommandTaxScreen.cpp:347-370,
 *                                                        MinHashHeap.h:45
 *   shared counts, depths, medians                       CommandScreen.cpp:133-151, 208-211, 235
 *   -w                                                   CommandScreen.cpp:153-202
 *   pValueWithin                                         CommandScreen.cpp:386-406
 * estimateIdentity (:259-278) stays with the caller, in double.
 *
 * A screen holds the table of one database: U, the sorted distinct union of its rows (rows
 * as in fpm_compare_grid, cut by the caller to the sketch size), a u32 counter per entry of U
 * (the reference's atomic<uint32_t>: it wraps at 2^32) and the running bottom-sketch_size row
 * of the pool.  Every row must be strictly ascending within its length, else FPM_EINVAL (-fp
 * made sketches).  n_db * stride must be below 2^32.  _create copies host rows, _create_dev
 * reads device rows; neither keeps them.  Both synchronise.  No CPU fallback. */
typedef struct fpm_screen fpm_screen;
int fpm_screen_create(fpm_ctx *ctx, const void *db, const uint32_t *db_len, uint64_t stride,
                      uint32_t n_db, uint32_t hash_bytes, uint32_t sketch_size, fpm_screen **out);
int fpm_screen_create_dev(fpm_ctx *ctx, const void *d_db, const uint32_t *d_db_len,
                          uint64_t stride, uint32_t n_db, uint32_t hash_bytes,
                          uint32_t sketch_size, fpm_screen **out);
void fpm_screen_free(fpm_screen *sc);
/* One slice of the pool (CommandTaxScreen.cpp:262-329 hands hashSequence 1 MB at a time): `job`
 * is a sketch job staged as ONE group with the database's parameters and sketch size
 * (fpm_sketch_stage / fpm_sketch_stage_seq).  Runs the job, min-merges its row into the
 * screen's running row (:347-361) and counts every valid window of its tiles.  Counts add and
 * bottom-s rows merge, so any slicing of a pool into whole records gives the same result. */
int fpm_screen_add_job(fpm_screen *sc, fpm_sketch_job *job, void *stream);
/* n keys hashed elsewhere (device u64, u32 hashes zero-extended): counted like window keys;
 * the set-size row is not touched. */
int fpm_screen_add_hashes_dev(fpm_screen *sc, const uint64_t *d_keys, uint64_t n, void *stream);
/* MinHashHeap::estimateSetSize of the pool so far (MinHashHeap.h:45: 2^64, or 2^32 for u32
 * hashes, x len / max, truncated; 0 for an empty row).  Synchronises. */
int fpm_screen_set_size(fpm_screen *sc, uint64_t *set_size);
/* U and its counters (either array may be NULL; *n_distinct is always set).  Synchronises. */
int fpm_screen_counts(fpm_screen *sc, uint64_t *out_keys, uint32_t *out_counts,
                      uint64_t *n_distinct);
/* Per reference i: shared = #{h in row i : count[h] >= 1}, median = the counts of those
 * hashes in ascending order, at position shared / 2 (0 when shared is 0).  Host outputs. */
int fpm_screen_rows(fpm_screen *sc, uint32_t *out_shared, uint32_t *out_median);
/* -w: every entry of U with count >= 1 goes to one of the references that hold it: the
 * greatest scores[i] (the caller's estimateIdentity of the plain shared counts, compared as
 * doubles, never recomputed), then the greatest lengths[i] (Reference::length), then the
 * lowest i.  The reference breaks that last tie by the visiting order of an unordered set;
 * the lowest index replaces it.  shared / median as above over the entries each reference won. */
int fpm_screen_rows_winner(fpm_screen *sc, const double *scores, const uint64_t *lengths,
                           uint32_t *out_shared, uint32_t *out_median);
/* pValueWithin(shared[i], setSize, kmer_space, size_i) with the screen's current set size; r =
 * setSize / kmer_space is clamped to [0, 1] without the reference's message (:395-399). */
int fpm_screen_pvalues(fpm_screen *sc, const uint32_t *shared, double kmer_space, double *out_p);
/* The instance of screen_rows_kernel the last fpm_screen_rows / _rows_winner launched (a
 * test hook like fpm_ctx_last_contain_kernel): the reference's counters held in LDS, or
 * gathered from global memory in every selection pass when the longest row exceeds
 * fpm_screen_lds_cap cells.  NONE: no reference. */
#define FPM_SK_NONE 0
#define FPM_SK_ROWS_LDS 1
#define FPM_SK_ROWS_GLOBAL 2
int fpm_ctx_last_screen_kernel(fpm_ctx *ctx, int *kernel);
int fpm_screen_lds_cap(fpm_ctx *ctx, uint32_t *cap);
/* What the table build chose (a test hook like fpm_ctx_last_screen_kernel; any output may be
 * NULL): *cells the database's cells within the row lengths, *n_distinct = |U|, *sbits the bits
 * of the counting sort's bucket index (about two cells per bucket, at most 22; 0 for a database
 * without cells) and *dbits those of the lookup directory (2^dbits >= 2 |U|, at most 24). */
int fpm_screen_table_info(fpm_screen *sc, uint64_t *cells, uint64_t *n_distinct, uint32_t *sbits,
                          uint32_t *dbits);

/* ---- taxscreen ----------------------------------------------------------------------
 * `mash taxscreen` after its pool pass (the same as screen's): one lowest-common-ancestor fold
 * per entry of U over the taxa of its holders, per-taxon tallies and clade sums:
 *   the fold per distinct database hash                  CommandTaxScreen.cpp:386-397
 *   getLowestCommonAncestor                              taxdb.hpp:158-190
 *   taxHashCount / taxCount (minCov = 1)                 CommandTaxScreen.cpp:398-403
 *   cladeCount / cladeHashCount up the ancestors         CommandTaxScreen.cpp:406-437
 * Parsing the dump, the reference -> taxID mapping and writeReport (taxdb.hpp:192-236) stay
 * with the caller.
 *
 * The taxonomy is n_nodes dense node indices: parent[v] is an index or FPM_TAX_ROOT (a node
 * that is its own parent in nodes.dmp, taxdb.hpp:97-99, or whose parent has no line).  top is
 * the node of taxID 1, the value of the reference's `return 1` (:167, :173, :189), or
 * FPM_TAX_UNKNOWN when the dump has none.  ref_node[i] is reference i's node, FPM_TAX_NONE for
 * taxID 0 (`if (a == 0) return b`, :159-160) or FPM_TAX_UNKNOWN for a taxID without a node.
 *
 * out_lca[u], with T the ref_node values of u's holders that are not NONE: NONE when T is
 * empty; its one element (maybe UNKNOWN) when it has one; else top when any is UNKNOWN, when
 * they share no ancestor or when their deepest common ancestor is a root (the path of `a`
 * stops before a root and before taxID 1, :176, and so does the walk from `b`, :183); else that
 * ancestor.  The result does not depend on the order of the holders (the reference visits an
 * unordered set).  tax_hashes[v] = #{u : lca[u] = v}, tax_count[v] the same over the entries
 * with count >= 1; clade_*[v] = the sums of tax_* over v and its descendants (every tallied
 * taxon visited once; the reference inserts into the map it iterates).  out_totals[0] = the
 * entries with count >= 1, out_totals[1] = |U|: entries whose lca is NONE or UNKNOWN count
 * there and nowhere else (getEntry fails for them, :417).
 *
 * Host buffers in and out (out_lca and the four arrays may be NULL); synchronises; may follow
 * any number of fpm_screen_add_* calls and leaves the counters as they are.  FPM_EINVAL,
 * before anything is launched, for parent links that hold a cycle, a parent index or a
 * ref_node out of range, or a top that is no node.  No CPU fallback. */
#define FPM_TAX_ROOT    0xFFFFFFFFu
#define FPM_TAX_NONE    0xFFFFFFFFu   /* in ref_node / out_lca */
#define FPM_TAX_UNKNOWN 0xFFFFFFFEu
int fpm_screen_tax(fpm_screen *sc, const uint32_t *parent, uint32_t n_nodes, uint32_t top,
                   const uint32_t *ref_node,
                   uint32_t *out_lca,            /* |U|, in U's order; may be NULL */
                   uint32_t *out_tax_hashes, uint32_t *out_tax_count,
                   uint32_t *out_clade_hashes, uint32_t *out_clade_count,  /* n_nodes each */
                   uint64_t out_totals[2]);      /* total_count, total_hashes */
/* How the last fpm_screen_tax folded its posting lists (a test hook like
 * fpm_ctx_last_screen_kernel): every list by one lane (THREAD), or at least one list of
 * fpm_screen_tax_wave_cut holders or more by a whole wave (WAVE).  NONE: U is empty. */
#define FPM_TK_NONE 0
#define FPM_TK_THREAD 1
#define FPM_TK_WAVE 2
int fpm_ctx_last_tax_kernel(fpm_ctx *ctx, int *kernel);
int fpm_screen_tax_wave_cut(fpm_ctx *ctx, uint32_t *cut);

/* ---- communicator: RCCL over xGMI for the cross-GPU min-merge ------------------------
 * north_star reserves the collective for "the final min-merge only where the reference set
 * exceeds one GPU's HBM" (or one sketch is split over GPUs).  The reference has no collective:
 * one process, one pthreads pool (ThreadPool.h:13-61) feeding one MinHashHeap per genome
 * (Sketch.cpp:1354-1422).  The communicator lives on the context's device and HIP runtime
 * (librccl is dlopen'ed on first use); the caller carries the 128-byte unique id from one rank
 * to the others over any host channel (ncclGetUniqueId / ncclCommInitRank's contract). */
#define FPM_COMM_ID_BYTES 128
typedef struct fpm_comm fpm_comm;
int fpm_comm_unique_id(uint8_t id[FPM_COMM_ID_BYTES]);
/* waits until all nranks ranks have called it with the same id, up to FPM_COMM_INIT_TIMEOUT_S
 * seconds (default 120; a non-blocking RCCL set-up, aborted past the limit): then FPM_EHIP and a
 * message naming the limit, instead of blocking for ever on a peer that never joins */
int fpm_comm_create(fpm_ctx *ctx, int nranks, int rank, const uint8_t id[FPM_COMM_ID_BYTES],
                    fpm_comm **out);
void fpm_comm_destroy(fpm_comm *comm);
/* every rank's `bytes` of d_send, in rank order, into d_recv (nranks x bytes), enqueued on
 * `stream` (NULL: the context stream) */
int fpm_comm_all_gather(fpm_comm *comm, const void *d_send, void *d_recv, size_t bytes,
                        void *stream);
/* The min-merge of one sketch computed in parts (MinHashHeap.cpp:68-146: the s smallest
 * distinct of a union = the s smallest of the union of the parts' s smallest): every rank's
 * ascending bottom-s row (s hashes, d_count valid) all-gathered into library buffers and merged
 * on the device (fpm_sketch_merge_dev) into d_out / d_out_count on every rank; enqueued on
 * `stream` (NULL: the context stream). */
int fpm_sketch_min_merge_comm(fpm_comm *comm, const uint64_t *d_row, const uint32_t *d_count,
                              uint32_t s, uint64_t *d_out, uint32_t *d_out_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FPMASH_H */
