"""fpmash — Python binding of the gfx950 sketch + dist C ABI (include/fpmash.h).

A ctypes mirror of the reference's engine calls for this path:
  Sketch sketching (addMinHashes/MinHashHeap, Sketch.cpp:664-735, 1490-1517) -> Context.sketch
  -fp line hashing (getHashFingerPrint, hash.cpp:45-73)                    -> Context.fp_hash_lines
  lyn2vec CFL k-fingers (fingerprint_utils.py:95-110, 443-476) + their hashes -> Context.kfinger
    (factorization="ICFL" / "CFL_ICFL-<T>": factorizations.py:143-248, 265-301; "CFL_COMB" /
    "ICFL_COMB" / "CFL_ICFL_COMB-<T>": factorizations_comb.py:178-246; split=N: the long-read
    fingerprints, fingerprint_utils.py:114-130, 480-518; fact_text=True: the --fact create text)
  compare/compareSketches/pValue (CommandDistance.cpp:335-450)             -> Context.dist
  contain/containSketches (CommandContain.cpp:314-412)                     -> Context.contain
  screen: hashSequence, sums, -w, pValueWithin (CommandScreen.cpp:133-406) -> Context.screen
  taxscreen: the LCA fold, tallies and clade sums (CommandTaxScreen.cpp:386-437) -> Context.taxscreen
The shared library is built in-tree (fp-mash_amd/lib/libfpmash.so).  There is no
CPU fallback: if the library is missing this import fails, and without a gfx950
device Context() raises FpmError(FPM_ENODEV).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# FPMASH_LIB: another build of the same ABI (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("FPMASH_LIB") or os.path.join(PKG_ROOT, "lib", "libfpmash.so")
BIN_PATH = os.path.join(PKG_ROOT, "bin", "fpmash")

FPM_OK, FPM_EINVAL, FPM_ENODEV, FPM_EHIP, FPM_ENOMEM = 0, -1, -2, -3, -4
(K_SKETCH, K_MERGE, K_FPHASH, K_COMPARE, K_FINALIZE, K_INDEX, K_PROBE, K_FPTEXT, K_FILL,
 K_SEQPARSE, K_SCREEN, K_KFINGER, K_KFINGER_OUT) = range(13)
NO_GROUP = 0xFFFFFFFF
KERNEL_NAMES = {K_SKETCH: "sketch_tiles_kernel", K_MERGE: "merge_kernel",
                K_FPHASH: "fp_hash_kernel",
                K_COMPARE: "candidate compare (rank_rows/walk_cand/compare_grid), contain_rows/contain_literal",
                K_FINALIZE: "dist finalize (dense / candidate cells)", K_INDEX: "dist index build",
                K_PROBE: "probe_rows_kernel", K_FPTEXT: "fp text parse (nl index + fp_line)",
                K_FILL: "dist_fill_kernel", K_SEQPARSE: "FASTA parse (seq chunk scan + emit)",
                K_SCREEN: "screen_count_kernel",
                K_KFINGER: "kf_hash_kernel (Duval + line hash)",
                K_KFINGER_OUT: "kfinger pass two (sizes + scan + kf_emit_kernel)"}
DIST_AUTO, DIST_DENSE, DIST_SPARSE = 0, 1, 2
# fpm_ctx_last_dist_stats path codes
DIST_PATHS = ["dense walk", "bucket index + literal walk", "bucket index + bucketed rank"]
# fpm_ctx_last_dist_kernel codes (FPM_DK_*)
(DK_NONE, DK_GRID_GLOBAL, DK_GRID_LDS, DK_GRID_IMG, DK_CAND_WALK, DK_CAND_RANK_1024,
 DK_CAND_RANK_2048) = range(7)
DIST_KERNELS = ["none", "compare_grid_kernel", "compare_grid_lds_kernel",
                "compare_grid_img_kernel", "walk_cand_kernel", "rank_rows_kernel<1024>",
                "rank_rows_kernel<2048>"]
# fpm_ctx_last_dist_probe codes (FPM_PROBE_*)
PROBE_NONE, PROBE_FULL, PROBE_HALF = range(3)
# fpm_ctx_set_contain_mode (FPM_CONTAIN_*) and fpm_ctx_last_contain_kernel (FPM_CK_*) codes
CONTAIN_AUTO, CONTAIN_LITERAL = range(2)
CK_NONE, CK_ROWS_LDS, CK_ROWS_GLOBAL, CK_LITERAL = range(4)
CONTAIN_KERNELS = ["none", "contain_rows_kernel<lds>", "contain_rows_kernel<global>",
                   "contain_literal_kernel"]
CONTAIN_BLOCK_REFS = 64                          # FPM_CONTAIN_BLOCK_REFS
# fpm_ctx_last_screen_kernel codes (FPM_SK_*)
SK_NONE, SK_ROWS_LDS, SK_ROWS_GLOBAL = range(3)
SCREEN_KERNELS = ["none", "screen_rows_kernel<lds>", "screen_rows_kernel<global>"]
# fpm_screen_tax node codes (FPM_TAX_*) and fpm_ctx_last_tax_kernel codes (FPM_TK_*)
TAX_ROOT, TAX_NONE, TAX_UNKNOWN = 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE
TK_NONE, TK_THREAD, TK_WAVE = range(3)
TAX_KERNELS = ["none", "tax_lca_kernel (lane per entry)", "tax_lca_kernel (wave on long lists)"]

ALPHABET_NUCLEOTIDE = "ACGT"                     # Sketch.h alphabetNucleotide
ALPHABET_PROTEIN = "ACDEFGHIKLMNPQRSTVWY"         # Sketch.h alphabetProtein

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
f64p = C.POINTER(C.c_double)
u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
vp = C.c_void_p

# every symbol include/fpmash.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("fpm_abi_version", C.c_int, []),
    ("fpm_build_id", C.c_char_p, []),
    ("fpm_last_error", C.c_char_p, []),
    ("fpm_device_count", C.c_int, [C.POINTER(C.c_int)]),
    ("fpm_ctx_create", C.c_int, [C.c_int, C.POINTER(vp)]),
    ("fpm_ctx_destroy", None, [vp]),
    ("fpm_ctx_stream", vp, [vp]),
    ("fpm_stream_create", C.c_int, [vp, C.POINTER(vp)]),
    ("fpm_stream_destroy", C.c_int, [vp, vp]),
    ("fpm_event_create", C.c_int, [vp, C.POINTER(vp)]),
    ("fpm_event_destroy", C.c_int, [vp, vp]),
    ("fpm_event_record", C.c_int, [vp, vp, vp]),
    ("fpm_stream_wait_event", C.c_int, [vp, vp, vp]),
    ("fpm_ctx_synchronize", C.c_int, [vp]),
    ("fpm_ctx_warm", C.c_int, [vp]),
    ("fpm_malloc", C.c_int, [vp, C.POINTER(vp), C.c_size_t]),
    ("fpm_free", C.c_int, [vp, vp]),
    ("fpm_memcpy_h2d", C.c_int, [vp, vp, vp, C.c_size_t]),
    ("fpm_memcpy_d2h", C.c_int, [vp, vp, vp, C.c_size_t]),
    ("fpm_memcpy_d2d", C.c_int, [vp, vp, vp, C.c_size_t]),
    ("fpm_memset", C.c_int, [vp, vp, C.c_int, C.c_size_t]),
    ("fpm_ctx_set_timing", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_reset_timing", C.c_int, [vp]),
    ("fpm_ctx_kernel_time", C.c_int, [vp, C.c_int, f64p, u64p]),
    ("fpm_scan_limits", None, [u32p, u32p]),
    ("fpm_exscan_dev", C.c_int, [vp, vp, C.c_uint64, vp, vp, vp]),
    ("fpm_ctx_set_dist_mode", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_last_dist_stats", C.c_int, [vp, C.POINTER(C.c_int), u64p, u64p]),
    ("fpm_ctx_last_dist_kernel", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("fpm_ctx_set_probe_half", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_last_dist_probe", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("fpm_ctx_set_index_cut", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_last_index_cut", C.c_int, [vp, C.POINTER(C.c_int), u64p, u64p]),
    ("fpm_ctx_set_rank_compact", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_last_rank_compact", C.c_int, [vp, C.POINTER(C.c_int), u64p, u64p]),
    ("fpm_ctx_set_poison", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_poison_now", C.c_int, [vp]),
    ("fpm_sketch_batch", C.c_int, [vp, vp, C.c_char_p, u64p, C.c_uint32, u32p, C.c_uint32,
                                   u64p, u32p]),
    ("fpm_sketch_stage", C.c_int, [vp, vp, C.c_char_p, u64p, C.c_uint32, u32p, C.c_uint32,
                                   C.POINTER(vp)]),
    ("fpm_sketch_run", C.c_int, [vp, vp]),
    ("fpm_sketch_device_output", C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), u32p, u32p]),
    ("fpm_sketch_fetch", C.c_int, [vp, u64p, u32p]),
    ("fpm_sketch_mult", C.c_int, [vp, vp, u32p]),
    ("fpm_sketch_job_set_min_copies", C.c_int, [vp, C.c_uint32]),
    ("fpm_sketch_reads_run", C.c_int, [vp, vp]),
    ("fpm_sketch_reads_fetch", C.c_int, [vp, u64p, u32p, u32p, u64p]),
    ("fpm_sketch_job_reads_rounds", C.c_int, [vp, C.POINTER(C.c_int32), u32p]),
    ("fpm_sketch_job_reads_sampled", C.c_int, [vp, C.POINTER(C.c_int32)]),
    ("fpm_merge_small_spills", C.c_int, [vp, u64p]),
    ("fpm_sketch_job_info", C.c_int, [vp, u64p, u64p, u64p]),
    ("fpm_sketch_job_redo_tiles", C.c_int, [vp, C.POINTER(C.c_int32)]),
    ("fpm_sketch_job_short_groups", C.c_int, [vp, C.POINTER(C.c_int32)]),
    ("fpm_sketch_job_sample_short", C.c_int, [vp, C.POINTER(C.c_int32)]),
    ("fpm_sketch_job_plan", C.c_int, [vp, vp]),
    ("fpm_sketch_job_reads_plan", C.c_int, [vp, vp, u32p]),
    ("fpm_sketch_job_free", None, [vp]),
    ("fpm_fp_hash_lines", C.c_int, [vp, u64p, u64p, C.c_uint64, C.c_uint32, C.c_uint32, vp]),
    ("fpm_fp_hash_lines_dev", C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp,
                                        vp]),
    ("fpm_fp_text_stage", C.c_int, [vp, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                    C.c_uint32, C.POINTER(vp), u64p]),
    ("fpm_fp_text_fetch", C.c_int, [vp, u64p, u32p, u32p, vp, u8p]),
    ("fpm_fp_text_refs", C.c_int, [vp, C.c_uint64, u64p, u64p, u64p, u32p, u64p]),
    ("fpm_fp_text_free", None, [vp]),
    ("fpm_fp_text_limits", None, [u32p, u32p, u32p]),
    ("fpm_kfinger_stage", C.c_int, [vp, C.c_char_p, u64p, C.c_uint32, C.c_uint32, C.c_uint64,
                                    C.POINTER(vp), u64p]),
    ("fpm_kfinger_stage_seq", C.c_int, [vp, vp, u8p, C.c_uint32, C.c_uint64, C.POINTER(vp),
                                        u64p]),
    ("fpm_kfinger_set_factorization", C.c_int, [vp, C.c_uint32, C.c_uint32]),
    ("fpm_kfinger_set_comb", C.c_int, [vp, C.c_uint32]),
    ("fpm_kfinger_run", C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
    ("fpm_kfinger_fetch", C.c_int, [vp, u64p, vp, u32p]),
    ("fpm_kfinger_device_output", C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), u64p, u32p]),
    ("fpm_kfinger_values", C.c_int, [vp, u64p, u16p, C.c_uint64, u64p]),
    ("fpm_kfinger_text", C.c_int, [vp, C.c_char_p, u64p, vp, C.c_uint64, u64p]),
    ("fpm_kfinger_free", None, [vp]),
    ("fpm_kfinger_stage_split", C.c_int, [vp, C.c_char_p, u64p, C.c_uint32, C.c_uint32,
                                          C.POINTER(vp), u64p]),
    ("fpm_kfinger_stage_split_seq", C.c_int, [vp, vp, u8p, C.c_uint32, C.POINTER(vp), u64p]),
    ("fpm_kfinger_fact_text", C.c_int, [vp, C.c_char_p, u64p, vp, C.c_uint64, u64p]),
    ("fpm_kfinger_limits", None, [u32p, u32p]),
    ("fpm_kfinger_wide_groups", C.c_int, [vp, u32p]),
    ("fpm_kfinger_lds_window", C.c_int, [C.c_uint32, C.c_uint32, u32p]),
    ("fpm_compare_grid", C.c_int, [vp, vp, u32p, C.c_uint64, C.c_uint32, vp, u32p, C.c_uint64,
                                   C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]),
    ("fpm_compare_grid_dev", C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64,
                                       C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
    ("fpm_dist_finalize_dev", C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]),
    ("fpm_pvalue_batch_dev", C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, C.c_uint64, C.c_uint32,
                                       C.c_double, vp, vp, vp]),
    ("fpm_dist_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint64,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                               C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
    ("fpm_dist_dev16", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp, C.c_uint64,
                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double,
                                 C.c_double, C.c_double, vp, vp, vp, vp, vp, vp]),
    ("fpm_dist_list_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, vp,
                                    C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]),
    ("fpm_dist_list_prefill", C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]),
    ("fpm_fp_positional_grid", C.c_int, [vp, vp, u32p, C.c_uint64, C.c_uint32, vp, u32p,
                                         C.c_uint64, C.c_uint32, C.c_uint32, C.c_double,
                                         C.c_double, u32p, u32p, f64p, f64p, u8p]),
    ("fpm_dist", C.c_int, [vp, vp, u32p, u64p, C.c_uint64, C.c_uint32, vp, u32p, u64p,
                           C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                           C.c_double, C.c_double, C.c_double, u32p, u32p, f64p, f64p, u8p]),
    ("fpm_contain", C.c_int, [vp, vp, u32p, C.c_uint64, C.c_uint32, vp, u32p, C.c_uint64,
                              C.c_uint32, C.c_uint32, u32p, u32p]),
    ("fpm_contain_dev", C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint64,
                                  C.c_uint32, C.c_uint32, vp, vp, vp]),
    ("fpm_ctx_set_contain_mode", C.c_int, [vp, C.c_int]),
    ("fpm_ctx_last_contain_kernel", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("fpm_contain_lds_cap", C.c_int, [vp, C.c_uint32, u32p]),
    ("fpm_screen_create", C.c_int, [vp, vp, u32p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.POINTER(vp)]),
    ("fpm_screen_create_dev", C.c_int, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.POINTER(vp)]),
    ("fpm_screen_free", None, [vp]),
    ("fpm_screen_add_job", C.c_int, [vp, vp, vp]),
    ("fpm_screen_add_hashes_dev", C.c_int, [vp, vp, C.c_uint64, vp]),
    ("fpm_screen_set_size", C.c_int, [vp, u64p]),
    ("fpm_screen_counts", C.c_int, [vp, u64p, u32p, u64p]),
    ("fpm_screen_rows", C.c_int, [vp, u32p, u32p]),
    ("fpm_screen_rows_winner", C.c_int, [vp, f64p, u64p, u32p, u32p]),
    ("fpm_screen_pvalues", C.c_int, [vp, u32p, C.c_double, f64p]),
    ("fpm_ctx_last_screen_kernel", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("fpm_screen_lds_cap", C.c_int, [vp, u32p]),
    ("fpm_screen_table_info", C.c_int, [vp, u64p, u64p, u32p, u32p]),
    ("fpm_screen_tax", C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p,
                                 u32p, u64p]),
    ("fpm_ctx_last_tax_kernel", C.c_int, [vp, C.POINTER(C.c_int)]),
    ("fpm_screen_tax_wave_cut", C.c_int, [vp, u32p]),
    ("fpm_refset_create", C.c_int, [vp, vp, u32p, u64p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.POINTER(vp)]),
    ("fpm_refset_create_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                        C.c_uint32, C.POINTER(vp)]),
    ("fpm_refset_dist_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double,
                                      vp, vp, vp, vp, vp, vp]),
    ("fpm_refset_dist_mirror_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_double, C.c_double,
                                             C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                             vp]),
    ("fpm_refset_dist_list_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                           C.c_uint32, C.c_double, C.c_double, C.c_double, vp,
                                           vp, vp, vp]),
    ("fpm_refset_dist_mirror_list_dev", C.c_int, [vp, vp, vp, vp, C.c_uint64, C.c_uint32,
                                                  C.c_uint32, C.c_uint32, C.c_double, C.c_double,
                                                  C.c_double, vp, vp, vp, vp, vp, vp, vp]),
    ("fpm_refset_reindex", C.c_int, [vp, vp]),
    ("fpm_ctx_index_rebuilds", C.c_int, [vp, u64p]),
    ("fpm_ctx_spec_stats", C.c_int, [vp, u64p, u64p]),
    ("fpm_refset_dist", C.c_int, [vp, vp, u32p, u64p, C.c_uint64, C.c_uint32, C.c_uint32,
                                  C.c_uint32, C.c_double, C.c_double, C.c_double, u32p, u32p,
                                  f64p, f64p, u8p]),
    ("fpm_refset_dist_list", C.c_int, [vp, vp, u32p, u64p, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_double, C.c_double, C.c_double,
                                       C.c_uint32, vp, vp, u32p, u32p, f64p, f64p, u8p,
                                       C.c_uint64, u64p]),
    ("fpm_refset_free", None, [vp]),
    ("fpm_sketch_merge_dev", C.c_int, [vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]),
    ("fpm_seq_parse", C.c_int, [vp, C.POINTER(C.c_char_p), u64p, C.c_uint32, C.POINTER(vp),
                                u64p, C.POINTER(C.c_int)]),
    ("fpm_seq_records", C.c_int, [vp, u32p, u64p, u64p, u64p]),
    ("fpm_seq_packed", C.c_int, [vp, u64p, u8p, C.c_uint64, u64p]),
    ("fpm_sketch_stage_seq", C.c_int, [vp, vp, vp, u32p, C.c_uint32, C.POINTER(vp)]),
    ("fpm_seq_free", None, [vp]),
    ("fpm_host_alloc", C.c_int, [vp, C.POINTER(vp), C.c_size_t]),
    ("fpm_host_free", C.c_int, [vp, vp]),
    ("fpm_comm_unique_id", C.c_int, [C.c_char_p]),
    ("fpm_comm_create", C.c_int, [vp, C.c_int, C.c_int, C.c_char_p, C.POINTER(vp)]),
    ("fpm_comm_destroy", None, [vp]),
    ("fpm_comm_all_gather", C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    ("fpm_sketch_min_merge_comm", C.c_int, [vp, vp, vp, C.c_uint32, vp, vp, vp]),
]
COMM_ID_BYTES = 128


class CellListStruct(C.Structure):
    """fpm_cell_list (include/fpmash.h): device arrays of the compact dist output's list"""
    _fields_ = [("qry", vp), ("ref", vp), ("dist", vp), ("pvalue", vp), ("pass_", vp),
                ("cap", C.c_uint64), ("count", vp)]


TILE_CLASSES = 6                                  # FPM_TILE_CLASSES: class c = 256 << c starts
MK_LDS, MK_GLOBAL = range(2)                      # fpm_sketch_plan.merge_kernel (FPM_MK_*)


class SketchPlan(C.Structure):
    """fpm_sketch_plan (include/fpmash.h): the routes staging chose for a sketch job"""
    _fields_ = [("tiles", C.c_uint32 * TILE_CLASSES), ("sample_tiles", C.c_uint32 * TILE_CLASSES),
                ("thr4", C.c_uint32), ("n_slots", C.c_uint32), ("tight", C.c_uint32),
                ("n_ssel", C.c_uint32), ("n_sel", C.c_uint32),
                ("rounds", C.c_uint32), ("rounds_small", C.c_uint32),
                ("sample_rounds", C.c_uint32), ("sample_rounds_small", C.c_uint32),
                ("merge_kernel", C.c_uint32)]


class FpmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fpmash error {code}: {msg}")
        self.code = code


class SketchParams(C.Structure):
    """fpm_sketch_params == Sketch::Parameters subset (Sketch.h:40-113)."""
    _fields_ = [
        ("kmer_size", C.c_uint32),
        ("sketch_size", C.c_uint32),
        ("seed", C.c_uint32),
        ("use64", C.c_uint32),
        ("noncanonical", C.c_uint32),
        ("preserve_case", C.c_uint32),
        ("alphabet", C.c_uint8 * 256),
    ]


def make_params(k=21, s=1000, seed=42, alphabet=ALPHABET_NUCLEOTIDE, noncanonical=False,
                preserve_case=False, fingerprint=False, protein=False):
    """sketchParameterSetup (sketchParameterSetup.cpp:9-126) + setAlphabetFromString
    (Sketch.cpp:1260-1289)."""
    if fingerprint:                      # -fp: k=1, noncanonical, "0123456789"
        k, noncanonical, alphabet = 1, True, "0123456789"
    elif protein:
        noncanonical, alphabet = True, ALPHABET_PROTEIN
    P = SketchParams()
    P.kmer_size, P.sketch_size, P.seed = k, s, seed
    P.noncanonical, P.preserve_case = int(noncanonical), int(preserve_case)
    n = 0
    for ch in alphabet.encode():
        if not preserve_case and 96 < ch < 123:
            ch -= 32
        if not P.alphabet[ch]:
            n += 1
        P.alphabet[ch] = 1
    P.use64 = int(float(n) ** k > 2.0 ** 32)
    return P


_LIB = None


def build_id(path=None):
    """The build id a libfpmash.so carries (fpm_build_id: a hash of the sources it was
    compiled from), read from the file's "fpm-build-id:<id>" text without loading it, so a
    process that must not touch the GPU (tools/pmc_traffic.py) can stamp its profiles with it.
    None when the file is absent or carries no id."""
    import mmap
    import re
    path = path or LIB_PATH
    try:
        with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
            hit = re.search(rb"fpm-build-id:([0-9a-f]{16})", m)
            return bytes(hit.group(1)).decode() if hit else None
    except (OSError, ValueError):
        return None


def lib():
    """Load libfpmash.so (raises if the HIP build is absent: no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built (run `make -C fp-mash_amd`); "
                              "fpmash has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            # (an older build under FPMASH_LIB, a same-box A/B, may lack the newest entry
            # points; tests/test_abi.py checks the product exports every one)
            f = getattr(L, name, None)
            if f is None:
                continue
            f.restype = res
            f.argtypes = args
        _LIB = L
    return _LIB


def _check(rc):
    if rc != FPM_OK:
        raise FpmError(rc, lib().fpm_last_error().decode(errors="replace"))


def device_count():
    n = C.c_int(0)
    _check(lib().fpm_device_count(C.byref(n)))
    return n.value


def fp_text_limits():
    """(text bytes per newline-index workgroup, largest wave span fp_line_kernel stages in
    LDS, lines per head-count workgroup) of the -fp text kernels (fpm_fp_text_limits)."""
    c, s, h = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().fpm_fp_text_limits(C.byref(c), C.byref(s), C.byref(h))
    return c.value, s.value, h.value


def kfinger_limits():
    """(widest window, run length: window starts per workgroup) of the k-finger kernels
    (fpm_kfinger_limits)."""
    w, r = C.c_uint32(), C.c_uint32()
    lib().fpm_kfinger_limits(C.byref(w), C.byref(r))
    return w.value, r.value


def scan_limits():
    """(elements per scan block, the most blocks the two-launch form of the u32 exclusive scan
    takes: past their product it runs three launches) (fpm_scan_limits; a test hook)."""
    b, f = C.c_uint32(), C.c_uint32()
    lib().fpm_scan_limits(C.byref(b), C.byref(f))
    return b.value, f.value


KF_CFL, KF_ICFL, KF_CFL_ICFL = 0, 1, 2   # FPM_KF_*


def parse_factorization(name: str, max_threshold=None):
    """("CFL" | "ICFL" | "CFL_ICFL", T) of lyn2vec's --type_factorization spelling
    (lyn2vec.py:47-59): CFL, ICFL or CFL_ICFL-<T> with T >= 1 in plain decimal digits (and at
    most max_threshold, when given); ("CFL_COMB" | "ICFL_COMB" | "CFL_ICFL_COMB", T) of the
    combined forms CFL_COMB, ICFL_COMB and CFL_ICFL_COMB-<T> (lyn2vec.py:60-72) by the same
    rules; ValueError for anything else."""
    if name in ("CFL", "ICFL", "CFL_COMB", "ICFL_COMB"):
        return name, 0
    head, sep, t = name.partition("-")
    if head in ("CFL_ICFL", "CFL_ICFL_COMB") and sep and t.isascii() and t.isdigit() and \
            len(t) <= 9 and int(t) >= 1:
        if max_threshold is None or int(t) <= max_threshold:
            return head, int(t)
    raise ValueError(f"unknown factorization {name!r}: CFL, ICFL, CFL_ICFL-<T>, CFL_COMB, "
                     "ICFL_COMB or CFL_ICFL_COMB-<T>")


def kfinger_factorization(name):
    """(FPM_KF_* kind, threshold) of lyn2vec's spelling "CFL", "ICFL" or "CFL_ICFL-<T>"
    (lyn2vec.py:47-59), T from 1 to the widest window; (kind, threshold, 1) of the combined
    "CFL_COMB", "ICFL_COMB" or "CFL_ICFL_COMB-<T>" (the 1: fpm_kfinger_set_comb); ValueError for
    anything else."""
    kind, thr = parse_factorization(name, kfinger_limits()[0])
    comb = kind.endswith("_COMB")
    k = {"CFL": KF_CFL, "ICFL": KF_ICFL, "CFL_ICFL": KF_CFL_ICFL}[kind[:-5] if comb else kind]
    return (k, thr, 1) if comb else (k, thr)


def kfinger_lds_window(name):
    """the widest window whose working memory stays in LDS under the factorization of that
    spelling (fpm_kfinger_lds_window; no device needed): the next one keeps it in device memory"""
    kind, _thr, *comb = kfinger_factorization(name)
    w = C.c_uint32()
    _check(lib().fpm_kfinger_lds_window(kind, 1 if comb else 0, C.byref(w)))
    return w.value


def kfinger_id(header: bytes) -> bytes:
    """The ID of a record's k-finger lines from its header line (the bytes after '>' / '@'): the
    first whitespace-separated token of the kseq comment (lyn2vec's s_list[1]), or the record's
    name when the header has no comment, followed by "_0"."""
    tok = header.split(None, 2)
    if not tok or header[:1].isspace():
        # an empty kseq name: the whole line is the comment
        name, rest = b"", tok
    else:
        name, rest = tok[0], tok[1:]
    return (rest[0] if rest else name) + b"_0"


def kfinger_long_id(header: bytes) -> bytes:
    """The ID of a record's long-read line (kfinger split=N, `fpmash kfinger -L`) from its header
    line: the record's name, its first whitespace-separated token, with no "_0"."""
    if header[:1].isspace():
        return b""
    tok = header.split(None, 1)
    return tok[0] if tok else b""


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def pack_records(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), off


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = vp()
        _check(lib().fpm_malloc(ctx.h, C.byref(p), self.nbytes))
        self.ptr = p.value

    @classmethod
    def from_array(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        b = cls(ctx, arr.nbytes)
        _check(lib().fpm_memcpy_h2d(ctx.h, b.ptr, arr.ctypes.data, arr.nbytes))
        return b

    def to_array(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        _check(lib().fpm_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().fpm_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CellList:
    """Device buffers of a compact dist output's cell list (fpm_cell_list) with room for
    `cap` entries.  .struct is what the *_list_dev calls take (by reference)."""

    def __init__(self, ctx, cap):
        self.ctx, self.cap = ctx, int(max(cap, 1))
        self.bufs = [DeviceBuffer(ctx, self.cap * b) for b in (4, 4, 8, 8, 1)] + \
            [DeviceBuffer(ctx, 8)]
        q, r, d, p, a, c = (b.ptr for b in self.bufs)
        self.struct = CellListStruct(q, r, d, p, a, self.cap, c)

    @property
    def ref(self):
        return C.byref(self.struct)

    def count(self):
        """cells with numer > 0 the last call listed (may exceed cap: then re-run larger)"""
        return int(self.bufs[5].to_array(np.uint64, 1)[0])

    def fetch(self):
        """-> dict of the listed cells' qry, ref, distance, pvalue, pass (host arrays)"""
        n = self.count()
        if n > self.cap:
            raise FpmError(FPM_ENOMEM, f"cell list holds {self.cap} entries, {n} needed")
        m = max(n, 1)
        out = {k: b.to_array(t, m)[:n] for k, b, t in zip(
            ("qry", "ref", "distance", "pvalue", "pass"), self.bufs[:5],
            (np.uint32, np.uint32, np.float64, np.float64, np.uint8))}
        out["pass"] = out["pass"].astype(bool)
        return out

    def free(self):
        for b in self.bufs:
            b.free()


def expand_compact(numer, denom, listed, n_ref, max_dist=-1.0, max_pvalue=-1.0):
    """The five per-cell outputs of a compact result (fpm_dist_list_dev: counts of every
    cell + the list of cells with numer > 0), by the rule include/fpmash.h states: an unlisted
    cell has distance 0 if denom == 0 else 1, p-value 1, and the -d / -v filters at those
    values (CommandDistance.cpp:404-408, 435-437 at common = 0).  numer / denom: flat
    query-major arrays; listed: CellList.fetch()."""
    numer = np.asarray(numer)
    denom = np.asarray(denom)
    dist = np.where(denom == 0, 0.0, 1.0)
    pval = np.ones(len(numer), np.float64)
    ok = np.ones(len(numer), bool)
    if max_dist >= 0:
        ok &= dist <= max_dist
    if max_pvalue >= 0:
        ok &= 1.0 <= max_pvalue
    idx = listed["qry"].astype(np.int64) * n_ref + listed["ref"].astype(np.int64)
    if len(idx) and np.any(numer[idx] == 0):
        raise AssertionError("a listed cell has numer 0")
    if int(np.count_nonzero(numer)) != len(idx) or len(np.unique(idx)) != len(idx):
        raise AssertionError("the list is not exactly the cells with numer > 0")
    dist[idx] = listed["distance"]
    pval[idx] = listed["pvalue"]
    ok[idx] = listed["pass"]
    return {"numer": numer, "denom": denom, "distance": dist, "pvalue": pval, "pass": ok}


class SketchJob:
    """fpm_sketch_stage/run/fetch: inputs staged once in HBM, kernels re-runnable."""

    def __init__(self, ctx, params, seqs, groups=None, n_groups=None, min_copies=1):
        self.ctx, self.params = ctx, params
        if min_copies < 1:
            raise FpmError(FPM_EINVAL, "min_copies must be >= 1")
        data, off = pack_records(seqs)
        self._keep = (data, off)
        n_rec = len(seqs)
        if groups is not None:
            g = np.ascontiguousarray(groups, dtype=np.uint32)
            self.n_groups = int(n_groups if n_groups is not None else (int(g.max()) + 1 if n_rec else 0))
            gp = _p(g, u32p)
        else:
            self.n_groups, gp = n_rec, None
        h = vp()
        _check(lib().fpm_sketch_stage(ctx.h, C.byref(params), data, _p(off, u64p), n_rec, gp,
                                      self.n_groups, C.byref(h)))
        self.h = h.value
        if min_copies != 1:
            self.set_min_copies(min_copies)

    def run(self, stream=None):
        _check(lib().fpm_sketch_run(self.h, stream))

    # --- reads mode (sketch -r / -m N) ---
    def set_min_copies(self, min_copies):
        _check(lib().fpm_sketch_job_set_min_copies(self.h, min_copies))

    def run_reads(self, stream=None):
        """fpm_sketch_reads_run: the sketches of the hashes seen >= min_copies times."""
        _check(lib().fpm_sketch_reads_run(self.h, stream))

    def fetch_reads(self):
        """-> rows [n_groups, s] u64, counts per row u32, multiplicities [n_groups, s] u32,
        set-size estimates u64 (MinHashHeap::estimateSetSize; 0 for an empty sketch)."""
        s, n = int(self.params.sketch_size), self.n_groups
        out = np.zeros(max(n, 1) * s, dtype=np.uint64)
        cnt = np.zeros(max(n, 1), dtype=np.uint32)
        mult = np.zeros(max(n, 1) * s, dtype=np.uint32)
        est = np.zeros(max(n, 1), dtype=np.uint64)
        _check(lib().fpm_sketch_reads_fetch(self.h, _p(out, u64p), _p(cnt, u32p), _p(mult, u32p),
                                            _p(est, u64p)))
        return out[: n * s].reshape(n, s), cnt[:n], mult[: n * s].reshape(n, s), est[:n]

    def reads_rounds(self):
        """widening rounds of the last run_reads() (-1: none yet) and, per group, the round
        that completed it"""
        r = C.c_int32()
        per = np.zeros(max(self.n_groups, 1), dtype=np.uint32)
        _check(lib().fpm_sketch_job_reads_rounds(self.h, C.byref(r), _p(per, u32p)))
        return r.value, per[: self.n_groups]

    def reads_sampled(self):
        """long groups the last round's wide sketch of the last run_reads() sampled (-1: none
        yet)"""
        n = C.c_int32()
        _check(lib().fpm_sketch_job_reads_sampled(self.h, C.byref(n)))
        return n.value

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().fpm_sketch_job_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"seq_bytes": a.value, "n_tiles": b.value, "n_kmers": c.value}

    def redo_tiles(self):
        """tiles of the last run() the survivors-only kernel handed to the plain one (-1: the
        job does not use that kernel); waits for the device"""
        n = C.c_int32()
        _check(lib().fpm_sketch_job_redo_tiles(self.h, C.byref(n)))
        return n.value

    def short_groups(self):
        """long groups of the last run() redone under the sample's s-th smallest hash after
        the tight bound left them short (-1: no tight bounds in this job)"""
        n = C.c_int32()
        _check(lib().fpm_sketch_job_short_groups(self.h, C.byref(n)))
        return n.value

    def sample_short(self):
        """samples of the last run() the a-priori sample bound left short, redone unbounded
        (-1: the job's samples carry no such bound)"""
        n = C.c_int32()
        _check(lib().fpm_sketch_job_sample_short(self.h, C.byref(n)))
        return n.value

    def plan(self):
        """fpm_sketch_job_plan: the routes staging chose (a test hook) -> dict: tiles and
        sample_tiles per class (lists), thr4, n_slots, tight, n_ssel, n_sel, rounds,
        rounds_small, sample_rounds, sample_rounds_small, merge_kernel (MK_*)"""
        p = SketchPlan()
        _check(lib().fpm_sketch_job_plan(self.h, C.byref(p)))
        return self._plan_dict(p)

    @staticmethod
    def _plan_dict(p):
        out = {n: getattr(p, n) for n, _ in SketchPlan._fields_}
        out["tiles"], out["sample_tiles"] = list(p.tiles), list(p.sample_tiles)
        return out

    def reads_plan(self):
        """fpm_sketch_job_reads_plan: the plan (as plan()) of the wide job of the last round of
        the last run_reads() and that round's width (a test hook) -> (dict, width); FPM_EINVAL
        before any round"""
        p, w = SketchPlan(), C.c_uint32()
        _check(lib().fpm_sketch_job_reads_plan(self.h, C.byref(p), C.byref(w)))
        return self._plan_dict(p), w.value

    def device_output(self):
        dh, dc = vp(), vp()
        ng, st = C.c_uint32(), C.c_uint32()
        _check(lib().fpm_sketch_device_output(self.h, C.byref(dh), C.byref(dc), C.byref(ng),
                                              C.byref(st)))
        return dh.value, dc.value, ng.value, st.value

    def fetch(self):
        s = int(self.params.sketch_size)
        out = np.zeros(max(self.n_groups, 1) * s, dtype=np.uint64)
        cnt = np.zeros(max(self.n_groups, 1), dtype=np.uint32)
        _check(lib().fpm_sketch_fetch(self.h, _p(out, u64p), _p(cnt, u32p)))
        return out[: self.n_groups * s].reshape(self.n_groups, s), cnt[: self.n_groups]

    def mult(self, stream=None):
        """-M: fpm_sketch_mult -> [n_groups, s] u32 multiplicities (after run())."""
        s = int(self.params.sketch_size)
        out = np.zeros(max(self.n_groups, 1) * s, dtype=np.uint32)
        _check(lib().fpm_sketch_mult(self.h, stream, _p(out, u32p)))
        return out[: self.n_groups * s].reshape(self.n_groups, s)

    def free(self):
        if self.h:
            lib().fpm_sketch_job_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    """fpm_comm_unique_id: the 128-byte RCCL unique id one rank makes and the others receive
    over a host channel (bench.Group broadcasts it over gloo)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().fpm_comm_unique_id(buf))
    return buf.raw


class Comm:
    """fpm_comm: an RCCL communicator on the context's device and HIP runtime (the library's
    own), for the cross-GPU min-merge.  Blocks in the constructor until all nranks ranks
    have joined with the same id."""

    def __init__(self, ctx, nranks, rank, uid: bytes):
        if len(uid) != COMM_ID_BYTES:
            raise ValueError("RCCL unique id must be 128 bytes")
        h = vp()
        _check(lib().fpm_comm_create(ctx.h, int(nranks), int(rank), uid, C.byref(h)))
        self.h, self.ctx, self.nranks, self.rank = h.value, ctx, int(nranks), int(rank)

    def all_gather(self, d_send, d_recv, nbytes, stream=None):
        _check(lib().fpm_comm_all_gather(self.h, d_send, d_recv, int(nbytes), stream))

    def min_merge(self, d_row, d_count, s, d_out, d_out_count, stream=None):
        """fpm_sketch_min_merge_comm: every rank's bottom-s row gathered and merged on the
        device (enqueued on the stream)"""
        _check(lib().fpm_sketch_min_merge_comm(self.h, d_row, d_count, int(s), d_out,
                                               d_out_count, stream))

    def close(self):
        if self.h:
            lib().fpm_comm_destroy(self.h)
            self.h = None


def estimate_identity(common, denom, k):
    """estimateIdentity (CommandScreen.cpp:259-278), in double as the reference computes it"""
    if common == denom:
        return 1.0
    if common == 0:
        return 0.0
    return (float(common) / float(denom)) ** (1.0 / k)


class Screen:
    """fpm_screen: the table of one sketch database (rows: a 2-D u64 or u32 matrix, lens: the
    valid entries per row) with its pool counters and the pool's running bottom-s row."""

    def __init__(self, ctx, rows, lens, sketch_size):
        rows = np.ascontiguousarray(rows)
        if rows.dtype not in (np.uint64, np.uint32):
            raise ValueError("Screen: rows must be u64 or u32")
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        self.ctx, self.n, self.s = ctx, len(lens), int(sketch_size)
        self.use64 = rows.dtype == np.uint64
        self.sizes = lens.copy()
        stride = rows.shape[1] if rows.ndim == 2 else 0
        h = vp()
        _check(lib().fpm_screen_create(ctx.h, rows.ctypes.data, _p(lens, u32p), stride, self.n,
                                       rows.dtype.itemsize, self.s, C.byref(h)))
        self.h = h.value

    @classmethod
    def from_lists(cls, ctx, lists, sketch_size, use64=True):
        R, rl = _dense(lists, max([len(x) for x in lists] + [1]), np.uint64 if use64 else np.uint32)
        return cls(ctx, R[:len(lists)], rl[:len(lists)], sketch_size)

    def add_job(self, job, stream=None):
        """fpm_screen_add_job: one slice of the pool, a SketchJob staged as one group"""
        _check(lib().fpm_screen_add_job(self.h, job.h, stream))

    def add_records(self, params, recs):
        """one slice of the pool given as records: staged as one group, added, released"""
        job = SketchJob(self.ctx, params, recs, groups=[0] * len(recs), n_groups=1)
        try:
            self.add_job(job)
            self.ctx.synchronize()
        finally:
            job.free()

    def add_hashes(self, keys):
        """fpm_screen_add_hashes_dev over a host array of u64 keys"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        if not len(keys):
            return
        b = DeviceBuffer.from_array(self.ctx, keys)
        try:
            _check(lib().fpm_screen_add_hashes_dev(self.h, b.ptr, len(keys), None))
            self.ctx.synchronize()
        finally:
            b.free()

    def set_size(self):
        v = np.zeros(1, np.uint64)
        _check(lib().fpm_screen_set_size(self.h, _p(v, u64p)))
        return int(v[0])

    def counts(self):
        """-> (U, the sorted distinct union of the rows as u64; its u32 counters)"""
        n = np.zeros(1, np.uint64)
        _check(lib().fpm_screen_counts(self.h, None, None, _p(n, u64p)))
        n = int(n[0])
        U, c = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
        nn = np.zeros(1, np.uint64)
        _check(lib().fpm_screen_counts(self.h, _p(U, u64p), _p(c, u32p), _p(nn, u64p)))
        return U[:n], c[:n]

    def rows(self):
        """-> (shared, median) per reference, u32"""
        sh, me = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.uint32)
        _check(lib().fpm_screen_rows(self.h, _p(sh, u32p), _p(me, u32p)))
        return sh[:self.n], me[:self.n]

    def rows_winner(self, scores, lengths):
        """-w -> (shared, median) over the entries each reference won"""
        sc = np.ascontiguousarray(scores, dtype=np.float64)
        le = np.ascontiguousarray(lengths, dtype=np.uint64)
        if len(sc) != self.n or len(le) != self.n:
            raise ValueError("rows_winner: one score and one length per reference")
        sh, me = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.uint32)
        _check(lib().fpm_screen_rows_winner(self.h, _p(sc, f64p), _p(le, u64p), _p(sh, u32p),
                                            _p(me, u32p)))
        return sh[:self.n], me[:self.n]

    def pvalues(self, shared, kmer_space):
        sh = np.ascontiguousarray(shared, dtype=np.uint32)
        out = np.zeros(max(self.n, 1), np.float64)
        _check(lib().fpm_screen_pvalues(self.h, _p(sh, u32p), float(kmer_space), _p(out, f64p)))
        return out[:self.n]

    def tax(self, parent, top, ref_node, lca=True):
        """fpm_screen_tax: parent (u32 per node, TAX_ROOT for a root), top (the node of taxID 1
        or TAX_UNKNOWN), ref_node (u32 per reference: a node, TAX_NONE or TAX_UNKNOWN) -> dict:
        lca (u32 per entry of U; None with lca=False), tax_hashes, tax_count, clade_hashes,
        clade_count (u32 per node), total_count, total_hashes"""
        parent = np.ascontiguousarray(parent, dtype=np.uint32)
        ref_node = np.ascontiguousarray(ref_node, dtype=np.uint32)
        if len(ref_node) != self.n:
            raise ValueError("tax: one ref_node per reference")
        n = len(parent)
        nu = np.zeros(1, np.uint64)
        _check(lib().fpm_screen_counts(self.h, None, None, _p(nu, u64p)))
        nu = int(nu[0])
        out = np.zeros(max(nu, 1), np.uint32) if lca else None
        arr = [np.zeros(max(n, 1), np.uint32) for _ in range(4)]
        tot = np.zeros(2, np.uint64)
        _check(lib().fpm_screen_tax(self.h, _p(parent, u32p), n, int(top), _p(ref_node, u32p),
                                    _p(out, u32p) if lca else None, _p(arr[0], u32p),
                                    _p(arr[1], u32p), _p(arr[2], u32p), _p(arr[3], u32p),
                                    _p(tot, u64p)))
        return {"lca": out[:nu] if lca else None, "tax_hashes": arr[0][:n],
                "tax_count": arr[1][:n], "clade_hashes": arr[2][:n], "clade_count": arr[3][:n],
                "total_count": int(tot[0]), "total_hashes": int(tot[1])}

    def table_info(self):
        """fpm_screen_table_info: what the build chose (a test hook) -> dict: cells, n_distinct,
        sbits (sort bucket bits), dbits (directory bits)"""
        e, n = C.c_uint64(), C.c_uint64()
        sb, db = C.c_uint32(), C.c_uint32()
        _check(lib().fpm_screen_table_info(self.h, C.byref(e), C.byref(n), C.byref(sb),
                                           C.byref(db)))
        return {"cells": e.value, "n_distinct": n.value, "sbits": sb.value, "dbits": db.value}

    def free(self):
        if self.h:
            lib().fpm_screen_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One gfx950 device (fpm_ctx)."""

    def __init__(self, device=0):
        h = vp()
        _check(lib().fpm_ctx_create(device, C.byref(h)))
        self.h = h.value
        self.device = device

    def close(self):
        if self.h:
            lib().fpm_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def stream(self):
        return lib().fpm_ctx_stream(self.h)

    def synchronize(self):
        _check(lib().fpm_ctx_synchronize(self.h))

    def new_stream(self):
        """fpm_stream_create: a non-blocking stream of the library's runtime (free with
        free_stream)."""
        s = vp()
        _check(lib().fpm_stream_create(self.h, C.byref(s)))
        return s.value

    def free_stream(self, s):
        _check(lib().fpm_stream_destroy(self.h, s))

    def new_event(self):
        e = vp()
        _check(lib().fpm_event_create(self.h, C.byref(e)))
        return e.value

    def free_event(self, e):
        _check(lib().fpm_event_destroy(self.h, e))

    def record(self, event, stream):
        _check(lib().fpm_event_record(self.h, event, stream))

    def wait(self, stream, event):
        _check(lib().fpm_stream_wait_event(self.h, stream, event))

    def set_timing(self, on=True):
        _check(lib().fpm_ctx_set_timing(self.h, int(on)))

    def reset_timing(self):
        _check(lib().fpm_ctx_reset_timing(self.h))

    def kernel_time(self, kernel):
        t, n = C.c_double(), C.c_uint64()
        _check(lib().fpm_ctx_kernel_time(self.h, kernel, C.byref(t), C.byref(n)))
        return t.value, n.value

    def exscan_dev(self, d_in, n, d_out, d_out2=None, d_total=None):
        """fpm_exscan_dev: the library's u32 exclusive scan over device pointers (d_out2 and
        d_total may be None; a test hook; synchronises)"""
        _check(lib().fpm_exscan_dev(self.h, d_in, int(n), d_out, d_out2, d_total))

    def merge_small_spills(self):
        """fpm_merge_small_spills: small-list merges that overflowed the LDS cap (resets)."""
        v = np.zeros(1, np.uint64)
        _check(lib().fpm_merge_small_spills(self.h, _p(v, u64p)))
        return int(v[0])

    def set_dist_mode(self, mode):
        _check(lib().fpm_ctx_set_dist_mode(self.h, mode))

    def index_rebuilds(self):
        """one-pass index builds redone by the exact build (a level-1 slot overflowed)"""
        v = C.c_uint64()
        _check(lib().fpm_ctx_index_rebuilds(self.h, C.byref(v)))
        return v.value

    def spec_stats(self):
        """(kept, dropped) speculated probes since the context was created (fpm_ctx_spec_stats)"""
        h, m = C.c_uint64(), C.c_uint64()
        _check(lib().fpm_ctx_spec_stats(self.h, C.byref(h), C.byref(m)))
        return h.value, m.value

    def last_dist_stats(self):
        sp, ev, ca = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(lib().fpm_ctx_last_dist_stats(self.h, C.byref(sp), C.byref(ev), C.byref(ca)))
        return {"sparse": sp.value, "events": ev.value, "candidates": ca.value}

    def last_dist_kernel(self):
        """fpm_ctx_last_dist_kernel: the compare kernel of the last compare (a DK_* code; a
        test hook)"""
        k = C.c_int()
        _check(lib().fpm_ctx_last_dist_kernel(self.h, C.byref(k)))
        return k.value

    def set_probe_half(self, on=True):
        """fpm_ctx_set_probe_half: the symmetric self probe reads only the first half of each
        row (default on; same results)"""
        _check(lib().fpm_ctx_set_probe_half(self.h, int(on)))

    def last_dist_probe(self):
        """fpm_ctx_last_dist_probe: the form of the last compare's row probe (a PROBE_* code;
        a test hook)"""
        f = C.c_int()
        _check(lib().fpm_ctx_last_dist_probe(self.h, C.byref(f)))
        return f.value

    def set_index_cut(self, on=True):
        """fpm_ctx_set_index_cut: the index of one sorted set against itself leaves out the
        hashes no half probe can reach (default on; same results)"""
        _check(lib().fpm_ctx_set_index_cut(self.h, int(on)))

    def last_index_cut(self):
        """fpm_ctx_last_index_cut: {"cut": whether the last compare's index was cut, "indexed":
        the entries it holds, "entries": the entries its rows hold} (a test hook)"""
        c, i, e = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(lib().fpm_ctx_last_index_cut(self.h, C.byref(c), C.byref(i), C.byref(e)))
        return {"cut": bool(c.value), "indexed": i.value, "entries": e.value}

    def set_rank_compact(self, on=True):
        """fpm_ctx_set_rank_compact: the candidates of one sorted set against itself are ranked
        on rows without the probed hashes no other row holds (default on; same results)"""
        _check(lib().fpm_ctx_set_rank_compact(self.h, int(on)))

    def set_poison(self, byte):
        """fpm_ctx_set_poison: every device buffer the library hands out is first filled with
        `byte` (0..255; -1 or None turns it off; a test hook)"""
        _check(lib().fpm_ctx_set_poison(self.h, -1 if byte is None else int(byte)))

    def poison_now(self):
        """fpm_ctx_poison_now: fills the context's scratch slots and the free buffers of its
        pool with the poison byte (synchronises; an error while poison is off; a test hook)"""
        _check(lib().fpm_ctx_poison_now(self.h))

    def last_rank_compact(self):
        """fpm_ctx_last_rank_compact: {"compact": whether the last compare ranked compacted
        rows, "kept": the entries those hold, "entries": the entries of the rows themselves}
        (a test hook; synchronises)"""
        c, k, e = C.c_int(), C.c_uint64(), C.c_uint64()
        _check(lib().fpm_ctx_last_rank_compact(self.h, C.byref(c), C.byref(k), C.byref(e)))
        return {"compact": bool(c.value), "kept": k.value, "entries": e.value}

    # --- sketch -----------------------------------------------------------
    def sketch(self, params, seqs, groups=None, n_groups=None, counts=False, min_copies=1):
        """-> list of ascending u64 arrays (one per sketch); counts=True (-M): also the list
        of their u32 multiplicities.  min_copies > 1: reads mode, only hashes seen at least
        min_copies times (sketch_reads has the estimates too)."""
        if min_copies != 1:
            r = self.sketch_reads(params, seqs, groups, n_groups, min_copies)
            return (r["hashes"], r["counts"]) if counts else r["hashes"]
        job = SketchJob(self, params, seqs, groups, n_groups)
        try:
            job.run()
            rows, cnt = job.fetch()
            mult = job.mult() if counts else None
        finally:
            job.free()
        hashes = [rows[i, : cnt[i]].copy() for i in range(len(cnt))]
        if counts:
            return hashes, [mult[i, : cnt[i]].copy() for i in range(len(cnt))]
        return hashes

    def sketch_job(self, params, seqs, groups=None, n_groups=None, min_copies=1):
        return SketchJob(self, params, seqs, groups, n_groups, min_copies)

    @staticmethod
    def _reads_result(job):
        job.run_reads()
        rows, cnt, mult, est = job.fetch_reads()
        rounds, per = job.reads_rounds()
        plan, width = job.reads_plan() if rounds > 0 else (None, 0)      # no groups: no round
        return {"plan": plan, "width": width, "hashes": [rows[i, : cnt[i]].copy() for i in range(len(cnt))],
                "counts": [mult[i, : cnt[i]].copy() for i in range(len(cnt))],
                "estimate": est.copy(), "rounds": rounds, "group_round": per,
                "sampled": job.reads_sampled()}

    def sketch_reads(self, params, seqs, groups=None, n_groups=None, min_copies=1):
        """Reads mode (sketch -r -m min_copies): per group the s smallest hashes seen at least
        min_copies times -> dict of hashes, counts (lists of arrays), estimate (u64 set-size
        estimates), rounds and group_round (the widening rounds hook), plan and width (the
        last round's wide job, SketchJob.reads_plan)."""
        job = SketchJob(self, params, seqs, groups, n_groups, min_copies)
        try:
            return self._reads_result(job)
        finally:
            job.free()

    # --- FASTA text on the device -------------------------------------------------
    def seq_parse(self, files):
        """fpm_seq_parse over file images -> (handle, records dict, quality_lines flag).
        records: seg, hdr_off, hdr_len, seq_len per record (kseq record rules)."""
        n_seg = len(files)
        ptrs = (C.c_char_p * max(n_seg, 1))(*files)
        lens = np.array([len(f) for f in files] + [0], dtype=np.uint64)
        job, n, q = vp(), C.c_uint64(), C.c_int()
        _check(lib().fpm_seq_parse(self.h, ptrs, _p(lens, u64p), n_seg, C.byref(job),
                                   C.byref(n), C.byref(q)))
        n = n.value
        seg = np.zeros(max(n, 1), np.uint32)
        ho, hl, sl = (np.zeros(max(n, 1), np.uint64) for _ in range(3))
        try:
            _check(lib().fpm_seq_records(job, _p(seg, u32p), _p(ho, u64p), _p(hl, u64p),
                                         _p(sl, u64p)))
        except Exception:
            lib().fpm_seq_free(job)
            raise
        return job.value, {"seg": seg[:n], "hdr_off": ho[:n], "hdr_len": hl[:n],
                           "seq_len": sl[:n]}, bool(q.value)

    def seq_packed(self, seq_job, n_rec=None, cap=None):
        """fpm_seq_packed: the packed records of a parse handle that has not been staged (a
        test hook) -> (bytes, seq_off): every record's sequence bytes and one 0x00, and each
        record's offset.  n_rec: the record count seq_parse returned (default: the 0x00 bytes
        of the buffer, sequence bytes being isgraph); cap: the buffer size handed over
        (default: the size the call reports)."""
        nb = C.c_uint64()
        _check(lib().fpm_seq_packed(seq_job, None, None, 0, C.byref(nb)))
        size = nb.value if cap is None else cap
        out = np.zeros(max(size, 1), np.uint8)
        # one offset per record; the packed size bounds the record count (a 0x00 each)
        off = np.zeros(max(nb.value, 1), np.uint64)
        _check(lib().fpm_seq_packed(seq_job, _p(off, u64p), _p(out, u8p), size, C.byref(nb)))
        if n_rec is None:
            n_rec = int(np.count_nonzero(out[:nb.value] == 0))
        return out[:nb.value].tobytes(), off[:n_rec].copy()

    def sketch_seq_job(self, params, seq_job, groups, n_groups):
        """fpm_sketch_stage_seq: the staged SketchJob over parsed records (it takes the packed
        records; free it, and the parse handle with seq_free, afterwards)."""
        g = np.ascontiguousarray(groups, dtype=np.uint32)
        if g.size == 0:
            g = np.zeros(1, np.uint32)
        h = vp()
        _check(lib().fpm_sketch_stage_seq(self.h, C.byref(params), seq_job, _p(g, u32p),
                                          n_groups, C.byref(h)))
        job = SketchJob.__new__(SketchJob)
        job.ctx, job.params, job.n_groups, job.h, job._keep = self, params, n_groups, h.value, None
        return job

    def sketch_seq(self, params, seq_job, groups, n_groups, counts=False, min_copies=1):
        """fpm_sketch_stage_seq + run + fetch over parsed records (the job takes the packed
        records; free the parse handle with seq_free afterwards).  min_copies > 1: reads mode,
        only hashes seen at least min_copies times."""
        job = self.sketch_seq_job(params, seq_job, groups, n_groups)
        if min_copies != 1:
            try:
                job.set_min_copies(min_copies)
                r = self._reads_result(job)
            finally:
                job.free()
            return (r["hashes"], r["counts"]) if counts else r["hashes"]
        try:
            job.run()
            rows, cnt = job.fetch()
            mult = job.mult() if counts else None
        finally:
            job.free()
        hashes = [rows[i, : cnt[i]].copy() for i in range(len(cnt))]
        if counts:
            return hashes, [mult[i, : cnt[i]].copy() for i in range(len(cnt))]
        return hashes

    @staticmethod
    def seq_free(seq_job):
        lib().fpm_seq_free(seq_job)

    # --- -fp ----------------------------------------------------------------
    def fp_hash_lines(self, values_per_line, seed=42, use64=False):
        off = np.zeros(len(values_per_line) + 1, dtype=np.uint64)
        if values_per_line:
            off[1:] = np.cumsum([len(v) for v in values_per_line])
        vals = (np.concatenate([np.asarray(v, dtype=np.uint64) for v in values_per_line])
                if values_per_line else np.zeros(0, np.uint64))
        return self.fp_hash_flat(vals, off, seed, use64)

    def fp_hash_flat(self, vals, line_off, seed=42, use64=False):
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        line_off = np.ascontiguousarray(line_off, dtype=np.uint64)
        n = len(line_off) - 1
        out = np.zeros(max(n, 1), dtype=np.uint64 if use64 else np.uint32)
        if vals.size == 0:
            vals = np.zeros(1, np.uint64)
        _check(lib().fpm_fp_hash_lines(self.h, _p(vals, u64p), _p(line_off, u64p), n, seed,
                                       int(use64), out.ctypes.data))
        return out[:n]

    # --- dist ---------------------------------------------------------------
    def dist(self, ref_lists, qry_lists, sketch_size, use64=True, k=21, kmer_space=None,
             ref_lengths=None, qry_lengths=None, max_dist=-1.0, max_pvalue=-1.0,
             finalize=True):
        """All pairs, query-major: returns dict of flat arrays (index q*n_ref + r)."""
        dt = np.uint64 if use64 else np.uint32
        w = max([len(x) for x in list(ref_lists) + list(qry_lists)] + [1])
        R, rl = _dense(ref_lists, w, dt)
        # the same list object on both sides: one upload, and the library may use the
        # pair symmetry of one set against itself
        Q, ql = (R, rl) if qry_lists is ref_lists else _dense(qry_lists, w, dt)
        n = len(ref_lists) * len(qry_lists)
        nu = np.zeros(max(n, 1), np.uint32)
        de = np.zeros(max(n, 1), np.uint32)
        if not finalize:
            _check(lib().fpm_compare_grid(self.h, R.ctypes.data, _p(rl, u32p), w, len(ref_lists),
                                          Q.ctypes.data, _p(ql, u32p), w, len(qry_lists),
                                          8 if use64 else 4, sketch_size, _p(nu, u32p),
                                          _p(de, u32p)))
            return {"numer": nu[:n], "denom": de[:n]}
        if kmer_space is None:
            kmer_space = 4.0 ** k
        rL = np.ascontiguousarray(ref_lengths, dtype=np.uint64)
        qL = np.ascontiguousarray(qry_lengths, dtype=np.uint64)
        di = np.zeros(max(n, 1), np.float64)
        pv = np.zeros(max(n, 1), np.float64)
        pa = np.zeros(max(n, 1), np.uint8)
        _check(lib().fpm_dist(self.h, R.ctypes.data, _p(rl, u32p), _p(rL, u64p), w,
                              len(ref_lists), Q.ctypes.data, _p(ql, u32p), _p(qL, u64p), w,
                              len(qry_lists), 8 if use64 else 4, sketch_size, k, kmer_space,
                              max_dist, max_pvalue, _p(nu, u32p), _p(de, u32p), _p(di, f64p),
                              _p(pv, f64p), _p(pa, u8p)))
        return {"numer": nu[:n], "denom": de[:n], "distance": di[:n], "pvalue": pv[:n],
                "pass": pa[:n].astype(bool)}

    # --- contain ------------------------------------------------------------
    def set_contain_mode(self, mode):
        """fpm_ctx_set_contain_mode: CONTAIN_AUTO, or CONTAIN_LITERAL to force the literal walk
        (same results)"""
        _check(lib().fpm_ctx_set_contain_mode(self.h, mode))

    def last_contain_kernel(self):
        """fpm_ctx_last_contain_kernel: the kernel of the last contain call (a CK_* code; a
        test hook)"""
        k = C.c_int()
        _check(lib().fpm_ctx_last_contain_kernel(self.h, C.byref(k)))
        return k.value

    def contain_lds_cap(self, use64=True):
        """fpm_contain_lds_cap: the longest query row contain_rows_kernel stages in LDS"""
        v = np.zeros(1, np.uint32)
        _check(lib().fpm_contain_lds_cap(self.h, 8 if use64 else 4, _p(v, u32p)))
        return int(v[0])

    def contain_rows(self, R, ref_len, Q, qry_len):
        """fpm_contain on dense row matrices (2-D u64 or u32 arrays, row stride = their width)
        -> dict of flat query-major u32 arrays (index q*n_ref + r): common, steps"""
        R, Q = np.ascontiguousarray(R), np.ascontiguousarray(Q)
        if R.dtype != Q.dtype or R.dtype not in (np.uint64, np.uint32):
            raise ValueError("contain_rows: both matrices u64 or both u32")
        rl = np.ascontiguousarray(ref_len, dtype=np.uint32)
        ql = np.ascontiguousarray(qry_len, dtype=np.uint32)
        nr, nq = len(rl), len(ql)
        n = nr * nq
        co = np.zeros(max(n, 1), np.uint32)
        stp = np.zeros(max(n, 1), np.uint32)
        _check(lib().fpm_contain(self.h, R.ctypes.data, _p(rl, u32p), R.shape[1] if R.ndim == 2 else 0,
                                 nr, Q.ctypes.data, _p(ql, u32p), Q.shape[1] if Q.ndim == 2 else 0,
                                 nq, R.dtype.itemsize, _p(co, u32p), _p(stp, u32p)))
        return {"common": co[:n], "steps": stp[:n]}

    def contain(self, ref_lists, qry_lists, use64=True):
        """All pairs of containSketches (CommandContain.cpp:368-412), query-major: common and
        steps (the walk's final j); score = common / steps, error bound = 1 / sqrt(steps)."""
        dt = np.uint64 if use64 else np.uint32
        R, rl = _dense(ref_lists, max([len(x) for x in ref_lists] + [1]), dt)
        Q, ql = _dense(qry_lists, max([len(x) for x in qry_lists] + [1]), dt)
        return self.contain_rows(R, rl[:len(ref_lists)], Q, ql[:len(qry_lists)])

    def contain_dev(self, d_ref, d_ref_len, ref_stride, n_ref, d_qry, d_qry_len, qry_stride,
                    n_qry, use64, d_common, d_steps, stream=None):
        """fpm_contain_dev on device pointers (stream-ordered after its one read-back)"""
        _check(lib().fpm_contain_dev(self.h, d_ref, d_ref_len, ref_stride, n_ref, d_qry,
                                     d_qry_len, qry_stride, n_qry, 8 if use64 else 4, d_common,
                                     d_steps, stream))

    # --- screen -------------------------------------------------------------
    def last_screen_kernel(self):
        """fpm_ctx_last_screen_kernel: the screen_rows_kernel instance of the last rows call (an
        SK_* code; a test hook)"""
        k = C.c_int()
        _check(lib().fpm_ctx_last_screen_kernel(self.h, C.byref(k)))
        return k.value

    def screen_lds_cap(self):
        """fpm_screen_lds_cap: the longest reference row screen_rows_kernel holds in LDS"""
        v = np.zeros(1, np.uint32)
        _check(lib().fpm_screen_lds_cap(self.h, _p(v, u32p)))
        return int(v[0])

    def last_tax_kernel(self):
        """fpm_ctx_last_tax_kernel: how the last Screen.tax folded its posting lists (a TK_*
        code; a test hook)"""
        k = C.c_int()
        _check(lib().fpm_ctx_last_tax_kernel(self.h, C.byref(k)))
        return k.value

    def tax_wave_cut(self):
        """fpm_screen_tax_wave_cut: the holders from which a posting list is folded by a wave"""
        v = np.zeros(1, np.uint32)
        _check(lib().fpm_screen_tax_wave_cut(self.h, _p(v, u32p)))
        return int(v[0])

    def taxscreen(self, params, db_lists, pool, parent, top, ref_node, slices=1):
        """`mash taxscreen` without its files: the pool pass of screen(), then Screen.tax over
        the taxonomy (parent, top) and the references' nodes -> Screen.tax's dict plus
        set_size."""
        s = int(params.sketch_size)
        sc = Screen.from_lists(self, [l[:s] for l in db_lists], s, use64=bool(params.use64))
        try:
            step = max(1, -(-len(pool) // max(slices, 1)))
            for at in range(0, len(pool), step):
                sc.add_records(params, pool[at:at + step])
            r = sc.tax(parent, top, ref_node)
            r["set_size"] = sc.set_size()
            return r
        finally:
            sc.free()

    def screen(self, params, db_lists, pool, lengths=None, winner=False, slices=1):
        """The documented `mash screen` over a database (lists of ascending hashes, cut to the
        sketch size) and a pool of records, given to the device in `slices` parts -> dict:
        shared, median, size (u32 per reference), identity, pvalue (float64), set_size.
        winner: -w, with lengths the references' Reference::length."""
        k, s = int(params.kmer_size), int(params.sketch_size)
        n_alpha = int(sum(params.alphabet))
        sc = Screen.from_lists(self, [l[:s] for l in db_lists], s, use64=bool(params.use64))
        try:
            step = max(1, -(-len(pool) // max(slices, 1)))
            for at in range(0, len(pool), step):
                sc.add_records(params, pool[at:at + step])
            shared, median = sc.rows()
            if winner:
                scores = [estimate_identity(int(c), int(d), k) for c, d in zip(shared, sc.sizes)]
                shared, median = sc.rows_winner(scores, lengths if lengths is not None
                                                else [0] * sc.n)
            pv = sc.pvalues(shared, float(n_alpha) ** k)
            ident = np.array([estimate_identity(int(c), int(d), k)
                              for c, d in zip(shared, sc.sizes)], np.float64)
            return {"shared": shared, "median": median, "size": sc.sizes.copy(),
                    "identity": ident, "pvalue": pv, "set_size": sc.set_size()}
        finally:
            sc.free()

    def dist16(self, ref_lists, qry_lists, sketch_size, use64=True, k=21, kmer_space=None,
               ref_lengths=None, qry_lengths=None, max_dist=-1.0, max_pvalue=-1.0):
        """dist() through fpm_dist_dev16 (device buffers, u16 numer / denom cells)."""
        dt = np.uint64 if use64 else np.uint32
        w = max([len(x) for x in list(ref_lists) + list(qry_lists)] + [1])
        R, rl = _dense(ref_lists, w, dt)
        Q, ql = (R, rl) if qry_lists is ref_lists else _dense(qry_lists, w, dt)
        nr, nq = len(ref_lists), len(qry_lists)
        n = nr * nq
        if kmer_space is None:
            kmer_space = 4.0 ** k
        bufs = []

        def up(a):
            b = DeviceBuffer.from_array(self, a)
            bufs.append(b)
            return b.ptr
        try:
            dR, drl = up(R), up(rl)
            dQ, dql = (dR, drl) if qry_lists is ref_lists else (up(Q), up(ql))
            drL = up(np.ascontiguousarray(ref_lengths, dtype=np.uint64))
            dqL = drL if qry_lists is ref_lists and qry_lengths is ref_lengths else \
                up(np.ascontiguousarray(qry_lengths, dtype=np.uint64))
            outs = [DeviceBuffer(self, max(n, 1) * b) for b in (2, 2, 8, 8, 1)]
            bufs += outs
            _check(lib().fpm_dist_dev16(self.h, dR, drl, drL, w, nr, dQ, dql, dqL, w, nq,
                                        8 if use64 else 4, sketch_size, k, kmer_space, max_dist,
                                        max_pvalue, *[o.ptr for o in outs], None))
            self.synchronize()
            res = [o.to_array(t, n) for o, t in zip(outs, (np.uint16, np.uint16, np.float64,
                                                           np.float64, np.uint8))]
        finally:
            for b in bufs:
                b.free()
        return {"numer": res[0], "denom": res[1], "distance": res[2], "pvalue": res[3],
                "pass": res[4].astype(bool)}

    def dist_list(self, ref_lists, qry_lists, sketch_size, use64=True, k=21, kmer_space=None,
                  ref_lengths=None, qry_lengths=None, max_dist=-1.0, max_pvalue=-1.0, cap=None,
                  expand=True, prefill=False):
        """dist() through fpm_dist_list_dev (the compact output: u16 counts + the list of
        cells with numer > 0).  expand=True: the five per-cell arrays (expand_compact), else
        (numer, denom, listed).  prefill=True: the counts prefilled first
        (fpm_dist_list_prefill, taken over by the dist call)."""
        dt = np.uint64 if use64 else np.uint32
        w = max([len(x) for x in list(ref_lists) + list(qry_lists)] + [1])
        R, rl = _dense(ref_lists, w, dt)
        Q, ql = (R, rl) if qry_lists is ref_lists else _dense(qry_lists, w, dt)
        nr, nq = len(ref_lists), len(qry_lists)
        n = nr * nq
        if kmer_space is None:
            kmer_space = 4.0 ** k
        bufs = []

        def up(a):
            b = DeviceBuffer.from_array(self, a)
            bufs.append(b)
            return b.ptr
        lst = None
        try:
            dR, drl = up(R), up(rl)
            dQ, dql = (dR, drl) if qry_lists is ref_lists else (up(Q), up(ql))
            drL = up(np.ascontiguousarray(ref_lengths, dtype=np.uint64))
            dqL = drL if qry_lists is ref_lists and qry_lengths is ref_lengths else \
                up(np.ascontiguousarray(qry_lengths, dtype=np.uint64))
            outs = [DeviceBuffer(self, max(n, 1) * 2) for _ in range(2)]
            bufs += outs
            lst = CellList(self, cap if cap is not None else max(n, 1))
            if prefill:
                _check(lib().fpm_dist_list_prefill(self.h, outs[0].ptr, outs[1].ptr, nr, nq,
                                                   sketch_size, None))
            _check(lib().fpm_dist_list_dev(self.h, dR, drl, drL, w, nr, dQ, dql, dqL, w, nq,
                                           8 if use64 else 4, sketch_size, k, kmer_space,
                                           max_dist, max_pvalue, outs[0].ptr, outs[1].ptr,
                                           lst.ref, None))
            self.synchronize()
            nu, de = (o.to_array(np.uint16, n) for o in outs)
            listed = lst.fetch()
        finally:
            for b in bufs:
                b.free()
            if lst is not None:
                lst.free()
        if not expand:
            return nu, de, listed
        return expand_compact(nu, de, listed, nr, max_dist, max_pvalue)

    def pvalue_batch(self, numer, denom, len_ref, len_qry, k=21, kmer_space=None):
        """fpm_pvalue_batch_dev on host arrays: (distance, p-value) of each cell from its
        counts (u16 or u32) and genome lengths."""
        numer = np.ascontiguousarray(numer)
        denom = np.ascontiguousarray(denom, dtype=numer.dtype)
        if numer.dtype not in (np.uint16, np.uint32):
            raise ValueError("counts must be uint16 or uint32")
        n = len(numer)
        if kmer_space is None:
            kmer_space = 4.0 ** k
        bufs = [DeviceBuffer.from_array(self, a) for a in
                (numer, denom, np.ascontiguousarray(len_ref, dtype=np.uint64),
                 np.ascontiguousarray(len_qry, dtype=np.uint64))]
        outs = [DeviceBuffer(self, max(n, 1) * 8) for _ in range(2)]
        try:
            _check(lib().fpm_pvalue_batch_dev(self.h, bufs[0].ptr, bufs[1].ptr,
                                              numer.dtype.itemsize, bufs[2].ptr, bufs[3].ptr, n,
                                              k, kmer_space, outs[0].ptr, outs[1].ptr, None))
            self.synchronize()
            return outs[0].to_array(np.float64, n), outs[1].to_array(np.float64, n)
        finally:
            for b in bufs + outs:
                b.free()

    def refset(self, ref_lists, sketch_size, use64=True, ref_lengths=None, width=None):
        """A resident reference set (fpm_refset_create): rows uploaded and indexed once."""
        return RefSet(self, ref_lists, sketch_size, use64, ref_lengths, width)

    def fp_text(self, text, max_lines=1_000_000, seed=42, use64=False):
        """-fp file image -> per line: ID (offset, length), value count, hash, new-ID flag."""
        job, n = vp(), C.c_uint64()
        _check(lib().fpm_fp_text_stage(self.h, text, len(text), max_lines, seed, int(use64),
                                       C.byref(job), C.byref(n)))
        n = n.value
        io = np.zeros(max(n, 1), np.uint64)
        il = np.zeros(max(n, 1), np.uint32)
        nv = np.zeros(max(n, 1), np.uint32)
        h = np.zeros(max(n, 1), np.uint64 if use64 else np.uint32)
        ni = np.zeros(max(n, 1), np.uint8)
        try:
            _check(lib().fpm_fp_text_fetch(job, _p(io, u64p), _p(il, u32p), _p(nv, u32p),
                                           h.ctypes.data, _p(ni, u8p)))
        finally:
            lib().fpm_fp_text_free(job)
        return {"id_off": io[:n], "id_len": il[:n], "n_vals": nv[:n], "hash": h[:n],
                "new_id": ni[:n]}

    def fp_refs(self, text, max_lines=1_000_000, seed=42, use64=False):
        """-fp file image -> its References as initFromFingerprints groups them (Sketch.cpp:
        104-145), grouped on the device (fpm_fp_text_refs): first line, ID (offset, length in
        the text), length, and the line hashes (the only per-line fetch)."""
        job, n = vp(), C.c_uint64()
        _check(lib().fpm_fp_text_stage(self.h, text, len(text), max_lines, seed, int(use64),
                                       C.byref(job), C.byref(n)))
        n = n.value
        try:
            nr = C.c_uint64()
            _check(lib().fpm_fp_text_refs(job, 0, C.byref(nr), None, None, None, None))
            m = nr.value
            first = np.zeros(max(m, 1), np.uint64)
            io = np.zeros(max(m, 1), np.uint64)
            il = np.zeros(max(m, 1), np.uint32)
            ln = np.zeros(max(m, 1), np.uint64)
            if m:
                _check(lib().fpm_fp_text_refs(job, m, C.byref(nr), _p(first, u64p), _p(io, u64p),
                                              _p(il, u32p), _p(ln, u64p)))
            h = np.zeros(max(n, 1), np.uint64 if use64 else np.uint32)
            _check(lib().fpm_fp_text_fetch(job, None, None, None, h.ctypes.data, None))
        finally:
            lib().fpm_fp_text_free(job)
        return {"first": first[:m], "id_off": io[:m], "id_len": il[:m], "length": ln[:m],
                "hash": h[:n], "n_lines": n}

    # --- k-fingers from sequence ----------------------------------------------------
    @staticmethod
    def _kfinger_out(job, n, n_rec, seed, use64, ids, values, text, fact=(KF_CFL, 0),
                     fact_text=False):
        """run + fetch (+ the pass-two outputs) of a staged k-finger job under the factorization
        fact = (FPM_KF_* kind, threshold) or, combined, (kind, threshold, 1); frees it"""
        L = lib()
        try:
            kind, thr, *comb = fact
            if kind != KF_CFL:
                _check(L.fpm_kfinger_set_factorization(job, kind, thr))
            if comb and comb[0]:
                _check(L.fpm_kfinger_set_comb(job, 1))
            _check(L.fpm_kfinger_run(job, seed, int(use64), None))
            first = np.zeros(n_rec + 1, np.uint64)
            h = np.zeros(max(n, 1), np.uint64 if use64 else np.uint32)
            nv = np.zeros(max(n, 1), np.uint32)
            _check(L.fpm_kfinger_fetch(job, _p(first, u64p), h.ctypes.data, _p(nv, u32p)))
            groups = C.c_uint32()
            _check(L.fpm_kfinger_wide_groups(job, C.byref(groups)))
            res = {"n_lines": n, "rec_first_line": first, "hash": h[:n], "n_vals": nv[:n],
                   "wide_groups": groups.value}
            if values:
                tot = C.c_uint64()
                _check(L.fpm_kfinger_values(job, None, None, 0, C.byref(tot)))
                vals = np.zeros(max(tot.value, 1), np.uint16)
                off = np.zeros(n + 1, np.uint64)
                _check(L.fpm_kfinger_values(job, _p(off, u64p), _p(vals, u16p), tot.value,
                                            C.byref(tot)))
                res["val_off"], res["vals"] = off, vals[:tot.value]
            for want, key, call in ((text, "text", L.fpm_kfinger_text),
                                    (fact_text, "fact_text", L.fpm_kfinger_fact_text)):
                if not want:
                    continue
                if ids is None or len(ids) != n_rec:
                    raise ValueError("text=True and fact_text=True need one ID per record")
                blob, off = pack_records([bytes(i) for i in ids])
                nb = C.c_uint64()
                _check(call(job, blob, _p(off, u64p), None, 0, C.byref(nb)))
                out = np.zeros(max(nb.value, 1), np.uint8)
                _check(call(job, blob, _p(off, u64p), out.ctypes.data, nb.value, C.byref(nb)))
                res[key] = out[:nb.value].tobytes()
            return res
        finally:
            L.fpm_kfinger_free(job)

    def kfinger(self, seqs, window=100, seed=42, use64=False, max_lines=None, ids=None,
                values=False, text=False, factorization="CFL", split=None, fact_text=False):
        """k-fingers of the records `seqs` (lyn2vec --type basic --type_factorization CFL,
        fingerprint_utils.py:95-110, 443-476; factorization "ICFL" or "CFL_ICFL-<T>" for lyn2vec's
        factorizations of those names, fpm_kfinger_set_factorization; "CFL_COMB", "ICFL_COMB" or
        "CFL_ICFL_COMB-<T>" for the combined ones, fpm_kfinger_set_comb) and their line hashes
        (hash.cpp:45-73), on the device.  -> n_lines, rec_first_line (len(seqs) + 1), hash and n_vals per line; with
        values the factor lengths (vals u16, line l's at val_off[l] .. val_off[l + 1]); with
        text the lines' text, ids[r] being record r's full ID bytes (lyn2vec's "<id>_0").
        wide_groups: fpm_kfinger_wide_groups of the run (a test hook).
        max_lines: only the first so many lines exist (None: all).
        split=N: the long-read job instead (lyn2vec --type generalized --split N,
        fpm_kfinger_stage_split): a line is one of a record's consecutive pieces of N bytes, the
        text has one line per record, "<id>  <lengths> | <lengths> | ", and ids[r] is the ID as
        it is to appear; window and max_lines do not apply.  fact_text: also the factor text
        (lyn2vec --fact create, fpm_kfinger_fact_text), the text with each factor's bytes in
        place of its length."""
        fact = kfinger_factorization(factorization)      # (refused before anything is staged)
        data, off = pack_records([bytes(s) for s in seqs])
        job, n = vp(), C.c_uint64()
        if split is not None:
            if max_lines is not None:
                raise ValueError("a split job has no max_lines")
            _check(lib().fpm_kfinger_stage_split(self.h, data, _p(off, u64p), len(seqs), int(split),
                                                 C.byref(job), C.byref(n)))
        else:
            cap = 0xFFFFFFFFFFFFFFFF if max_lines is None else int(max_lines)
            _check(lib().fpm_kfinger_stage(self.h, data, _p(off, u64p), len(seqs), window, cap,
                                           C.byref(job), C.byref(n)))
        return self._kfinger_out(job, n.value, len(seqs), seed, use64, ids, values, text, fact,
                                 fact_text)

    def kfinger_fasta(self, files, take=None, window=100, seed=42, use64=False, max_lines=None,
                      ids=None, values=False, text=False, factorization="CFL", split=None,
                      fact_text=False):
        """kfinger over the records of FASTA / FASTQ file images parsed on the device
        (fpm_seq_parse + fpm_kfinger_stage_seq); take[r] false leaves record r out.  ids None:
        each record's ID by kfinger_id of its header line (with split, kfinger_long_id: the
        record's name).  split, fact_text: as in kfinger (fpm_kfinger_stage_split_seq).  Also
        returns the parse's records."""
        fact = kfinger_factorization(factorization)
        if split is not None and max_lines is not None:
            raise ValueError("a split job has no max_lines")
        seq_job, recs, quality = self.seq_parse(files)
        try:
            if quality:
                raise ValueError("quality lines: walk such input on the host")
            n_rec = len(recs["seg"])
            if ids is None:
                ids = []
                for r in range(n_rec):
                    img = files[int(recs["seg"][r])]
                    o, ln = int(recs["hdr_off"][r]), int(recs["hdr_len"][r])
                    ids.append((kfinger_id if split is None else kfinger_long_id)(img[o + 1:o + ln]))
            t = None
            if take is not None:
                t = np.ascontiguousarray(np.asarray(take, dtype=bool), dtype=np.uint8)
                if t.size == 0:
                    t = np.zeros(1, np.uint8)
            job, n = vp(), C.c_uint64()
            if split is not None:
                _check(lib().fpm_kfinger_stage_split_seq(self.h, seq_job, _p(t, u8p), int(split),
                                                         C.byref(job), C.byref(n)))
            else:
                cap = 0xFFFFFFFFFFFFFFFF if max_lines is None else int(max_lines)
                _check(lib().fpm_kfinger_stage_seq(self.h, seq_job, _p(t, u8p), window, cap,
                                                   C.byref(job), C.byref(n)))
        finally:
            lib().fpm_seq_free(seq_job)
        res = self._kfinger_out(job, n.value, n_rec, seed, use64, ids, values, text, fact,
                                fact_text)
        res["records"] = recs
        return res

    def positional(self, ref_lists, qry_lists, use64=False, max_dist=1.0, max_pvalue=1.0):
        """triangle -fp's positional compare over the grid (query-major)."""
        dt = np.uint64 if use64 else np.uint32
        w = max([len(x) for x in list(ref_lists) + list(qry_lists)] + [1])
        R, rl = _dense(ref_lists, w, dt)
        Q, ql = _dense(qry_lists, w, dt)
        n = len(ref_lists) * len(qry_lists)
        nu = np.zeros(max(n, 1), np.uint32)
        de = np.zeros(max(n, 1), np.uint32)
        di = np.zeros(max(n, 1), np.float64)
        pv = np.zeros(max(n, 1), np.float64)
        pa = np.zeros(max(n, 1), np.uint8)
        _check(lib().fpm_fp_positional_grid(self.h, R.ctypes.data, _p(rl, u32p), w, len(ref_lists),
                                            Q.ctypes.data, _p(ql, u32p), w, len(qry_lists),
                                            8 if use64 else 4, max_dist, max_pvalue, _p(nu, u32p),
                                            _p(de, u32p), _p(di, f64p), _p(pv, f64p), _p(pa, u8p)))
        return {"numer": nu[:n], "denom": de[:n], "distance": di[:n], "pvalue": pv[:n],
                "pass": pa[:n].astype(bool)}


class RefSet:
    """fpm_refset_*: the reference rows stay on the device with their bucket index built
    once; dist() runs one query block against them (results as Context.dist)."""

    def __init__(self, ctx, ref_lists, sketch_size, use64=True, ref_lengths=None, width=None):
        self.ctx, self.use64, self.S = ctx, use64, int(sketch_size)
        self.dt = np.uint64 if use64 else np.uint32
        self.w = int(width or max([len(x) for x in ref_lists] + [1]))
        R, rl = _dense(ref_lists, self.w, self.dt)
        self.n = len(ref_lists)
        rL = np.ascontiguousarray(ref_lengths if ref_lengths is not None else
                                  [0] * self.n, dtype=np.uint64)
        h = vp()
        _check(lib().fpm_refset_create(ctx.h, R.ctypes.data, _p(rl, u32p), _p(rL, u64p), self.w,
                                       self.n, 8 if use64 else 4, self.S, C.byref(h)))
        self.h = h.value

    def dist(self, qry_lists, k=21, kmer_space=None, qry_lengths=None, max_dist=-1.0,
             max_pvalue=-1.0):
        Q, ql = _dense(qry_lists, self.w, self.dt)
        nq = len(qry_lists)
        n = self.n * nq
        qL = np.ascontiguousarray(qry_lengths if qry_lengths is not None else [0] * nq,
                                  dtype=np.uint64)
        if kmer_space is None:
            kmer_space = 4.0 ** k
        nu = np.zeros(max(n, 1), np.uint32)
        de = np.zeros(max(n, 1), np.uint32)
        di = np.zeros(max(n, 1), np.float64)
        pv = np.zeros(max(n, 1), np.float64)
        pa = np.zeros(max(n, 1), np.uint8)
        _check(lib().fpm_refset_dist(self.h, Q.ctypes.data, _p(ql, u32p), _p(qL, u64p), self.w,
                                     nq, self.S, k, kmer_space, max_dist, max_pvalue,
                                     _p(nu, u32p), _p(de, u32p), _p(di, f64p), _p(pv, f64p),
                                     _p(pa, u8p)))
        return {"numer": nu[:n], "denom": de[:n], "distance": di[:n], "pvalue": pv[:n],
                "pass": pa[:n].astype(bool)}

    def free(self):
        if self.h:
            lib().fpm_refset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dense(lists, width, dtype):
    m = np.zeros((max(len(lists), 1), max(width, 1)), dtype=dtype)
    lens = np.zeros(max(len(lists), 1), dtype=np.uint32)
    for i, l in enumerate(lists):
        m[i, : len(l)] = l
        lens[i] = len(l)
    return m, lens
