// sketch_plan.hpp — the plan of a sketch job: which tiles cover the records, which row of the
// device matrix each tile, selection and merge writes, and in which order they run.  Pure
// integer bookkeeping over the record lengths: no device call, no record byte.
// fpm_sketch_api.cpp packs the records, calls plan_sketch and uploads the result;
// tools/sketchplan_check.cpp checks the planner alone on the CPU.
//
// Rows.  One device matrix d_rows[n_rows][s]: rows [0, n_groups) are the final sketches, the
// rows above them hold per-tile and intermediate lists.  Row numbers are handed out in this
// order, which is part of the contract (n_rows, n_fb_rows and the device layout rest on it):
//   the groups' final rows, tiles, sample tiles, sample selection rows (each sample's sketch row,
//   then its chunk rows), sample merge rows, main selection chunk rows, main merge rows,
//   and last the fallback schedules' rows (sample fallback, then main fallback).
// Rows >= n_rows (the fallback rows) live in a buffer that is allocated only if a selection fails.
#pragma once

#include "fpm_kernels.hpp"

#include <cstdint>
#include <vector>

namespace fpm {

// Tile sizing: small records are packed up to kPackKmers k-mer starts per tile,
// long records are cut into kChunkKmers-start chunks (k-1 bytes of halo).
constexpr uint32_t kPackKmers = 2048;
// (2048-start chunks: the tile kernel 1.3 ms faster on C5, the group selection 1.3 ms slower)
constexpr uint32_t kChunkKmers = 4096;
// the least sample rate of a long group: every kSampleEvery-th tile (choose_samples)
constexpr uint32_t kSampleEvery = 16;
// a selection is split into a further level past this many estimated keys or rows per workgroup
constexpr uint64_t kKeysPerWG = 1u << 19;
constexpr size_t kRowsPerWG = 4096;

// rows a and b merged into row c
struct MergeStep { uint32_t a, b, c; };

// pairwise merge rounds: round r runs steps[round_begin[r] .. round_begin[r + 1]);
// round_small[r]: its input lists are estimated at most kMergeSmallCap long
struct MergeSchedule {
    std::vector<MergeStep> steps;
    std::vector<uint32_t> round_begin;
    std::vector<uint8_t> round_small;
    size_t rounds() const { return round_begin.empty() ? 0 : round_begin.size() - 1; }
};

// The records to plan for, in the order their groups stream them (StageRecords without the
// bytes): record r has len[r] bytes at offset pos[r] of the packed buffer.
struct PlanRecords {
    const std::vector<uint32_t> &order;
    const std::vector<uint64_t> &pos, &len;
    const std::vector<uint32_t> &group;
    uint32_t n_groups;
};

struct PlanParams {
    uint32_t k, s;
    bool use64;
};

struct SketchPlan {
    // the main and the sample tiles, ordered by capacity class
    std::vector<TileDesc> tiles, stiles;
    uint32_t class_begin[kTileClasses + 1] = {0}, sclass_begin[kTileClasses + 1] = {0};
    uint32_t n_groups = 0;
    uint32_t n_rows = 0;        // the core rows
    uint32_t n_fb_rows = 0;     // the fallback schedules' intermediate rows, [n_rows, n_rows + n_fb_rows)
    uint64_t n_kmers = 0;
    // long groups: a 1-in-`every` sample of their tiles is sketched first; its s-th smallest
    // hash bounds what every tile of the group keeps.  Per slot (sampled group):
    uint32_t n_slots = 0;
    std::vector<uint32_t> srow;         // the sample's sketch row
    std::vector<uint64_t> sbound;       // the a-priori bound of the sample's own tiles (~0: none)
    std::vector<uint32_t> kt;           // tight bounds: the sample's kt-th smallest hash
    std::vector<uint32_t> slot_group;   // the slot's group
    // sampled groups: one-workgroup selections from their bounded tile lists; sel holds the
    // sample levels, then the main levels, level l of each at [begin[l], begin[l + 1])
    std::vector<SelDesc> sel;
    std::vector<uint32_t> sel_rows;     // the rows the selections read (SelDesc::row_begin)
    std::vector<uint32_t> ssel_begin, sel_begin;
    std::vector<uint32_t> ssel_tag;     // each sample selection's slot
    uint32_t n_ssel() const { return ssel_begin.back(); }
    uint32_t n_sel() const { return sel_begin.back() - sel_begin.front(); }
    // class-4 tiles all bounded (C5's genomes): the survivors-only tile kernel
    bool thr4 = false;
    uint32_t n4 = 0;                    // class-4 tiles (the redo list's capacity)
    bool tight = false;                 // kt / slot_group are set
    bool sbounded = false;              // tight, and some sample carries an a-priori bound
    // pairwise merges: groups without a selection (main, sample), and the selections' fallbacks
    MergeSchedule merge, smerge, fmerge, sfmerge;
};

// false: a tile exceeds the largest capacity class (an internal error; *out is unspecified)
bool plan_sketch(const PlanRecords &R, const PlanParams &p, SketchPlan *out);

}  // namespace fpm
