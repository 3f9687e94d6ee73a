// ScreenPool.h — what `screen` and `taxscreen` share, which is everything up to the pool's set
// size: the database (.msh) loaded and refused, the pool arguments checked, the device table
// of the database's hashes (fpm_screen_create), and the pool files streamed once through the
// device in bounded slices of whole records (fpm_screen_add_job: hashSequence's counting,
// CommandScreen.cpp:280-384, and the pool's one MinHashHeap, CommandTaxScreen.cpp:347-361).
// The verbs call ScreenRun's steps in order, put their own refusals and host work between
// them, and differ only in what they read from the table afterwards.
#pragma once

#include "Device.h"
#include "Sketch.h"
#include "SketchRows.h"

#include <string>
#include <vector>

namespace fpmhost {

// One run of either verb over args = <queries>.msh <pool> [<pool>] ...  Every step but
// openTable and streamPool is host work; a step that returns false has printed its message
// and the verb returns 1.
struct ScreenRun {
    const char *verb;                       // "screen" / "taxscreen", as the messages name it
    const std::vector<std::string> &args;
    Sketch sketch;
    PackedRows rows;                        // len[] and length[]; the matrix goes once it is uploaded
    fpm_ctx *ctx = nullptr;
    fpm_screen *sc = nullptr;
    fpm_sketch_params fp{};                 // the database's parameters, its sketch size at least 1
    uint64_t records = 0;   // kseq records read, short ones included (CommandTaxScreen.cpp:315)

    ScreenRun(const char *v, const std::vector<std::string> &a) : verb(v), args(a) {}
    // the .msh suffix, the load, the protein refusal
    bool loadDatabase();
    // (CommandTaxScreen.cpp:229-250; checked before any device work)
    bool checkPoolArguments() const;
    // rows packed and uploaded, the table of their distinct hashes built
    bool openTable();
    // every pool file through the device; then the pool's set size
    bool streamPool();

  private:
    // one pool file: parsed and packed on the device when it fits a slice and has no FASTQ
    // quality lines, else walked on the host
    bool poolFile(const std::string &image);
    bool hostWalk(const std::string &image, size_t budget);
    void add(fpm_sketch_job *job);
};

}  // namespace fpmhost
