// ScreenPool.cpp — the steps of a `screen` / `taxscreen` run that both verbs take (ScreenPool.h)
#include "ScreenPool.h"
#include "Command.h"
#include "ParsedFile.h"
#include "SeqReader.h"
#include "Timing.h"

#include <cstdlib>
#include <iostream>

namespace fpmhost {

// device bytes of pool text per slice (FPMASH_SCREEN_SLICE overrides, in bytes)
static size_t sliceBytes()
{
    const char *v = getenv("FPMASH_SCREEN_SLICE");
    const long long n = v ? atoll(v) : 0;
    return n > 0 ? (size_t)n : (size_t)256 << 20;
}

void ScreenRun::add(fpm_sketch_job *job)
{
    check(fpm_screen_add_job(sc, job, nullptr), "screen");
    check(fpm_ctx_synchronize(ctx), "screen");
    fpm_sketch_job_free(job);
}

// records walked on the host by kseq's rules, given to the device `budget` bytes at a time
bool ScreenRun::hostWalk(const std::string &image, size_t budget)
{
    SeqReader rd(image.data(), image.size());
    std::string packed;
    std::vector<uint64_t> off{0};
    std::vector<uint32_t> grp;
    auto flush = [&] {
        if (grp.empty()) return;
        fpm_sketch_job *job = nullptr;
        check(fpm_sketch_stage(ctx, &fp, packed.data(), off.data(), (uint32_t)grp.size(),
                               grp.data(), 1, &job),
              "screen");
        add(job);
        packed.clear();
        off.assign(1, 0);
        grp.clear();
    };
    int l;
    while ((l = rd.read()) >= 0) {
        records++;
        if ((uint32_t)l < fp.kmer_size) continue;   // (CommandTaxScreen.cpp:317)
        if (packed.size() + rd.seq.size() > budget) flush();
        packed += rd.seq;
        off.push_back(packed.size());
        grp.push_back(0);
    }
    flush();
    return l == -1;
}

bool ScreenRun::poolFile(const std::string &image)
{
    const size_t budget = sliceBytes();
    if (image.size() > budget) return hostWalk(image, budget);
    {
        ParsedFile parsed;
        if (parsed.parse(ctx, image)) {
            std::vector<uint32_t> groupOf(parsed.nRec, FPM_NO_GROUP);
            bool any = false;
            for (uint64_t r = 0; r < parsed.nRec; r++) {
                if (!parsed.isRecord(r)) continue;
                records++;
                if (parsed.seqLen[r] >= fp.kmer_size) { groupOf[r] = 0; any = true; }
            }
            if (any) {
                fpm_sketch_job *job = nullptr;
                check(fpm_sketch_stage_seq(ctx, &fp, parsed.text, groupOf.data(), 1, &job), "screen");
                add(job);
            }
            return true;
        }
    }
    return hostWalk(image, budget);
}

bool ScreenRun::loadDatabase()
{
    if (!hasSuffix(args[0], suffixSketch)) {
        std::cerr << "ERROR: " << args[0] << " does not look like a sketch (.msh)" << std::endl;
        return false;
    }
    sketch.initFromFiles({args[0]}, Parameters());
    phaseMark("load database");
    std::string alphabet;
    sketch.getAlphabetAsString(alphabet);
    if (alphabet == alphabetProtein) {
        std::cerr << "ERROR: " << args[0] << " is an amino acid sketch; translated screening "
                     "is not supported" << std::endl;
        return false;
    }
    return true;
}

bool ScreenRun::checkPoolArguments() const { return checkInputArguments(args, 1, "query"); }

bool ScreenRun::openTable()
{
    std::cerr << "Loading " << args[0] << "..." << std::endl;
    rows = PackedRows(sketch.references, sketch.getUse64());
    ctx = device();
    fp = sketchParams(sketch.parameters);
    fp.sketch_size = std::max(1u, fp.sketch_size);
    const int rc = fpm_screen_create(ctx, rows.data(), rows.len.data(), rows.width, (uint32_t)rows.n,
                                     rows.hashBytes, fp.sketch_size, &sc);
    if (rc == FPM_EINVAL) {
        std::cerr << "ERROR: " << args[0] << ": " << verb << " needs sketches whose hashes are in "
                     "strictly ascending order (" << fpm_last_error() << ")" << std::endl;
        return false;
    }
    check(rc, verb);
    rows.rows.reset();
    uint64_t nDistinct = 0;
    check(fpm_screen_counts(sc, nullptr, nullptr, &nDistinct), verb);
    std::cerr << "   " << nDistinct << " distinct hashes." << std::endl;
    phaseMark("database table");
    return true;
}

bool ScreenRun::streamPool()
{
    const size_t queryCount = args.size() - 1;                    // (CommandTaxScreen.cpp:207-219)
    std::cerr << "Streaming from ";
    if (queryCount == 1) std::cerr << args[1];
    else std::cerr << queryCount << " inputs";
    std::cerr << "..." << std::endl;

    // one file image at a time: device and host memory follow the largest file's slices
    for (size_t f = 1; f < args.size(); f++) {
        std::string image;
        if (!loadSequenceFile(args[f], image)) {
            std::cerr << "ERROR: could not open " << args[f] << std::endl;
            return false;
        }
        if (!poolFile(image)) {
            std::cerr << "\nERROR: reading inputs" << std::endl;
            return false;
        }
    }
    phaseMark("pool (read + parse + sketch + count)");
    if (records == 0) {                                      // (:363-368)
        std::cerr << "\nERROR: Did not find sequence records in inputs" << std::endl;
        return false;
    }
    uint64_t setSize = 0;
    check(fpm_screen_set_size(sc, &setSize), verb);
    std::cerr << "   Estimated distinct k-mers in pool: " << setSize << std::endl;   // (:371-376)
    if (setSize == 0) std::cerr << "WARNING: no valid k-mers in input." << std::endl;
    return true;
}

}  // namespace fpmhost
