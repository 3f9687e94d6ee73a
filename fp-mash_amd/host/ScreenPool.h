// ScreenPool.h — the pool side of `screen` and `taxscreen`: pool files streamed once through the
// device in bounded slices of whole records (fpm_screen_add_job: hashSequence's counting,
// CommandScreen.cpp:280-384, and the pool's one MinHashHeap, CommandTaxScreen.cpp:347-361).  Both
// verbs include it; neither changes it.
#pragma once

#include "Device.h"
#include "SeqReader.h"

#include <cstdlib>
#include <string>
#include <vector>

namespace fpmhost {

// device bytes of pool text per slice (FPMASH_SCREEN_SLICE overrides, in bytes)
inline size_t sliceBytes()
{
    const char *v = getenv("FPMASH_SCREEN_SLICE");
    const long long n = v ? atoll(v) : 0;
    return n > 0 ? (size_t)n : (size_t)256 << 20;
}

struct Pool {
    fpm_ctx *ctx;
    fpm_screen *sc;
    fpm_sketch_params fp;
    uint64_t records = 0;   // kseq records read, short ones included (CommandTaxScreen.cpp:315)

    void add(fpm_sketch_job *job)
    {
        check(fpm_screen_add_job(sc, job, nullptr), "screen");
        check(fpm_ctx_synchronize(ctx), "screen");
        fpm_sketch_job_free(job);
    }

    // records walked on the host by kseq's rules, given to the device `budget` bytes at a time
    bool hostWalk(const std::string &image, size_t budget)
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

    // one pool file: parsed and packed on the device when it fits a slice and has no FASTQ
    // quality lines, else walked on the host
    bool file(const std::string &image)
    {
        const size_t budget = sliceBytes();
        if (image.size() > budget) return hostWalk(image, budget);
        fpm_seqtext *parsed = nullptr;
        uint64_t nRec = 0;
        int quality = 0;
        const char *ptr = image.data();
        const uint64_t len = image.size();
        check(fpm_seq_parse(ctx, &ptr, &len, 1, &parsed, &nRec, &quality), "sequence parse");
        if (quality) {
            fpm_seq_free(parsed);
            return hostWalk(image, budget);
        }
        std::vector<uint32_t> seg(nRec), groupOf(nRec, FPM_NO_GROUP);
        std::vector<uint64_t> ho(nRec), hl(nRec), sl(nRec);
        check(fpm_seq_records(parsed, seg.data(), ho.data(), hl.data(), sl.data()), "sequence parse");
        bool any = false;
        for (uint64_t r = 0; r < nRec; r++) {
            // a '>' / '@' as the last byte of a file starts no record (kseq_read returns -1)
            if (ho[r] + 1 >= image.size()) continue;
            records++;
            if (sl[r] >= fp.kmer_size) { groupOf[r] = 0; any = true; }
        }
        if (any) {
            fpm_sketch_job *job = nullptr;
            check(fpm_sketch_stage_seq(ctx, &fp, parsed, groupOf.data(), 1, &job), "screen");
            add(job);
        }
        fpm_seq_free(parsed);
        return true;
    }
};

}  // namespace fpmhost
