// ParsedFile.h — one file image parsed on the device (fpm_seq_parse) with its record table on
// the host: what `screen`, `taxscreen` and `kfinger` stage their jobs from.
#pragma once

#include "Device.h"

#include <string>
#include <vector>

namespace fpmhost {

struct ParsedFile {
    fpm_seqtext *text = nullptr;
    uint64_t nRec = 0;
    std::vector<uint32_t> seg;
    std::vector<uint64_t> headOff, headLen, seqLen;   // per record: its header line, its bases

    // false: the image has FASTQ quality lines, which the device parser hands back; the caller
    // walks the records on the host
    bool parse(fpm_ctx *ctx, const std::string &image)
    {
        int quality = 0;
        const char *ptr = image.data();
        const uint64_t len = imageBytes = image.size();
        check(fpm_seq_parse(ctx, &ptr, &len, 1, &text, &nRec, &quality), "sequence parse");
        if (quality) return false;
        seg.resize(nRec);
        headOff.resize(nRec);
        headLen.resize(nRec);
        seqLen.resize(nRec);
        check(fpm_seq_records(text, seg.data(), headOff.data(), headLen.data(), seqLen.data()),
              "sequence parse");
        return true;
    }
    // a '>' / '@' as the last byte of a file starts no record (kseq_read returns -1)
    bool isRecord(uint64_t r) const { return headOff[r] + 1 < imageBytes; }

    ParsedFile() = default;
    ParsedFile(const ParsedFile &) = delete;
    ParsedFile &operator=(const ParsedFile &) = delete;
    ~ParsedFile() { if (text) fpm_seq_free(text); }

  private:
    uint64_t imageBytes = 0;
};

}  // namespace fpmhost
