// SketchRows.h — a sketch set as the dense row matrix the device calls take: one zero-padded
// row per Reference (u64 hashes, or u32 when !use64), with the rows' hash counts and sequence
// lengths beside it.  The one packer of dist, triangle, contain, screen and taxscreen; it
// touches no device, so it links without libfpmash.
#pragma once

#include "HostRows.h"
#include "Sketch.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

namespace fpmhost {

inline uint64_t maxRowLength(const std::vector<Reference> &refs)
{
    uint64_t w = 0;
    for (const Reference &r : refs) w = std::max<uint64_t>(w, r.hashes.size());
    return w;
}

struct PackedRows {
    std::unique_ptr<HostRows<uint8_t>> rows;   // n x width hashes of hashBytes each
    std::vector<uint32_t> len;                 // hashes per row
    std::vector<uint64_t> length;              // Reference::length per row
    uint64_t width = 1, n = 0;
    uint32_t hashBytes = 8;

    PackedRows() = default;
    // rows as wide as the longest of `refs`, and at least minWidth
    PackedRows(const std::vector<Reference> &refs, bool use64, uint64_t minWidth = 1)
        : len(refs.size()), length(refs.size()), width(std::max(minWidth, maxRowLength(refs))),
          n(refs.size()), hashBytes(use64 ? 8 : 4)
    {
        // (zero pages, populated in one call: a value-initialised vector paid a memset and ~20k
        // page faults on one thread for C2's 80 MB)
        rows = std::make_unique<HostRows<uint8_t>>(std::max<uint64_t>(1, n * width) * hashBytes);
        uint8_t *m = rows->data();
        auto pack = [&](uint64_t a, uint64_t b) {
            for (uint64_t i = a; i < b; i++) {
                const Reference &r = refs[i];
                len[i] = (uint32_t)r.hashes.size();
                length[i] = r.length;
                if (use64) {
                    if (!r.hashes.empty()) memcpy(&m[i * width * 8], r.hashes.data(), r.hashes.size() * 8);
                } else {
                    uint32_t *row = reinterpret_cast<uint32_t *>(&m[i * width * 4]);
                    for (uint64_t j = 0; j < r.hashes.size(); j++) row[j] = (uint32_t)r.hashes[j];
                }
            }
        };
        // several threads past a few thousand rows (C2: 80 MB)
        const uint64_t nt = n >= 4096 ? std::max(1u, std::min(8u, std::thread::hardware_concurrency())) : 1;
        std::vector<std::thread> th;
        for (uint64_t t = 1; t < nt; t++) th.emplace_back(pack, n * t / nt, n * (t + 1) / nt);
        pack(0, n / nt);
        for (auto &x : th) x.join();
    }

    const uint8_t *data() const { return rows->p; }
    size_t bytes() const { return (size_t)n * width * hashBytes; }
};

}  // namespace fpmhost
