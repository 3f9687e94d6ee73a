// hostrows_check.cpp — the host's row packer (host/SketchRows.h) against a one-thread, per-hash
// loop, and its number formatters (host/TextOut.h) against snprintf / std::to_string.  No device
// and no libfpmash.  Built with a host sanitizer by tests/test_hostrows_host.py; prints
// "hostrows ok" and exits 0, or names the first check that failed.
#include "../host/SketchRows.h"
#include "../host/TextOut.h"

#include <cstdio>

using namespace fpmhost;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "hostrows_check:%d: %s\n", __LINE__, #cond);   \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// the packing as the verbs used to write it: one hash at a time into zeroed vectors
static bool samePack(const std::vector<Reference> &refs, bool use64, uint64_t minWidth)
{
    const uint32_t hb = use64 ? 8 : 4;
    uint64_t width = minWidth;
    for (const Reference &r : refs) width = std::max<uint64_t>(width, r.hashes.size());
    std::vector<uint8_t> M(refs.size() * width * hb, 0);
    std::vector<uint32_t> len(refs.size());
    std::vector<uint64_t> length(refs.size());
    for (size_t i = 0; i < refs.size(); i++) {
        len[i] = (uint32_t)refs[i].hashes.size();
        length[i] = refs[i].length;
        for (size_t j = 0; j < refs[i].hashes.size(); j++) {
            if (use64) memcpy(&M[(i * width + j) * 8], &refs[i].hashes[j], 8);
            else { const uint32_t v = (uint32_t)refs[i].hashes[j]; memcpy(&M[(i * width + j) * 4], &v, 4); }
        }
    }
    const PackedRows p(refs, use64, minWidth);
    return p.n == refs.size() && p.width == width && p.hashBytes == hb && p.bytes() == M.size() &&
           (M.empty() || memcmp(p.data(), M.data(), M.size()) == 0) && p.len == len &&
           p.length == length;
}

static Reference row(std::vector<uint64_t> hashes, uint64_t length)
{
    Reference r;
    r.hashes = std::move(hashes);
    r.length = length;
    return r;
}

static bool sameNum(double x)
{
    char a[64], b[64];
    *numTo(a, x) = 0;
    snprintf(b, sizeof b, "%g", x);
    std::string s = "x";
    putNum(s, x);
    return strcmp(a, b) == 0 && s == std::string("x") + b;
}

static bool sameU(uint64_t x)
{
    char a[32];
    *uTo(a, x) = 0;
    std::string s = "x";
    putU(s, x);
    return std::to_string(x) == a && s == "x" + std::to_string(x);
}

int main()
{
    const uint64_t big = (7ULL << 32) | 0x89abcdefULL;   // narrows to 0x89abcdef
    // rows of length 0, 1 and exactly `width`
    const std::vector<Reference> small{row({}, 0), row({big}, 11), row({1, 2, big, ~0ULL}, 1ULL << 40),
                                       row({5, 6}, 3)};
    CHECK(maxRowLength(small) == 4);
    CHECK(maxRowLength({}) == 0);
    for (const bool use64 : {true, false}) {
        CHECK(samePack(small, use64, 1));
        CHECK(samePack(small, use64, 9));     // a minimum width larger than every row
        CHECK(samePack({}, use64, 1));        // n = 0
        CHECK(samePack({row({}, 7)}, use64, 1));
    }
    {
        const PackedRows p(small, false, 1);
        CHECK(reinterpret_cast<const uint32_t *>(p.data())[1 * p.width] == 0x89abcdefu);
        CHECK(PackedRows({}, true, 1).width == 1);
    }
    {   // past 4096 rows the packer runs on several threads
        std::vector<Reference> many;
        uint64_t x = 88172645463325252ULL;
        for (int i = 0; i < 4097; i++) {
            std::vector<uint64_t> h;
            for (int j = i % 4; j > 0; j--) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                h.push_back(x);
            }
            many.push_back(row(std::move(h), x % 1000));
        }
        CHECK(samePack(many, true, 1));
        CHECK(samePack(many, false, 1));
    }
    for (const double x : {1.0, 0.0, -0.0, 0.5, 1e-300, 0.000123456789, 123456789.0}) CHECK(sameNum(x));
    {
        char a[32];
        *numTo(a, -0.0) = 0;
        CHECK(strcmp(a, "-0") == 0);
    }
    for (const uint64_t x : {0ULL, 9ULL, 10ULL, 99ULL, 100ULL, 999ULL, 1000ULL, 9999ULL, 10000ULL, ~0ULL})
        CHECK(sameU(x));
    printf("hostrows ok\n");
    return 0;
}
