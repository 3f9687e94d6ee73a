// TextOut.h — the verbs' text output: numbers as an ostream prints them by default (%g,
// precision 6) and the buffered stdout writer.  No device dependency.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace fpmhost {

// into a caller's buffer (the one-append-per-line path); at most 32 bytes
inline char *numTo(char *p, double x)
{
    if (x == 1.0) { *p++ = '1'; return p; }     // most cells: no shared hash
    if (x == 0.0 && !std::signbit(x)) { *p++ = '0'; return p; }
    return p + snprintf(p, 32, "%g", x);
}
// counts of up to 4 digits (a sketch size of 1000 and below: every count of the C2 text) by
// two-digit table lookups, the rest digit by digit (14.6 against 17.6 ns per list line); at
// most 20 bytes
constexpr char kDigits2[] =
    "00010203040506070809101112131415161718192021222324252627282930313233343536373839"
    "40414243444546474849505152535455565758596061626364656667686970717273747576777879"
    "8081828384858687888990919293949596979899";
inline char *uTo(char *p, uint64_t x)
{
    if (x < 100) {
        if (x < 10) { *p = (char)('0' + x); return p + 1; }
        memcpy(p, kDigits2 + 2 * x, 2);
        return p + 2;
    }
    if (x < 10000) {
        const uint32_t a = (uint32_t)x / 100, b = (uint32_t)x % 100;
        if (a < 10) {
            *p = (char)('0' + a);
            memcpy(p + 1, kDigits2 + 2 * b, 2);
            return p + 3;
        }
        memcpy(p, kDigits2 + 2 * a, 2);
        memcpy(p + 2, kDigits2 + 2 * b, 2);
        return p + 4;
    }
    char t[20];
    int n = 0;
    do { t[19 - n++] = (char)('0' + x % 10); x /= 10; } while (x);
    memcpy(p, t + 20 - n, n);
    return p + n;
}
inline void putNum(std::string &o, double x)
{
    char t[32];
    o.append(t, (size_t)(numTo(t, x) - t));
}
inline void putU(std::string &o, uint64_t x)
{
    char t[20];
    o.append(t, (size_t)(uTo(t, x) - t));
}

// stdout through one string, written out whenever it passes 4 MB and by flush()
struct StdoutText {
    std::string buf;
    void flush() { fwrite(buf.data(), 1, buf.size(), stdout); buf.clear(); }
    void flushIfLarge() { if (buf.size() > (1 << 22)) flush(); }
    // everything written and stdout flushed
    void finish() { flush(); fflush(stdout); }
};

}  // namespace fpmhost
