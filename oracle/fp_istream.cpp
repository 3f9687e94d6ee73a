// fp_istream.cpp — TEST INFRASTRUCTURE ONLY (part of liboracle.so).
//
// The -fp text parse through libstdc++ itself: std::getline over an std::istringstream of the
// whole text, `ss >> id`, then `while (ss >> v)` into a uint64_t — the statements
// Sketch::initFromFingerprints is written in.  orc_fp_parse (fpm_oracle.c) restates what
// those statements do in C, and the device kernel restates it again; this is the thing both
// restate, so tests/test_fptext_model.py can hold the restatement to it.  Same outputs as
// orc_fp_parse: per line the ID (byte offset in the text, length), then the values, line l's
// at vals[line_val_off[l] .. line_val_off[l + 1]).
//
// The stream gives the ID as a string, not a position: the offset is that of the first
// non-space run of the line, and the bytes there must be the string the stream extracted
// (UINT64_MAX is returned where they are not).

#include <cstdint>
#include <cstring>
#include <sstream>
#include <string>

static bool space_byte(char c)
{
    return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r';
}

extern "C" uint64_t orc_fp_parse_istream(const char *text, uint64_t text_len, uint64_t limit,
                                         uint64_t *lines_used, uint64_t max_lines,
                                         uint64_t max_vals, uint64_t *id_off, uint32_t *id_len,
                                         uint64_t *vals, uint64_t *line_val_off)
{
    std::istringstream in(std::string(text, (size_t)text_len));
    std::string line;
    uint64_t nl = 0, nv = 0, at = 0;            // at: the line's first byte in the text
    line_val_off[0] = 0;
    while (*lines_used < limit && nl < max_lines && std::getline(in, line)) {
        ++*lines_used;
        std::istringstream ss(line);
        std::string id;
        ss >> id;
        size_t b = 0;
        while (b < line.size() && space_byte(line[b])) b++;
        if (b + id.size() > line.size() || memcmp(line.data() + b, id.data(), id.size()) != 0)
            return UINT64_MAX;
        if (b + id.size() < line.size() && !id.empty() && !space_byte(line[b + id.size()]))
            return UINT64_MAX;                   // the run goes on past what the stream took
        id_off[nl] = at + b;
        id_len[nl] = (uint32_t)id.size();
        uint64_t v;
        while (nv < max_vals && ss >> v) vals[nv++] = v;
        nl++;
        line_val_off[nl] = nv;
        at += line.size() + 1;
    }
    return nl;
}
