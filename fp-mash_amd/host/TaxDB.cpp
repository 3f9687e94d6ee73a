// TaxDB.cpp — see TaxDB.h.  The two dump parsers restate the stream calls of
// taxdb.hpp:105-156 over a byte cursor, so a file the reference reads gives the same taxa here.
#include "TaxDB.h"

#include "fpmash.h"

#include <algorithm>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

namespace fpmhost {

namespace {

bool slurp(const std::string &file, std::string &out)
{
    std::ifstream in(file, std::ios::binary);
    if (!in.is_open()) return false;
    std::ostringstream ss;
    ss << in.rdbuf();
    out = ss.str();
    return true;
}

inline bool isSpace(char c)
{
    return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r';
}

// a byte cursor with the istream calls the reference's parsers make
struct In {
    const std::string &b;
    size_t at = 0;
    explicit In(const std::string &s) : b(s) {}

    void skipSpace() { while (at < b.size() && isSpace(b[at])) at++; }
    // operator>>(uint64_t &): false when no digits follow or the value does not fit
    bool uint(uint64_t &v)
    {
        skipSpace();
        size_t p = at;
        if (p < b.size() && b[p] == '+') p++;
        const size_t first = p;
        uint64_t x = 0;
        bool fits = true;
        for (; p < b.size() && b[p] >= '0' && b[p] <= '9'; p++) {
            const uint64_t d = (uint64_t)(b[p] - '0');
            if (x > (UINT64_MAX - d) / 10) fits = false;
            x = x * 10 + d;
        }
        if (p == first) return false;
        at = p;
        v = x;
        return fits;
    }
    // operator>>(char &)
    bool chr()
    {
        skipSpace();
        if (at >= b.size()) return false;
        at++;
        return true;
    }
    void ignore(size_t n) { at = std::min(b.size(), at + n); }
    void ignore(size_t n, char delim)
    {
        const size_t end = std::min(b.size(), at + n);
        const void *hit = memchr(b.data() + at, delim, end - at);
        at = hit ? (size_t)((const char *)hit - b.data()) + 1 : end;
    }
    // getline(in, s, delim)
    std::string upto(char delim)
    {
        const size_t i = b.find(delim, at);
        const size_t end = i == std::string::npos ? b.size() : i;
        std::string s = b.substr(at, end - at);
        at = i == std::string::npos ? b.size() : i + 1;
        return s;
    }
};

}  // namespace

bool TaxDB::load(const std::string &namesDumpFile, const std::string &nodesDumpFile,
                 std::string &error)
{
    std::string text;
    if (!slurp(nodesDumpFile, text)) {
        error = "unable to open nodes file " + nodesDumpFile;
        return false;
    }
    // parseNodesDump (taxdb.hpp:105-127): taxID | parent | rank |; the first line of a taxID wins
    std::vector<TaxID> parentID;
    {
        In f(text);
        for (;;) {
            TaxID taxID = 0, parentTaxID = 0;
            if (!f.uint(taxID) || !f.chr() || !f.uint(parentTaxID) || !f.chr()) break;
            f.ignore(1);
            std::string r = f.upto('\t');
            if (index.emplace(taxID, (uint32_t)ids.size()).second) {
                ids.push_back(taxID);
                parentID.push_back(parentTaxID);
                rank.push_back(std::move(r));
            }
            f.ignore(2560, '\n');
        }
    }
    if (ids.size() > 0xFFFFFFF0ull) {
        error = nodesDumpFile + " holds too many taxa";
        return false;
    }
    // parent links (taxdb.hpp:89-100): its own parent is a root; so is, here, a node whose parent
    // has no line (the reference leaves that pointer uninitialised)
    const uint32_t n = (uint32_t)ids.size();
    parent.assign(n, FPM_TAX_ROOT);
    for (uint32_t v = 0; v < n; v++) {
        if (parentID[v] == ids[v]) continue;
        auto p = index.find(parentID[v]);
        if (p == index.end())
            std::cerr << "Could not find parent with tax ID " << parentID[v] << " for tax ID "
                      << ids[v] << std::endl;
        else
            parent[v] = p->second;
    }
    // depths, and with them the proof that every chain ends: walk up to the first node whose
    // depth is known, then number the path back down
    constexpr uint32_t kUnset = 0xFFFFFFFFu;
    depth.assign(n, kUnset);
    std::vector<uint32_t> path;
    for (uint32_t v = 0; v < n; v++) {
        if (depth[v] != kUnset) continue;
        path.clear();
        uint32_t x = v, base = 0;
        for (;;) {
            if (path.size() > n) {
                error = nodesDumpFile + ": the parent chain of tax ID " + std::to_string(ids[v]) +
                        " never reaches a root";
                return false;
            }
            path.push_back(x);
            const uint32_t p = parent[x];
            if (p == FPM_TAX_ROOT) { base = 0; break; }
            if (depth[p] != kUnset) { base = depth[p] + 1; break; }
            x = p;
        }
        for (size_t i = path.size(); i-- > 0;) depth[path[i]] = base + (uint32_t)(path.size() - 1 - i);
    }
    auto one = index.find(1);
    top = one == index.end() ? FPM_TAX_UNKNOWN : one->second;

    // parseNamesDump (taxdb.hpp:129-156): only `scientific name` lines, the last one wins
    name.assign(n, std::string());
    if (!slurp(namesDumpFile, text)) {
        error = "unable to open names file " + namesDumpFile;
        return false;
    }
    In f(text);
    for (;;) {
        TaxID taxID = 0;
        if (!f.uint(taxID)) break;
        f.ignore(3);
        std::string nm = f.upto('\t');
        f.ignore(3);
        f.ignore(256, '|');
        f.ignore(1);
        const std::string type = f.upto('\t');
        if (type == "scientific name") {
            auto it = index.find(taxID);
            if (it == index.end())
                std::cerr << "Entry for " << taxID << " does not exist - it should!" << '\n';
            else
                name[it->second] = std::move(nm);
        }
        f.ignore(2560, '\n');
    }
    std::cerr << "   " << ids.size() << " distinct taxa\n";
    return true;
}

uint32_t TaxDB::nodeOf(TaxID taxID) const
{
    if (taxID == 0) return FPM_TAX_NONE;
    auto it = index.find(taxID);
    return it == index.end() ? FPM_TAX_UNKNOWN : it->second;
}

void TaxDB::writeReport(FILE *fp, const std::vector<uint32_t> &taxCount,
                        const std::vector<uint32_t> &taxHashCount,
                        const std::vector<uint32_t> &cladeCount,
                        const std::vector<uint32_t> &cladeHashCount, uint64_t totalCounts) const
{
    // (taxdb.hpp:206: the column names say taxID, rank; the rows print rank, taxID)
    fprintf(fp, "%%\thashes\ttaxHashes\thashesDB\ttaxHashesDB\ttaxID\trank\tname\n");
    if (top == FPM_TAX_UNKNOWN) return;
    // a taxon's children: those with any tally in their clade (:422-429), as one list per
    // parent in ascending node order
    const uint32_t n = (uint32_t)ids.size();
    std::vector<uint32_t> kidStart(n + 1, 0), kids;
    for (uint32_t v = 0; v < n; v++)
        if (parent[v] != FPM_TAX_ROOT && cladeHashCount[v]) kidStart[parent[v] + 1]++;
    for (uint32_t v = 0; v < n; v++) kidStart[v + 1] += kidStart[v];
    kids.resize(kidStart[n]);
    {
        std::vector<uint32_t> fill(kidStart.begin(), kidStart.end() - 1);
        for (uint32_t v = 0; v < n; v++)
            if (parent[v] != FPM_TAX_ROOT && cladeHashCount[v]) kids[fill[parent[v]]++] = v;
    }
    // the recursion of :213-235 from taxID 1 on an explicit stack; children by cladeCount
    // descending, ties by ascending taxID (the reference's std::sort leaves ties open)
    std::vector<std::pair<uint32_t, uint32_t>> stack{{top, 0}};
    std::vector<uint32_t> order;
    while (!stack.empty()) {
        const auto [v, d] = stack.back();
        stack.pop_back();
        if (cladeCount[v] == 0) continue;
        fprintf(fp, "%.4f\t%i\t%i\t%i\t%i\t%s\t%lu\t%s%s\n",
                100 * cladeCount[v] / double(totalCounts), (int)cladeCount[v], (int)taxCount[v],
                (int)cladeHashCount[v], (int)taxHashCount[v], rank[v].c_str(),
                (unsigned long)ids[v], std::string(2 * (size_t)d, ' ').c_str(), name[v].c_str());
        order.assign(kids.begin() + kidStart[v], kids.begin() + kidStart[v + 1]);
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return cladeCount[a] != cladeCount[b] ? cladeCount[a] > cladeCount[b] : ids[a] < ids[b];
        });
        for (size_t i = order.size(); i-- > 0;) stack.push_back({order[i], d + 1});
    }
}

bool readTaxMapping(const std::string &file, std::unordered_map<std::string, TaxID> &out)
{
    std::string text;
    if (!slurp(file, text)) return false;
    In f(text);
    for (;;) {
        TaxID taxID = 0;
        if (!f.uint(taxID)) break;
        f.ignore(1);
        out.emplace(f.upto('\n'), taxID);
    }
    return true;
}

TaxID commentTaxID(const std::string &comment)
{
    In f(comment);
    TaxID taxID = 0;
    for (;;) {
        f.skipSpace();
        const size_t from = f.at;
        while (f.at < comment.size() && !isSpace(comment[f.at])) f.at++;
        if (f.at == from) return taxID;
        if (comment.compare(from, f.at - from, "taxid") == 0 && !f.uint(taxID)) return 0;
    }
}

}  // namespace fpmhost
