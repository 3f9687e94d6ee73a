// TaxDB.h — the NCBI taxonomy dump as `taxscreen` needs it (taxdb.hpp:26-236): nodes.dmp and
// names.dmp parsed into dense node arrays for the device (fpm_screen_tax), the reference ->
// taxID rules of CommandTaxScreen.cpp:127-180, and writeReport from the arrays that come back.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

namespace fpmhost {

using TaxID = uint64_t;

class TaxDB {
public:
    // parseNodesDump + parseNamesDump + the parent links (taxdb.hpp:85-156).  False with
    // `error` set when a file cannot be read or a parent chain never reaches a root.
    bool load(const std::string &namesDumpFile, const std::string &nodesDumpFile,
              std::string &error);

    // nodes in nodes.dmp order
    std::vector<TaxID> ids;
    std::vector<std::string> rank, name;
    std::vector<uint32_t> parent;   // node index, FPM_TAX_ROOT for a root
    std::vector<uint32_t> depth;    // links up to the root
    uint32_t top = 0;               // the node of taxID 1, FPM_TAX_UNKNOWN without one
    std::unordered_map<TaxID, uint32_t> index;

    // FPM_TAX_NONE for taxID 0, FPM_TAX_UNKNOWN for a taxID without a node
    uint32_t nodeOf(TaxID taxID) const;

    // writeReport (taxdb.hpp:192-236) from per-node arrays
    void writeReport(FILE *fp, const std::vector<uint32_t> &taxCount,
                     const std::vector<uint32_t> &taxHashCount,
                     const std::vector<uint32_t> &cladeCount,
                     const std::vector<uint32_t> &cladeHashCount, uint64_t totalCounts) const;
};

// the mapping file (CommandTaxScreen.cpp:137-142): taxID, one separator byte, the rest of the
// line as the reference name; the first line of a name wins.  False when it cannot be read.
bool readTaxMapping(const std::string &file, std::unordered_map<std::string, TaxID> &out);
// the number after each word `taxid` of a comment, the last one wins; a failed read ends the
// scan with 0 (:163-170)
TaxID commentTaxID(const std::string &comment);

}  // namespace fpmhost
