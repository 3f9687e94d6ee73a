// CommandTaxScreen.cpp — `fpmash taxscreen` (CommandTaxScreen.cpp:39-446).  The taxonomy dump,
// the reference -> taxID mapping and the report are host work (TaxDB.h); the pool is streamed
// through the device exactly as `screen` streams it (ScreenPool.h); then one call,
// fpm_screen_tax, folds every distinct database hash's holders to their lowest common ancestor
// (:386-397), tallies the taxa (:398-403) and sums the clades (:406-437) on the device.
// Every refusal happens before any device work.
#include "CommandTaxScreen.h"
#include "Device.h"
#include "ScreenPool.h"
#include "Sketch.h"
#include "TaxDB.h"
#include "Timing.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

namespace fpmhost {

CommandTaxScreen::CommandTaxScreen()
{
    name = "taxscreen";
    summary = "Create Kraken-style taxonomic report based on mash screen.";
    description = "Create Kraken-style taxonomic report based on how well query sequences are "
                  "contained within a pool of sequences. The queries must be formatted as a "
                  "single Mash sketch file (.msh), created with the mash sketch command. The "
                  "<pool> files can be contigs or reads, in fasta or fastq, gzipped or not, and "
                  "\"-\" can be given for <pool> to read from standard input. The <pool> "
                  "sequences are assumed to be nucleotides (amino acid queries are not "
                  "supported). The output fields are [total percent of hashes, number of "
                  "contained hashes in the clade, number of contained hashes in the taxon, total "
                  "number of hashes in the clade, total number of hashes in the taxon, rank, "
                  "taxonomy ID, padded name].";
    argumentString = "<queries>.msh <pool> [<pool>] ...";
    useOption("help");
    useOption("threads");
    // -i and -v are parsed and unused, as in the reference (:72-73)
    addOption("identity", Option(Option::Number, "i", "Output",
        "Minimum identity to report. Inclusive unless set to zero, in which case only identities "
        "greater than zero (i.e. with at least one shared hash) will be reported. Set to -1 to "
        "output everything.", "0", -1., 1.));
    addOption("pvalue", Option(Option::Number, "v", "Output", "Maximum p-value to report.", "1.0",
                               0., 1.));
    addOption("mapping-file", Option(Option::String, "m", "",
                                     "Mapping file from reference name to taxonomy ID", ""));
    addOption("taxonomy-dir", Option(Option::String, "t", "",
                                     "Directory containing NCBI taxonomy dump", "."));
}

namespace {

// file_exists (CommandTaxScreen.cpp:33-36)
bool fileExists(const std::string &name)
{
    std::ifstream f(name.c_str());
    return f.good();
}

}  // namespace

int CommandTaxScreen::run() const
{
    if (arguments.size() < 2 || options.at("help").active) {
        print();
        return 0;
    }
    const std::string taxonomyDir = options.at("taxonomy-dir").argument;
    const std::string mappingFileName = options.at("mapping-file").argument;

    ScreenRun db{"taxscreen", arguments};
    if (!db.loadDatabase()) return 1;
    const Sketch &sketch = db.sketch;
    const std::string namesDumpFile = taxonomyDir + "/names.dmp";
    const std::string nodesDumpFile = taxonomyDir + "/nodes.dmp";
    if (!fileExists(namesDumpFile) || !fileExists(nodesDumpFile)) {   // (:114-122)
        std::cerr << "ERROR: Could not find a file names.dmp or nodes.dmp in directory "
                  << taxonomyDir << std::endl;
        return 1;
    }
    if (!db.checkPoolArguments()) return 1;

    std::cerr << "Loading taxonomy files ..." << std::endl;
    TaxDB taxdb;
    std::string error;
    if (!taxdb.load(namesDumpFile, nodesDumpFile, error)) {
        std::cerr << "ERROR: " << error << std::endl;
        return 1;
    }
    phaseMark("taxonomy");

    const uint64_t nRef = sketch.getReferenceCount();
    std::cerr << "Reading mapping file ..." << std::endl;
    std::vector<TaxID> referenceTaxIDs(nRef, 0);
    if (mappingFileName != "") {                                       // (:128-156)
        std::unordered_map<std::string, TaxID> refTaxMap;
        if (!readTaxMapping(mappingFileName, refTaxMap)) {
            std::cerr << "ERROR: unable to open mapping file " << mappingFileName << std::endl;
            return 1;
        }
        for (uint64_t i = 0; i < nRef; i++) {
            auto it = refTaxMap.find(sketch.getReference(i).name);
            if (it != refTaxMap.end()) referenceTaxIDs[i] = it->second;
        }
    }
    std::vector<uint32_t> refNode(nRef);
    for (uint64_t i = 0; i < nRef; i++) {                              // (:157-180)
        if (referenceTaxIDs[i] == 0) referenceTaxIDs[i] = commentTaxID(sketch.getReference(i).comment);
        if (referenceTaxIDs[i] == 0)
            std::cerr << "Could not find taxID for reference " << sketch.getReference(i).name
                      << " in comment field or mapping file!" << std::endl;
        refNode[i] = taxdb.nodeOf(referenceTaxIDs[i]);
    }

    warmDevices();
    if (!db.openTable() || !db.streamPool()) return 1;
    fpm_screen *sc = db.sc;

    std::cerr << "Assigning LCA taxIDs to hashes ..." << std::endl;               // (:378)
    const size_t nNodes = taxdb.ids.size();
    std::vector<uint32_t> taxHashCount(nNodes), taxCount(nNodes), cladeHashCount(nNodes),
        cladeCount(nNodes);
    uint64_t totals[2] = {0, 0};
    check(fpm_screen_tax(sc, taxdb.parent.data(), (uint32_t)nNodes, taxdb.top, refNode.data(),
                         nullptr, taxHashCount.data(), taxCount.data(), cladeHashCount.data(),
                         cladeCount.data(), totals),
          "taxscreen");
    phaseMark("LCA + clades");

    std::cerr << "Writing output..." << std::endl;                                // (:439)
    taxdb.writeReport(stdout, taxCount, taxHashCount, cladeCount, cladeHashCount, totals[0]);
    fflush(stdout);
    fpm_screen_free(sc);
    phaseMark("output");
    return 0;
}

}  // namespace fpmhost
