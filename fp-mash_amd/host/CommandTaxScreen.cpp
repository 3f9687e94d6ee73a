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
    if (!hasSuffix(arguments[0], suffixSketch)) {
        std::cerr << "ERROR: " << arguments[0] << " does not look like a sketch (.msh)" << std::endl;
        return 1;
    }
    const std::string taxonomyDir = options.at("taxonomy-dir").argument;
    const std::string mappingFileName = options.at("mapping-file").argument;

    Sketch sketch;
    Parameters parameters;
    sketch.initFromFiles({arguments[0]}, parameters);
    phaseMark("load database");
    std::string alphabet;
    sketch.getAlphabetAsString(alphabet);
    if (alphabet == alphabetProtein) {
        std::cerr << "ERROR: " << arguments[0] << " is an amino acid sketch; translated screening "
                     "is not supported" << std::endl;
        return 1;
    }
    const std::string namesDumpFile = taxonomyDir + "/names.dmp";
    const std::string nodesDumpFile = taxonomyDir + "/nodes.dmp";
    if (!fileExists(namesDumpFile) || !fileExists(nodesDumpFile)) {   // (:114-122)
        std::cerr << "ERROR: Could not find a file names.dmp or nodes.dmp in directory "
                  << taxonomyDir << std::endl;
        return 1;
    }
    // (:229-250; checked before any device work)
    for (size_t f = 1; f < arguments.size(); f++) {
        if (arguments[f] == "-") {
            if (f > 1) {
                std::cerr << "ERROR: '-' for stdin must be first query" << std::endl;
                return 1;
            }
        } else if (FILE *fp = fopen(arguments[f].c_str(), "r")) {
            fclose(fp);
        } else {
            std::cerr << "ERROR: could not open " << arguments[f] << std::endl;
            return 1;
        }
    }

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
    const int kmerSize = sketch.getKmerSize();
    const bool use64 = sketch.getUse64();
    const uint32_t hb = use64 ? 8 : 4;

    std::cerr << "Loading " << arguments[0] << "..." << std::endl;
    uint64_t stride = 1;
    for (uint64_t i = 0; i < nRef; i++)
        stride = std::max<uint64_t>(stride, sketch.getReference(i).hashes.size());
    std::vector<uint8_t> M((size_t)nRef * stride * hb, 0);
    std::vector<uint32_t> L(nRef);
    for (uint64_t i = 0; i < nRef; i++) {
        const Reference &r = sketch.getReference(i);
        L[i] = (uint32_t)r.hashes.size();
        for (uint64_t j = 0; j < r.hashes.size(); j++) {
            if (use64) memcpy(&M[(i * stride + j) * 8], &r.hashes[j], 8);
            else { const uint32_t v = (uint32_t)r.hashes[j]; memcpy(&M[(i * stride + j) * 4], &v, 4); }
        }
    }
    fpm_ctx *ctx = device();
    fpm_screen *sc = nullptr;
    const uint32_t s = (uint32_t)std::max<uint64_t>(1, sketch.parameters.minHashesPerWindow);
    const int rc = fpm_screen_create(ctx, M.data(), L.data(), stride, (uint32_t)nRef, hb, s, &sc);
    if (rc == FPM_EINVAL) {
        std::cerr << "ERROR: " << arguments[0] << ": taxscreen needs sketches whose hashes are in "
                     "strictly ascending order (" << fpm_last_error() << ")" << std::endl;
        return 1;
    }
    check(rc, "taxscreen");
    std::vector<uint8_t>().swap(M);
    uint64_t nDistinct = 0;
    check(fpm_screen_counts(sc, nullptr, nullptr, &nDistinct), "taxscreen");
    std::cerr << "   " << nDistinct << " distinct hashes." << std::endl;          // (:201)
    phaseMark("database table");

    const size_t queryCount = arguments.size() - 1;                               // (:207-219)
    std::cerr << "Streaming from ";
    if (queryCount == 1) std::cerr << arguments[1];
    else std::cerr << queryCount << " inputs";
    std::cerr << "..." << std::endl;

    Pool pool{ctx, sc, {}};
    pool.fp.kmer_size = (uint32_t)kmerSize;
    pool.fp.sketch_size = s;
    pool.fp.seed = sketch.getHashSeed();
    pool.fp.use64 = use64;
    pool.fp.noncanonical = sketch.getNoncanonical();
    pool.fp.preserve_case = sketch.getPreserveCase();
    for (int c = 0; c < 256; c++) pool.fp.alphabet[c] = sketch.parameters.alphabet[c] ? 1 : 0;

    // one file image at a time: device and host memory follow the largest file's slices
    for (size_t f = 1; f < arguments.size(); f++) {
        std::string image;
        if (!loadSequenceFile(arguments[f], image)) {
            std::cerr << "ERROR: could not open " << arguments[f] << std::endl;
            return 1;
        }
        if (!pool.file(image)) {
            std::cerr << "\nERROR: reading inputs" << std::endl;
            return 1;
        }
    }
    phaseMark("pool (read + parse + sketch + count)");
    if (pool.records == 0) {                                                      // (:363-368)
        std::cerr << "\nERROR: Did not find sequence records in inputs" << std::endl;
        return 1;
    }
    uint64_t setSize = 0;
    check(fpm_screen_set_size(sc, &setSize), "taxscreen");
    std::cerr << "   Estimated distinct k-mers in pool: " << setSize << std::endl;   // (:371-376)
    if (setSize == 0) std::cerr << "WARNING: no valid k-mers in input." << std::endl;

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
