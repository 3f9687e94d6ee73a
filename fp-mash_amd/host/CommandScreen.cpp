// CommandScreen.cpp — `fpmash screen`: the documented verb (doc/man/mash-screen.1), not the
// fork's CommandScreen::run, which sketches the pool instead of streaming it and never calls
// hashSequence.  Parameters come from the .msh (CommandTaxScreen.cpp:95-105); the
// pool is streamed once through the device in bounded slices of whole records
// (fpm_screen_add_job: hashSequence's counting, CommandScreen.cpp:280-384, and the pool's one
// MinHashHeap, CommandTaxScreen.cpp:347-361); shared counts, medians, -w and p-values come back
// per reference (CommandScreen.cpp:153-253); identities are formed here in double
// (estimateIdentity, :259-278), and so are the -w scores, between the two row calls.
#include "CommandScreen.h"
#include "Device.h"
#include "ScreenPool.h"
#include "Sketch.h"
#include "Timing.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

namespace fpmhost {

CommandScreen::CommandScreen()
{
    name = "screen";
    summary = "Determine whether query sequences are within a larger mixture of sequences.";
    description = "Determine how well query sequences are contained within a mixture of "
                  "sequences. The queries must be formatted as a single Mash sketch file (.msh), "
                  "created with the `mash sketch` command. The <mixture> files can be contigs or "
                  "reads, in fasta or fastq, gzipped or not, and \"-\" can be given for <mixture> "
                  "to read from standard input. The <mixture> sequences are assumed to be "
                  "nucleotides (amino acid queries are not supported). The output fields are "
                  "[identity, shared-hashes, median-multiplicity, p-value, query-ID, "
                  "query-comment], where median-multiplicity is computed for shared hashes, based "
                  "on the number of observations of those hashes within the mixture.";
    argumentString = "<queries>.msh <mixture> [<mixture>] ...";
    useOption("help");
    useOption("threads");
    addOption("winning", Option(Option::Boolean, "w", "",
        "Winner-takes-all strategy for identity estimates. After counting hashes for each query, "
        "hashes that appear in multiple queries will be removed from all except the one with the "
        "best identity (ties broken by larger query), and other identities will be reduced. This "
        "removes output redundancy, providing a rough compositional outline.", ""));
    addOption("identity", Option(Option::Number, "i", "Output",
        "Minimum identity to report. Inclusive unless set to zero, in which case only identities "
        "greater than zero (i.e. with at least one shared hash) will be reported. Set to -1 to "
        "output everything.", "0", -1., 1.));
    addOption("pvalue", Option(Option::Number, "v", "Output", "Maximum p-value to report.", "1.0",
                               0., 1.));
}

namespace {

// estimateIdentity (CommandScreen.cpp:259-278)
double estimateIdentity(uint64_t common, uint64_t denom, int kmerSize)
{
    const double jaccard = double(common) / denom;
    if (common == denom) return 1.;
    if (common == 0) return 0.;
    return pow(jaccard, 1. / kmerSize);
}

}  // namespace

int CommandScreen::run() const
{
    if (arguments.size() < 2 || options.at("help").active) {
        print();
        return 0;
    }
    if (!hasSuffix(arguments[0], suffixSketch)) {
        std::cerr << "ERROR: " << arguments[0] << " does not look like a sketch (.msh)" << std::endl;
        return 1;
    }
    const bool winning = options.at("winning").active;
    const double pValueMax = options.at("pvalue").getArgumentAsNumber();
    const double identityMin = options.at("identity").getArgumentAsNumber();

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
    // (CommandTaxScreen.cpp:229-250; checked before any device work)
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
    warmDevices();
    const int kmerSize = sketch.getKmerSize();
    const bool use64 = sketch.getUse64();
    const uint32_t hb = use64 ? 8 : 4;
    const uint64_t nRef = sketch.getReferenceCount();

    std::cerr << "Loading " << arguments[0] << "..." << std::endl;
    uint64_t stride = 1;
    for (uint64_t i = 0; i < nRef; i++)
        stride = std::max<uint64_t>(stride, sketch.getReference(i).hashes.size());
    std::vector<uint8_t> M((size_t)nRef * stride * hb, 0);
    std::vector<uint32_t> L(nRef);
    std::vector<uint64_t> lengths(nRef);
    for (uint64_t i = 0; i < nRef; i++) {
        const Reference &r = sketch.getReference(i);
        L[i] = (uint32_t)r.hashes.size();
        lengths[i] = r.length;
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
        std::cerr << "ERROR: " << arguments[0] << ": screen needs sketches whose hashes are in "
                     "strictly ascending order (" << fpm_last_error() << ")" << std::endl;
        return 1;
    }
    check(rc, "screen");
    std::vector<uint8_t>().swap(M);
    uint64_t nDistinct = 0;
    check(fpm_screen_counts(sc, nullptr, nullptr, &nDistinct), "screen");
    std::cerr << "   " << nDistinct << " distinct hashes." << std::endl;
    phaseMark("database table");

    const size_t queryCount = arguments.size() - 1;
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
    if (pool.records == 0) {
        std::cerr << "\nERROR: Did not find sequence records in inputs" << std::endl;
        return 1;
    }
    uint64_t setSize = 0;
    check(fpm_screen_set_size(sc, &setSize), "screen");
    std::cerr << "   Estimated distinct k-mers in pool: " << setSize << std::endl;
    if (setSize == 0) std::cerr << "WARNING: no valid k-mers in input." << std::endl;

    std::vector<uint32_t> shared(nRef), median(nRef);
    check(fpm_screen_rows(sc, shared.data(), median.data()), "screen");
    if (winning) {
        std::cerr << "Reallocating to winners..." << std::endl;
        std::vector<double> scores(nRef);
        for (uint64_t i = 0; i < nRef; i++)
            scores[i] = estimateIdentity(shared[i], L[i], kmerSize);
        check(fpm_screen_rows_winner(sc, scores.data(), lengths.data(), shared.data(), median.data()),
              "screen");
    }
    std::cerr << "Computing coverage medians..." << std::endl;
    std::vector<double> pValues(nRef);
    check(fpm_screen_pvalues(sc, shared.data(), sketch.getKmerSpace(), pValues.data()), "screen");
    phaseMark("rows + p-values");

    std::cerr << "Writing output..." << std::endl;
    std::string out;
    char num[160];
    for (uint64_t i = 0; i < nRef; i++) {
        if (!(shared[i] != 0 || identityMin < 0.0)) continue;
        const double identity = estimateIdentity(shared[i], L[i], kmerSize);
        if (identity < identityMin) continue;
        const double pValue = pValues[i];
        if (pValue > pValueMax) continue;
        const Reference &r = sketch.getReference(i);
        const int n = snprintf(num, sizeof num, "%g\t%u/%u\t%u\t%g\t", identity, shared[i], L[i],
                               median[i], pValue);
        out.append(num, n);
        out += r.name;
        out += '\t';
        out += r.comment;
        out += '\n';
        if (out.size() > (1 << 22)) { fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
    }
    fwrite(out.data(), 1, out.size(), stdout);
    fflush(stdout);
    fpm_screen_free(sc);
    phaseMark("output");
    return 0;
}

}  // namespace fpmhost
