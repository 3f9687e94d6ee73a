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
#include "TextOut.h"
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
    const bool winning = options.at("winning").active;
    const double pValueMax = options.at("pvalue").getArgumentAsNumber();
    const double identityMin = options.at("identity").getArgumentAsNumber();

    ScreenRun db{"screen", arguments};
    if (!db.loadDatabase() || !db.checkPoolArguments()) return 1;
    warmDevices();
    if (!db.openTable() || !db.streamPool()) return 1;
    const Sketch &sketch = db.sketch;
    fpm_screen *sc = db.sc;
    const int kmerSize = sketch.getKmerSize();
    const uint64_t nRef = sketch.getReferenceCount();
    const std::vector<uint32_t> &L = db.rows.len;
    const std::vector<uint64_t> &lengths = db.rows.length;

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
    StdoutText text;
    std::string &out = text.buf;
    char num[160];
    for (uint64_t i = 0; i < nRef; i++) {
        if (!(shared[i] != 0 || identityMin < 0.0)) continue;
        const double identity = estimateIdentity(shared[i], L[i], kmerSize);
        if (identity < identityMin) continue;
        const double pValue = pValues[i];
        if (pValue > pValueMax) continue;
        const Reference &r = sketch.getReference(i);
        char *p = numTo(num, identity);
        *p++ = '\t';
        p = uTo(p, shared[i]);
        *p++ = '/';
        p = uTo(p, L[i]);
        *p++ = '\t';
        p = uTo(p, median[i]);
        *p++ = '\t';
        p = numTo(p, pValue);
        *p++ = '\t';
        out.append(num, (size_t)(p - num));
        out += r.name;
        out += '\t';
        out += r.comment;
        out += '\n';
        text.flushIfLarge();
    }
    text.finish();
    fpm_screen_free(sc);
    phaseMark("output");
    return 0;
}

}  // namespace fpmhost
