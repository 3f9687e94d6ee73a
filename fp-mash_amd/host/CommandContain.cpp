// CommandContain.cpp — `fpmash contain` (CommandContain.cpp:20-300): same inputs as dist (a
// .msh or sequence reference, queries as .msh / sequence files / -l lists), same messages, the
// same query-major ordered text.  The walk of every ref x query pair (containSketches,
// :368-412) runs on the MI355X (fpm_contain_dev), which returns the walk's two integers; score
// and error bound are formed here in double exactly as the reference writes them (:408-411).
#include "CommandContain.h"
#include "Device.h"
#include "Sketch.h"
#include "SketchRows.h"
#include "TextOut.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>

namespace fpmhost {

CommandContain::CommandContain()
{
    name = "contain";
    summary = "Estimate the containment of query sequences within references.";
    description = "Estimate the containment of each query file (or sequence with -i) in the "
                  "reference. Both the reference and queries can be fasta or fastq, gzipped or "
                  "not, or mash sketch files (.msh) with matching k-mer sizes. Query files can "
                  "also be files of file names (see -l). The score is the number of intersecting "
                  "min-hashes divided by the query set size. The output format is [score, "
                  "error-bound, reference-ID, query-ID].";
    argumentString = "<reference> <query> [<query>] ...";
    addOption("list", Option(Option::Boolean, "l", "Input",
        "List input. Each query file contains a list of sequence files, one per line. The "
        "reference file is not affected.", ""));
    addOption("errorThreshold", Option(Option::Number, "e", "Output",
        "Error bound threshold for reporting scores values. Error bounds can generally be "
        "increased by increasing the sketch size of the reference.", "0.05"));
    useOption("help");
    useSketchOptions();
}

namespace {

// one packed sketch set on the device
struct DeviceRows {
    void *rows = nullptr, *len = nullptr;
    uint64_t stride = 1;
    uint32_t n = 0;
    void upload(const PackedRows &p)
    {
        stride = p.width;
        n = (uint32_t)p.n;
        check(fpm_malloc(device(), &rows, p.bytes()), "contain");
        check(fpm_malloc(device(), &len, (size_t)n * 4), "contain");
        check(fpm_memcpy_h2d(device(), rows, p.data(), p.bytes()), "contain");
        check(fpm_memcpy_h2d(device(), len, p.len.data(), (size_t)n * 4), "contain");
    }
    void release()
    {
        if (rows) fpm_free(device(), rows);
        if (len) fpm_free(device(), len);
        rows = len = nullptr;
    }
};

}  // namespace

int CommandContain::run() const
{
    if (arguments.size() < 2 || options.at("help").active) {
        print();
        return 0;
    }
    const bool list = options.at("list").active;
    Parameters parameters;
    parameters.error = options.at("errorThreshold").getArgumentAsNumber();
    if (sketchParameterSetup(parameters, *this)) return 1;

    Sketch sketchRef;
    const std::string &fileReference = arguments[0];
    const bool isSketch = hasSuffix(fileReference, suffixSketch);
    if (isSketch) {
        // (CommandContain.cpp:111-131: -k and -n stop the run; the -a / -z messages print and
        // the run goes on.  Unlike dist's, these name the option without its dash.)
        if (refuseSketchOptions(*this, "", false)) return 1;
    } else {
        std::cerr << "Sketching " << fileReference
                  << " (provide sketch file made with \"mash sketch\" to skip)...";
    }
    warmDevices();
    std::vector<std::string> refArg{fileReference};
    sketchRef.initFromFiles(refArg, parameters);
    if (isSketch) {
        inheritFromSketch(parameters, sketchRef);
    } else {
        std::cerr << "done.\n";
    }
    const std::vector<std::string> queryFiles = inputFiles(arguments, 1, list);
    Sketch sketchQuery;
    sketchQuery.initFromFiles(queryFiles, parameters, 0, true, true);

    const uint64_t nR = sketchRef.getReferenceCount(), nQ = sketchQuery.getReferenceCount();
    if (!nR || !nQ) return 0;
    // writeOutput(ContainOutput *, float error) (:264): the threshold is compared as a float
    const double errorMax = (double)(float)parameters.error;
    const bool use64 = sketchRef.getUse64();
    DeviceRows R, Q;
    R.upload(PackedRows(sketchRef.references, use64));
    Q.upload(PackedRows(sketchQuery.references, use64));
    const uint32_t hb = use64 ? 8 : 4;

    // query-row blocks of at most 2^25 pairs: 8 B per pair on the device and on the host
    const uint64_t qBlock = std::max<uint64_t>(1, (uint64_t(1) << 25) / nR);
    const uint64_t cells = std::min(nQ, qBlock) * nR;
    void *dCommon = nullptr, *dSteps = nullptr;
    check(fpm_malloc(device(), &dCommon, cells * 4), "contain");
    check(fpm_malloc(device(), &dSteps, cells * 4), "contain");
    std::vector<uint32_t> common(cells), steps(cells);
    StdoutText text;
    std::string &out = text.buf;
    for (uint64_t q0 = 0; q0 < nQ; q0 += qBlock) {
        const uint64_t nq = std::min(qBlock, nQ - q0);
        check(fpm_contain_dev(device(), R.rows, (const uint32_t *)R.len, R.stride, (uint32_t)nR,
                              (const uint8_t *)Q.rows + q0 * Q.stride * hb,
                              (const uint32_t *)Q.len + q0, Q.stride, (uint32_t)nq, hb,
                              (uint32_t *)dCommon, (uint32_t *)dSteps, nullptr),
              "contain");
        check(fpm_memcpy_d2h(device(), common.data(), dCommon, nq * nR * 4), "contain");
        check(fpm_memcpy_d2h(device(), steps.data(), dSteps, nq * nR * 4), "contain");
        for (uint64_t q = 0; q < nq; q++) {
            const std::string &qname = sketchQuery.getReference(q0 + q).name;
            for (uint64_t r = 0; r < nR; r++) {
                const uint32_t j = steps[q * nR + r];
                const double error = 1. / sqrt((double)j);
                if (!(error <= errorMax)) continue;
                const double score = double(common[q * nR + r]) / (double)j;
                putNum(out, score);
                out += '\t';
                putNum(out, error);
                out += '\t';
                out += sketchRef.getReference(r).name;
                out += '\t';
                out += qname;
                out += '\n';
            }
            text.flushIfLarge();
        }
    }
    text.finish();
    fpm_free(device(), dCommon);
    fpm_free(device(), dSteps);
    R.release();
    Q.release();
    return 0;
}

}  // namespace fpmhost
