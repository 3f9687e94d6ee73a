// CommandKFinger.cpp — `fpmash kfinger`: FASTA / FASTQ records -> CFL k-finger lines on the
// device (fpm_kfinger_*: the cyclic windows, Duval and the line text of lyn2vec's
// fingerprint_utils.py:95-110, 443-476 and factorizations.py:102-126), or with -F the ICFL or
// CFL_ICFL-T lines (ICFL_recursive, CFL_icfl, factorizations.py:143-248, 265-301; the names of
// lyn2vec.py:47-59) or their combined forms CFL_COMB, ICFL_COMB and CFL_ICFL_COMB-T (d_cfl, d_icfl,
// d_cfl_icfl, factorizations_comb.py:178-246; lyn2vec.py:60-72).  By default the lines
// are written as one text, the input of `sketch -fp`; with -S they are hashed where they are
// made (getHashFingerPrint, hash.cpp:45-73) and grouped into the References
// Sketch::initFromFingerprints (Sketch.cpp:56-151) makes of that text, so the .msh is the one
// `sketch -fp` writes for it, with no text in between.  Records are found by kseq's rules, like
// every other verb's; the inputs are streamed in slices of whole records bounded by bytes.
// -L N is lyn2vec's long-read mode (`--type generalized --split N`, lyn2vec.py:100-177,
// fingerprint_utils.py:114-130, 480-518): a record's consecutive pieces of N bases are factorized
// each on its own and the record is one line; -f writes the factor text of `--fact create`
// (fingerprint_utils.py:471-474, 509-511) beside the k-finger text, in either mode.
#include "CommandKFinger.h"
#include "Device.h"
#include "ParsedFile.h"
#include "SeqReader.h"
#include "Sketch.h"
#include "Timing.h"

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>

namespace fpmhost {

namespace {

const uint64_t kLimitReadFingerprint = 1000000;   // Sketch.cpp:37

// sequence bytes per slice (FPMASH_KFINGER_SLICE overrides, in bytes): a slice of n bases makes
// up to n lines
size_t kfingerSliceBytes()
{
    const char *v = getenv("FPMASH_KFINGER_SLICE");
    const long long n = v ? atoll(v) : 0;
    return n > 0 ? (size_t)n : (size_t)16 << 20;
}

uint32_t maxWindow()
{
    uint32_t w = 0;
    fpm_kfinger_limits(&w, nullptr);
    return w;
}

// The ID of a record's lines: the first whitespace-separated token of its comment (lyn2vec's
// s_list[1]), or its name when the header has no comment, then "_0" (the forward strand; lyn2vec
// writes no other, fingerprint_utils.py:276-307).
std::string lineId(const std::string &name, const std::string &comment)
{
    size_t a = 0;
    while (a < comment.size() && isspace((unsigned char)comment[a])) a++;
    size_t b = a;
    while (b < comment.size() && !isspace((unsigned char)comment[b])) b++;
    return (b > a ? comment.substr(a, b - a) : name) + "_0";
}

// the factor text's path beside the k-finger text's: <prefix>.fact.txt for <prefix>.txt
std::string factPathOf(const std::string &textPath)
{
    return textPath.substr(0, textPath.size() - 4) + ".fact.txt";
}

// lyn2vec's --type_factorization spelling -> FPM_KF_*, the threshold and whether the form is a
// combined one: CFL, ICFL, or CFL_ICFL-<T> with T in 1 .. the widest window, plain decimal
// digits; CFL_COMB, ICFL_COMB or CFL_ICFL_COMB-<T> by the same rules
bool parseFactorization(const std::string &name, uint32_t &kind, uint32_t &threshold, bool &comb)
{
    threshold = 0;
    comb = false;
    if (name == "CFL") { kind = FPM_KF_CFL; return true; }
    if (name == "ICFL") { kind = FPM_KF_ICFL; return true; }
    if (name == "CFL_COMB") { kind = FPM_KF_CFL; comb = true; return true; }
    if (name == "ICFL_COMB") { kind = FPM_KF_ICFL; comb = true; return true; }
    std::string head = "CFL_ICFL-";
    if (name.compare(0, head.size(), head) != 0) {
        head = "CFL_ICFL_COMB-";
        if (name.compare(0, head.size(), head) != 0) return false;
        comb = true;
    }
    const std::string t = name.substr(head.size());
    if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
        return false;
    const unsigned long v = strtoul(t.c_str(), nullptr, 10);
    if (v < 1 || v > maxWindow()) return false;
    kind = FPM_KF_CFL_ICFL;
    threshold = (uint32_t)v;
    return true;
}

struct Generator {
    fpm_ctx *ctx = nullptr;
    uint32_t window = 100;
    uint32_t factKind = FPM_KF_CFL, factThreshold = 0;
    bool factComb = false;
    uint32_t split = 0;                   // -L: the long-read mode's piece length (0: windows)
    bool factText = false;                // -f
    bool sketch = false;
    uint32_t seed = 42;
    bool use64 = false;
    std::string outPath;
    FILE *out = nullptr;
    std::string factPath;
    FILE *factOut = nullptr;
    uint64_t records = 0;                 // kseq records read, empty ones included
    uint64_t linesLeft = ~0ull;           // -S: what is left of the 1,000,000 lines (Sketch.cpp:37, 82)
    // -S: the lines' hashes and their References so far
    std::vector<uint64_t> h64;
    std::vector<uint32_t> h32;
    std::vector<FingerprintRef> heads;
    bool haveId = false;
    std::string lastId;

    bool done() const { return sketch && linesLeft == 0; }

    [[noreturn]] void die(const std::string &msg)
    {
        if (out) {
            fclose(out);
            remove(outPath.c_str());
        }
        if (factOut) {
            fclose(factOut);
            remove(factPath.c_str());
        }
        std::cerr << "ERROR: " << msg << std::endl;
        fatalExit();
    }

    void openText()
    {
        if (out || sketch) return;
        out = fopen(outPath.c_str(), "wb");
        if (!out) die("could not open " + outPath + " for writing.");
        if (!factText) return;
        factOut = fopen(factPath.c_str(), "wb");
        if (!factOut) die("could not open " + factPath + " for writing.");
    }

    // a record's ID: the long-read mode's is the name alone (lyn2vec appends "_0" only under
    // --rev_comb true, lyn2vec.py:179-183)
    std::string idOf(const std::string &name, const std::string &comment) const
    {
        return split ? name : lineId(name, comment);
    }

    // Run a staged job over records with the IDs `ids` and take its lines.  false: the job's
    // text would reach 2^32 bytes (nothing was taken; the caller splits its records).
    bool consume(fpm_kfinger *job, uint64_t n, const std::vector<std::string> &ids)
    {
        std::unique_ptr<fpm_kfinger, void (*)(fpm_kfinger *)> hold(job, fpm_kfinger_free);
        if (factKind != FPM_KF_CFL)
            check(fpm_kfinger_set_factorization(job, factKind, factThreshold), "kfinger");
        if (factComb) check(fpm_kfinger_set_comb(job, 1), "kfinger");
        check(fpm_kfinger_run(job, seed, use64, nullptr), "kfinger");
        if (sketch) {
            std::vector<uint64_t> first(ids.size() + 1);
            std::vector<uint32_t> nv(n);
            const size_t at = use64 ? h64.size() : h32.size();
            if (use64) h64.resize(at + n);
            else h32.resize(at + n);
            check(fpm_kfinger_fetch(job, first.data(),
                                    use64 ? (void *)(h64.data() + at) : (void *)(h32.data() + at),
                                    nv.data()),
                  "kfinger");
            for (size_t r = 0; r < ids.size(); r++) {
                if (first[r + 1] == first[r]) continue;
                // a new Reference where the ID changes (Sketch.cpp:104-129)
                if (!haveId || ids[r] != lastId) {
                    heads.push_back(FingerprintRef{ids[r], at + first[r], nv[first[r]]});
                    lastId = ids[r];
                    haveId = true;
                }
                for (uint64_t l = first[r]; l < first[r + 1]; l++) heads.back().length += nv[l];
            }
            linesLeft -= n;
            return true;
        }
        std::string blob;
        std::vector<uint64_t> off(ids.size() + 1, 0);
        for (size_t r = 0; r < ids.size(); r++) {
            blob += ids[r];
            off[r + 1] = blob.size();
        }
        // both texts are sized before either is written
        uint64_t bytes = 0, factBytes = 0;
        int rc = fpm_kfinger_text(job, blob.data(), off.data(), nullptr, 0, &bytes);
        if (rc == FPM_EINVAL && bytes > 0xFFFFFFFFull) return false;
        check(rc, "kfinger");
        if (factText) {
            rc = fpm_kfinger_fact_text(job, blob.data(), off.data(), nullptr, 0, &factBytes);
            if (rc == FPM_EINVAL && factBytes > 0xFFFFFFFFull) return false;
            check(rc, "kfinger");
        }
        openText();
        if (factText) {
            std::unique_ptr<char[]> text(new char[factBytes ? factBytes : 1]);
            check(fpm_kfinger_fact_text(job, blob.data(), off.data(), text.get(), factBytes,
                                        &factBytes),
                  "kfinger");
            if (fwrite(text.get(), 1, factBytes, factOut) != factBytes)
                die("could not write " + factPath + ".");
        }
        std::unique_ptr<char[]> text(new char[bytes ? bytes : 1]);
        check(fpm_kfinger_text(job, blob.data(), off.data(), text.get(), bytes, &bytes), "kfinger");
        if (fwrite(text.get(), 1, bytes, out) != bytes) die("could not write " + outPath + ".");
        return true;
    }

    // host records [lo, hi) of one slice
    void hostJob(const std::string &packed, const std::vector<uint64_t> &off,
                 const std::vector<std::string> &ids, size_t lo, size_t hi)
    {
        if (lo == hi || done()) return;
        fpm_kfinger *job = nullptr;
        uint64_t n = 0;
        if (split)
            check(fpm_kfinger_stage_split(ctx, packed.data(), off.data() + lo, (uint32_t)(hi - lo),
                                          split, &job, &n),
                  "kfinger");
        else
            check(fpm_kfinger_stage(ctx, packed.data(), off.data() + lo, (uint32_t)(hi - lo),
                                    window, linesLeft, &job, &n),
                  "kfinger");
        if (consume(job, n, std::vector<std::string>(ids.begin() + lo, ids.begin() + hi))) return;
        if (hi - lo == 1)
            die("the k-finger text of record " + ids[lo] + " reaches 2^32 bytes; one record is "
                "not split over jobs.");
        hostJob(packed, off, ids, lo, lo + (hi - lo) / 2);
        hostJob(packed, off, ids, lo + (hi - lo) / 2, hi);
    }

    // records walked on the host by kseq's rules, given to the device `budget` bytes at a time
    bool hostWalk(const std::string &image, size_t budget)
    {
        SeqReader rd(image.data(), image.size());
        std::string packed;
        std::vector<uint64_t> off{0};
        std::vector<std::string> ids;
        auto flush = [&] {
            hostJob(packed, off, ids, 0, ids.size());
            packed.clear();
            off.assign(1, 0);
            ids.clear();
        };
        int l;
        while ((l = rd.read()) >= 0) {
            records++;
            if (done()) continue;
            if (!ids.empty() && packed.size() + rd.seq.size() > budget) flush();
            packed += rd.seq;
            off.push_back(packed.size());
            ids.push_back(idOf(rd.name, rd.comment));
        }
        flush();
        return l == -1;
    }

    // one input file: parsed and packed on the device when it fits a slice and has no FASTQ
    // quality lines, else walked on the host
    bool file(const std::string &image)
    {
        const size_t budget = kfingerSliceBytes();
        if (image.size() > budget) return hostWalk(image, budget);
        bool ok = true;
        {
            ParsedFile parsed;
            if (parsed.parse(ctx, image)) {
                std::vector<uint8_t> take(parsed.nRec ? parsed.nRec : 1, 0);
                std::vector<std::string> ids(parsed.nRec);
                uint64_t found = 0;
                for (uint64_t r = 0; r < parsed.nRec; r++) {
                    if (!parsed.isRecord(r)) continue;
                    found++;
                    take[r] = 1;
                    std::string name, comment;
                    splitHeader(image.data() + parsed.headOff[r] + 1, parsed.headLen[r] - 1, name,
                                comment);
                    ids[r] = idOf(name, comment);
                }
                if (found && !done()) {
                    fpm_kfinger *job = nullptr;
                    uint64_t n = 0;
                    if (split)
                        check(fpm_kfinger_stage_split_seq(ctx, parsed.text, take.data(), split, &job,
                                                          &n),
                              "kfinger");
                    else
                        check(fpm_kfinger_stage_seq(ctx, parsed.text, take.data(), window, linesLeft,
                                                    &job, &n),
                              "kfinger");
                    ok = consume(job, n, ids);
                }
                if (ok) {
                    records += found;
                    return true;
                }
            }
        }
        return hostWalk(image, budget);   // (counts the records itself)
    }
};

}  // namespace

CommandKFinger::CommandKFinger()
{
    name = "kfinger";
    summary = "Create k-finger fingerprints (CFL, ICFL, CFL_ICFL-T, their _COMB forms) from sequences.";
    description = "Create the k-finger lines of sequences (lyn2vec --type basic "
                  "--type_factorization CFL, ICFL or CFL_ICFL-T, chosen with -F): for every "
                  "record and every cyclic window of it, the lengths of the window's Lyndon "
                  "factors (CFL), of its inverse Lyndon factors (ICFL), or of its Lyndon factors "
                  "with each one longer than T replaced by its own inverse Lyndon factors "
                  "(CFL_ICFL-T). CFL_COMB, ICFL_COMB and CFL_ICFL_COMB-T cut the window where that "
                  "factorization cuts it and, mirrored, where it cuts the window's reverse "
                  "complement (there CFL_ICFL runs at T = 30 whatever T is given, as lyn2vec's "
                  "does). Inputs can be fasta or fastq files "
                  "(gzipped or not), and \"-\" can be given to read from standard input. The lines "
                  "of all inputs are written to <prefix>.txt, the input of `sketch -fp`; with -S "
                  "they are sketched instead, into the <prefix>.msh that `sketch -fp` writes for "
                  "that text. With -L <N> the long-read fingerprints are made instead (lyn2vec "
                  "--type generalized --split N): each record is cut into consecutive pieces of N "
                  "bases, each piece is factorized on its own, and the record is one line, its "
                  "ID, two spaces, then per piece the lengths and \" | \". With -f the factors "
                  "themselves are also written, to <prefix>.fact.txt (lyn2vec --fact create): the "
                  "same lines with each factor's bases in place of its length.";
    argumentString = "<input> [<input>] ...";
    useOption("help");
    addOption("window", Option(Option::Integer, "w", "Input",
        "Window size. Each record of at least this many bases gives one line per cyclic window "
        "start, a shorter record one line.", "100", 1, maxWindow()));
    addOption("factorization", Option(Option::String, "F", "Input",
        "Factorization of a window: CFL, ICFL, CFL_ICFL-<T>, CFL_COMB, ICFL_COMB or "
        "CFL_ICFL_COMB-<T>, T from 1 to the largest window size.", "CFL"));
    addOption("long", Option(Option::String, "L", "Input",
        "Long-read mode: cut each record into consecutive pieces of this many bases (1 to the "
        "largest window size) and write one line per record. Not with -w or -S.", ""));
    addOption("prefix", Option(Option::File, "o", "Output",
        "Output prefix (first input file used if unspecified). The suffix '.txt' (or '.msh' with "
        "-S) will be appended.", ""));
    addOption("sketch", Option(Option::Boolean, "S", "Output",
        "Write the sketch of the k-finger lines (as `sketch -fp` of the text) instead of the "
        "text.", ""));
    addOption("factors", Option(Option::Boolean, "f", "Output",
        "Also write the factors themselves, one line per k-finger line, to <prefix>.fact.txt. "
        "Not with -S.", ""));
    // the sketch options of `sketch -fp` (its -w, the k-mer size warning, does not apply to
    // fingerprints; its seed is -seed here, -S and -w being taken)
    for (const char *n : {"threads", "kmer", "noncanonical", "protein", "alphabet", "case",
                          "sketchSize", "individual", "reads", "memory", "minCov", "targetCov",
                          "genome"})
        useOption(n);
    addOption("seed", Option(Option::Integer, "seed", "Sketch",
        "Seed to provide to the hash function.", "42", 0, 0xFFFFFFFF));
}

int CommandKFinger::run() const
{
    if (arguments.empty() || options.at("help").active) {
        print();
        return 0;
    }
    Parameters parameters;
    if (sketchParameterSetup(parameters, *this)) return 1;
    if (parameters.reads) {
        std::cerr << "ERROR: the reads options do not apply to k-finger lines." << std::endl;
        return 1;
    }
    // what -fp makes of the sketch options (sketchParameterSetup.cpp:100-106)
    parameters.fingerprint = true;
    parameters.kmerSize = 1;
    parameters.noncanonical = true;
    setAlphabetFromString(parameters, "0123456789");
    // (the window's range was checked when the option was read)
    const uint32_t window = (uint32_t)options.at("window").getArgumentAsNumber();
    Generator g;
    const std::string &fact = options.at("factorization").argument;
    if (!parseFactorization(fact, g.factKind, g.factThreshold, g.factComb)) {
        std::cerr << "ERROR: unknown factorization " << fact << " for -F: CFL, ICFL, CFL_ICFL-<T>, "
                  << "CFL_COMB, ICFL_COMB or CFL_ICFL_COMB-<T> with T from 1 to " << maxWindow()
                  << "." << std::endl;
        return 1;
    }
    g.sketch = options.at("sketch").active;
    g.factText = options.at("factors").active;
    if (options.at("long").active) {
        // plain decimal digits, 1 .. the widest window
        const std::string &v = options.at("long").argument;
        const bool digits = !v.empty() && v.size() <= 9 &&
                            v.find_first_not_of("0123456789") == std::string::npos;
        const unsigned long n = digits ? strtoul(v.c_str(), nullptr, 10) : 0;
        if (n < 1 || n > maxWindow()) {
            std::cerr << "ERROR: Argument to -L must be an integer from 1 to " << maxWindow()
                      << " (" << v << " given)." << std::endl;
            return 1;
        }
        if (options.at("window").active) {
            std::cerr << "ERROR: -L cuts records into pieces and takes no window: -w does not "
                      << "apply with it." << std::endl;
            return 1;
        }
        g.split = (uint32_t)n;
    }
    if (g.sketch && (g.split || g.factText)) {
        std::cerr << "ERROR: -S sketches the k-finger lines of windows: it does not apply with "
                  << (g.split ? "-L" : "-f") << "." << std::endl;
        return 1;
    }
    if (!checkInputArguments(arguments, 0, "input")) return 1;
    warmDevices();
    g.window = window;
    g.seed = parameters.seed;
    g.use64 = parameters.use64;
    if (g.sketch) g.linesLeft = kLimitReadFingerprint;
    std::string prefix;
    if (!options.at("prefix").argument.empty()) prefix = options.at("prefix").argument;
    else prefix = arguments[0] == "-" ? "stdin" : arguments[0];
    const char *suffix = g.sketch ? suffixSketch : ".txt";
    if (!hasSuffix(prefix, suffix)) prefix += suffix;
    g.outPath = prefix;
    if (g.factText) g.factPath = factPathOf(prefix);
    g.ctx = device();
    phaseMark("device context");

    // one file image at a time: device and host memory follow the slices
    for (size_t f = 0; f < arguments.size(); f++) {
        if (g.done() && g.records) break;
        std::string image;
        if (!loadSequenceFile(arguments[f], image)) g.die("could not open " + arguments[f]);
        if (!g.file(image)) g.die("reading " + arguments[f] + ".");
    }
    phaseMark("k-fingers (read + parse + factorize)");
    if (g.records == 0) g.die("Did not find sequence records in inputs");
    if (!g.sketch) {
        g.openText();   // records without a base: an empty text
        if (fclose(g.out) != 0) {
            g.out = nullptr;
            g.die("could not write " + g.outPath + ".");
        }
        g.out = nullptr;
        if (g.factOut && fclose(g.factOut) != 0) {
            g.factOut = nullptr;
            remove(g.outPath.c_str());
            g.die("could not write " + g.factPath + ".");
        }
        phaseMark("text write");
        return 0;
    }
    std::unique_ptr<Sketch> owned(new Sketch());
    const uint64_t nLines = parameters.use64 ? g.h64.size() : g.h32.size();
    owned->initFromFingerprintLines(g.heads, nLines, parameters.use64 ? g.h64.data() : nullptr,
                                    parameters.use64 ? nullptr : g.h32.data(), parameters);
    std::cerr << "Writing to " << prefix << "..." << std::endl;
    owned->writeToMsh(prefix);
    if (!cleanExit()) (void)owned.release();
    return 0;
}

}  // namespace fpmhost
