// CommandDistance.cpp — `fpmash dist` (CommandDistance.cpp:38-333): same inputs
// (.msh, sequence files, -fp .txt / .msh), same messages, same ordered text
// output.  The shared-hash walk, distance and p-value of every ref x query pair
// run on the MI355X (fpm_dist); the host formats the lines in query-major order.
#include "Command.h"
#include "Device.h"
#include "Sketch.h"
#include "SketchRows.h"
#include "TextOut.h"
#include "Timing.h"

#include <algorithm>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <mutex>
#include <thread>

#include <fcntl.h>
#include <climits>
#include <sys/uio.h>
#include <sys/stat.h>
#include <unistd.h>

namespace fpmhost {

CommandDistance::CommandDistance()
{
    name = "dist";
    summary = "Estimate the distance of query sequences to references.";
    description = "Estimate the distance of each query sequence to the reference. Both the "
                  "reference and queries can be fasta or fastq, gzipped or not, or Mash sketch "
                  "files (.msh) with matching k-mer sizes, or (-fp) k-finger fingerprint files. "
                  "The output fields are [reference-ID, query-ID, distance, p-value, "
                  "shared-hashes].";
    argumentString = "<reference> <query> [<query>] ...";
    useOption("help");
    addOption("list", Option(Option::Boolean, "l", "Input",
        "List input. Lines in each <query> specify paths to sequence files, one per line. The "
        "reference file is not affected.", ""));
    addOption("table", Option(Option::Boolean, "t", "Output",
        "Table output (will not report p-values, but fields will be blank if they do not meet "
        "the p-value threshold).", ""));
    addOption("pvalue", Option(Option::Number, "v", "Output", "Maximum p-value to report.",
                               "1.0", 0., 1.));
    addOption("distance", Option(Option::Number, "d", "Output", "Maximum distance to report.",
                                 "1.0", 0., 1.));
    addOption("comment", Option(Option::Boolean, "C", "Output",
        "Show comment fields with reference/query names (denoted with ':').", "1.0", 0., 1.));
    addOption("fingerprint", Option(Option::Boolean, "fp", "Input",
        "Indicates that the input files are fingerprints instead of sequences.", ""));
    useSketchOptions();
}

namespace {

// a list line's two numbers, two counts and four separators (numTo, uTo: TextOut.h) at most
constexpr size_t kLineNums = 2 * 32 + 2 * 20 + 4;

// Allocates the output file's pages ahead of the writer: the file's size set to an estimate of
// the text's end, then fallocate (sizes kept) in 64 MB steps from the output position, on a
// thread of its own that starts while the HIP runtime comes up and the rows are packed (idle
// cores).  pwrite into allocated tmpfs pages copies at ~9.7 GB/s against ~6.0 GB/s when every
// page is allocated on the way, and fallocate alone runs at ~18 GB/s (4 GB into /dev/shm on the
// MI355X box, tools/micro/write_rate.cpp).  The file's size stays the caller's to change; the
// pages past the final size are cut by trim().
class Prealloc {
  public:
    void start(int fd, off_t from, off_t upto)
    {
        struct stat st {};
        if (fstat(fd, &st) != 0) return;
        if (st.st_size < upto) {
            fatalCutsOutput(fd, st.st_size);    // an error exit leaves the file as it was
            if (ftruncate(fd, upto) != 0) return;
        }
        fd_ = fd;
        pos_ = from;
        upto_ = upto;
        th_ = std::thread([this] {
            // pwrite mode: only until the writer starts (allocating beside its writes made them
            // queue on the file's inode lock, CLI A/B on the box: 1.0-1.7 s against 1.05-1.28 s);
            // writes through a mapping take no inode lock and run beside it
            while (!stop_.load(std::memory_order_relaxed) && !started_.load(std::memory_order_relaxed)) {
                const off_t n = std::min<off_t>(kStep, upto_ - pos_);
                if (n <= 0 || fallocate(fd_, FALLOC_FL_KEEP_SIZE, pos_, n) != 0) break;
                pos_ += n;
            }
        });
    }
    void writerAt(off_t) { started_.store(true, std::memory_order_relaxed); }
    // stop allocating; the file cut back to `final_size` (fallocate may have extended it)
    bool trim(off_t final_size)
    {
        if (!th_.joinable()) return true;
        stop_ = true;
        th_.join();
        struct stat st {};
        return fstat(fd_, &st) != 0 || st.st_size <= final_size || ftruncate(fd_, final_size) == 0;
    }
    ~Prealloc()
    {
        stop_ = true;
        if (th_.joinable()) th_.join();
    }

  private:
    static constexpr off_t kStep = off_t(64) << 20;
    int fd_ = -1;
    off_t pos_ = 0, upto_ = 0;
    std::atomic<bool> stop_{false}, started_{false};
    std::thread th_;
};

// writes the pieces at `at` in one pwritev() per IOV_MAX pieces (short writes resumed); false on
// an error.  One call per block: the formatter threads keep formatting instead of queueing on
// the file's inode lock, which serialises writes to one file anyway (tmpfs on the MI355X box:
// one stream 5.6-6.1 GB/s; a shared mapping of the file faulted in at 3.5 GB/s and, with the
// pages allocated ahead, still lost to this path in the CLI: tools/micro/write_rate.cpp, DESIGN
// §5).
bool writePieces(int fd, off_t at, const std::vector<std::string> &pieces)
{
    std::vector<struct iovec> iov;
    iov.reserve(pieces.size());
    for (const auto &t : pieces)
        if (!t.empty()) iov.push_back({(void *)t.data(), t.size()});
    size_t i = 0;
    while (i < iov.size()) {
        const int n = (int)std::min<size_t>(iov.size() - i, IOV_MAX);
        const ssize_t w = pwritev(fd, &iov[i], n, at);
        if (w <= 0) return false;
        at += (off_t)w;
        for (size_t left = (size_t)w; left;) {
            if (left >= iov[i].iov_len) {
                left -= iov[i].iov_len;
                i++;
            } else {
                iov[i].iov_base = (char *)iov[i].iov_base + left;
                iov[i].iov_len -= left;
                left = 0;
            }
        }
    }
    return true;
}

struct DistOptions {
    bool list, table, comment, fingerprint;
    double pValueMax, distanceMax;
    bool filtered;                      // -d or -v given
};

// The reference set and the query set; `dist X.msh X.msh` has only the first
struct Inputs {
    Sketch ref, queryOwn;
    bool isSketch = false, tagMSH = false, tagTXT = false, sameSet = false;
    KmerWarning warning;
    const Sketch &query() const { return sameSet ? ref : queryOwn; }
};

// false: the run is refused (the message is printed)
bool loadReference(const Command &c, const std::string &fileReference, bool fingerprint,
                   Parameters &parameters, Inputs &in)
{
    in.isSketch = hasSuffix(fileReference, suffixSketch);
    if (in.isSketch) {
        if (refuseSketchOptions(c, "-", true)) return false;
    } else {
        std::cerr << "Sketching " << fileReference
                  << " (provide sketch file made with \"mash sketch\" to skip)...";
    }
    std::vector<std::string> refArg{fileReference};
    in.tagMSH = containsSub(refArg, ".msh");
    in.tagTXT = containsSub(refArg, ".txt");
    if (fingerprint && in.tagMSH) in.ref.initFromFiles(refArg, parameters);
    else if (fingerprint && in.tagTXT) in.ref.initFromFingerprints(refArg, parameters);
    else in.ref.initFromFiles(refArg, parameters);

    phaseMark("reference sketch loaded");
    if (in.isSketch) {
        // (CommandDistance.cpp:137-144)
        if (c.getOption("sketchSize").active && parameters.reads &&
            parameters.minHashesPerWindow != (uint64_t)in.ref.getMinHashesPerWindow()) {
            std::cerr << "ERROR: The sketch size must match the reference when using a bloom "
                         "filter (leave this option out to inherit from the reference sketch)."
                      << std::endl;
            return false;
        }
        inheritFromSketch(parameters, in.ref);
    } else {
        in.warning.scan(in.ref, parameters);
        std::cerr << "done.\n";
    }
    return true;
}

void writeTableHeader(const Sketch &ref)
{
    StdoutText out;
    out.buf = "#query";
    for (uint64_t i = 0; i < ref.getReferenceCount(); i++) {
        out.buf += '\t';
        out.buf += ref.getReference(i).name;
    }
    out.buf += '\n';
    out.finish();
}

void loadQueries(const std::vector<std::string> &arguments, const DistOptions &opt,
                 const Parameters &parameters, Inputs &in)
{
    const std::vector<std::string> queryFiles = inputFiles(arguments, 1, opt.list);
    // `dist X.msh X.msh`: the query set is the reference set (same file, same parameters), so
    // it is parsed and packed once
    in.sameSet = in.isSketch && !opt.fingerprint && queryFiles.size() == 1 &&
                 queryFiles[0] == arguments[0];
    if (in.sameSet) {}
    else if (opt.fingerprint && in.tagMSH) in.queryOwn.initFromFiles(queryFiles, parameters);
    else if (opt.fingerprint && in.tagTXT) in.queryOwn.initFromFingerprints(queryFiles, parameters);
    else in.queryOwn.initFromFiles(queryFiles, parameters, 0, true);
    phaseMark("query sketch loaded");
}

// stdout a regular file (not O_APPEND): the text goes in at its offsets, one pwritev() per
// block; otherwise (pipes, terminals) by fwrite.
struct OutputTarget {
    int fd = -1;
    off_t pos = -1;                     // direct: where the next block's text goes
    bool direct() const { return pos >= 0; }
};

OutputTarget outputTarget(bool anyPairs)
{
    std::cout.flush();
    fflush(stdout);
    OutputTarget o;
    o.fd = fileno(stdout);
    struct stat st {};
    const int fl = fcntl(o.fd, F_GETFL);
    if (anyPairs && fl >= 0 && !(fl & O_APPEND) && fstat(o.fd, &st) == 0 && S_ISREG(st.st_mode))
        o.pos = lseek(o.fd, 0, SEEK_CUR);
    return o;
}

// The list text's size, about, with no -d / -v filter: every line names its pair and most
// carry "1\t1\t0/<denom>" (pairs sharing hashes write a few bytes more, past the estimate,
// into pages allocated on the way)
off_t listTextEstimate(const Inputs &in, bool comment, uint64_t sketchSize)
{
    const uint64_t nR = in.ref.getReferenceCount(), nQ = in.query().getReferenceCount();
    uint64_t rn = 0, qn = 0;
    for (const Reference &r : in.ref.references)
        rn += r.name.size() + (comment ? 1 + r.comment.size() : 0);
    for (const Reference &r : in.query().references)
        qn += 2 + r.name.size() + (comment ? 1 + r.comment.size() : 0);
    const uint64_t digits = std::to_string(sketchSize).size();
    const long double est = (long double)nQ * rn + (long double)nR * qn +
                            (long double)nR * nQ * (7 + digits);
    return (off_t)std::min<long double>(est, (long double)(1ULL << 46));
}

// One block's results in pinned buffers, in the compact form (fpm_refset_dist_list): u16 numer /
// denom of every pair, and distance / p-value / pass of the pairs that share hashes (numer > 0);
// a pair sharing none has distance 1 (0 for two empty sketches) and p-value 1
// (CommandDistance.cpp:404-408, 435-437), its line needs nothing else.  4 B per pair over PCIe
// instead of 21.  No destructor: the buffers are unpinned only by unpin(), see run().
struct Slot {
    void *nu = nullptr, *de = nullptr;
    uint32_t *lq = nullptr, *lr = nullptr;
    double *ld = nullptr, *lp = nullptr;
    uint8_t *la = nullptr;
    uint64_t cap = 0, nl = 0;           // listed cells: room, count
    std::vector<uint32_t> rowStart;     // per query row of the block: its listed cells,
    std::vector<uint32_t> byRow;        // ordered by reference (indexes into l*)
    uint64_t b = ~0ULL;                 // block held
    std::vector<std::string> text;      // formatted pieces
    int pending = 0;                    // pieces still being formatted
    bool ready = false;
    uint64_t nextB = 0;                 // the next block this slot may take

    void freeList()
    {
        for (void *p : {(void *)lq, (void *)lr, (void *)ld, (void *)lp, (void *)la})
            if (p) fpm_host_free(device(0), p);
    }
    void growList(uint64_t room)
    {
        fpm_ctx *c = device(0);
        freeList();
        cap = room;
        check(fpm_host_alloc(c, (void **)&lq, cap * 4), "pinned buffers");
        check(fpm_host_alloc(c, (void **)&lr, cap * 4), "pinned buffers");
        check(fpm_host_alloc(c, (void **)&ld, cap * 8), "pinned buffers");
        check(fpm_host_alloc(c, (void **)&lp, cap * 8), "pinned buffers");
        check(fpm_host_alloc(c, (void **)&la, cap), "pinned buffers");
    }
    // The buffers for blocks of np pairs with counts of cb bytes.  The list starts at 1/16 of
    // the block's pairs and grows when a block lists more.
    void pin(uint64_t np, uint32_t cb)
    {
        fpm_ctx *c = device(0);
        check(fpm_host_alloc(c, &nu, np * cb), "pinned buffers");
        check(fpm_host_alloc(c, &de, np * cb), "pinned buffers");
        growList(std::max<uint64_t>(4096, np / 16));
    }
    void unpin()
    {
        for (void *p : {nu, de})
            if (p) fpm_host_free(device(0), p);
        freeList();
    }
    // the listed cells by query row, each row's in reference order (the device lists them
    // unordered)
    void orderRows(uint64_t nq)
    {
        rowStart.assign(nq + 1, 0);
        for (uint64_t e = 0; e < nl; e++) rowStart[lq[e] + 1]++;
        for (uint64_t i = 0; i < nq; i++) rowStart[i + 1] += rowStart[i];
        byRow.resize(nl);
        {
            std::vector<uint32_t> fill(rowStart.begin(), rowStart.end() - 1);
            for (uint64_t e = 0; e < nl; e++) byRow[fill[lq[e]]++] = (uint32_t)e;
        }
        for (uint64_t i = 0; i < nq; i++)
            std::sort(byRow.begin() + rowStart[i], byRow.begin() + rowStart[i + 1],
                      [this](uint32_t x, uint32_t y) { return lr[x] < lr[y]; });
    }
};

// What the block formatter reads; fixed before the first block
struct LineContext {
    const Sketch *query = nullptr;
    std::vector<std::string> refTag;    // reference name (+ ":" comment) of each line, built once
    bool table = false, comment = false;
    uint32_t cb = 2;                    // bytes per count in Slot::nu / de
    // the -d / -v filters at the values of a pair sharing no hash (compareSketches, :421-429)
    bool passNone = true;
    bool passEmpty = true;              // distance 0: two empty sketches
};

LineContext lineContext(const Inputs &in, const DistOptions &opt, uint32_t cb)
{
    LineContext cx;
    cx.query = &in.query();
    cx.table = opt.table;
    cx.comment = opt.comment;
    cx.cb = cb;
    for (const Reference &rr : in.ref.references) {
        cx.refTag.push_back(rr.name);
        if (opt.comment) { cx.refTag.back().push_back(':'); cx.refTag.back() += rr.comment; }
    }
    const bool pCuts = opt.pValueMax >= 0 && 1.0 > opt.pValueMax;
    cx.passNone = !(opt.distanceMax >= 0 && 1.0 > opt.distanceMax) && !pCuts;
    cx.passEmpty = !pCuts;
    return cx;
}

// The text of query rows [qa, qb) of the block in `sl`, whose first row is query q0, into `o`
// (the piece's buffer from earlier blocks: no regrowth)
void formatRows(const LineContext &cx, const Slot &sl, uint64_t q0, uint64_t qa, uint64_t qb,
                std::string &o)
{
    char line[512];
    const uint64_t nR = cx.refTag.size();
    o.clear();
    for (uint64_t qi = qa; qi < qb; qi++) {
        const Reference &qr = cx.query->getReference(q0 + qi);
        if (cx.table) o += qr.name;
        std::string qtail;              // "\t<query>[:comment]\t"
        if (!cx.table) {
            qtail.push_back('\t');
            qtail += qr.name;
            if (cx.comment) { qtail.push_back(':'); qtail += qr.comment; }
            qtail.push_back('\t');
        }
        uint32_t cur = sl.rowStart[qi];   // the row's listed cells, in reference order
        for (uint64_t j = 0; j < nR; j++) {
            const uint64_t k = qi * nR + j;
            const uint32_t nm = cx.cb == 2 ? ((const uint16_t *)sl.nu)[k] : ((const uint32_t *)sl.nu)[k];
            const uint32_t dn = cx.cb == 2 ? ((const uint16_t *)sl.de)[k] : ((const uint32_t *)sl.de)[k];
            double di, pv;
            bool pa;
            if (nm == 0) {
                di = dn == 0 ? 0.0 : 1.0;
                pv = 1.0;
                pa = dn == 0 ? cx.passEmpty : cx.passNone;
            } else {
                const uint32_t e = sl.byRow[cur++];
                di = sl.ld[e];
                pv = sl.lp[e];
                pa = sl.la[e] != 0;
            }
            if (cx.table) {
                o.push_back('\t');
                if (pa) putNum(o, di);
                continue;
            }
            if (!pa) continue;
            // one append per line: the line is assembled in a stack buffer where it fits
            const std::string &tag = cx.refTag[j];
            const bool fits = tag.size() + qtail.size() + kLineNums <= sizeof(line);
            char *p = line;
            if (fits) {
                memcpy(p, tag.data(), tag.size());
                p += tag.size();
                memcpy(p, qtail.data(), qtail.size());
                p += qtail.size();
            } else {
                o += tag;
                o += qtail;
            }
            p = numTo(p, di);
            *p++ = '\t';
            p = numTo(p, pv);
            *p++ = '\t';
            p = uTo(p, nm);
            *p++ = '/';
            p = uTo(p, dn);
            *p++ = '\n';
            o.append(line, (size_t)(p - line));
        }
        if (cx.table) o.push_back('\n');
    }
}

// query rows [qa, qb) of a slot's block, to be formatted into the slot's text[p]
struct Piece {
    Slot *slot;
    uint64_t q0, qa, qb, p;
};

// The grid in query blocks (CommandDistance.cpp:224-261 chunks it for the pool): every device
// holds the reference set with its index built once (fpm_refset_create) and takes blocks in
// turn; results land in pinned buffers; formatter threads (-p) turn each block into text
// pieces, which are written strictly in block order (writeOutput, :276-333, consumes the pool's
// outputs in order).  One Grid is the state the three roles share.
struct Grid {
    // fixed before the threads start
    LineContext lines;
    const Sketch *ref = nullptr;
    const PackedRows *Q = nullptr;      // the query rows, as wide as the reference's
    uint64_t nR = 0, nQ = 0, sketchSize = 0, block = 1, nBlocks = 0;
    uint32_t cb = 2;
    double distanceMax = 1, pValueMax = 1;
    std::vector<fpm_refset *> sets;     // per device
    std::vector<Slot> slots;
    // under mu
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Piece> pieces;
    bool stop = false;
    std::atomic<uint64_t> next{0};
    std::atomic<uint64_t> devUs{0};     // device calls + the listed cells' row order
    // the writer's
    bool writeFailed = false;
    double waitMs = 0, writeMs = 0;

    void deviceThread(int d);
    void formatterThread();
    void writerLoop(OutputTarget &out, Prealloc &prealloc);
};

void Grid::deviceThread(int d)
{
    const uint64_t nSlots = slots.size();
    for (;;) {
        const uint64_t b = next.fetch_add(1);
        if (b >= nBlocks) return;
        Slot &sl = slots[b % nSlots];
        {
            // the slot's previous block must be written out first
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return sl.nextB == b; });
        }
        const uint64_t q0 = b * block, nq = std::min(block, nQ - q0);
        const auto tb0 = std::chrono::steady_clock::now();
        for (;;) {
            check(fpm_refset_dist_list(sets[d], Q->data() + q0 * Q->width * Q->hashBytes,
                                       Q->len.data() + q0, Q->length.data() + q0, Q->width,
                                       (uint32_t)nq, (uint32_t)sketchSize,
                                       (uint32_t)ref->getKmerSize(), ref->getKmerSpace(),
                                       distanceMax, pValueMax, cb, sl.nu, sl.de, sl.lq, sl.lr,
                                       sl.ld, sl.lp, sl.la, sl.cap, &sl.nl),
                  "dist");
            if (sl.nl <= sl.cap) break;
            sl.growList(sl.nl + sl.nl / 4);        // more pairs share hashes: room
        }
        sl.orderRows(nq);
        devUs += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(
                     std::chrono::steady_clock::now() - tb0).count();
        // pieces of ~256 K pairs (at least one query row) for the formatter threads:
        // four per block keep the writer fed (C2 command, same box: writer waiting
        // 81-107 -> 24-29 ms, wall 0.93-1.07 -> 0.87-0.92 s against pieces of 1 M; 128 K
        // pieces 0.97-1.06 s)
        const uint64_t per = std::max<uint64_t>(1, (1ULL << 18) / nR);
        const uint64_t parts = (nq + per - 1) / per;
        std::lock_guard<std::mutex> lk(mu);
        sl.b = b;
        sl.pending = (int)parts;
        sl.ready = false;
        sl.text.resize(parts);
        for (uint64_t p = 0; p < parts; p++)
            pieces.push_back(Piece{&sl, q0, p * per, std::min(nq, p * per + per), p});
        cv.notify_all();
    }
}

void Grid::formatterThread()
{
    for (;;) {
        Piece pc;
        std::string t;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return stop || !pieces.empty(); });
            if (pieces.empty()) return;
            pc = pieces.front();
            pieces.pop_front();
            t.swap(pc.slot->text[pc.p]);
        }
        formatRows(lines, *pc.slot, pc.q0, pc.qa, pc.qb, t);
        std::lock_guard<std::mutex> lk(mu);
        pc.slot->text[pc.p].swap(t);
        if (--pc.slot->pending == 0) pc.slot->ready = true;
        cv.notify_all();
    }
}

// the blocks' pieces, in block order, to the output
void Grid::writerLoop(OutputTarget &out, Prealloc &prealloc)
{
    const uint64_t nSlots = slots.size();
    for (uint64_t b = 0; b < nBlocks; b++) {
        Slot &sl = slots[b % nSlots];
        std::vector<std::string> text;
        auto t0 = std::chrono::steady_clock::now();
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return sl.b == b && sl.ready; });
            text.swap(sl.text);
        }
        auto t1 = std::chrono::steady_clock::now();
        if (out.direct()) {
            prealloc.writerAt(out.pos);
            if (!writeFailed && !writePieces(out.fd, out.pos, text)) writeFailed = true;
            for (auto &t : text) out.pos += (off_t)t.size();
        } else {
            for (auto &t : text) fwrite(t.data(), 1, t.size(), stdout);
        }
        auto t2 = std::chrono::steady_clock::now();
        waitMs += std::chrono::duration<double, std::milli>(t1 - t0).count();
        writeMs += std::chrono::duration<double, std::milli>(t2 - t1).count();
        {
            // the piece buffers go back to the slot for its next block: allocating and
            // unmapping ~40 MB strings per piece cost ~0.4 s of page faults and munmap
            std::lock_guard<std::mutex> lk(mu);
            text.swap(sl.text);
            sl.nextB = b + nSlots;
        }
        cv.notify_all();
    }
}

}  // namespace

int CommandDistance::run() const
{
    if (arguments.size() < 2 || options.at("help").active) {
        print();
        return 0;
    }
    warmDevices();
    const DistOptions opt{options.at("list").active, options.at("table").active,
                          options.at("comment").active, options.at("fingerprint").active,
                          options.at("pvalue").getArgumentAsNumber(),
                          options.at("distance").getArgumentAsNumber(),
                          options.at("distance").active || options.at("pvalue").active};
    Parameters parameters;
    if (sketchParameterSetup(parameters, *this)) return 1;

    Inputs in;
    if (!loadReference(*this, arguments[0], opt.fingerprint, parameters, in)) return 1;
    if (opt.table) writeTableHeader(in.ref);
    loadQueries(arguments, opt, parameters, in);

    Grid g;
    g.ref = &in.ref;
    g.nR = in.ref.getReferenceCount();
    g.nQ = in.query().getReferenceCount();
    g.sketchSize = (uint64_t)std::min(in.query().getMinHashesPerWindow(), in.ref.getMinHashesPerWindow());
    g.distanceMax = opt.distanceMax;
    g.pValueMax = opt.pValueMax;
    const uint64_t nR = g.nR, nQ = g.nQ;
    OutputTarget out = outputTarget(nR && nQ);
    // The output file's pages allocated ahead (Prealloc) while the devices come up: the list
    // format and no -d / -v filter, so the text size is about known
    Prealloc prealloc;
    const char *pa_env = getenv("FPMASH_DIST_PREALLOC");   // A/B: 0 = pages allocated on the way
    if (out.direct() && !opt.table && !opt.filtered && !(pa_env && strcmp(pa_env, "0") == 0))
        prealloc.start(out.fd, out.pos, out.pos + listTextEstimate(in, opt.comment, g.sketchSize));

    const int nDev = nR && nQ ? deviceCount() : 0;
    // 1 M pairs per block (16 M-pair slots made pinning and unpinning the slots cost ~0.6 s of
    // the C2 command; C2 `dist` wall: 4 M 1.27 s, 2 M 1.15 s, 1 M 1.06-1.09 s, 512 K 1.50 s)
    uint64_t blockPairs = 1ULL << 20;
    if (const char *bp = getenv("FPMASH_DIST_BLOCK_PAIRS")) blockPairs = std::max(1ULL, strtoull(bp, nullptr, 10));
    g.block = nR ? std::max<uint64_t>(1, blockPairs / nR) : 1;
    g.nBlocks = nR ? (nQ + g.block - 1) / g.block : 0;
    const int nSlots = std::max(2, 2 * nDev + 1);
    const int nFmt = std::max(1, std::min(parameters.parallelism > 1 ? parameters.parallelism
                                          : (int)std::thread::hardware_concurrency(), 64));
    // u16 counts (every count is <= the sketch size), u32 past 65535
    g.cb = g.sketchSize <= 65535 ? 2 : 4;
    g.slots = std::vector<Slot>(nSlots);
    for (int i = 0; i < nSlots; i++) g.slots[i].nextB = (uint64_t)i;
    // pinned result buffers (page locking costs ~0.6 ms per MB): one thread per slot, beside
    // the row packing and the reference sets
    std::vector<std::thread> pinner;
    for (int i = 0; i < nSlots && g.nBlocks; i++)
        pinner.emplace_back(&Slot::pin, &g.slots[i], g.block * nR, g.cb);
    // both sets at the common width of the two
    const bool use64 = in.ref.getUse64();
    const uint64_t width = std::max(maxRowLength(in.ref.references), maxRowLength(in.query().references));
    const PackedRows R(in.ref.references, use64, std::max<uint64_t>(1, width));
    const PackedRows Qown = in.sameSet ? PackedRows() : PackedRows(in.queryOwn.references, use64, R.width);
    g.Q = in.sameSet ? &R : &Qown;
    g.sets.assign(nDev, nullptr);
    for (int d = 0; d < nDev; d++)
        check(fpm_refset_create(device(d), R.data(), R.len.data(), R.length.data(), R.width,
                                (uint32_t)nR, R.hashBytes, (uint32_t)g.sketchSize, &g.sets[d]),
              "dist reference set");
    for (auto &t : pinner) t.join();
    phaseMark("rows packed + reference sets on the devices");

    g.lines = lineContext(in, opt, g.cb);
    std::vector<std::thread> fmt, gpu;
    for (int t = 0; t < nFmt; t++) fmt.emplace_back(&Grid::formatterThread, &g);
    for (int d = 0; d < nDev; d++) gpu.emplace_back(&Grid::deviceThread, &g, d);
    g.writerLoop(out, prealloc);
    bool writeFailed = g.writeFailed;
    if (out.direct() && !prealloc.trim(out.pos)) writeFailed = true;   // pages allocated past the text
    if (!writeFailed) fatalCutsOutput(-1, 0);                // the text is complete
    if (out.direct()) lseek(out.fd, out.pos, SEEK_SET);   // later output (if any) follows the grid
    if (writeFailed) {
        std::cerr << "ERROR: writing the distance output failed." << std::endl;
        fatalExit();
    }
    if (timingOn())
        fprintf(stderr, "[fpmash] writer waiting for blocks: %.1f ms\n[fpmash] writer copying "
                        "pieces out (%s): %.1f ms\n", g.waitMs,
                out.direct() ? "pwritev" : "stdout", g.writeMs);
    if (timingOn())
        fprintf(stderr, "[fpmash] device blocks (compare + fetch + row order, summed): %.1f ms\n",
                g.devUs.load() / 1e3);
    phaseMark("blocks computed, formatted and written");
    for (auto &t : gpu) t.join();
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.stop = true;
    }
    g.cv.notify_all();
    for (auto &t : fmt) t.join();
    if (cleanExit()) {
        // (the process otherwise leaves by _exit once the output is flushed: unpinning the
        // slots cost ~50 ms of the C2 command)
        for (auto &sl : g.slots) sl.unpin();
        for (auto *rs : g.sets) fpm_refset_free(rs);
    }
    fflush(stdout);
    in.warning.print(parameters, *this);
    if (!cleanExit()) {
        // every output is written: leave before this function's destructors free the ~10^5
        // reference vectors, the row images and the text pieces (~25 ms of the C2 command)
        phaseMark("command done");
        std::cout.flush();
        std::cerr.flush();
        fflush(nullptr);
        _exit(0);
    }
    return 0;
}

}  // namespace fpmhost
