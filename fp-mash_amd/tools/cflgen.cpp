// cflgen — synthetic CFL / ICFL / CFL_ICFL k-finger text at C3 scale (5,000 x
// 2 kb -> 10 M lines).  cflgen <window> <threads> [CFL|ICFL|CFL_ICFL-<T>|CFL_COMB|ICFL_COMB|
// CFL_ICFL_COMB-<T>], CFL when not given.
//
// Same output as fpmash.datagen.cfl_text (lyn2vec `--type basic --type_factorization CFL`,
// fingerprint_utils.py:95-110, 443-476; Duval, factorizations.py:102-126), which is pinned
// byte for byte against the fork's DNA1-CFL.txt; the Python version takes ~47 ms per 2 kb
// sequence, this one a few hundred microseconds.  Test tooling only (tests/test_cli.py checks
// it against datagen); not part of libfpmash.  ICFL and CFL_ICFL-T restate
// fpmash.datagen.icfl_lengths / cfl_icfl_lengths (lyn2vec's ICFL_recursive and CFL_icfl,
// factorizations.py:143-248, 265-301, as loops; the end of the word out of band).  The _COMB
// forms restate fpmash.datagen.comb_lengths (lyn2vec's d_duval_, factorizations_comb.py:213-246):
// the cuts of the window's factorization and, mirrored, those of its reverse complement's, whose
// CFL_ICFL runs at threshold 30 whatever T is.
//
// stdin: one record per line, "<id>\t<sequence>".  stdout: for every record and every cyclic
// window start (one window of the whole sequence when it is shorter than the window):
// "G00000<id>_0 l1 l2 ...\n", the Lyndon factor lengths of the upper-cased window.
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

// 0: CFL; -1: ICFL; T >= 1: CFL_ICFL-T
static int g_fact = 0;
static bool g_comb = false;
static const int kCombRevThreshold = 30;   // cfl_icfl_'s default cfl_max

static void put(int len, std::string &out) {
    char num[16];
    int m = snprintf(num, sizeof num, " %d", len);
    out.append(num, m);
}

// the inverse Lyndon factor lengths of w[0 .. n) (datagen.icfl_lengths)
static void icfl(const char *word, int n, std::vector<int> &out) {
    const unsigned char *w0 = (const unsigned char *)word;
    std::vector<int> start, last, f;
    int s = 0;
    for (;;) {
        const unsigned char *w = w0 + s;
        const int m = n - s;
        int i = 0, j = 1;
        while (j < m && w[j] <= w[i]) {
            i = w[j] < w[i] ? 0 : i + 1;
            ++j;
        }
        if (j >= m) break;
        f.assign(j, 0);
        for (int e = 1, k = 0; e < j; ++e) {
            while (k > 0 && w[k] != w[e]) k = f[k - 1];
            if (w[k] == w[e]) ++k;
            f[e] = k;
        }
        int b = f[j - 1], l = b;
        for (;;) {
            if (w[b] < w[j]) l = b;
            if (!b) break;
            b = f[b - 1];
        }
        start.push_back(s);
        last.push_back(l);
        s += j - l;
    }
    // right to left: the factor lengths, last factor first
    std::vector<int> len{n - s};
    int end = s;
    for (size_t k = start.size(); k-- > 0;) {
        if (len.back() > last[k]) len.push_back(end - start[k]);
        else len.back() += end - start[k];
        end = start[k];
    }
    for (size_t k = len.size(); k-- > 0;) out.push_back(len[k]);
}

// fact as g_fact
static void duval(const char *w, int n, int fact, std::vector<int> &out) {
    int k = 0;
    while (k < n) {
        int i = k, j = k + 1;
        while (j < n && (unsigned char)w[i] <= (unsigned char)w[j]) {
            i = ((unsigned char)w[i] < (unsigned char)w[j]) ? k : i + 1;
            ++j;
        }
        while (k <= i) {
            int len = j - i;
            if (fact > 0 && len > fact) icfl(w + k, len, out);
            else out.push_back(len);
            k += len;
        }
    }
}

static void lengths(const char *w, int n, int fact, std::vector<int> &out) {
    if (fact < 0) {
        if (n) icfl(w, n, out);
    } else {
        duval(w, n, fact, out);
    }
}

static char complement(char c) {
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    default: return c;   // N, and every byte lyn2vec has no complement for
    }
}

static void factorize(const char *w, int n, std::string &out) {
    std::vector<int> fwd;
    lengths(w, n, g_fact, fwd);
    if (!g_comb) {
        for (int len : fwd) put(len, out);
        return;
    }
    std::string rc(n, 0);
    for (int i = 0; i < n; ++i) rc[i] = complement(w[n - 1 - i]);
    std::vector<int> rev;
    lengths(rc.data(), n, g_fact > 0 ? kCombRevThreshold : g_fact, rev);
    std::vector<char> cut(n + 1, 0);
    int at = 0;
    for (int len : fwd) cut[at += len] = 1;
    at = 0;
    for (int len : rev) { cut[n - at] = 1; at += len; }
    int prev = 0;
    for (int c = 1; c <= n; ++c)
        if (cut[c]) { put(c - prev, out); prev = c; }
}

static void record(const std::string &id, std::string seq, int window, std::string &out) {
    for (auto &c : seq) c = (char)toupper((unsigned char)c);
    const std::string head = "G00000" + id + "_0";
    if ((int)seq.size() < window) {
        out += head;
        factorize(seq.data(), (int)seq.size(), out);
        out += '\n';
        return;
    }
    std::string ss = seq + seq.substr(0, window);
    for (size_t i = 0; i < seq.size(); ++i) {
        out += head;
        factorize(ss.data() + i, window, out);
        out += '\n';
    }
}

int main(int argc, char **argv) {
    int window = argc > 1 ? atoi(argv[1]) : 100;
    int threads = argc > 2 ? atoi(argv[2]) : (int)std::max(1u, std::thread::hardware_concurrency());
    if (argc > 3) {
        std::string f = argv[3];
        if (f == "CFL_COMB" || f == "ICFL_COMB") {
            g_comb = true;
            f.resize(f.size() - 5);
        } else if (f.rfind("CFL_ICFL_COMB-", 0) == 0) {
            g_comb = true;
            f.erase(8, 5);
        }
        const std::string t = f.rfind("CFL_ICFL-", 0) == 0 ? f.substr(9) : "";
        if (f == "ICFL") g_fact = -1;
        else if (!t.empty() && t.size() <= 9 && t.find_first_not_of("0123456789") == std::string::npos &&
                 atoi(t.c_str()) >= 1) g_fact = atoi(t.c_str());
        else if (f != "CFL") {
            fprintf(stderr, "cflgen: unknown factorization %s\n", argv[3]);
            return 1;
        }
    }
    std::ios::sync_with_stdio(false);
    std::vector<std::string> ids, seqs;
    std::string line;
    while (std::getline(std::cin, line)) {
        size_t t = line.find('\t');
        if (t == std::string::npos) continue;
        ids.push_back(line.substr(0, t));
        seqs.push_back(line.substr(t + 1));
    }
    const size_t n = seqs.size();
    std::vector<std::string> out(n);
    threads = std::max(1, std::min<int>(threads, 64));
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] {
            for (size_t r = t; r < n; r += threads) record(ids[r], seqs[r], window, out[r]);
        });
    for (auto &th : pool) th.join();
    for (auto &o : out) fwrite(o.data(), 1, o.size(), stdout);
    return 0;
}
