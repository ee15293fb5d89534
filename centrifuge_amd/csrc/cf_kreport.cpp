// cf_kreport.cpp — `centrifuge-kreport`: Kraken-style report from classification output
// (SURVEY.md §8f row 4).  Same command line and bytes on stdout as the reference's Perl script
// `centrifuge-kreport` (cited below by its line numbers), but the taxonomy comes straight from
// <index>.3.cf instead of two `centrifuge-inspect` child processes (centrifuge-kreport:233-260),
// and a 10^8-row classification file is read at file-system speed instead of Perl speed.
//
//   centrifuge-kreport -x <index> [--no-lca] [--show-zeros] [--is-count-table]
//                      [--min-score N] [--min-length N] [<centrifuge output file>...]
#include <algorithm>
#include <cerrno>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include <zlib.h>

#include "cf_index.hpp"
#include "cf_kreport_tree.hpp"

using namespace cfamd;
using namespace cfamd::kreport;

namespace {

struct Opts {
    std::string index;
    bool noLca = false, showZeros = false, countTable = false, haveMinScore = false, haveMinLength = false;
    double minScore = 0, minLength = 0;
    std::vector<std::string> files;
};

[[noreturn]] void usage(int code) {                                        // centrifuge-kreport:37-60
    std::fputs("\nUsage: centrifuge-kreport -x <index name> OPTIONS <centrifuge output file(s)>\n\n"
               "centrifuge-kreport creates Kraken-style reports from centrifuge out files.\n\n"
               "Options:\n"
               "    -x INDEX            (REQUIRED) Centrifuge index\n\n"
               "    --no-lca             Do not report the LCA of multiple assignments, but report count fractions at the taxa.\n"
               "    --show-zeros         Show clades that have zero reads, too\n"
               "    --is-count-table     The format of the file is 'taxID<tab>COUNT' instead of the standard\n"
               "                         Centrifuge output format\n\n"
               "    --min-score SCORE    Require a minimum score for reads to be counted\n"
               "    --min-length LENGTH  Require a minimum alignment length to the read\n  \n  ", stderr);
    std::exit(code);
}

Opts parse(int argc, char **argv) {
    Opts o;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i], v;
        bool hasV = false;
        if (a == "--") { for (i++; i < argc; i++) o.files.push_back(argv[i]); break; }
        if (a.size() > 1 && a[0] == '-') {
            std::string n = a.substr(a[1] == '-' ? 2 : 1);                // Getopt::Long takes -opt and --opt alike
            const size_t eq = n.find('=');
            if (eq != std::string::npos) { v = n.substr(eq + 1); n = n.substr(0, eq); hasV = true; }
            auto val = [&]() -> std::string { if (hasV) return v; if (i + 1 >= argc) usage(64); return argv[++i]; };
            if (n == "x") o.index = val();
            else if (n == "no-lca") o.noLca = true;
            else if (n == "show-zeros") o.showZeros = true;
            else if (n == "is-count-table") o.countTable = true;
            else if (n == "min-score") { o.minScore = std::strtod(val().c_str(), nullptr); o.haveMinScore = true; }
            else if (n == "min-length") { o.minLength = std::strtod(val().c_str(), nullptr); o.haveMinLength = true; }
            else if (n == "help" || n == "h") usage(0);
            else { std::fprintf(stderr, "Unknown option: %s\n", n.c_str()); usage(64); }
        } else o.files.push_back(a);
    }
    if (o.index.empty()) usage(64);
    return o;
}

// concatenation of the input files ('-' or none = stdin) — Perl's <>.  An input whose first bytes are the gzip magic is inflated as
// it is read (what centrifuge-class --out-bgzf writes: BGZF is concatenated gzip members); anything else is taken as it is.
struct Lines {
    std::vector<std::string> files;
    size_t next = 0;
    std::FILE *f = nullptr;
    std::vector<char> buf, zin;        // buf[lo, hi): text not handed out yet
    size_t lo = 0, hi = 0;
    bool eof = false, first = true, gz = false, zEnd = false;
    z_stream z{};
    explicit Lines(std::vector<std::string> fs) : files(std::move(fs)), buf(1u << 20), zin(1u << 18) { if (files.empty()) files.push_back("-"); }
    ~Lines() { closeFile(); }
    void closeFile() { if (gz) { inflateEnd(&z); gz = false; } if (f && f != stdin) std::fclose(f); f = nullptr; }
    // more text behind buf[hi); false at the end of the file
    bool fill() {
        if (eof) return false;
        if (lo > 0) { std::memmove(buf.data(), buf.data() + lo, hi - lo); hi -= lo; lo = 0; }
        if (hi == buf.size()) buf.resize(buf.size() * 2);
        if (first) {                                           // the file's first bytes decide
            first = false;
            const size_t n = std::fread(buf.data(), 1, 2, f);
            if (n == 2 && (uint8_t)buf[0] == 0x1f && (uint8_t)buf[1] == 0x8b) {
                z = z_stream{};
                if (inflateInit2(&z, 15 + 16) != Z_OK) throw std::runtime_error("zlib: inflateInit2 failed");
                gz = true; zEnd = false;
                std::memcpy(zin.data(), buf.data(), 2);
                z.next_in = reinterpret_cast<Bytef *>(zin.data()); z.avail_in = 2;
            } else { hi = n; if (n < 2) eof = true; return n > 0; }
        }
        if (!gz) {
            const size_t n = std::fread(buf.data() + hi, 1, buf.size() - hi, f);
            if (n == 0) { eof = true; return false; }
            hi += n;
            return true;
        }
        for (;;) {
            if (z.avail_in == 0) {
                const size_t n = std::fread(zin.data(), 1, zin.size(), f);
                if (n == 0) {                                  // (in the middle of a member: what was inflated so far has been handed out)
                    if (!zEnd) std::fprintf(stderr, "centrifuge-kreport: the gzip input ends in the middle of a member: the report covers what came before\n");
                    eof = true; return false;
                }
                z.next_in = reinterpret_cast<Bytef *>(zin.data()); z.avail_in = (uInt)n;
            }
            if (zEnd) {                                        // a further member?
                if ((uint8_t)z.next_in[0] != 0x1f) {
                    std::fprintf(stderr, "centrifuge-kreport: bytes that are no gzip member behind the last member of the input: ignored\n");
                    eof = true; return false;
                }
                inflateReset(&z); zEnd = false;
            }
            const size_t room = std::min<size_t>(buf.size() - hi, 1u << 30);
            z.next_out = reinterpret_cast<Bytef *>(buf.data() + hi); z.avail_out = (uInt)room;
            const int rc = inflate(&z, Z_NO_FLUSH);
            const size_t got = room - z.avail_out;
            if (rc == Z_STREAM_END) zEnd = true;
            else if (rc != Z_OK && rc != Z_BUF_ERROR) { std::fprintf(stderr, "centrifuge-kreport: corrupt gzip input\n"); eof = true; if (got) { hi += got; return true; } return false; }
            if (got) { hi += got; return true; }
        }
    }
    // line without its '\n'; false at the end of the last file
    bool get(const char *&p, size_t &n) {
        for (;;) {
            if (!f) {
                if (next >= files.size()) return false;
                const std::string &path = files[next++];
                if (path == "-") f = stdin;
                else {
                    f = std::fopen(path.c_str(), "rb");
                    if (!f) { std::fprintf(stderr, "Can't open %s: %s.\n", path.c_str(), std::strerror(errno)); continue; }
                }
                lo = hi = 0; eof = false; first = true;
            }
            size_t from = lo;
            for (;;) {
                if (const char *nl = static_cast<const char *>(std::memchr(buf.data() + from, '\n', hi - from))) {
                    p = buf.data() + lo; n = (size_t)(nl - p); lo = (size_t)(nl - buf.data()) + 1;
                    return true;
                }
                from = hi - lo;                                // (fill moves the text to the front)
                if (!fill()) break;
            }
            if (hi > lo) { p = buf.data() + lo; n = hi - lo; lo = hi; return true; }      // a last line without '\n'
            closeFile();
        }
    }
};

bool parseId(const char *p, size_t n, uint64_t &v) {
    if (n == 0) return false;
    v = 0;
    for (size_t i = 0; i < n; i++) { if (p[i] < '0' || p[i] > '9') return false; v = v * 10 + (uint64_t)(p[i] - '0'); }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const Opts o = parse(argc, argv);
    if (o.files.empty()) std::fprintf(stderr, "Reading centrifuge out file from STDIN ... \n");
    try {
        Taxonomy tx;
        std::fprintf(stderr, "Loading taxonomy ...\n");
        {
            HostIndex h;
            std::string base = o.index;                                      // adjustEbwtBase bt2_idx.cpp:38-66, as centrifuge-inspect resolves it
            if (std::FILE *t = std::fopen((base + ".1.cf").c_str(), "rb")) std::fclose(t);
            else if (const char *e = std::getenv("CENTRIFUGE_INDEXES")) base = std::string(e) + "/" + o.index;
            h.load(base, nullptr);
            tx.load(h, true);
        }
        Report rp(tx);
        rp.showZeros = o.showZeros;
        Lines in(o.files);
        const char *p; size_t n;
        if (o.countTable) {                                                  // centrifuge-kreport:74-79
            while (in.get(p, n)) {
                std::string s(p, n);
                char *save = nullptr;
                char *a = strtok_r(&s[0], " \t\r\n\f\v", &save);
                char *b = a ? strtok_r(nullptr, " \t\r\n\f\v", &save) : nullptr;
                if (!a) continue;
                uint64_t id;
                if (!parseId(a, std::strlen(a), id)) id = kJunk;
                const double c = b ? std::strtod(b, nullptr) : 0.0;
                rp.taxo[id] = c;
                rp.seqCount += c;
            }
        } else {
            int cRead = 0, cTax = 0, cScore = 0, cHit = 0, cNum = 0;        // a missing column reads column 0, as `$cols[undef]` does
            if (in.get(p, n)) {
                size_t i = 0; int col = 0;
                while (i <= n) {
                    size_t j = i; while (j < n && p[j] != '\t') j++;
                    const std::string name(p + i, j - i);
                    if (name == "readID") cRead = col; else if (name == "taxID") cTax = col; else if (name == "score") cScore = col;
                    else if (name == "hitLength") cHit = col; else if (name == "numMatches") cNum = col;
                    col++; i = j + 1;
                }
            }
            std::string prevRead; bool havePrev = false; uint64_t prevTax = 0;
            std::vector<std::pair<const char *, size_t>> f;
            while (in.get(p, n)) {
                f.clear();
                for (size_t i = 0; i <= n;) { size_t j = i; while (j < n && p[j] != '\t') j++; f.emplace_back(p + i, j - i); i = j + 1; }
                auto fld = [&](int c) -> std::pair<const char *, size_t> { return (size_t)c < f.size() ? f[c] : std::pair<const char *, size_t>{"", 0}; };
                auto num = [&](int c) { const auto x = fld(c); return std::strtod(std::string(x.first, x.second).c_str(), nullptr); };
                if (o.haveMinLength && num(cHit) < o.minLength) continue;
                if (o.haveMinScore && num(cScore) < o.minScore) continue;
                const auto rd = fld(cRead), tf = fld(cTax);
                uint64_t tax;
                if (!parseId(tf.first, tf.second, tax)) tax = kJunk;
                if (!tx.inTree(tax)) tax = 1;
                if (o.noLca) {                                               // centrifuge-kreport:106-108
                    const double nm = num(cNum);
                    if (nm == 0) { std::fprintf(stderr, "Illegal division by zero (numMatches column) in the classification file.\n"); return 255; }
                    rp.taxo[tax] += 1 / nm;
                    rp.seqCount += 1 / nm;
                } else if (havePrev && prevRead.size() == rd.second && std::memcmp(prevRead.data(), rd.first, rd.second) == 0) {
                    rp.taxo[prevTax] -= 1;                                   // :110-113
                    prevTax = tx.lca(prevTax, tax);
                    rp.taxo[prevTax] += 1;
                } else {
                    rp.taxo[tax] += 1;                                       // :115-117
                    rp.seqCount += 1;
                    prevTax = tax;
                }
                prevRead.assign(rd.first, rd.second); havePrev = true;
            }
        }
        if (const int rc = rp.emit(argv[0])) return rc;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "centrifuge-kreport: %s\n", e.what());
        return 1;
    }
    return 0;
}
