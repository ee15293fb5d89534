// cf_kreport_tree.hpp — the taxonomy and the report of `centrifuge-kreport` (the reference's Perl script, cited by its line
// numbers), shared by the tool (cf_kreport.cpp: the tally comes from a classification file) and the library
// (cf_kreport_enable / cf_kreport_write: the tally comes from the device, kreport_body) — so that the tree sums, the `%6.2f`, the
// stable sort of the children and the "No sequence matches" case are the same code, and the device's lca_body has its
// specification (Taxonomy::lca behind the inTree rule) next to the table it reads.
#pragma once
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "cf_index.hpp"

namespace cfamd {
namespace kreport {

constexpr uint64_t kJunk = ~0ull;          // a taxID field that is not a number (e.g. the header line of a second file)
constexpr int kMaxDepth = 4096;
inline const char *deepMessage() { return "taxonomy tree is deeper than 4096 levels (a cycle?)"; }

struct Taxonomy {
    std::vector<uint64_t> tid, parent;          // ascending tid: the order `centrifuge-inspect --taxonomy-tree` lists them
    std::vector<uint8_t> rank;
    std::unordered_map<uint64_t, uint32_t> at;  // tid -> position
    std::unordered_map<uint64_t, std::vector<uint64_t>> children;
    std::unordered_map<uint64_t, std::string> names;
    bool quiet = false;                         // (the library asks about every taxon of an index: no warnings then)

    // names and nodes of an index (centrifuge-kreport:233-260)
    void load(const HostIndex &h, bool progress) {
        if (progress) std::fprintf(stderr, "Loading names file ...\n");
        for (const auto &e : h.names) names[e.first] = e.second;          // a repeated taxid keeps the last name
        if (progress) std::fprintf(stderr, "Loading nodes file ...\n");
        for (const auto &nd : h.tree) {                                    // centrifuge-kreport:247-259
            const uint64_t par = nd.tid == 1 ? 0 : nd.parent;
            at[nd.tid] = (uint32_t)tid.size();
            tid.push_back(nd.tid); parent.push_back(par); rank.push_back(nd.rank);
            children[par].push_back(nd.tid);
        }
    }
    bool parentOf(uint64_t a, uint64_t &p) const { auto it = at.find(a); if (it == at.end()) return false; p = parent[it->second]; return true; }
    void warnNoParent(uint64_t a) const { if (!quiet) std::fprintf(stderr, "Couldn't find parent of taxID %" PRIu64 " - directly assigned to root.\n", a); }

    bool inTree(uint64_t a) const {                                        // centrifuge-kreport:161-175
        if (a == kJunk) return true;
        while (a > 1) {
            uint64_t p;
            if (!parentOf(a, p)) { warnNoParent(a); return false; }
            if (a == p) break;
            a = p;
        }
        return true;
    }
    uint64_t lca(uint64_t a, uint64_t b) const {                           // centrifuge-kreport:177-203
        if (a == 0) return b;
        if (b == 0) return a;
        if (a == b) return a;
        std::unordered_set<uint64_t> path;
        while (a != 0) {                                                   // Perl: `$a ge 1` on the decimal string
            path.insert(a);
            uint64_t p;
            if (a == kJunk || !parentOf(a, p)) { warnNoParent(a); break; }
            if (a == p) break;
            a = p;
        }
        while (b > 1 && b != kJunk) {
            if (path.count(b)) return b;
            uint64_t p;
            if (!parentOf(b, p)) { warnNoParent(b); break; }
            if (b == p) break;
            b = p;
        }
        return 1;
    }
};

inline const char *rankCode(const char *r) {                               // centrifuge-kreport:205-218
    static const std::pair<const char *, const char *> k[] = {{"species", "S"}, {"genus", "G"}, {"family", "F"}, {"order", "O"},
                                                              {"class", "C"}, {"phylum", "P"}, {"kingdom", "K"}, {"superkingdom", "D"}};
    for (const auto &e : k) if (std::strcmp(r, e.first) == 0) return e.second;
    return "-";
}

struct Report {
    const Taxonomy &tx;
    std::unordered_map<uint64_t, double> taxo, clade;
    double seqCount = 0;
    bool showZeros = false;
    std::FILE *to = stdout;
    std::string out;

    explicit Report(const Taxonomy &t) : tx(t) { taxo[0] = 0; }
    double cladeOf(uint64_t t) const { auto it = clade.find(t); return it == clade.end() ? 0.0 : it->second; }
    double taxoOf(uint64_t t) const { auto it = taxo.find(t); return it == taxo.end() ? 0.0 : it->second; }

    void sum(uint64_t node, int depth) {                                   // dfs_summation, centrifuge-kreport:220-230
        if (depth > kMaxDepth) throw std::runtime_error(deepMessage());
        auto it = tx.children.find(node);
        if (it == tx.children.end()) return;
        for (uint64_t c : it->second) {
            sum(c, depth + 1);
            clade[node] += cladeOf(c);
        }
    }
    void line(double cladeCnt, double taxoCnt, const char *code, uint64_t id, int depth, const std::string &name) {
        char b[128];
        std::snprintf(b, sizeof b, "%6.2f\t%lld\t%lld\t%s\t%" PRIu64 "\t", cladeCnt * 100 / seqCount, (long long)cladeCnt, (long long)taxoCnt, code, id);
        out += b;
        out.append((size_t)depth * 2, ' ');
        out += name;
        out.push_back('\n');
        if (out.size() > (1u << 20)) { std::fwrite(out.data(), 1, out.size(), to); out.clear(); }
    }
    void report(uint64_t node, int depth) {                                // dfs_report, centrifuge-kreport:138-159
        const double c = cladeOf(node);
        if (c == 0 && !showZeros) return;
        auto at = tx.at.find(node);
        auto nm = tx.names.find(node);
        line(c, taxoOf(node), rankCode(at == tx.at.end() ? "" : rankString(tx.rank[at->second])), node, depth, nm == tx.names.end() ? std::string() : nm->second);
        auto it = tx.children.find(node);
        if (it == tx.children.end()) return;
        std::vector<uint64_t> kids = it->second;
        std::stable_sort(kids.begin(), kids.end(), [&](uint64_t a, uint64_t b) { return cladeOf(a) > cladeOf(b); });   // Perl's sort is a stable merge sort
        for (uint64_t k : kids) report(k, depth + 1);
    }
    // the tree sums and the lines, from taxo and seqCount (centrifuge-kreport:124-136).  0, or 255 with the script's message when
    // nothing was counted (nothing is printed then)
    int emit(const char *prog) {
        clade = taxo;
        sum(1, 0);
        if (!(seqCount > 0)) { std::fprintf(stderr, "No sequence matches with given settings at %s line 133.\n", prog); return 255; }
        line(cladeOf(0), taxoOf(0), "U", 0, 0, "unclassified");
        report(1, 0);
        std::fwrite(out.data(), 1, out.size(), to);
        out.clear();
        std::fflush(to);
        return 0;
    }
};

// The tree as lca_body (cf_kernels.hpp) reads it, one entry per dense taxon of the index (HostIndex::taxa): parent's dense index |
// depth << 32; a root — taxon 1, a self-parented node, a node whose parent is 0 — is its own parent at depth 0; `outside` (bit 31
// of the depth) marks a taxon that inTree() refuses, which the fold replaces by taxon 1.  With this table lca_body returns, for
// every pair of dense taxa a, b, the dense index of lca(inTree(a) ? a : 1, inTree(b) ? b : 1): the first node of b's chain on a's
// chain is where two chains of equal depth meet, and two chains that never meet (different roots; taxon 1 is always a root, in the
// tree or not) give 1 there as here.  Throws when a chain is longer than kMaxDepth (a cycle: inTree() would not return).
inline std::vector<uint64_t> lcaTable(const Taxonomy &tx, const std::vector<uint64_t> &taxa, uint32_t outside) {
    std::unordered_map<uint64_t, uint32_t> dense;
    for (size_t i = 0; i < taxa.size(); i++) dense[taxa[i]] = (uint32_t)i;
    constexpr uint32_t kUnknown = 0xffffffffu;
    std::vector<uint32_t> depth(taxa.size(), kUnknown), par(taxa.size(), 0);
    std::vector<uint32_t> chain;
    for (size_t i = 0; i < taxa.size(); i++) {
        if (depth[i] != kUnknown) continue;
        chain.clear();
        uint32_t cur = (uint32_t)i, top = 0;                               // top: depth of the node the chain hangs from, or `outside`
        for (;;) {
            if (depth[cur] != kUnknown) { top = depth[cur] == outside ? outside : depth[cur] + 1; break; }
            if (chain.size() > (size_t)kMaxDepth) throw std::runtime_error(deepMessage());
            const uint64_t t = taxa[cur];
            uint64_t p = 0;
            if (t <= 1) { par[cur] = cur; depth[cur] = 0; top = 1; break; }                  // (0 is never climbed from; 1 is a root)
            if (!tx.parentOf(t, p)) { par[cur] = cur; depth[cur] = outside; top = outside; break; }
            if (p == t || p == 0) { par[cur] = cur; depth[cur] = 0; top = 1; break; }
            auto it = dense.find(p);
            if (it == dense.end()) { par[cur] = cur; depth[cur] = outside; top = outside; break; }   // (every tree node is a dense taxon)
            chain.push_back(cur);
            par[cur] = it->second;
            cur = it->second;
        }
        for (size_t j = chain.size(); j-- > 0;) {
            const uint32_t c = chain[j];
            if (top == outside) { depth[c] = outside; par[c] = c; }
            else {
                if (top > (uint32_t)kMaxDepth) throw std::runtime_error(deepMessage());
                depth[c] = top++;
            }
        }
    }
    std::vector<uint64_t> tab(taxa.size());
    for (size_t i = 0; i < taxa.size(); i++) tab[i] = (uint64_t)par[i] | ((uint64_t)depth[i] << 32);
    return tab;
}

// --split-taxids: the selection as the read splitter looks it up (split_sel_size_body, cf_textio.hpp), a byte per dense taxon of the
// index (HostIndex::taxa) and one more behind them for taxID 0 as the one row of a read without an assignment prints it.  A byte is
// 1 when the taxon or a node of its parent chain — the chain above, the root included — is among `listed`; a taxon the tree lacks
// (a reference's taxID without a node, taxID 0 itself) has no chain, so only when it is listed itself.  Repeats in the list change
// nothing, a list that selects nothing is legal.  Returns the listed IDs that are no taxon of the index, each once, in the list's
// order.  Throws when a chain is longer than kMaxDepth (a cycle), as lcaTable does.
inline std::vector<uint64_t> splitTaxaMask(const Taxonomy &tx, const std::vector<uint64_t> &taxa, const uint64_t *listed, uint64_t n, std::vector<uint8_t> &mask) {
    const std::unordered_set<uint64_t> want(listed, listed + n);
    std::unordered_map<uint64_t, uint8_t> known;                          // tid -> selected, for the nodes a chain has gone through
    std::vector<uint64_t> chain;
    mask.assign(taxa.size() + 1, 0);
    for (size_t i = 0; i < taxa.size(); i++) {
        chain.clear();
        uint64_t t = taxa[i];
        uint8_t sel = 0;
        for (;;) {
            auto it = known.find(t);
            if (it != known.end()) { sel = it->second; break; }
            if (chain.size() > (size_t)kMaxDepth) throw std::runtime_error(deepMessage());
            chain.push_back(t);
            if (want.count(t)) { sel = 1; break; }
            uint64_t p = 0;
            if (!tx.parentOf(t, p) || p == t || p == 0) break;            // (no node, a root)
            t = p;
        }
        for (uint64_t c : chain) known[c] = sel;
        mask[i] = sel;
    }
    mask[taxa.size()] = want.count(0) ? 1 : 0;
    std::vector<uint64_t> unknown;
    std::unordered_set<uint64_t> seen;
    for (uint64_t k = 0; k < n; k++)
        if (!std::binary_search(taxa.begin(), taxa.end(), listed[k]) && seen.insert(listed[k]).second) unknown.push_back(listed[k]);
    return unknown;
}

}  // namespace kreport
}  // namespace cfamd
