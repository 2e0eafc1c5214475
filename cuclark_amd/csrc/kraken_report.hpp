// kraken_report.hpp — Kraken's sample report ("kreport": what Pavian, Krona's ktImportTaxonomy, KrakenTools, Bracken and MultiQC read)
// from the abundance counters (csrc/mic_abund.h), for exe/cuCLARK --kraken-report and exe/estimate_abundance --kraken-report (host
// only, no device, no library; the lineage is rank_report.hpp's).  No new counting: the counters are --abundance's, the tree is the
// lineage's groups over the targets.
//   line        pct\tclade\ttaxon\tcode\ttaxid\t<indent>name\n
//   pct         100 * clade / all objects, rounded half up to hundredths in integers: h = (20000 * clade + all) / (2 * all), printed
//               %3u.%02u; all == 0: "  0.00"
//   first line  (count above 0) code U, taxid 0, name unclassified; clade = taxon = buckets 0 + 1 (no hit + dropped by the filter)
//   second line (any read classified) code R, taxid 1, name root; clade = all classified reads, taxon 0
//   the tree    depth first; nodes are the groups of levels L .. 1 and the targets.  A group's parent is its group one level up,
//               top-level groups hang under the root.  A group that has a child with its own name and taxid is left out and its
//               children take its place (an inherited rank, rank_report.hpp:6-7).  Only nodes with clade above 0; siblings by clade
//               descending, then name in byte order, then level and index ascending; taxon is non-zero at targets only; <indent> is
//               two blanks per printed ancestor, the root included
//   code        from the level's rank name: superkingdom / domain D, kingdom K, phylum P, class C, order O, family F, genus G,
//               species S, anything else -.  Level 0 (the targets) takes the rank named by --kraken-target-rank (default species,
//               set_targets.sh's default)
//   taxid       the TaxID --rank-report prints, 0 where that is UNKNOWN
// Without a lineage (no --lineage, no taxonomy) the report is flat: the targets under the root.
#ifndef MIC_KRAKEN_REPORT_HPP
#define MIC_KRAKEN_REPORT_HPP

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <vector>

#include "rank_report.hpp"

namespace mic {
namespace kraken {

inline char rank_code(const std::string& r) {
  static const struct { const char* name; char code; } kCodes[] = {{"superkingdom", 'D'}, {"domain", 'D'}, {"kingdom", 'K'}, {"phylum", 'P'}, {"class", 'C'},
                                                                   {"order", 'O'}, {"family", 'F'}, {"genus", 'G'}, {"species", 'S'}};
  for (const auto& c : kCodes) if (r == c.name) return c.code;
  return '-';
}

// a lineage of no levels: the targets alone, named from the taxonomy when there is one
inline void flat_lineage(const std::vector<std::string>& labels, const abund::Taxonomy* tax, rank::Lineage& lin) {
  lin = rank::Lineage();
  lin.rank.assign(1, "target");
  rank::set_targets(labels, tax, lin);
}

// the labels of a --lineage file in the file's order (for a caller that has no targets file: exe/estimate_abundance on result CSVs)
inline bool lineage_labels(const std::string& path, std::vector<std::string>& labels, std::string& err) {
  std::ifstream in(path);
  if (!in) { err = "Failed to open the lineage file: " + path; return false; }
  std::string line;
  labels.clear();
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    labels.push_back(line.substr(0, line.find('\t')));
  }
  return true;
}

// The lineage of a report: from `file` when given, else from the taxonomy in `tax_dir` when there is one, else flat.  False (err set)
// only for a file or a taxonomy that is there and cannot be used.
inline bool report_lineage(const std::string& file, const std::string& tax_dir, const std::vector<std::string>& labels, rank::Lineage& lin, std::string& err) {
  if (!file.empty()) return rank::lineage_from_file(file, labels, lin, err);
  abund::Taxonomy tax;
  if (!tax_dir.empty() && !labels.empty() && rank::load_taxonomy(tax_dir, tax)) return rank::lineage_from_taxonomy(labels, tax, lin, err);
  flat_lineage(labels, nullptr, lin);
  return true;
}

inline std::string pct(uint64_t clade, uint64_t all) {
  const uint64_t h = all ? (uint64_t)(((unsigned __int128)20000u * clade + all) / ((unsigned __int128)2u * all)) : 0;
  char b[48];
  snprintf(b, sizeof(b), "%3u.%02u", (unsigned)(h / 100), (unsigned)(h % 100));
  return b;
}

// counts: [0] unassigned, [1] filtered out, [t + 2] target t of lin (include/mi_clark.h: mic_abundance_fetch)
inline std::string format_report(const std::vector<uint64_t>& counts, const rank::Lineage& lin, const std::string& target_rank = "species") {
  const size_t L = lin.n_levels, T = lin.n_targets();
  uint64_t all = 0;
  for (uint64_t c : counts) all += c;
  const uint64_t unclassified = (counts.size() > 0 ? counts[0] : 0) + (counts.size() > 1 ? counts[1] : 0), classified = all - unclassified;
  // clade per node, children per group (every node of level l - 1 lies in one group of level l: found through any of its targets)
  std::vector<std::vector<uint64_t>> clade(L + 1);
  std::vector<std::vector<std::vector<size_t>>> kids(L + 1);
  clade[0].assign(T, 0);
  for (size_t t = 0; t < T && t + 2 < counts.size(); ++t) clade[0][t] = counts[t + 2];
  for (size_t l = 1; l <= L; ++l) {
    clade[l].assign(lin.groups[l].size(), 0);
    kids[l].assign(lin.groups[l].size(), std::vector<size_t>());
    std::vector<char> done(lin.groups[l - 1].size(), 0);
    for (size_t t = 0; t < T; ++t) {
      const size_t lo = l >= 2 ? lin.group_of[(l - 2) * T + t] : t, hi = lin.group_of[(l - 1) * T + t];
      if (!done[lo]) { done[lo] = 1; clade[l][hi] += clade[l - 1][lo]; kids[l][hi].push_back(lo); }
    }
  }
  struct Node { size_t l, g; };
  auto inherited = [&](const Node& n) {
    if (n.l == 0) return false;
    const rank::Group& me = lin.groups[n.l][n.g];
    for (size_t c : kids[n.l][n.g]) if (lin.groups[n.l - 1][c].name == me.name && lin.groups[n.l - 1][c].taxid == me.taxid) return true;
    return false;
  };
  std::string out;
  auto line = [&](uint64_t cl, uint64_t tx, char code, const std::string& taxid, size_t depth, const std::string& name) {
    out += pct(cl, all) + "\t" + std::to_string((unsigned long long)cl) + "\t" + std::to_string((unsigned long long)tx) + "\t" + code + "\t" +
           (taxid == "UNKNOWN" ? std::string("0") : taxid) + "\t" + std::string(2 * depth, ' ') + name + "\n";
  };
  // the printed siblings behind a set of nodes: inherited groups give way to their children, empty nodes go, the rest is ordered
  auto siblings = [&](std::vector<Node> in) {
    std::vector<Node> outv;
    while (!in.empty()) {
      const Node n = in.back(); in.pop_back();
      if (inherited(n)) { for (size_t c : kids[n.l][n.g]) in.push_back({n.l - 1, c}); continue; }
      if (clade[n.l][n.g]) outv.push_back(n);
    }
    std::sort(outv.begin(), outv.end(), [&](const Node& a, const Node& b) {
      if (clade[a.l][a.g] != clade[b.l][b.g]) return clade[a.l][a.g] > clade[b.l][b.g];
      const std::string &na = lin.groups[a.l][a.g].name, &nb = lin.groups[b.l][b.g].name;
      if (na != nb) return na < nb;
      if (a.l != b.l) return a.l < b.l;
      return a.g < b.g;
    });
    return outv;
  };
  struct Frame { Node n; size_t depth; };
  if (unclassified) line(unclassified, unclassified, 'U', "0", 0, "unclassified");
  if (classified) line(classified, 0, 'R', "1", 0, "root");
  std::vector<Node> top;
  for (size_t g = 0; g < (L ? lin.groups[L].size() : T); ++g) top.push_back({L, g});
  std::vector<Frame> stack;
  { const std::vector<Node> s = siblings(top); for (size_t i = s.size(); i-- > 0;) stack.push_back({s[i], 1}); }
  while (!stack.empty()) {
    const Frame f = stack.back(); stack.pop_back();
    const rank::Group& g = lin.groups[f.n.l][f.n.g];
    line(clade[f.n.l][f.n.g], f.n.l == 0 ? clade[0][f.n.g] : 0, rank_code(f.n.l == 0 ? target_rank : lin.rank[f.n.l]), g.taxid, f.depth, g.name);
    if (f.n.l == 0) continue;
    std::vector<Node> ch;
    for (size_t c : kids[f.n.l][f.n.g]) ch.push_back({f.n.l - 1, c});
    const std::vector<Node> s = siblings(ch);
    for (size_t i = s.size(); i-- > 0;) stack.push_back({s[i], f.depth + 1});
  }
  return out;
}

}  // namespace kraken
}  // namespace mic
#endif
