// abundance_table.hpp — the abundance profile as CSV text, for exe/cuCLARK --abundance and exe/estimate_abundance (host only, no
// device, no library).  CLARK's documented columns:
//   Name,TaxID,Lineage,Count,Proportion_All(%),Proportion_Classified(%)
//   one row per target with Count > 0, Count descending, ties by label in byte order
//   UNKNOWN,UNKNOWN,UNKNOWN,<unassigned + filtered>,<pct>,-
// Proportion_All = 100 count / all objects, Proportion_Classified = 100 count / (all - UNKNOWN), both "%g" of the double quotient,
// "0" when the denominator is 0.  A minimum abundance a = num / den (-a) leaves out the target rows whose Proportion_Classified is
// below it, compared exactly: 100 count den < num classified in 128 bits.
// Names come from <taxonomy>/names.dmp (scientific names) and nodes.dmp: Name = the label's scientific name, TaxID = the label,
// Lineage = the names of its ancestors at superkingdom (NCBI's newer dumps call it domain), phylum, class, order, family and genus
// joined with ';', for the ranks above the node's own (a rank outside the six counts as below genus), UNKNOWN for a missing one.
// A label that is not a taxid of nodes.dmp (custom labels), or no taxonomy at all: Name = the label, TaxID and Lineage UNKNOWN.
#ifndef MIC_ABUNDANCE_TABLE_HPP
#define MIC_ABUNDANCE_TABLE_HPP

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <fstream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace mic {
namespace abund {

struct Taxonomy {
  bool loaded = false;
  std::unordered_map<uint32_t, std::pair<uint32_t, std::string>> nodes;   // taxid -> (parent, rank)
  std::unordered_map<uint32_t, std::string> names;                         // taxid -> scientific name
};

// the fields of a .dmp line ("a\t|\tb\t|\t...\t|")
inline std::vector<std::string> dmp_fields(const std::string& line) {
  std::vector<std::string> out;
  size_t a = 0;
  for (;;) {
    const size_t b = line.find("\t|", a);
    if (b == std::string::npos) { if (a < line.size()) out.push_back(line.substr(a)); break; }
    out.push_back(line.substr(a, b - a));
    a = b + 2;
    if (a < line.size() && line[a] == '\t') ++a;
  }
  return out;
}

inline bool parse_taxid(const std::string& s, uint32_t& id) {
  if (s.empty() || s.size() > 9) return false;
  uint32_t v = 0;
  for (char c : s) { if (c < '0' || c > '9') return false; v = v * 10 + (uint32_t)(c - '0'); }
  id = v;
  return true;
}

// dir = the taxonomy directory (nodes.dmp, names.dmp); false (and an empty taxonomy) when either file is missing
inline bool load_taxonomy(const std::string& dir, Taxonomy& t) {
  t = Taxonomy();
  std::ifstream nodes(dir + "/nodes.dmp"), names(dir + "/names.dmp");
  if (!nodes || !names) return false;
  std::string line;
  while (std::getline(nodes, line)) {
    const std::vector<std::string> f = dmp_fields(line);
    uint32_t id, parent;
    if (f.size() >= 3 && parse_taxid(f[0], id) && parse_taxid(f[1], parent)) t.nodes[id] = {parent, f[2]};
  }
  while (std::getline(names, line)) {
    const std::vector<std::string> f = dmp_fields(line);
    uint32_t id;
    if (f.size() >= 4 && f[3] == "scientific name" && parse_taxid(f[0], id)) t.names[id] = f[1];
  }
  t.loaded = true;
  return true;
}

// 0 superkingdom / domain, 1 phylum, 2 class, 3 order, 4 family, 5 genus, 6 anything else
inline int rank_level(const std::string& r) {
  static const char* const ranks[] = {"superkingdom", "phylum", "class", "order", "family", "genus"};
  if (r == "domain") return 0;
  for (int i = 0; i < 6; ++i) if (r == ranks[i]) return i;
  return 6;
}

// Name, TaxID, Lineage of a label
inline void describe(const std::string& label, const Taxonomy* tax, std::string& name, std::string& taxid, std::string& lineage) {
  name = label; taxid = "UNKNOWN"; lineage = "UNKNOWN";
  uint32_t id;
  if (!tax || !tax->loaded || !parse_taxid(label, id)) return;
  const auto node = tax->nodes.find(id);
  if (node == tax->nodes.end()) return;
  const auto nm = tax->names.find(id);
  if (nm != tax->names.end()) name = nm->second;
  taxid = label;
  const int own = rank_level(node->second.second);
  std::string at[6];
  uint32_t cur = node->second.first, prev = id;
  for (int steps = 0; steps < 256 && cur != prev; ++steps) {      // (the root is its own parent)
    const auto n = tax->nodes.find(cur);
    if (n == tax->nodes.end()) break;
    const int lv = rank_level(n->second.second);
    if (lv < 6 && at[lv].empty()) { const auto a = tax->names.find(cur); at[lv] = a != tax->names.end() ? a->second : "UNKNOWN"; }
    prev = cur; cur = n->second.first;
  }
  lineage.clear();
  for (int lv = 0; lv < own && lv < 6; ++lv) {
    if (lv) lineage += ';';
    lineage += at[lv].empty() ? "UNKNOWN" : at[lv];
  }
  if (lineage.empty()) lineage = "UNKNOWN";
}

inline std::string pct(uint64_t count, uint64_t den) {
  if (den == 0) return "0";
  char b[64];
  snprintf(b, sizeof(b), "%g", 100.0 * (double)count / (double)den);
  return b;
}

// counts[0] unassigned, counts[1] filtered out, counts[t + 2] target t (labels[t]); min_num / min_den: the -a threshold (0 / 1: none)
inline std::string format_table(const std::vector<uint64_t>& counts, const std::vector<std::string>& labels, const Taxonomy* tax,
                                uint64_t min_num = 0, uint64_t min_den = 1) {
  uint64_t all = 0;
  for (uint64_t c : counts) all += c;
  const uint64_t unknown = (counts.size() > 0 ? counts[0] : 0) + (counts.size() > 1 ? counts[1] : 0);
  const uint64_t classified = all - unknown;
  std::vector<size_t> rows;
  for (size_t t = 0; t < labels.size() && t + 2 < counts.size(); ++t) {
    const uint64_t c = counts[t + 2];
    if (c == 0) continue;
    if (min_num && (unsigned __int128)c * 100u * min_den < (unsigned __int128)min_num * classified) continue;
    rows.push_back(t);
  }
  std::sort(rows.begin(), rows.end(), [&](size_t a, size_t b) {
    if (counts[a + 2] != counts[b + 2]) return counts[a + 2] > counts[b + 2];
    return labels[a] < labels[b];
  });
  std::string out = "Name,TaxID,Lineage,Count,Proportion_All(%),Proportion_Classified(%)\n";
  std::string name, taxid, lineage;
  for (size_t t : rows) {
    describe(labels[t], tax, name, taxid, lineage);
    const uint64_t c = counts[t + 2];
    out += name + "," + taxid + "," + lineage + "," + std::to_string((unsigned long long)c) + "," + pct(c, all) + "," + pct(c, classified) + "\n";
  }
  out += "UNKNOWN,UNKNOWN,UNKNOWN," + std::to_string((unsigned long long)unknown) + "," + pct(unknown, all) + ",-\n";
  return out;
}

}  // namespace abund
}  // namespace mic
#endif
