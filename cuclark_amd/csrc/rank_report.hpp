// rank_report.hpp — lineages for the rank roll-up (csrc/mic_rollup.h) and its report, for exe/cuCLARK --rank-report and
// exe/estimate_abundance --rank-report (host only, no device, no library; next to abundance_table.hpp, whose Taxonomy it reuses).
//
// A lineage gives every target label its group at L levels above the targets.
//   from a taxonomy (nodes.dmp, names.dmp when present): L = 6, level 1 .. 6 = genus, family, order, class, phylum, superkingdom
//     (domain).  A label that is a taxid of nodes.dmp gets its ancestors at these ranks, only ranks above its own; a rank its
//     lineage does not have inherits the group of the level below; a label the taxonomy does not know stays alone at every level.
//   from a file (--lineage <tsv>): one line per target label, label<TAB>name_1<TAB>...<TAB>name_L, the same L (1 .. 7) on every
//     line, every label of the targets once, no others; a line that starts with '#' names the levels (#<anything><TAB>rank_1<TAB>...).
// Group ids are numbered by first appearance in target order; a level that is not a coarsening of the one below is an error that
// names the label.
// The report (CSV): Level,Rank,Name,TaxID,Reads,CladeReads,Proportion_All(%)
//   Reads = the reads assigned to the group at that level, CladeReads = Reads plus the Reads of every group below that it contains,
//   Proportion_All = 100 CladeReads / all objects (abund::pct).  Levels from the top down to 0 (the targets), inside a level
//   CladeReads descending, then the name in byte order; rows with CladeReads == 0 are left out.  Then
//   -,-,UNRESOLVED,UNKNOWN,<n>,<n>,<pct>   (hits, but no level passes the filter)
//   -,-,UNKNOWN,UNKNOWN,<n>,<n>,<pct>      (no hit)
#ifndef MIC_RANK_REPORT_HPP
#define MIC_RANK_REPORT_HPP

#include <stdint.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "abundance_table.hpp"

namespace mic {
namespace rank {

struct Group { std::string name, taxid; };

struct Lineage {
  uint32_t n_levels = 0;
  std::vector<std::string> rank;                  // [n_levels + 1]: the levels' names, rank[0] = "target"
  std::vector<uint16_t> group_of;                 // [n_levels][T], level 1 first (the C ABI's form)
  std::vector<std::vector<Group>> groups;         // [n_levels + 1][G_l], groups[0] = the targets
  uint32_t n_targets() const { return groups.empty() ? 0u : (uint32_t)groups[0].size(); }
  uint64_t n_counters() const { uint64_t n = 2; for (const auto& g : groups) n += g.size(); return n; }
};

// nodes.dmp is needed, names.dmp is not (groups are then named by their taxid)
inline bool load_taxonomy(const std::string& dir, abund::Taxonomy& t) {
  if (abund::load_taxonomy(dir, t)) return true;
  t = abund::Taxonomy();
  std::ifstream nodes(dir + "/nodes.dmp");
  if (!nodes) return false;
  std::string line;
  while (std::getline(nodes, line)) {
    const std::vector<std::string> f = abund::dmp_fields(line);
    uint32_t id, parent;
    if (f.size() >= 3 && abund::parse_taxid(f[0], id) && abund::parse_taxid(f[1], parent)) t.nodes[id] = {parent, f[2]};
  }
  t.loaded = true;
  return true;
}

// keys[l - 1][t] = what names target t's group at level l (equal keys = one group), shown[l - 1][t] = that group as the report shows
// it -> first-appearance ids, and the coarsening condition checked; false with a message that names the label
inline bool finish_lineage(const std::vector<std::string>& labels, const std::vector<std::vector<std::string>>& keys,
                           const std::vector<std::vector<Group>>& shown, Lineage& lin, std::string& err) {
  const size_t T = labels.size(), L = keys.size();
  lin.n_levels = (uint32_t)L;
  lin.group_of.assign(L * T, 0);
  lin.groups.resize(L + 1);
  for (size_t l = 1; l <= L; ++l) {
    std::unordered_map<std::string, uint16_t> ids;
    lin.groups[l].clear();
    for (size_t t = 0; t < T; ++t) {
      auto it = ids.find(keys[l - 1][t]);
      if (it == ids.end()) { it = ids.emplace(keys[l - 1][t], (uint16_t)ids.size()).first; lin.groups[l].push_back(shown[l - 1][t]); }
      lin.group_of[(l - 1) * T + t] = it->second;
    }
    if (l >= 2) {   // targets that share a group at l - 1 share one at l
      std::vector<int> parent(lin.groups[l - 1].size(), -1);
      std::vector<size_t> first(lin.groups[l - 1].size(), 0);
      for (size_t t = 0; t < T; ++t) {
        const uint16_t lo = lin.group_of[(l - 2) * T + t], hi = lin.group_of[(l - 1) * T + t];
        if (parent[lo] < 0) { parent[lo] = hi; first[lo] = t; }
        else if (parent[lo] != (int)hi) {
          err = "The lineage of target " + labels[t] + " is not nested: at level " + std::to_string(l - 1) + " (" + lin.rank[l - 1] + ") it is in " +
                lin.groups[l - 1][lo].name + " with target " + labels[first[lo]] + ", at level " + std::to_string(l) + " (" + lin.rank[l] +
                ") the two are in " + lin.groups[l][hi].name + " and " + lin.groups[l][parent[lo]].name + ".";
          return false;
        }
      }
    }
  }
  return true;
}

inline void set_targets(const std::vector<std::string>& labels, const abund::Taxonomy* tax, Lineage& lin) {
  lin.groups.assign(1, std::vector<Group>());
  std::string name, taxid, lineage;
  for (const std::string& lab : labels) { abund::describe(lab, tax, name, taxid, lineage); lin.groups[0].push_back({name, taxid}); }
}

inline bool lineage_from_taxonomy(const std::vector<std::string>& labels, const abund::Taxonomy& tax, Lineage& lin, std::string& err) {
  static const char* const kRanks[7] = {"target", "genus", "family", "order", "class", "phylum", "superkingdom"};
  const size_t T = labels.size(), L = 6;
  if (T == 0 || T > 65535) { err = "A lineage needs 1 .. 65535 targets."; return false; }
  lin = Lineage();
  lin.rank.assign(kRanks, kRanks + 7);
  set_targets(labels, &tax, lin);
  std::vector<std::vector<std::string>> keys(L, std::vector<std::string>(T));
  std::vector<std::vector<Group>> shown(L, std::vector<Group>(T));
  for (size_t t = 0; t < T; ++t) {
    uint32_t at[7] = {0, 0, 0, 0, 0, 0, 0};      // the ancestor at level 1 .. 6 (0: none)
    int own = 7;                                  // a label the taxonomy does not know keeps no ancestor
    uint32_t id;
    if (tax.loaded && abund::parse_taxid(labels[t], id)) {
      const auto node = tax.nodes.find(id);
      if (node != tax.nodes.end()) {
        const int r = abund::rank_level(node->second.second);       // 0 superkingdom .. 5 genus, 6 anything else
        own = r == 6 ? 0 : 6 - r;
        uint32_t cur = node->second.first, prev = id;
        for (int steps = 0; steps < 256 && cur != prev; ++steps) {
          const auto n = tax.nodes.find(cur);
          if (n == tax.nodes.end()) break;
          const int lr = abund::rank_level(n->second.second);
          if (lr < 6 && !at[6 - lr]) at[6 - lr] = cur;
          prev = cur; cur = n->second.first;
        }
      }
    }
    std::string key = "t" + std::to_string(t);
    Group g = lin.groups[0][t];
    for (size_t l = 1; l <= L; ++l) {
      if ((int)l > own && at[l]) {
        key = "n" + std::to_string(at[l]);
        const auto nm = tax.names.find(at[l]);
        g.taxid = std::to_string(at[l]);
        g.name = nm != tax.names.end() ? nm->second : g.taxid;
      }
      keys[l - 1][t] = key; shown[l - 1][t] = g;
    }
  }
  return finish_lineage(labels, keys, shown, lin, err);
}

inline bool lineage_from_file(const std::string& path, const std::vector<std::string>& labels, Lineage& lin, std::string& err) {
  const size_t T = labels.size();
  if (T == 0 || T > 65535) { err = "A lineage needs 1 .. 65535 targets."; return false; }
  std::ifstream in(path);
  if (!in) { err = "Failed to open the lineage file: " + path; return false; }
  std::unordered_map<std::string, size_t> index;
  for (size_t t = 0; t < T; ++t) index[labels[t]] = t;
  std::vector<std::vector<std::string>> rows(T);
  std::vector<std::string> ranks;
  size_t L = 0, ln = 0;
  std::string line;
  while (std::getline(in, line)) {
    ++ln;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    std::vector<std::string> f;
    for (size_t a = 0;;) { const size_t b = line.find('\t', a); f.push_back(line.substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; }
    const std::string where = "Line " + std::to_string(ln) + " of " + path;
    if (line[0] == '#') { ranks.assign(f.begin() + 1, f.end()); continue; }
    if (f.size() < 2) { err = where + ": expected label<TAB>name_1<TAB>...<TAB>name_L."; return false; }
    if (L == 0) L = f.size() - 1;
    if (f.size() - 1 != L) { err = where + " (" + f[0] + ") has " + std::to_string(f.size() - 1) + " levels, the lines before it " + std::to_string(L) + "."; return false; }
    for (size_t i = 1; i < f.size(); ++i) if (f[i].empty()) { err = where + " (" + f[0] + "): an empty name at level " + std::to_string(i) + "."; return false; }
    const auto it = index.find(f[0]);
    if (it == index.end()) { err = where + ": " + f[0] + " is not a label of the targets."; return false; }
    if (!rows[it->second].empty()) { err = where + ": the label " + f[0] + " appears twice."; return false; }
    rows[it->second].assign(f.begin() + 1, f.end());
  }
  if (L == 0 || L > 7) { err = "The lineage file " + path + " must give 1 .. 7 levels per label."; return false; }
  for (size_t t = 0; t < T; ++t) if (rows[t].empty()) { err = "The lineage file " + path + " has no line for the target " + labels[t] + "."; return false; }
  if (!ranks.empty() && ranks.size() != L) { err = "The '#' line of " + path + " names " + std::to_string(ranks.size()) + " levels, the labels have " + std::to_string(L) + "."; return false; }
  lin = Lineage();
  lin.rank.assign(1, "target");
  for (size_t l = 1; l <= L; ++l) lin.rank.push_back(ranks.empty() ? "level" + std::to_string(l) : ranks[l - 1]);
  set_targets(labels, nullptr, lin);
  std::vector<std::vector<std::string>> keys(L, std::vector<std::string>(T));
  std::vector<std::vector<Group>> shown(L, std::vector<Group>(T));
  for (size_t t = 0; t < T; ++t)
    for (size_t l = 0; l < L; ++l) { keys[l][t] = rows[t][l]; shown[l][t] = {rows[t][l], "UNKNOWN"}; }
  return finish_lineage(labels, keys, shown, lin, err);
}

// counts: [0] no hit, [1] unresolved, [2 + off_l + g] (include/mi_clark.h)
inline std::string format_report(const std::vector<uint64_t>& counts, const Lineage& lin) {
  const size_t L = lin.n_levels, T = lin.n_targets();
  uint64_t all = 0;
  for (uint64_t c : counts) all += c;
  std::vector<std::vector<uint64_t>> reads(L + 1), clade(L + 1);
  size_t off = 2;
  for (size_t l = 0; l <= L; ++l) {
    const size_t G = lin.groups[l].size();
    reads[l].assign(G, 0);
    for (size_t g = 0; g < G; ++g) if (off + g < counts.size()) reads[l][g] = counts[off + g];
    off += G;
    clade[l] = reads[l];
    if (l >= 1) {
      // every group of level l - 1 lies in one group of level l: its clade is added once, through any of its targets
      std::vector<char> done(lin.groups[l - 1].size(), 0);
      for (size_t t = 0; t < T; ++t) {
        const size_t lo = l >= 2 ? lin.group_of[(l - 2) * T + t] : t, hi = lin.group_of[(l - 1) * T + t];
        if (!done[lo]) { done[lo] = 1; clade[l][hi] += clade[l - 1][lo]; }
      }
    }
  }
  std::string out = "Level,Rank,Name,TaxID,Reads,CladeReads,Proportion_All(%)\n";
  for (size_t l = L + 1; l-- > 0;) {
    std::vector<size_t> rows;
    for (size_t g = 0; g < lin.groups[l].size(); ++g) if (clade[l][g]) rows.push_back(g);
    std::sort(rows.begin(), rows.end(), [&](size_t a, size_t b) {
      if (clade[l][a] != clade[l][b]) return clade[l][a] > clade[l][b];
      if (lin.groups[l][a].name != lin.groups[l][b].name) return lin.groups[l][a].name < lin.groups[l][b].name;
      return a < b;
    });
    for (size_t g : rows)
      out += std::to_string(l) + "," + lin.rank[l] + "," + lin.groups[l][g].name + "," + lin.groups[l][g].taxid + "," +
             std::to_string((unsigned long long)reads[l][g]) + "," + std::to_string((unsigned long long)clade[l][g]) + "," + abund::pct(clade[l][g], all) + "\n";
  }
  const uint64_t unresolved = counts.size() > 1 ? counts[1] : 0, unknown = counts.empty() ? 0 : counts[0];
  out += "-,-,UNRESOLVED,UNKNOWN," + std::to_string((unsigned long long)unresolved) + "," + std::to_string((unsigned long long)unresolved) + "," + abund::pct(unresolved, all) + "\n";
  out += "-,-,UNKNOWN,UNKNOWN," + std::to_string((unsigned long long)unknown) + "," + std::to_string((unsigned long long)unknown) + "," + abund::pct(unknown, all) + "\n";
  return out;
}

}  // namespace rank
}  // namespace mic
#endif
