// result_csv.hpp — the column reader of the post-processing tools (exe/estimate_abundance, exe/evaluate_density; host only): the
// last seven fields of a result line - Length, Gamma, 1st_assignment, score1, 2nd_assignment, score2, confidence - which plain and
// --extended result CSVs share.  Read from the right: the object name in front may hold commas.
#ifndef MIC_RESULT_CSV_HPP
#define MIC_RESULT_CSV_HPP

#include <stdint.h>

#include <string>

#include "decimal_text.hpp"

namespace mic {
namespace csv {

inline bool parse_u32(const std::string& s, uint64_t& v) {
  if (s.empty() || s.size() > 10) return false;
  v = 0;
  for (char c : s) { if (c < '0' || c > '9') return false; v = v * 10 + (uint64_t)(c - '0'); }
  return v <= 0xFFFFFFFFull;
}

// fld[0 .. 6] = the seven fields, *end = position of the comma in front of them; false: the line has fewer fields
inline bool last_seven(const std::string& line, std::string fld[7], size_t* end_out) {
  size_t end = line.size();
  for (int j = 6; j >= 0; --j) {
    const size_t c = line.rfind(',', end == 0 ? std::string::npos : end - 1);
    if (c == std::string::npos || end == 0) return false;
    fld[j] = line.substr(c + 1, end - c - 1);
    end = c;
  }
  *end_out = end;
  return true;
}

}  // namespace csv
}  // namespace mic
#endif
