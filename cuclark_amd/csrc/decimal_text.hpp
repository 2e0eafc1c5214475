// decimal_text.hpp — the printed "%g" fields of a result CSV read back as exact decimals (exe/estimate_abundance, exe/evaluate_density;
// host only).  Forms: "0.762887", "1", "5e-05", "1.21053", "-0"; anything else - "-nan", "inf" - is no number.
#ifndef MIC_DECIMAL_TEXT_HPP
#define MIC_DECIMAL_TEXT_HPP

#include <stdint.h>

#include <string>

namespace mic {
namespace decimal {

// value = m 10^exp10.  False: a sign '-' (a negative value, or -0), no digit, or anything that is no decimal number.
struct Value { unsigned __int128 m = 0; int exp10 = 0; };
inline bool parse(const std::string& s, Value& v) {
  size_t i = 0;
  if (i < s.size() && (s[i] == '-' || s[i] == '+')) { if (s[i] == '-') return false; ++i; }
  unsigned __int128 m = 0;
  int exp10 = 0, digits = 0;
  bool point = false;
  for (; i < s.size(); ++i) {
    const char c = s[i];
    if (c == '.') { if (point) return false; point = true; continue; }
    if (c < '0' || c > '9') break;
    ++digits;
    if (m < (unsigned __int128)1 << 100) { m = m * 10 + (unsigned)(c - '0'); if (point) --exp10; }
    else if (!point) ++exp10;
  }
  if (digits == 0) return false;
  if (i < s.size()) {
    if (s[i] != 'e' && s[i] != 'E') return false;
    ++i;
    int sign = 1, e = 0;
    if (i < s.size() && (s[i] == '-' || s[i] == '+')) { if (s[i] == '-') sign = -1; ++i; }
    if (i >= s.size()) return false;
    for (; i < s.size(); ++i) { if (s[i] < '0' || s[i] > '9') return false; if (e < 1000) e = e * 10 + (s[i] - '0'); }
    exp10 += sign * e;
  }
  v.m = m; v.exp10 = exp10;
  return true;
}

// value of the text >= num / den?  (no number, a negative one and zero fail every positive threshold)
inline bool at_least(const std::string& s, uint64_t num, uint64_t den) {
  if (num == 0) return true;
  Value v;
  if (!parse(s, v) || v.m == 0) return false;
  // m 10^exp10 >= num / den  <=>  m den 10^exp10 >= num
  unsigned __int128 lhs = v.m * den, rhs = num;
  if (v.exp10 >= 0) { if (v.exp10 > 12) return true; for (int j = 0; j < v.exp10; ++j) lhs *= 10; }
  else {
    int sh = -v.exp10;
    for (; sh > 0 && lhs % 10 == 0; --sh) lhs /= 10;       // (trailing zeros of a long mantissa first: rhs stays in range)
    if (sh > 26) return false;
    for (int j = 0; j < sh; ++j) rhs *= 10;
  }
  return lhs >= rhs;
}

// floor(100 value) clamped into 0 .. max_bin; no number, a negative one and -0: 0
inline uint32_t floor_hundredths(const std::string& s, uint32_t max_bin) {
  Value v;
  if (!parse(s, v) || v.m == 0) return 0;
  unsigned __int128 m = v.m;
  int e = v.exp10 + 2;
  for (; e > 0 && m <= max_bin; --e) m *= 10;
  for (; e < 0 && m != 0; ++e) m /= 10;
  return m > max_bin ? max_bin : (uint32_t)m;
}

// num / den with `decimals` digits behind the point, rounded half up, from integer arithmetic (den != 0, decimals <= 9): "44.44", "1.00"
inline std::string ratio_text(uint64_t num, uint64_t den, int decimals) {
  unsigned __int128 scale = 1;
  for (int j = 0; j < decimals; ++j) scale *= 10;
  const unsigned __int128 q = ((unsigned __int128)num * scale + den / 2) / den;
  const uint64_t whole = (uint64_t)(q / scale), frac = (uint64_t)(q % scale);
  std::string out = std::to_string((unsigned long long)whole);
  if (decimals > 0) {
    const std::string f = std::to_string((unsigned long long)frac);
    out += "." + std::string((size_t)decimals - f.size(), '0') + f;
  }
  return out;
}

}  // namespace decimal
}  // namespace mic
#endif
