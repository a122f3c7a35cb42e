// line_cands_shim.cpp -- test-only C wrapper around csrc/line_cands.h (host
// code, no HIP), compiled with g++ by tests/test_line_cands.py so the candidate
// list of the per-line done-neighbour rule is checked on the CPU with
// synthetic row_ptr arrays.
#include "line_cands.h"

extern "C" {

// out: [cap].  Returns the number of candidates (the first min(count, cap) are written).
long long lc_cands(const long long* row_ptr, long long nloc, long long min_deg, int* out, long long cap) {
  const std::vector<int32_t> c = gp::line_cands(reinterpret_cast<const int64_t*>(row_ptr), nloc, min_deg);
  for (size_t k = 0; k < c.size() && (long long)k < cap; ++k) out[k] = c[k];
  return (long long)c.size();
}

int lc_default_min_deg() { return GP_LINE_DONE_MIN_DEG; }

}  // extern "C"
