// block_order_shim.cpp -- test-only C wrapper around csrc/block_order.h (host
// code, no HIP), compiled with g++ by tests/test_block_order.py so the launch
// order of k_expand's blocks is checked on the CPU with synthetic row_ptr arrays.
#include "block_order.h"

extern "C" {

// out: [ceil(nloc / 64)].  Returns the number of blocks written.
long long bo_order(const long long* row_ptr, long long nloc, long long hub_thr, long long cut, int* out) {
  const std::vector<int32_t> o = gp::block_order(reinterpret_cast<const int64_t*>(row_ptr), nloc, hub_thr, cut);
  for (size_t k = 0; k < o.size(); ++k) out[k] = o[k];
  return (long long)o.size();
}

}  // extern "C"
