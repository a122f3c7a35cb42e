// line_pack_shim.cpp -- test-only C wrapper around csrc/line_pack.h (host
// code, no HIP), compiled with g++ by tests/test_line_pack.py so the packed
// gather's lane mapping is checked on the CPU for every live-line mask.
#include "line_pack.h"

extern "C" {

int lp_shim_count(unsigned mask) { return gp::lp_count(mask); }
int lp_shim_row_shift(unsigned mask) { return gp::lp_row_shift(mask); }
int lp_shim_slot(unsigned mask, int lane) { return gp::lp_slot(mask, lane); }
int lp_shim_piece(unsigned mask, int lane) { return gp::lp_piece(mask, lane); }
int lp_shim_lane(unsigned mask, int slot, int piece) { return gp::lp_lane(mask, slot, piece); }

}  // extern "C"
