// records_shim.cpp -- test-only C wrapper around the state part of
// csrc/records.h (plain C++, no HIP), compiled with g++ by
// tests/test_record_state.py: the records' flag transitions, the refusal
// precedence of their reads and the mask of frontier-row users.
#include "records.h"

extern "C" {

// flags: bit 0 want, bit 1 on, bit 2 valid
static gp::RecordState unpack(int flags) {
  gp::RecordState s;
  s.want = flags & 1;
  s.on = flags & 2;
  s.valid = flags & 4;
  return s;
}
static int pack(const gp::RecordState& s) { return (s.want ? 1 : 0) | (s.on ? 2 : 0) | (s.valid ? 4 : 0); }

int rs_take_effect(int flags, int wanted_now) {
  gp::RecordState s = unpack(flags);
  gp::record_take_effect(s, wanted_now != 0);
  return pack(s);
}
int rs_off(int flags) {
  gp::RecordState s = unpack(flags);
  gp::record_off(s);
  return pack(s);
}
int rs_restored(int flags, int round) {
  gp::RecordState s = unpack(flags);
  gp::record_restored(s, round);
  return pack(s);
}
int rs_refusal(int flags, int partitioned, int keeps_partition, int state_ready) {
  return gp::record_refusal(unpack(flags), partitioned != 0, keeps_partition != 0, state_ready != 0);
}
int rs_delay_rows_needed(int delay_want, int dist_want, int uniform, int force_rows) {
  return gp::delay_rows_needed(delay_want != 0, dist_want != 0, uniform, force_rows != 0) ? 1 : 0;
}
// needs: bit k = record k needs the rows
unsigned rs_frx_mask(int msg_forwards, int local, int loss, int lag, unsigned needs) {
  bool n[gp::R_COUNT];
  for (int k = 0; k < gp::R_COUNT; ++k) n[k] = (needs >> k) & 1u;
  return gp::frx_mask(msg_forwards != 0, local != 0, loss != 0, lag != 0, n);
}
int rs_record_count() { return gp::R_COUNT; }
int rs_record0() { return gp::FRX_RECORD0; }
int rs_enotrack() { return GP_ENOTRACK; }
int rs_estate() { return GP_ESTATE; }

}  // extern "C"
