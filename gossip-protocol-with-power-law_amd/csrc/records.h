// records.h -- the per-run records as one lifecycle: what a
// record keeps in the context, how that state moves, and the table every
// gp_reset, round, checkpoint load and free walks (records.hip).  A new record
// is a RecordId, one RecordOps in its own unit and one line of kRecords.
//
// Plain C++, no HIP: tests/test_record_state.py drives the state part with g++.
#pragma once
#include <cstdint>

#include "../../include/gossip_capi.h"

namespace gp {

struct Ctx;

// kRecords' order, which is the order of the rounds' counting passes
enum RecordId {
  R_LOAD = 0, R_CURVE, R_FRESH, R_MULT, R_FRESH_CURVE, R_LINK, R_DELAY, R_DELAY_DIST, R_WATCH, R_COUNT
};

// want: what the record's gp_track_* call asked for, for the next gp_reset;
// on: what the run since the last gp_reset keeps; valid: falls when a
// checkpoint restores the run past round 0 (no record is in the blob)
struct RecordState {
  bool want = false, on = false, valid = false;
};

// gp_reset: the request takes effect
inline void record_take_effect(RecordState& s, bool wanted_now) { s.on = s.valid = wanted_now; }
inline void record_off(RecordState& s) { s.on = s.valid = false; }
// gp_checkpoint_load restored the run at `round`
inline void record_restored(RecordState& s, int32_t round) {
  if (s.on && round > 0) s.valid = false;
}
// why a read is refused (0: it is not).  keeps_partition: the record is kept
// by a vertex-partitioned context too, for its owned slice
inline int record_refusal(const RecordState& s, bool partitioned, bool keeps_partition, bool state_ready) {
  if (partitioned && !keeps_partition) return GP_ENOTRACK;
  if (!s.on || !state_ready) return GP_ENOTRACK;
  if (!s.valid) return GP_ESTATE;
  return 0;
}

// the receipt delays and their distributions read the receivers' new rows only
// when the table's messages start in more than one round (uniform < 0), or
// when GP_DELAY_ROWS forces the row pass
inline bool delay_rows_needed(bool delay_want, bool dist_want, int32_t uniform, bool force_rows) {
  return (delay_want || dist_want) && (uniform < 0 || force_rows);
}

// who wants the exact frontier rows (Ctx::d_frx): bit FRX_RECORD0 + id for the
// records, one bit each for the others.  alloc_state sizes the rows for the
// mask and stores it; gp_reset reallocates when it changed
constexpr uint32_t FRX_MSG_FORWARDS = 1u << 0;   // cfg.track_msg_forwards
constexpr uint32_t FRX_LOCAL = 1u << 1;          // a vertex partition's boundary exchange
constexpr uint32_t FRX_LOSS = 1u << 2;           // lossy links (lossy.hip)
constexpr uint32_t FRX_LAG = 1u << 3;            // delayed links (delayed.hip)
constexpr int FRX_RECORD0 = 4;
inline uint32_t frx_mask(bool msg_forwards, bool local, bool loss, bool lag, const bool record_needs[R_COUNT]) {
  uint32_t m = (msg_forwards ? FRX_MSG_FORWARDS : 0u) | (local ? FRX_LOCAL : 0u) | (loss ? FRX_LOSS : 0u) |
               (lag ? FRX_LAG : 0u);
  for (int k = 0; k < R_COUNT; ++k)
    if (record_needs[k]) m |= 1u << (FRX_RECORD0 + k);
  return m;
}

// one record.  A null hook means the default named beside it
struct RecordOps {
  RecordId id;
  const char* noun;         // "fresh deliveries": the refusals' subject
  const char* call;         // "gp_track_fresh": the call that turns it on
  bool single_rank_only;    // not kept by a vertex-partitioned context
  int walks_arcs;           // 0: no.  Else the record counts deliveries over arcs, which lossy and delayed links
                            // refuse; the value orders their refusal's choice among several (1 first)
  bool (*wanted)(const Ctx*);       // null: the state's want flag
  bool (*needs_frx)(const Ctx*);    // null: wanted
  int (*reset)(Ctx*);               // gp_reset of a run that keeps it: buffers for this run, cleared
  void (*free)(Ctx*);               // buffers gone, the record off
  int (*count_round)(Ctx*);         // null: none.  After E_r, on the engine stream
  void (*forget)(Ctx*);             // null: nothing.  A new overlay: the request named the old one's vertices
  bool (*outlives_restore)(const Ctx*);   // null: never.  The record is a function of the restored state
};

// A record's unit defines its ops as GP_RECORD_OPS(X_record) = {...}.  The
// device pass of a .hip unit would emit a namespace-scope constant for the GPU
// as well, where the hooks -- host functions -- do not exist: there the ops
// become a unit-local constant that nothing reads
#ifdef __HIP_DEVICE_COMPILE__
#define GP_RECORD_OPS(name) [[maybe_unused]] static const RecordOps name##_host_only
#else
#define GP_RECORD_OPS(name) const RecordOps name
#endif
extern const RecordOps load_record, curve_record, fresh_record, mult_record, fresh_curve_record, link_record,
    delay_record, delay_dist_record, watch_record;
extern const RecordOps* const kRecords[R_COUNT];

// records.hip: the table's walks ...
bool record_wanted(const Ctx* c, const RecordOps& o);   // asked for, whatever the partition
uint32_t frx_users(const Ctx* c);
int records_reset(Ctx* c);                        // gp_reset: every request takes effect
void records_free(Ctx* c);
int records_count_round(Ctx* c);
void records_restored(Ctx* c, int32_t round);
void records_forget(Ctx* c);
const RecordOps* records_arc_walker(const Ctx* c);   // the wanted record lossy / delayed links refuse first (null: none)
// ... and what every record's unit shares
int record_readable(Ctx* c, const RecordOps& o);                  // a read's refusals (record_refusal), with their messages
int record_need_rows(Ctx* c, const RecordOps& o, int64_t rows);   // GP_ESTATE unless d_frx covers `rows` vertices
int record_track(Ctx* c, const RecordOps& o, int32_t on);         // the gp_track_* bodies

}  // namespace gp
