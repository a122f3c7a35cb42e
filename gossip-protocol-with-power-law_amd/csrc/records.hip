// records.hip -- the table of per-run records and its walks (records.h).  The
// order is the order of the rounds' counting passes; resets, frees and restores
// follow it too, which is free: every record writes its own buffers and flags
// only (each X_reset clears what X_free frees), and reads the run state that
// gp_reset has put in place before records_reset.
#include "gp_device.h"

namespace gp {

#ifndef __HIP_DEVICE_COMPILE__   // (host data: see GP_RECORD_OPS)
const RecordOps* const kRecords[R_COUNT] = {&load_record, &curve_record, &fresh_record, &mult_record, &fresh_curve_record,
                                            &link_record, &delay_record, &delay_dist_record, &watch_record};
#endif

bool record_wanted(const Ctx* c, const RecordOps& o) { return o.wanted ? o.wanted(c) : c->rec[o.id].want; }

static bool record_needs_frx(const Ctx* c, const RecordOps& o) { return o.needs_frx ? o.needs_frx(c) : record_wanted(c, o); }

uint32_t frx_users(const Ctx* c) {
  bool needs[R_COUNT];
  for (int k = 0; k < R_COUNT; ++k) needs[kRecords[k]->id] = record_needs_frx(c, *kRecords[k]);
  return frx_mask(c->cfg.track_msg_forwards != 0, c->local, c->loss_want || c->repair_want, c->lag_want, needs);   // (repair reads them as loss does)
}

int records_reset(Ctx* c) {
  for (const RecordOps* o : kRecords) {
    if (!record_wanted(c, *o) || (o->single_rank_only && c->nranks != 1)) {
      o->free(c);
      continue;
    }
    GP_TRY(o->reset(c));
    record_take_effect(c->rec[o->id], true);
  }
  return 0;
}

void records_free(Ctx* c) {
  for (const RecordOps* o : kRecords) o->free(c);
}

int records_count_round(Ctx* c) {
  for (const RecordOps* o : kRecords) {
    const RecordState& s = c->rec[o->id];
    if (o->count_round && s.on && s.valid) GP_TRY(o->count_round(c));
  }
  return 0;
}

void records_restored(Ctx* c, int32_t round) {
  for (const RecordOps* o : kRecords)
    if (!o->outlives_restore || !o->outlives_restore(c)) record_restored(c->rec[o->id], round);
}

void records_forget(Ctx* c) {
  for (const RecordOps* o : kRecords)
    if (o->forget) o->forget(c);
}

const RecordOps* records_arc_walker(const Ctx* c) {
  const RecordOps* first = nullptr;
  for (const RecordOps* o : kRecords)
    if (o->walks_arcs && record_wanted(c, *o) && (!first || o->walks_arcs < first->walks_arcs)) first = o;
  return first;
}

int record_readable(Ctx* c, const RecordOps& o) {
  const int rc = record_refusal(c->rec[o.id], c->nranks > 1, !o.single_rank_only, state_ready(c));
  if (rc == 0) return 0;
  if (rc == GP_ESTATE)
    return set_error(rc, std::string("the run was restored past round 0: ") + o.noun + " not kept (gp_reset)");
  if (c->nranks > 1 && o.single_rank_only)
    return set_error(rc, std::string(o.noun) + ": not kept by a vertex-partitioned context");
  return set_error(rc, std::string(o.call) + ", then gp_reset");
}

int record_need_rows(Ctx* c, const RecordOps& o, int64_t rows) {
  if (!c->d_frx[0] || c->frx_rows < rows) return set_error(GP_ESTATE, std::string("internal: ") + o.noun + " without frontier rows");
  return 0;
}

int record_track(Ctx* c, const RecordOps& o, int32_t on) {
  if (!c) return set_error(GP_EINVAL, "null ctx");
  c->rec[o.id].want = on != 0;   // (allocated, and counted from, the next gp_reset)
  return 0;
}

}  // namespace gp
