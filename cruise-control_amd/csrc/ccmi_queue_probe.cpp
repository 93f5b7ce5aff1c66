// ccmi_queue_probe (diagnostics, declared in ccmi_session.h, not in the ABI): one queue scan on the session's current
// model — the call Engine::queueScan makes, over the keyed membership table, the mirror flattened or the snapshot
// directory, whichever the session's knobs select — next to the answer of a plain loop over the model. The loop takes
// nothing from the mirror, the table or the directory: a broker's rows are its replicas the Spec selects, in key order
// (entry 0 without the rows at or below skip_key), walked row-major over the columns; the first pair that is not
// blocked and that the host predicates accept wins. The winner is compared as (entry, replica, column), which does not
// depend on the path that served the scan. With the keyed table current the probe also audits it: every broker's rows
// in the mirror, and in the device table read back through its host mapping, against the model's.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/host_view.h"
#include "engine/predicates.h"
#include "engine/threadpin.h"

namespace {

using Row = std::pair<uint64_t, int32_t>;  // (Model::replicaKey, replica)

ccmi::Model::Spec specOf(const ccmi_queue_probe_args& a) {
  if (a.score_res < -1 || a.score_res > 3) throw std::invalid_argument("score resource out of range");
  ccmi::Model::Spec s;
  s.selLeaders = a.sel_leaders != 0;
  s.scoreRes = a.score_res;
  s.scoreReverse = a.score_reverse != 0;
  s.prioOffline = a.prio_offline != 0;
  s.prioImmigrants = a.prio_immigrants != 0;
  s.selExclTopics = a.sel_excl_topics != 0;
  return s;
}

// broker b's rows under `spec`, in key order, from the model alone
std::vector<Row> rowsOf(const ccmi::Model& m, const ccmi::Model::Spec& spec, int b) {
  std::vector<Row> v;
  for (int r : m.bRepl[b])
    if (m.selects(spec, r)) v.push_back({m.replicaKey(spec, r), r});
  std::sort(v.begin(), v.end());
  return v;
}

struct TableRow {
  uint64_t key;
  int32_t r, p, topic;
  bool operator<(const TableRow& o) const { return key != o.key ? key < o.key : r < o.r; }
  bool operator==(const TableRow& o) const { return key == o.key && r == o.r && p == o.p && topic == o.topic; }
};

}  // namespace

extern "C" ccmi_status ccmi_queue_probe_view(ccmi_session* s, const ccmi_queue_probe_args* a, int32_t broker,
                                             uint64_t* keys, int32_t* replicas, int32_t* slots, int32_t capacity,
                                             int32_t* count) {
  return guarded([&] {
    if (!s || !a || !count || capacity < 0 || (capacity > 0 && (!keys || !replicas)))
      throw std::invalid_argument("null argument");
    const ccmi::Model& m = s->model;
    const ccmi::KeyedMirror& mir = s->engine->queueMirror();
    if (broker < 0 || broker >= m.B) throw std::invalid_argument("broker out of range");
    const std::vector<Row> v = rowsOf(m, specOf(*a), broker);
    *count = (int32_t)v.size();
    for (size_t i = 0; i < v.size() && i < (size_t)capacity; ++i) {
      keys[i] = v[i].first;
      replicas[i] = v[i].second;
      if (slots) slots[i] = mir.brokers() == m.B && mir.brokerOf(v[i].second) == broker ? mir.slotOf(v[i].second) : -1;
    }
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_queue_probe(ccmi_session* s, const ccmi_queue_probe_args* a, ccmi_queue_probe_report* out) {
  return guarded([&] {
    if (!s || !a || !out) throw std::invalid_argument("null argument");
    if (a->num_accept < 0 || a->n_tail < 0 || a->n_cands < 0) throw std::invalid_argument("negative count");
    if (a->mode < 0 || a->mode > 2) throw std::invalid_argument("unknown probe mode");
    if ((a->num_accept > 0 && !a->accept_kinds) || (a->n_tail > 0 && !a->tail) || (a->n_cands > 0 && !a->cands))
      throw std::invalid_argument("null argument");
    ccmi::Engine& e = *s->engine;
    ccmi::Model& m = s->model;
    if (e.shard.count > 1 || e.shard.fn || s->group) throw std::invalid_argument("the queue probe takes one-shard sessions only");
    const ccmi::Model::Spec spec = specOf(*a);

    // every index against the model before anything reaches the device; a broker is one entry at most
    const int hasHead = a->head >= 0 ? 1 : 0, n = hasHead + a->n_tail, N = a->n_cands;
    if (a->head < -1 || a->head >= m.B) throw std::invalid_argument("broker out of range");
    if (a->has_skip && !hasHead) throw std::invalid_argument("a continuation needs a head entry");
    std::vector<int32_t> entries;
    if (hasHead) entries.push_back(a->head);
    entries.insert(entries.end(), a->tail, a->tail + a->n_tail);
    std::vector<uint8_t> seen((size_t)m.B, 0);
    for (int b : entries) {
      if (b < 0 || b >= m.B) throw std::invalid_argument("broker out of range");
      if (seen[(size_t)b]) throw std::invalid_argument("a broker is in the queue twice");
      seen[(size_t)b] = 1;
    }
    const std::vector<int32_t> cands(a->cands, a->cands + N);
    for (int b : cands)
      if (b < 0 || b >= m.B) throw std::invalid_argument("broker out of range");

    // the program: Engine::program's, with the caller's goals for the optimizing goal and the optimized ones
    const ccmi::GoalImpl* self = e.optimizedOfKind(a->self_kind);
    if (!self) throw std::invalid_argument("the session has not optimized goal kind " + std::to_string(a->self_kind));
    std::vector<const ccmi::GoalImpl*> accept;
    for (int g = 0; g < a->num_accept; ++g) {
      const ccmi::GoalImpl* goal = e.optimizedOfKind(a->accept_kinds[g]);
      if (!goal) throw std::invalid_argument("the session has not optimized goal kind " + std::to_string(a->accept_kinds[g]));
      accept.push_back(goal);
    }
    for (const ccmi::GoalImpl* g : accept)
      if (g->terminal || ccmi::isIntraGoalKind(g->kind)) throw std::invalid_argument("not a goal a queue scan evaluates");
    if (self->terminal || ccmi::isIntraGoalKind(self->kind)) throw std::invalid_argument("not a goal a queue scan evaluates");
    const ccmi::DevProgram prog = e.programOf(*self, accept.data(), accept.size(), ccmi::DA_MOVE);

    *out = ccmi_queue_probe_report{};
    out->dev_entry = out->dev_replica = out->dev_column = -1;
    out->ref_entry = out->ref_replica = out->ref_column = -1;
    out->win_slot = out->lowest_accepted_slot = out->highest_accepted_slot = -1;

    // ---- the host loop
    std::vector<Row> head;
    int masked = 0;
    if (hasHead) {
      head = rowsOf(m, spec, a->head);
      if (a->has_skip)
        while (masked < (int)head.size() && head[(size_t)masked].first <= a->skip_key) ++masked;
    }
    out->head_masked = masked;
    // (the view Engine::acceptance builds: every optimized goal's allowed brokers by slot)
    std::vector<const std::vector<uint8_t>*> allowedBySlot(ccmi::kMaxSlots, nullptr);
    for (auto& g : e.optimized) allowedBySlot[(size_t)g->dg.allowedSlot] = &g->allowed;
    const ccmi::HostView view{m, allowedBySlot, e.topicUpper, e.topicLower, e.brokerSetOf, e.replicaSetOf, e.minLeadOf,
                              e.topicLeadLim};
    auto firstAccepted = [&](int r) {  // row r's first column that is not blocked and that the program accepts, or -1
      for (int j = 0; j < N; ++j)
        if (!e.blocked(prog, r, cands[(size_t)j]) && ccmi::moveCandidateAccepted(prog, view, r, cands[(size_t)j])) return j;
      return -1;
    };
    std::vector<int32_t> accepted;  // the rows of the winner's entry (after the mask) with an accepted column
    for (int i = 0; i < n && out->ref_entry < 0 && N > 0; ++i) {
      const int first = i < hasHead ? masked : 0;
      const std::vector<Row> all = i < hasHead ? head : rowsOf(m, spec, entries[(size_t)i]);
      for (size_t k = (size_t)first; k < all.size(); ++k) {
        const int j = firstAccepted(all[k].second);
        if (j < 0) continue;
        if (out->ref_entry < 0) {  // the first one in key order wins; the later rows only count
          out->ref_entry = i;
          out->ref_replica = all[k].second;
          out->ref_column = j;
          out->win_key = all[k].first;
          out->win_rank = (int32_t)k;
          out->win_len = (int32_t)all.size();
        }
        accepted.push_back(all[k].second);
      }
      out->accepted_rows = (int32_t)accepted.size();
    }

    // ---- the device's answer: Engine::queueScan's call (the sync, the row flush, the scan and its decoding)
    if (a->mode == 2) return CCMI_OK;
    if (n > 0 && N > 0) {
      const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
      const int64_t served0 = s->device->perf.serverScans;
      const ccmi::Engine::QueueHit hit =
          e.queueScanProg(prog, spec, a->head, masked, a->skip_key, a->tail, a->n_tail, cands);
      out->served = s->device->perf.serverScans > served0 ? 1 : 0;
      out->n_active = out->served ? s->device->queueLastActive : 0;
      if (hit.key >= 0) {
        out->dev_entry = hit.entry;
        out->dev_replica = hit.r;
        out->dev_column = (int32_t)(hit.key % N);
      }
    }
    const bool keyed = n > 0 && N > 0 && e.queueKeyedCurrent();
    out->keyed = keyed ? 1 : 0;
    if (!keyed) return CCMI_OK;
    const ccmi::KeyedMirror& mir = e.queueMirror();
    out->stride = mir.stride();

    // ---- coverage facts: where the accepted rows of the winner's entry sit in its block
    if (out->ref_entry >= 0) {
      for (int32_t r : accepted) {
        const int slot = mir.slotOf(r);
        if (out->lowest_accepted_slot < 0 || slot < out->lowest_accepted_slot) out->lowest_accepted_slot = slot;
        out->highest_accepted_slot = std::max(out->highest_accepted_slot, slot);
      }
      out->win_slot = mir.slotOf(out->ref_replica);
    }

    // ---- the audit: per broker the model's rows against the mirror's and the device table's
    if (a->mode == 1) return CCMI_OK;
    const bool table = s->device->hasKeyedTable() && s->device->kqStride() == mir.stride();
    out->audited = 1 | (table ? 2 : 0);
    std::vector<TableRow> want, got;
    std::vector<ccmi::KeyedRow> block;
    for (int b = 0; b < m.B; ++b) {
      want.clear();
      for (const Row& row : rowsOf(m, spec, b)) {
        const int p = m.rPart[(size_t)row.second];
        want.push_back({row.first, row.second, p, m.pTopic[(size_t)p]});
      }
      bool same = mir.len(b) == (int)want.size();
      got.clear();
      for (int q = 0; same && q < mir.len(b); ++q) {
        const int r = mir.rep(b, q);
        if (r < 0 || r >= m.R || mir.slotOf(r) != q || mir.brokerOf(r) != b) {
          same = false;
          break;
        }
        const int p = m.rPart[(size_t)r];
        got.push_back({mir.key(b, q), r, p, m.pTopic[(size_t)p]});
      }
      std::sort(got.begin(), got.end());
      same = same && got == want;
      if (same && table) {
        same = s->device->kqLenAt(b) == (int32_t)want.size();
        got.clear();
        block.resize(want.size());
        if (same) s->device->kqReadBlock(b, (int)want.size(), block.data());
        for (int q = 0; same && q < (int)want.size(); ++q) {
          const ccmi::KeyedRow& row = block[(size_t)q];
          got.push_back({row.key, row.r, row.p, row.topic});
          same = row.r == mir.rep(b, q);  // the slot the mirror says
        }
        std::sort(got.begin(), got.end());
        same = same && got == want;
      }
      out->audit += same ? 0 : 1;
    }
    return CCMI_OK;
  });
}
