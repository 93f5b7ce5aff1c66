// ccmi_sorted_replicas (additive at ABI v13): per asked broker the list a freshly initialised SortedReplicas would
// iterate on the session's current model, selected, keyed, sorted and gathered on the device from the resident tables
// (Device::sortedReplicas, kernels/sorted_replicas.hip). A translation unit of its own: it holds the only caller of
// that launcher, which the test emulation of Device does not have. No per-replica work happens here: the host sends the
// static tail ranks once, and per call the broker -> segment map and the query's topic masks as given.
#include <stdexcept>
#include <vector>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/threadpin.h"

static_assert(sizeof(ccmi_sorted_replicas_query) == 64 && sizeof(ccmi_swap_replica) == 8, "ccmi.h struct sizes");

extern "C" ccmi_status ccmi_sorted_replicas(ccmi_session* s, const ccmi_sorted_replicas_query* q,
                                            const int32_t* brokers, int64_t n, int64_t* offsets,
                                            ccmi_swap_replica* records, double* scores, int64_t capacity,
                                            int64_t* num_records, int64_t* first_invalid) {
  if (first_invalid) *first_invalid = -1;
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (!q || !offsets || !num_records) throw std::invalid_argument("null argument");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    constexpr int32_t kAllSel = CCMI_SEL_LEADERS | CCMI_SEL_FOLLOWERS | CCMI_SEL_ONLINE | CCMI_SEL_OFFLINE |
                                CCMI_SEL_IMMIGRANTS | CCMI_SEL_IMMIGRANT_OR_OFFLINE;
    if (q->select_mask & ~kAllSel) throw std::invalid_argument("unknown bits in select_mask");
    if (q->num_priorities < 0 || q->num_priorities > 2) throw std::invalid_argument("num_priorities outside 0..2");
    for (int i = 0; i < q->num_priorities; ++i)
      if (q->priorities[i] != CCMI_PRIO_OFFLINE && q->priorities[i] != CCMI_PRIO_IMMIGRANTS)
        throw std::invalid_argument("a priority is CCMI_PRIO_OFFLINE or CCMI_PRIO_IMMIGRANTS");
    if (q->num_priorities == 2 && q->priorities[0] == q->priorities[1])
      throw std::invalid_argument("a priority named twice");
    for (int32_t res : {q->score_resource, q->above_resource, q->below_resource})
      if (res < -1 || res >= CCMI_NUM_RESOURCES) throw std::invalid_argument("resource outside [-1, 4)");
    if (q->score_reverse != 0 && q->score_reverse != 1) throw std::invalid_argument("score_reverse is 0 or 1");
    ccmi::Model& m = s->model;
    if (n < 0 || n > m.B) throw std::invalid_argument("n outside [0, B]");
    if (!brokers && n != m.B) throw std::invalid_argument("brokers == NULL needs n == B");
    std::vector<int32_t> seg((size_t)m.B, -1);  // per broker, never per replica
    for (int64_t i = 0; i < n; ++i) {
      const int64_t b = brokers ? brokers[i] : i;
      if (b < 0 || b >= m.B || seg[(size_t)b] >= 0) {
        if (first_invalid) *first_invalid = i;
        throw std::invalid_argument("broker " + std::to_string(b) +
                                    (b < 0 || b >= m.B ? " out of range" : " listed twice"));
      }
      seg[(size_t)b] = (int32_t)i;
    }
    offsets[0] = 0;
    *num_records = 0;
    if (n == 0) return CCMI_OK;
    if (m.R < 1) {
      for (int64_t i = 0; i <= n; ++i) offsets[i] = 0;
      return CCMI_OK;
    }
    ccmi::Device& dev = *s->device;
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    if (!dev.sortedStaticUploaded()) dev.uploadSortedStatic(m.rStatic.data());
    m.flushToDevice();    // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    m.flushChainLoads();  // and the Java loads, slot order and leaders those moves changed
    ccmi::SrQuery dq;
    dq.selectMask = q->select_mask;
    dq.prio[0] = q->num_priorities > 0 ? q->priorities[0] : -1;
    dq.prio[1] = q->num_priorities > 1 ? q->priorities[1] : -1;
    dq.scoreRes = q->score_resource;
    dq.scoreReverse = q->score_reverse;
    dq.aboveRes = q->above_resource;
    dq.belowRes = q->below_resource;
    dq.pad = 0;
    dq.aboveLimit = q->above_limit;
    dq.belowLimit = q->below_limit;
    dev.sortedReplicas(dq, seg.data(), (int)n, q->topic_excluded, q->topic_included, offsets, records, scores, capacity,
                       num_records);
    return CCMI_OK;
  });
}
