// ccmi_execution_plan (additive at ABI v13): what ExecutionTaskPlanner.addExecutionProposals builds from the proposals of
// the session's current model: the tasks, their execution ids, the per-broker task sets in strategy order and the broker
// order, classified, numbered, sorted and gathered on the device from the resident tables (Device::executionPlan,
// kernels/execution_plan.hip). A translation unit of its own: it holds the only caller of that launcher, which the test
// emulation of Device does not have. No per-partition work happens here: the arguments are checked before any launch,
// the chain is cut to the strategies that can decide, and the caller's two arrays go to the device as given.
#include <stdexcept>
#include <vector>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/threadpin.h"

static_assert(sizeof(ccmi_execution_plan_query) == 64 && sizeof(ccmi_plan_task) == 16 && sizeof(ccmi_plan_summary) == 64,
              "ccmi.h struct sizes");

extern "C" ccmi_status ccmi_execution_plan(ccmi_session* s, const ccmi_execution_plan_query* q,
                                           ccmi_plan_summary* summary, ccmi_plan_task* tasks, int64_t task_capacity,
                                           int64_t* inter_offsets, int32_t* inter_entries, int64_t inter_capacity,
                                           int32_t* broker_order, int64_t* intra_offsets, int32_t* intra_entries,
                                           int64_t intra_capacity, int32_t* leader_tasks, int64_t leader_capacity) {
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (!q || !summary || !inter_offsets || !intra_offsets) throw std::invalid_argument("null argument");
    if (task_capacity < 0 || inter_capacity < 0 || intra_capacity < 0 || leader_capacity < 0)
      throw std::invalid_argument("capacity < 0");
    if (q->num_strategies < 0 || q->num_strategies > 4) throw std::invalid_argument("num_strategies outside 0..4");
    bool named[CCMI_NUM_STRATEGIES] = {};
    for (int i = 0; i < q->num_strategies; ++i) {
      const int32_t st = q->strategies[i];
      if (st < 0 || st >= CCMI_NUM_STRATEGIES) throw std::invalid_argument("unknown strategy");
      if (named[st]) throw std::invalid_argument("a strategy named twice");
      named[st] = true;
    }
    if ((!tasks && task_capacity > 0) || (!inter_entries && inter_capacity > 0) ||
        (!intra_entries && intra_capacity > 0) || (!leader_tasks && leader_capacity > 0))
      throw std::invalid_argument("a NULL array with a capacity above 0");
    if (!broker_order && inter_capacity > 0) throw std::invalid_argument("null broker_order");
    ccmi::Model& m = s->model;
    *summary = ccmi_plan_summary{};
    for (int64_t b = 0; b <= m.B; ++b) inter_offsets[b] = intra_offsets[b] = 0;
    if (m.P < 1 || m.B < 1 || m.R < 1) {
      if (broker_order)
        for (int64_t b = 0; b < m.B; ++b) broker_order[b] = -1;
      return CCMI_OK;
    }
    // the chain as the kernels apply it: the strategies before BASE (BASE is appended when absent and nothing after it
    // decides), and one size strategy at most: after PRIORITIZE_LARGE, PRIORITIZE_SMALL only sees equal sizes
    ccmi::EpQuery dq{};
    bool size = false;
    for (int i = 0; i < q->num_strategies && q->strategies[i] != CCMI_STRATEGY_BASE; ++i) {
      const int32_t st = q->strategies[i];
      const bool isSize = st == CCMI_STRATEGY_PRIORITIZE_LARGE || st == CCMI_STRATEGY_PRIORITIZE_SMALL;
      if (isSize && size) continue;
      size = size || isSize;
      dq.strat[dq.n++] = st;
    }
    ccmi::Device& dev = *s->device;
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    const bool disks = m.D > 0;
    if (!dev.initialPlacementUploaded())
      dev.uploadInitialPlacement(s->initDist.data(), s->initLeaders.data(), disks ? s->initDisks.data() : nullptr,
                                 disks ? s->initLeaderDisks.data() : nullptr);
    m.flushToDevice();    // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    m.flushChainLoads();  // and the slot order and leaders those moves changed
    std::vector<int32_t> curDisks;
    if (disks) curDisks = m.replicaDisks();
    dev.executionPlan(dq, disks ? curDisks.data() : nullptr, q->proposal_rank, q->partition_state, summary, tasks,
                      task_capacity, inter_offsets, inter_entries, inter_capacity, broker_order, intra_offsets,
                      intra_entries, intra_capacity, leader_tasks, leader_capacity);
    return CCMI_OK;
  });
}
