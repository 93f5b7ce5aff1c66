// ccmi_proposal_diff (additive at ABI v13): the ExecutionProposals of the session's current model against its initial
// placement and their movement statistics, diffed, compacted and summed on the device from the resident tables
// (Device::proposalDiff, kernels/proposal_diff.hip). A translation unit of its own: it holds the only caller of that
// launcher, which the test emulation of Device does not have. No per-partition work happens here: the host sends the
// initial placement once and, on a model with disks, the current disk of every slot (Model::rDisk is not resident).
#include <stdexcept>
#include <vector>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/threadpin.h"

static_assert(sizeof(ccmi_proposal_record) == 160 && sizeof(ccmi_proposal_summary) == 64, "ccmi.h struct sizes");

extern "C" ccmi_status ccmi_proposal_diff(ccmi_session* s, ccmi_proposal_record* records, int64_t capacity,
                                          int64_t* num_records, ccmi_proposal_summary* summary) {
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (!num_records) throw std::invalid_argument("null num_records");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    ccmi::Model& m = s->model;
    if (!records && capacity > 0 && m.P > 0) throw std::invalid_argument("null records");
    *num_records = 0;
    if (summary) *summary = ccmi_proposal_summary{};
    if (m.P < 1) return CCMI_OK;
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
    dev.proposalDiff(disks ? curDisks.data() : nullptr, records, capacity, num_records, summary);
    return CCMI_OK;
  });
}
