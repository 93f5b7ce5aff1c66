// ccmi_partition_load (additive at ABI v13): the partition load response of the session's current model, keyed, sorted
// and gathered on the device from the resident tables (Device::partitionLoad, kernels/partition_load.hip). A
// translation unit of its own: it holds the only caller of that launcher, which the test emulation of Device does not
// have. No per-partition work happens here: the host sends the static partition numbers once and the query's arrays as
// given.
#include <algorithm>
#include <stdexcept>

#include "ccmi.h"
#include "ccmi_session.h"
#include "engine/threadpin.h"

static_assert(sizeof(ccmi_partition_load_query) == 64 && sizeof(ccmi_partition_load_record) == 80,
              "ccmi.h struct sizes");

extern "C" ccmi_status ccmi_partition_load(ccmi_session* s, const ccmi_partition_load_query* q,
                                           ccmi_partition_load_record* records, int64_t* num_records,
                                           int64_t* num_selected) {
  return guarded([&] {
    if (!s) throw std::invalid_argument("null session");
    if (!q || !num_records) throw std::invalid_argument("null argument");
    if ((q->want_max_load != 0 && q->want_max_load != 1) || (q->want_avg_load != 0 && q->want_avg_load != 1))
      throw std::invalid_argument("want_max_load and want_avg_load are 0 or 1");
    if (q->want_max_load && q->want_avg_load)  // Load.java:82-84
      throw std::invalid_argument("Attempt to request expected utilization with both max and avg load.");
    if (q->resource < 0 || q->resource >= CCMI_NUM_RESOURCES) throw std::invalid_argument("resource outside [0, 4)");
    if (q->entries < 0) throw std::invalid_argument("entries < 0");
    ccmi::Model& m = s->model;
    if (!records && q->entries > 0 && m.P > 0) throw std::invalid_argument("null records");
    *num_records = 0;
    if (num_selected) *num_selected = 0;
    if (m.P < 1 || q->partition_lower > q->partition_upper) return CCMI_OK;
    ccmi::Device& dev = *s->device;
    const ccmi::ThreadPin pin(s->deviceOrdinal);  // restored when the call returns
    if (!dev.partitionNumbersUploaded()) dev.uploadPartitionNumbers(m.pNumber.data());
    m.flushToDevice();    // the rows the host changed since the last launch (ccmi_session_apply, a goal's moves)
    m.flushChainLoads();  // and the Java loads, slot order and leaders those moves changed
    ccmi::PlQuery dq;
    dq.resource = q->resource;
    dq.mode = q->want_max_load ? 1 : (q->want_avg_load ? 2 : 0);
    dq.entries = q->entries;
    dq.lower = q->partition_lower;
    dq.upper = q->partition_upper;
    dev.partitionLoad(dq, q->topic_selected, q->broker_selected, q->tie_rank, records, num_records, num_selected);
    return CCMI_OK;
  });
}
