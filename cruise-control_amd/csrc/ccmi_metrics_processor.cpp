// ccmi_metrics_processor_* (additive at ABI v13): CruiseControlMetricsProcessor over raw records kept on the device
// (K20, kernels/metrics_processor.hip; the arithmetic is engine/broker_load.h). The host keeps what the reference keeps
// outside the holders: the interned topic names, _maxMetricTimestamp, the brokers seen and _cachedNumCoresByBroker.
// Per process call it turns the Cluster into per-partition columns (leader slot, dot-handled topic, replica count
// above one), which is a pass over P names and ids, and for the few nodes the kernels flag it replays the HashMap
// with jsem.h's JHashSet. A translation unit of its own: the test emulation of Device has none of this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "ccmi.h"
#include "ccmi_aggregator_impl.h"
#include "ccmi_session.h"
#include "engine/broker_load.h"
#include "engine/devbuf.h"
#include "engine/hip_check.h"
#include "engine/jsem.h"
#include "engine/metrics_processor.h"

static_assert(sizeof(ccmi_metrics_processor_config) == 32 && sizeof(ccmi_raw_metrics) == 72 &&
                  sizeof(ccmi_cluster_nodes) == 24 && sizeof(ccmi_processed_samples) == 120,
              "ccmi.h struct sizes");

namespace {
using ccmi::Carver;
using ccmi::hipCheck;
namespace bl = ccmi::bl;

struct RecordColumns {
  double* value = nullptr;
  long long* time = nullptr;
  int32_t *broker = nullptr, *topic = nullptr, *partition = nullptr;
  uint8_t* type = nullptr;
  void layout(Carver& c, size_t cap) {
    c.take(value, cap);
    c.take(time, cap);
    c.take(broker, cap);
    c.take(topic, cap);
    c.take(partition, cap);
    c.take(type, cap);
  }
};

int bitsFor(uint32_t v) {  // bits needed to hold v
  int b = 1;
  while (b < 32 && (v >> b)) b++;
  return b;
}

std::string replaceDots(const char* s) {
  std::string r(s);
  std::replace(r.begin(), r.end(), '.', '_');
  return r;
}
}  // namespace

struct ccmi_metrics_processor {
  int device = 0;
  hipStream_t st = nullptr;
  bl::CpuWeights w{0.7, 0.15, 0.15};
  std::unordered_map<std::string, int32_t> topicIds;
  std::vector<std::string> topicNames;
  std::vector<int32_t> topicHash;  // String.hashCode
  std::unordered_set<int32_t> brokersSeen;
  std::unordered_map<int32_t, double> cachedCores;
  long long maxTs = -1;
  bool processed = false;
  long long n = 0, cap = 0;
  ccmi::DevBuf rec, work, lists, outBuf;
  RecordColumns R;

  ~ccmi_metrics_processor() {
    if (st) (void)hipStreamDestroy(st);
  }
  void sync() { hipCheck(hipStreamSynchronize(st), "hipStreamSynchronize (metrics processor)"); }
  void up(void* dst, const void* src, size_t bytes) {
    if (bytes) hipCheck(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync (metrics processor, up)");
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (bytes) hipCheck(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (metrics processor, down)");
  }
  void zero(void* p, size_t bytes) {
    if (bytes) hipCheck(hipMemsetAsync(p, 0, bytes, st), "hipMemsetAsync (metrics processor)");
  }
  // room for `need` records, the buffered ones kept: the buffer grows by doubling
  void reserve(long long need) {
    if (need <= cap) return;
    long long nc = std::max<long long>(cap * 2, 4096);
    while (nc < need) nc *= 2;
    ccmi::DevBuf fresh;
    RecordColumns F;
    ccmi::carve(fresh, [&](Carver& c) { F.layout(c, (size_t)nc); });
    auto keep = [&](void* d, const void* s, size_t bytes) {
      if (bytes) hipCheck(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync (metrics processor, grow)");
    };
    const size_t k = (size_t)n;
    keep(F.value, R.value, k * 8);
    keep(F.time, R.time, k * 8);
    keep(F.broker, R.broker, k * 4);
    keep(F.topic, R.topic, k * 4);
    keep(F.partition, R.partition, k * 4);
    keep(F.type, R.type, k);
    sync();
    rec = std::move(fresh);
    R = F;
    cap = nc;
  }
};

namespace {

// what orders equal hashes inside a tree bin when a flagged node's keys are replayed through JHashSet (ids are insertion ranks)
struct TopicOps {
  const std::vector<const std::string*>* names;
  int cmp(int a, int b) const {  // String.compareTo on the names' bytes
    const int c = (*names)[a]->compare(*(*names)[b]);
    return c < 0 ? -1 : c > 0 ? 1 : 0;
  }
};
struct RankOps {
  int cmp(int a, int b) const { return a < b ? -1 : a > b ? 1 : 0; }  // ids are insertion ranks
};

void checkOut(const ccmi_processed_samples& o) {
  if (o.partition_capacity < 0 || o.broker_capacity < 0) throw std::invalid_argument("capacity < 0");
  if (o.partition_capacity > 0 && (!o.partition_entity || !o.partition_values))
    throw std::invalid_argument("null partition arrays with capacity > 0");
  if (o.broker_capacity > 0 && (!o.broker_node || !o.broker_values || !o.broker_version))
    throw std::invalid_argument("null broker arrays with capacity > 0");
}

}  // namespace

extern "C" ccmi_status ccmi_metrics_processor_create(int32_t device_ordinal, const ccmi_metrics_processor_config* config,
                                                     ccmi_metrics_processor** out) {
  return guarded([&] {
    if (!out) throw std::invalid_argument("null argument");
    *out = nullptr;
    if (config) {
      for (double v : {config->cpu_weight_of_leader_bytes_in_rate, config->cpu_weight_of_leader_bytes_out_rate,
                       config->cpu_weight_of_follower_bytes_in_rate})
        if (!(v >= 0.0)) throw std::invalid_argument("a CPU weight is negative or NaN");
    }
    int count = 0;
    hipCheck(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (device_ordinal < 0 || device_ordinal >= count) throw std::invalid_argument("device ordinal out of range");
    const ccmi::DeviceGuard dg(device_ordinal);
    std::unique_ptr<ccmi_metrics_processor> p(new ccmi_metrics_processor);
    p->device = device_ordinal;
    if (config)
      p->w = bl::CpuWeights{config->cpu_weight_of_leader_bytes_in_rate, config->cpu_weight_of_leader_bytes_out_rate,
                            config->cpu_weight_of_follower_bytes_in_rate};
    hipCheck(hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking), "hipStreamCreate (metrics processor)");
    *out = p.release();
    return CCMI_OK;
  });
}

extern "C" void ccmi_metrics_processor_destroy(ccmi_metrics_processor* p) {
  if (!p) return;
  try {
    const ccmi::DeviceGuard dg(p->device);
    delete p;
  } catch (...) {
  }
}

extern "C" ccmi_status ccmi_metrics_processor_add_metrics(ccmi_metrics_processor* p, const ccmi_raw_metrics* batch) {
  return guarded([&] {
    if (!p || !batch) throw std::invalid_argument("null argument");
    const ccmi_raw_metrics& b = *batch;
    if (b.n < 0 || b.num_topics < 0) throw std::invalid_argument("negative count");
    if (b.n > 0 && (!b.type || !b.broker_id || !b.time_ms || !b.value || !b.topic || !b.partition))
      throw std::invalid_argument("null record column");
    if (b.num_topics > 0 && !b.topic_names) throw std::invalid_argument("null topic_names");
    if (p->processed) throw ccmi::StateError("add_metrics after process: call clear first");
    if (p->n + b.n >= (1ll << 31)) throw std::invalid_argument("more than 2^31 - 1 buffered records");
    {
      std::unordered_set<std::string> seen;
      for (int t = 0; t < b.num_topics; ++t) {
        if (!b.topic_names[t]) throw std::invalid_argument("null topic name");
        if (!seen.insert(b.topic_names[t]).second)
          throw std::invalid_argument(std::string("duplicate topic name in the batch: ") + b.topic_names[t]);
      }
    }
    for (int64_t i = 0; i < b.n; ++i) {
      const int type = b.type[i];
      if (type >= bl::kNumRawTypes) throw std::invalid_argument("raw metric type above 62 at record " + std::to_string(i));
      const int scope = bl::scopeOf(type);
      const bool topicOk = scope == bl::kScopeBroker ? b.topic[i] == -1 : (b.topic[i] >= 0 && b.topic[i] < b.num_topics);
      const bool partOk = scope == bl::kScopePartition ? (b.partition[i] >= 0 && b.partition[i] <= bl::kMaxPartition)
                                                       : b.partition[i] == -1;
      if (!topicOk) throw std::invalid_argument("topic index does not fit the type's scope at record " + std::to_string(i));
      if (!partOk) throw std::invalid_argument("partition does not fit the type's scope at record " + std::to_string(i));
      if (b.time_ms[i] < 0) throw std::invalid_argument("negative time at record " + std::to_string(i));
    }
    size_t fresh = 0;
    for (int t = 0; t < b.num_topics; ++t) fresh += p->topicIds.count(b.topic_names[t]) ? 0 : 1;
    if (p->topicNames.size() + fresh > (size_t)bl::kMaxTopics) throw std::invalid_argument("more than 4194302 topics");
    const ccmi::DeviceGuard dg(p->device);
    p->reserve(p->n + b.n);
    std::vector<int32_t> remap((size_t)b.num_topics), topics((size_t)b.n);
    for (int t = 0; t < b.num_topics; ++t) {
      auto it = p->topicIds.find(b.topic_names[t]);
      if (it == p->topicIds.end()) {
        it = p->topicIds.emplace(b.topic_names[t], (int32_t)p->topicNames.size()).first;
        p->topicNames.push_back(b.topic_names[t]);
        p->topicHash.push_back(ccmi::jStringHash(b.topic_names[t]));
      }
      remap[t] = it->second;
    }
    for (int64_t i = 0; i < b.n; ++i) {
      topics[i] = b.topic[i] < 0 ? -1 : remap[b.topic[i]];
      p->maxTs = std::max<long long>(p->maxTs, b.time_ms[i]);
      p->brokersSeen.insert(b.broker_id[i]);
    }
    const size_t at = (size_t)p->n, k = (size_t)b.n;
    p->up(p->R.value + at, b.value, k * 8);
    p->up(p->R.time + at, b.time_ms, k * 8);
    p->up(p->R.broker + at, b.broker_id, k * 4);
    p->up(p->R.topic + at, topics.data(), k * 4);
    p->up(p->R.partition + at, b.partition, k * 4);
    p->up(p->R.type + at, b.type, k);
    p->sync();
    p->n += b.n;
    return CCMI_OK;
  });
}

namespace {

void checkAggregator(const ccmi_metrics_processor& p, const ccmi_aggregator* a, int E, int M, const char* which) {
  if (!a) return;
  if (a->cfg.num_entities != E || a->cfg.num_metrics != M)
    throw std::invalid_argument(std::string("the ") + which + " aggregator needs E = " + std::to_string(E) + " and M = " +
                                std::to_string(M));
  if (a->device != p.device) throw std::invalid_argument(std::string("the ") + which + " aggregator is on another device");
}

// ccmi_aggregator_add_samples(entity, time, values) over k rows the kernels left on the device, every sample at `time`
void feedAggregator(ccmi_aggregator& a, const int32_t* dEntity, const double* dValues, int64_t k, int64_t time) {
  if (k <= 0) return;
  const ccmi::AggAddPlan plan = ccmi::aggPlanAddSamples(a, nullptr, time, k);
  int64_t* dTime = nullptr;
  ccmi::AggAddScratch scratch;
  ccmi::carve(a.batch, [&](Carver& c) {
    c.take(dTime, (size_t)k);
    scratch.layout(c, (size_t)k, (size_t)a.cfg.num_entities, plan.events.size());
  });
  const std::vector<int64_t> times((size_t)k, time);
  a.up(dTime, times.data(), sizeof(int64_t) * (size_t)k);
  ccmi::aggAddSamplesOnDevice(a, plan, scratch, dEntity, dTime, dValues, k);  // synchronises: `times` may go
}

ccmi_status processImpl(ccmi_metrics_processor* p, const ccmi_partition_topology* cluster,
                        const ccmi_cluster_nodes* nodes, const uint8_t* interested, int32_t sampling_mode,
                        ccmi_aggregator* partitionAgg, ccmi_aggregator* brokerAgg, bool into,
                        ccmi_processed_samples* out) {
  return guarded([&] {
    if (!p || !cluster || !nodes || !out) throw std::invalid_argument("null argument");
    const int P = cluster->num_partitions, N = nodes->num_nodes, CT = cluster->num_topics;
    if (P < 0 || N < 0 || CT < 0) throw std::invalid_argument("negative count");
    if (N > bl::kMaxSlots) throw std::invalid_argument("more than 262143 nodes");
    if (CT > bl::kMaxTopics) throw std::invalid_argument("more than 4194302 topics");
    if (N > 0 && (!nodes->broker_id || !nodes->num_cores)) throw std::invalid_argument("null node column");
    if (P > 0 && (!cluster->partition_topic || !cluster->partition_number || !cluster->replica_offset ||
                  !cluster->leader_broker_id || !cluster->topic_names))
      throw std::invalid_argument("null topology column");
    if (sampling_mode < CCMI_SAMPLING_ALL || sampling_mode > CCMI_SAMPLING_ONGOING_EXECUTION)
      throw std::invalid_argument("unknown sampling mode");
    if (into) {
      checkAggregator(*p, partitionAgg, P, bl::kPartitionMetrics, "partition");
      checkAggregator(*p, brokerAgg, N, bl::kBrokerMetrics, "broker");
    } else {
      checkOut(*out);
    }
    std::unordered_map<int32_t, int32_t> slotOf;
    for (int s = 0; s < N; ++s)
      if (!slotOf.emplace(nodes->broker_id[s], s).second)
        throw std::invalid_argument("duplicate node id " + std::to_string(nodes->broker_id[s]));
    for (int q = 0; q < P; ++q)
      if (cluster->partition_topic[q] < 0 || cluster->partition_topic[q] >= CT)
        throw std::invalid_argument("partition_topic out of range at partition " + std::to_string(q));
    if (p->processed) throw ccmi::StateError("process after process: call clear first");
    const bool wantPartitions = sampling_mode != CCMI_SAMPLING_BROKER_METRICS_ONLY;
    const bool wantBrokers = sampling_mode != CCMI_SAMPLING_PARTITION_METRICS_ONLY;

    // updateCachedNumCoresByBroker
    for (int32_t b : p->brokersSeen) {
      if (p->cachedCores.count(b)) continue;
      const auto it = slotOf.find(b);
      if (it == slotOf.end()) continue;
      const double c = nodes->num_cores[it->second];
      if (c == c) p->cachedCores.emplace(b, c);
    }
    // the Cluster as columns
    std::vector<int32_t> nodeIdSorted(N), nodeSlotSorted(N);
    {
      std::vector<std::pair<int32_t, int32_t>> v(N);
      for (int s = 0; s < N; ++s) v[s] = {nodes->broker_id[s], s};
      std::sort(v.begin(), v.end());
      for (int s = 0; s < N; ++s) {
        nodeIdSorted[s] = v[s].first;
        nodeSlotSorted[s] = v[s].second;
      }
    }
    std::vector<double> cores(N);
    for (int s = 0; s < N; ++s) {
      const auto it = p->cachedCores.find(nodes->broker_id[s]);
      cores[s] = it == p->cachedCores.end() ? std::nan("") : it->second;
    }
    std::vector<int32_t> hidOfTopic(CT), metricOfTopic(CT);
    {
      std::unordered_map<std::string, int32_t> handled;
      for (int t = 0; t < CT; ++t) {
        if (!cluster->topic_names[t]) throw std::invalid_argument("null topic name");
        const std::string h = replaceDots(cluster->topic_names[t]);
        hidOfTopic[t] = handled.emplace(h, (int32_t)handled.size()).first->second;
        const auto it = p->topicIds.find(h);
        metricOfTopic[t] = it == p->topicIds.end() ? -1 : it->second;
      }
    }
    std::vector<int32_t> leaderSlot(P), metricTopic(P), hid(P);
    std::vector<uint8_t> multi(P);
    for (int q = 0; q < P; ++q) {
      const int32_t l = cluster->leader_broker_id[q];
      if (l < 0) leaderSlot[q] = -1;
      else {
        const auto it = slotOf.find(l);
        leaderSlot[q] = it == slotOf.end() ? -2 : it->second;
      }
      metricTopic[q] = metricOfTopic[cluster->partition_topic[q]];
      hid[q] = hidOfTopic[cluster->partition_topic[q]];
      multi[q] = cluster->replica_offset[q + 1] - cluster->replica_offset[q] > 1;
    }

    const ccmi::DeviceGuard dg(p->device);
    p->processed = true;
    const long long n = p->n;
    const size_t T = p->topicHash.size();
    ccmi::MpEntry *eA = nullptr, *eB = nullptr, *ledA = nullptr, *ledB = nullptr;
    uint32_t *counts = nullptr, *flags = nullptr, *blockSums = nullptr, *dropped = nullptr, *pFlags = nullptr,
             *bFlags = nullptr, *skippedByNode = nullptr;
    double *hval = nullptr, *dCores = nullptr, *pStaged = nullptr, *bStaged = nullptr;
    int32_t *dNodeId = nullptr, *dNodeSlot = nullptr, *dTopicHash = nullptr, *dLeaderSlot = nullptr,
            *dMetricTopic = nullptr, *dHid = nullptr, *dTopic = nullptr, *dNumber = nullptr;
    uint8_t *dMulti = nullptr, *dInterested = nullptr, *flaggedT = nullptr, *flaggedP = nullptr, *pSkip = nullptr,
            *bSkip = nullptr;
    bl::Prepared* prepared = nullptr;
    const long long big = std::max<long long>({n, (long long)P, (long long)N});
    ccmi::carve(p->work, [&](Carver& c) {
      c.take(eA, (size_t)n);
      c.take(eB, (size_t)n);
      c.take(ledA, (size_t)P);
      c.take(ledB, (size_t)P);
      c.take(counts, ccmi::mpSortCountWords(big));
      c.take(flags, (size_t)n + 1);
      c.take(blockSums, ccmi::mpScanBlocks(big) + 1);
      c.take(dropped, 1);
      c.take(hval, (size_t)n);
      c.take(dCores, (size_t)N);
      c.take(dNodeId, (size_t)N);
      c.take(dNodeSlot, (size_t)N);
      c.take(dTopicHash, T);
      c.take(dLeaderSlot, (size_t)P);
      c.take(dMetricTopic, (size_t)P);
      c.take(dHid, (size_t)P);
      c.take(dTopic, (size_t)P);
      c.take(dNumber, (size_t)P);
      c.take(dMulti, (size_t)P);
      c.take(dInterested, (size_t)P);
      c.take(flaggedT, (size_t)N);
      c.take(flaggedP, (size_t)N);
      c.take(prepared, (size_t)N);
      c.take(pSkip, (size_t)P);
      c.take(pFlags, (size_t)P + 1);
      c.take(pStaged, (size_t)P * bl::kPartitionMetrics);
      c.take(skippedByNode, (size_t)N + 1);
      c.take(bSkip, (size_t)N);
      c.take(bFlags, (size_t)N + 1);
      c.take(bStaged, (size_t)N * bl::kBrokerMetrics);
    });
    p->up(dNodeId, nodeIdSorted.data(), sizeof(int32_t) * (size_t)N);
    p->up(dNodeSlot, nodeSlotSorted.data(), sizeof(int32_t) * (size_t)N);
    p->up(dCores, cores.data(), sizeof(double) * (size_t)N);
    p->up(dTopicHash, p->topicHash.data(), sizeof(int32_t) * T);
    p->up(dLeaderSlot, leaderSlot.data(), sizeof(int32_t) * (size_t)P);
    p->up(dMetricTopic, metricTopic.data(), sizeof(int32_t) * (size_t)P);
    p->up(dHid, hid.data(), sizeof(int32_t) * (size_t)P);
    p->up(dTopic, cluster->partition_topic, sizeof(int32_t) * (size_t)P);
    p->up(dNumber, cluster->partition_number, sizeof(int32_t) * (size_t)P);
    p->up(dMulti, multi.data(), (size_t)P);
    if (interested) p->up(dInterested, interested, (size_t)P);
    p->zero(dropped, sizeof(uint32_t));
    p->zero(flaggedT, (size_t)N);
    p->zero(flaggedP, (size_t)N);
    p->zero(skippedByNode, sizeof(uint32_t) * ((size_t)N + 1));
    p->zero(flags, sizeof(uint32_t) * ((size_t)n + 1));

    const ccmi::MpRecords R{p->R.type, p->R.broker, p->R.time, p->R.value, p->R.topic, p->R.partition, n};
    const ccmi::MpCluster C{dLeaderSlot, dMetricTopic, dHid, dTopic, dNumber, dMulti, interested ? dInterested : nullptr, P};
    ccmi::mpLaunchKeys(R, dNodeId, dNodeSlot, N, eA, dropped, p->st);
    const ccmi::MpEntry* S = ccmi::mpLaunchSort(eA, eB, n, bl::kSlotShift + bitsFor((uint32_t)N), counts, p->st);
    ccmi::mpLaunchReduce(S, n, R, N, hval, p->st);
    ccmi::mpLaunchFlagPe(S, n, N, flags, p->st);
    ccmi::mpLaunchScan(flags, n, blockSums, p->st);
    ccmi::mpLaunchLedKeys(C, N, ledA, p->st);
    const ccmi::MpEntry* led = ccmi::mpLaunchSort(ledA, ledB, P, ccmi::kLedSlotShift + bitsFor((uint32_t)N), counts, p->st);
    hipCheck(hipGetLastError(), "metrics processor sort launch");
    uint32_t nPe = 0, nDropped = 0;
    p->down(&nPe, flags + n, sizeof(nPe));
    p->down(&nDropped, dropped, sizeof(nDropped));
    p->sync();

    ccmi::MpKeyList pe{}, te{};
    uint32_t* teFlags = nullptr;
    unsigned long long* teKey = nullptr;
    auto layoutList = [&](Carver& c, ccmi::MpKeyList& l, size_t k) {
      c.take(l.slot, k);
      c.take(l.hash, k);
      c.take(l.arr, k);
      c.take(l.ref, k);
      c.take(l.order, k);
    };
    ccmi::carve(p->lists, [&](Carver& c) {
      layoutList(c, pe, nPe);
      layoutList(c, te, nPe);
      c.take(teFlags, (size_t)nPe + 1);
      c.take(teKey, nPe);
    });
    pe.count = nPe;
    ccmi::mpLaunchGatherPe(S, n, flags, dTopicHash, pe, p->st);
    p->zero(teFlags, sizeof(uint32_t) * ((size_t)nPe + 1));
    ccmi::mpLaunchFlagTe(S, pe, teFlags, p->st);
    ccmi::mpLaunchScan(teFlags, nPe, blockSums, p->st);
    uint32_t nTe = 0;
    p->down(&nTe, teFlags + nPe, sizeof(nTe));
    p->sync();
    te.count = nTe;
    ccmi::mpLaunchGatherTe(S, pe, teFlags, dTopicHash, te, teKey, p->st);
    ccmi::mpLaunchHashOrder(pe, flaggedP, p->st);
    ccmi::mpLaunchHashOrder(te, flaggedT, p->st);
    hipCheck(hipGetLastError(), "metrics processor hash order launch");
    std::vector<uint8_t> fT(N), fP(N);
    p->down(fT.data(), flaggedT, (size_t)N);
    p->down(fP.data(), flaggedP, (size_t)N);
    p->sync();
    int fallback = 0;
    bool anyT = false, anyP = false;
    for (int s = 0; s < N; ++s) {
      fallback += (fT[s] | fP[s]) ? 1 : 0;
      anyT |= fT[s] != 0;
      anyP |= fP[s] != 0;
    }
    // the flagged nodes' orders from the HashMap emulation
    auto redo = [&](const ccmi::MpKeyList& l, const std::vector<uint8_t>& flagged, bool isTopics) {
      const size_t k = l.count;
      std::vector<uint32_t> slot(k), arr(k), ref(k), order(k);
      std::vector<int32_t> hash(k);
      p->down(slot.data(), l.slot, 4 * k);
      p->down(arr.data(), l.arr, 4 * k);
      p->down(ref.data(), l.ref, 4 * k);
      p->down(hash.data(), l.hash, 4 * k);
      p->down(order.data(), l.order, 4 * k);
      p->sync();
      for (size_t lo = 0; lo < k;) {
        size_t hi = lo;
        while (hi < k && slot[hi] == slot[lo]) hi++;
        if (flagged[slot[lo]]) {
          std::vector<uint32_t> byArrival(hi - lo);
          for (size_t i = lo; i < hi; ++i) byArrival[i - lo] = (uint32_t)i;
          std::sort(byArrival.begin(), byArrival.end(), [&](uint32_t a, uint32_t b) { return arr[a] < arr[b]; });
          std::vector<int32_t> it;
          if (isTopics) {
            std::vector<const std::string*> names(byArrival.size());
            for (size_t r = 0; r < byArrival.size(); ++r) names[r] = &p->topicNames[ref[byArrival[r]]];
            const TopicOps ops{&names};
            ccmi::JHashSet<TopicOps> set(&ops);
            for (size_t r = 0; r < byArrival.size(); ++r) set.add((int)r, hash[byArrival[r]]);
            set.order(it);
          } else {
            const RankOps ops;
            ccmi::JHashSet<RankOps> set(&ops);
            for (size_t r = 0; r < byArrival.size(); ++r) set.add((int)r, hash[byArrival[r]]);
            set.order(it);
          }
          for (size_t x = 0; x < it.size(); ++x) order[lo + x] = byArrival[(size_t)it[x]];
        }
        lo = hi;
      }
      p->up(l.order, order.data(), 4 * k);
      p->sync();  // `order` leaves scope
    };
    if (anyT) redo(te, fT, true);
    if (anyP) redo(pe, fP, false);

    const ccmi::MpSorted sorted{S, n, hval};
    ccmi::mpLaunchPrepare(sorted, pe, te, teKey, led, C, N, prepared, p->st);
    p->zero(pFlags, sizeof(uint32_t) * ((size_t)P + 1));
    p->zero(bFlags, sizeof(uint32_t) * ((size_t)N + 1));
    p->zero(pSkip, (size_t)P);
    p->zero(bSkip, (size_t)N);
    if (wantPartitions) {
      ccmi::mpLaunchPartitions(sorted, teKey, te.count, led, C, N, prepared, dCores, p->w, pSkip, pFlags, pStaged,
                               skippedByNode, p->st);
      ccmi::mpLaunchScan(pFlags, P, blockSums, p->st);
    }
    if (wantBrokers) {
      ccmi::mpLaunchBrokerRows(prepared, N, bSkip, bFlags, bStaged, p->st);
      ccmi::mpLaunchScan(bFlags, N, blockSums, p->st);
    }
    hipCheck(hipGetLastError(), "metrics processor sample launch");
    uint32_t nP = 0, nB = 0;
    if (wantPartitions) p->down(&nP, pFlags + P, sizeof(nP));
    if (wantBrokers) p->down(&nB, bFlags + N, sizeof(nB));
    p->sync();
    const long long kp = into ? nP : std::min<long long>(out->partition_capacity, nP);
    const long long kb = into ? nB : std::min<long long>(out->broker_capacity, nB);
    int32_t *oEntity = nullptr, *oNode = nullptr;
    double *oPValues = nullptr, *oBValues = nullptr;
    int8_t* oVersion = nullptr;
    ccmi::carve(p->outBuf, [&](Carver& c) {
      c.take(oEntity, (size_t)kp);
      c.take(oPValues, (size_t)kp * bl::kPartitionMetrics);
      c.take(oNode, (size_t)kb);
      c.take(oBValues, (size_t)kb * bl::kBrokerMetrics);
      c.take(oVersion, (size_t)kb);
    });
    ccmi::mpLaunchGatherRows(pFlags, P, bl::kPartitionMetrics, pStaged, kp, oEntity, oPValues, nullptr, nullptr, p->st);
    ccmi::mpLaunchGatherRows(bFlags, N, bl::kBrokerMetrics, bStaged, kb, oNode, oBValues, prepared, oVersion, p->st);
    hipCheck(hipGetLastError(), "metrics processor gather launch");
    if (!into) {
      p->down(out->partition_entity, oEntity, sizeof(int32_t) * (size_t)kp);
      p->down(out->partition_values, oPValues, sizeof(double) * (size_t)kp * bl::kPartitionMetrics);
      p->down(out->broker_node, oNode, sizeof(int32_t) * (size_t)kb);
      p->down(out->broker_values, oBValues, sizeof(double) * (size_t)kb * bl::kBrokerMetrics);
      p->down(out->broker_version, oVersion, (size_t)kb);
    }
    if (out->partition_skip) p->down(out->partition_skip, pSkip, (size_t)P);
    if (out->broker_skip) p->down(out->broker_skip, bSkip, (size_t)N);
    if (out->skipped_by_node) p->down(out->skipped_by_node, skippedByNode, sizeof(int32_t) * ((size_t)N + 1));
    p->sync();
    out->max_metric_timestamp = p->maxTs;
    out->num_partition_samples = nP;
    out->num_broker_samples = nB;
    out->num_skipped_brokers = wantBrokers ? N - (int32_t)nB : 0;
    out->num_hash_fallback_brokers = fallback;
    out->num_dropped_records = nDropped;
    if (into) {  // the rows are complete on the device (the sync above); each aggregator works on its own stream
      if (partitionAgg) feedAggregator(*partitionAgg, oEntity, oPValues, kp, p->maxTs);
      if (brokerAgg) feedAggregator(*brokerAgg, oNode, oBValues, kb, p->maxTs);
    }
    return CCMI_OK;
  });
}

}  // namespace

extern "C" ccmi_status ccmi_metrics_processor_process(ccmi_metrics_processor* p, const ccmi_partition_topology* cluster,
                                                      const ccmi_cluster_nodes* nodes, const uint8_t* interested,
                                                      int32_t sampling_mode, ccmi_processed_samples* out) {
  return processImpl(p, cluster, nodes, interested, sampling_mode, nullptr, nullptr, false, out);
}

extern "C" ccmi_status ccmi_metrics_processor_process_into(ccmi_metrics_processor* p,
                                                           const ccmi_partition_topology* cluster,
                                                           const ccmi_cluster_nodes* nodes, const uint8_t* interested,
                                                           int32_t sampling_mode, ccmi_aggregator* partition_aggregator,
                                                           ccmi_aggregator* broker_aggregator,
                                                           ccmi_processed_samples* out) {
  return processImpl(p, cluster, nodes, interested, sampling_mode, partition_aggregator, broker_aggregator, true, out);
}

extern "C" ccmi_status ccmi_metrics_processor_cached_num_cores(ccmi_metrics_processor* p, int32_t broker_id, double* out) {
  return guarded([&] {
    if (!p || !out) throw std::invalid_argument("null argument");
    const auto it = p->cachedCores.find(broker_id);
    *out = it == p->cachedCores.end() ? std::nan("") : it->second;
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_metrics_processor_clear(ccmi_metrics_processor* p) {
  return guarded([&] {
    if (!p) throw std::invalid_argument("null processor");
    p->n = 0;
    p->maxTs = -1;
    p->brokersSeen.clear();
    p->processed = false;
    return CCMI_OK;
  });
}
