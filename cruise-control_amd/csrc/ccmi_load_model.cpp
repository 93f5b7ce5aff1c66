// ccmi_builder_populate_from_aggregator (additive at ABI v13): the second half of LoadMonitor.clusterModel in one call.
// The aggregate's rows stay in the aggregator's device buffer; K18 (kernels/load_model.hip) checks every row's
// partition, compacts the ones MonitorUtils.populatePartitionLoad would populate and derives their replica loads
// (engine/replica_load.h); the finished columns come back in one copy and are appended to the builder. What needs
// strings stays on the host and is touched once per topic or logdir, not per partition. A translation unit of its own:
// the test emulation of Device has no aggregator and none of this.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ccmi.h"
#include "ccmi_aggregator_impl.h"
#include "ccmi_session.h"
#include "engine/aggregator.h"
#include "engine/hip_check.h"
#include "engine/model_builder.h"
#include "engine/replica_load.h"

static_assert(sizeof(ccmi_partition_topology) == 88, "ccmi.h struct sizes");
static_assert(CCMI_NUM_METRICS == ccmi::rload::kMetrics && CCMI_M_REPLICATION_BYTES_OUT == ccmi::rload::kReplicationBytesOut,
              "replica_load.h follows ccmi_metric");

namespace {

using ccmi::Carver;
using ccmi::hipCheck;

constexpr int kEvents = 7;
enum : int { kEvRows = 0, kEvUploaded, kEvClassified, kEvWrite, kEvColumns, kEvValues, kEvCopied };

struct Events {
  hipEvent_t e[kEvents] = {};
  Events() {
    for (hipEvent_t& x : e) hipCheck(hipEventCreate(&x), "hipEventCreate (load model)");
  }
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  void record(int i, hipStream_t st) { hipCheck(hipEventRecord(e[i], st), "hipEventRecord (load model)"); }
  double ms(int from, int to) {
    float t = 0.0f;
    hipCheck(hipEventElapsedTime(&t, e[from], e[to]), "hipEventElapsedTime (load model)");
    return (double)t;
  }
};

double wallMs(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Everything about the topology that needs no row: the shape against the aggregator, the index ranges, the offsets.
void checkTopology(const ccmi_partition_topology& t, int E) {
  if (t.num_partitions != E)
    throw std::invalid_argument("topology has " + std::to_string(t.num_partitions) + " partitions, the aggregator " +
                                std::to_string(E) + " entities");
  if (t.num_topics < 0 || t.num_logdirs < 0) throw std::invalid_argument("negative count in the topology");
  if (!t.topic_names || !t.partition_topic || !t.partition_number || !t.replica_offset || !t.replica_broker_id ||
      !t.leader_broker_id)
    throw std::invalid_argument("null array in the topology");
  if (t.replica_offset[0] != 0) throw std::invalid_argument("replica_offset does not start at 0");
  for (int p = 0; p < E; ++p) {
    const int64_t n = (int64_t)t.replica_offset[p + 1] - t.replica_offset[p];
    if (n < 0) throw std::invalid_argument("replica_offset decreases at partition " + std::to_string(p));
    if (n > ccmi::rload::kMaxReplicas)
      throw std::invalid_argument("partition " + std::to_string(p) + " has " + std::to_string(n) +
                                  " replicas (at most 8)");
    if (t.partition_topic[p] < 0 || t.partition_topic[p] >= t.num_topics)
      throw std::invalid_argument("topic index out of range at partition " + std::to_string(p));
  }
  for (int i = 0; i < t.num_topics; ++i)
    if (!t.topic_names[i]) throw std::invalid_argument("null topic name");
  if (t.replica_logdir) {
    const int R = t.replica_offset[E];
    for (int r = 0; r < R; ++r)
      if (t.replica_logdir[r] < -1 || t.replica_logdir[r] >= t.num_logdirs)
        throw std::invalid_argument("logdir index out of range at replica " + std::to_string(r));
    if (t.num_logdirs > 0 && !t.logdir_names) throw std::invalid_argument("null logdir_names");
    for (int i = 0; i < t.num_logdirs; ++i)
      if (!t.logdir_names[i]) throw std::invalid_argument("null logdir name");
  }
}

// The complaint of ccmi_builder_populate_partition about partition e, in its words; returns when it has none.
void complainAbout(const ccmi_model_builder& b, const ccmi_partition_topology& t, int e) {
  const int32_t* ids = t.replica_broker_id + t.replica_offset[e];
  const int n = t.replica_offset[e + 1] - t.replica_offset[e];
  for (int i = 0; i < n; ++i) {
    if (!b.brokerById.count(ids[i]))
      throw std::invalid_argument("replica on unknown broker " + std::to_string(ids[i]) +
                                  " (create it first: ccmi_builder_create_broker with alive = 0)");
    for (int j = 0; j < i; ++j)
      if (ids[j] == ids[i]) throw std::invalid_argument("duplicate replica broker");
  }
  const int32_t leader = t.leader_broker_id[e];
  if (n == 0 || leader < 0) return;
  int leaders = 0;
  for (int i = 0; i < n; ++i) leaders += ids[i] == leader ? 1 : 0;
  if (leaders != 1)
    throw std::invalid_argument("partition " + std::string(t.topic_names[t.partition_topic[e]]) + "-" +
                                std::to_string(t.partition_number[e]) + ": leader broker " + std::to_string(leader) +
                                " is not one of its replica brokers");
}

}  // namespace

extern "C" ccmi_status ccmi_builder_populate_from_aggregator(
    ccmi_model_builder* b, ccmi_aggregator* a, int64_t from_ms, int64_t to_ms, const ccmi_aggregation_options* options,
    const uint8_t* interested, const int32_t metric_of[6], const ccmi_partition_topology* topology,
    ccmi_aggregator_completeness* out, int64_t* num_rows, int64_t* num_populated) {
  return guarded([&] {
    if (!b || !a || !metric_of || !topology || !out || !num_rows || !num_populated)
      throw std::invalid_argument("null argument");
    ccmi::aggCheckOptions(options);
    *num_rows = *num_populated = 0;
    const auto tStart = std::chrono::steady_clock::now();
    const ccmi_partition_topology& t = *topology;
    const int E = a->cfg.num_entities, M = a->cfg.num_metrics;
    for (int m = 0; m < CCMI_NUM_METRICS; ++m)
      if (metric_of[m] < 0 || metric_of[m] >= M)
        throw std::invalid_argument("metric_of[" + std::to_string(m) + "] is not a metric of the aggregator");
    checkTopology(t, E);
    const int R = t.replica_offset[E];
    const double hostCheckMs = wallMs(tStart);

    const ccmi::DeviceGuard dg(a->device);
    const auto tAgg = std::chrono::steady_clock::now();
    ccmi::WalkResult walk;
    if (!ccmi::aggPrepareAggregate(*a, from_ms, to_ms, *options, interested, out, &walk)) return CCMI_OK;
    const int W = out->num_valid_windows;
    if (W != b->W)
      throw std::invalid_argument("the aggregate has " + std::to_string(W) + " valid windows, the builder " +
                                  std::to_string(b->W));
    const ccmi::AggDeviceRows rows =
        ccmi::aggRowsOnDevice(*a, options->include_invalid_entities ? 0 : 1, walk.validWindows,
                              options->max_allowed_extrapolations_per_entity, INT64_MAX, false);
    *num_rows = rows.covered;
    const size_t k = (size_t)rows.k;
    if (k == 0) return CCMI_OK;
    const double aggregateMs = wallMs(tAgg);
    Events ev;
    ev.record(kEvRows, a->st);

    // the topology, the builder's broker ids and the per-row scratch
    std::vector<int32_t> known;
    known.reserve(b->brokerById.size());
    for (const auto& kv : b->brokerById) known.push_back(kv.first);  // a std::map: ascending
    const size_t P = (size_t)E, B = known.size();
    int32_t *dTopic, *dNumber, *dOff, *dBroker, *dLeader, *dLogdir, *dKnown;
    uint8_t* dOffline;
    ccmi::LoadScratch S{};
    size_t inputBytes = 0;
    ccmi::carve(a->loadIn, [&](Carver& c) {
      c.take(dTopic, P);
      c.take(dNumber, P);
      c.take(dOff, P + 1);
      c.take(dBroker, (size_t)R);
      c.take(dLeader, P);
      c.take(dOffline, (size_t)R);
      c.take(dLogdir, (size_t)R);
      c.take(dKnown, B);
      inputBytes = c.off;  // what the host sends; the rest is the kernels' own
      c.take(S.kept, k);
      c.take(S.leaderIdx, k);
      c.take(S.rank, k);
      c.take(S.replicaBase, k);
      c.take(S.state, (size_t)ccmi::kLoadStateWords);
    });
    char* dIn = (char*)a->loadIn.get();
    // one copy in: the caller's arrays gathered into pinned memory in the device block's own layout
    char* hIn = (char*)a->pinUp.ensure(inputBytes);
    auto stage = [&](const void* device, const void* src, size_t bytes) {
      if (bytes) std::memcpy(hIn + ((const char*)device - dIn), src, bytes);
    };
    stage(dTopic, t.partition_topic, sizeof(int32_t) * P);
    stage(dNumber, t.partition_number, sizeof(int32_t) * P);
    stage(dOff, t.replica_offset, sizeof(int32_t) * (P + 1));
    stage(dBroker, t.replica_broker_id, sizeof(int32_t) * (size_t)R);
    stage(dLeader, t.leader_broker_id, sizeof(int32_t) * P);
    if (t.replica_offline) stage(dOffline, t.replica_offline, (size_t)R);
    if (t.replica_logdir) stage(dLogdir, t.replica_logdir, sizeof(int32_t) * (size_t)R);
    stage(dKnown, known.data(), sizeof(int32_t) * B);
    a->up(dIn, hIn, inputBytes);
    ev.record(kEvUploaded, a->st);
    const ccmi::LoadTopology T{dTopic, dNumber, dOff, dBroker, dLeader, t.replica_offline ? dOffline : nullptr,
                               t.replica_logdir ? dLogdir : nullptr, dKnown, (int32_t)B};
    ccmi::LoadRows Rw{};
    Rw.entities = rows.entities;
    Rw.values = rows.values;
    Rw.k = (long long)k;
    Rw.M = M;
    Rw.W = W;
    for (int m = 0; m < CCMI_NUM_METRICS; ++m) Rw.metricOf[m] = metric_of[m];
    ccmi::loadLaunchClassify(T, Rw, S, a->st);
    hipCheck(hipGetLastError(), "load model classify launch");
    ev.record(kEvClassified, a->st);
    unsigned long long state[ccmi::kLoadStateWords];
    a->down(state, S.state, sizeof(state));
    a->sync();
    if (state[ccmi::kLoadStateError] != ccmi::kLoadNoError) {  // nothing has been appended
      complainAbout(*b, t, (int)(state[ccmi::kLoadStateError] >> 2));
      throw std::runtime_error("the device refused partition " + std::to_string(state[ccmi::kLoadStateError] >> 2) +
                               " and the host check of it passed");
    }
    const size_t nP = (size_t)state[ccmi::kLoadStatePartitions], nR = (size_t)state[ccmi::kLoadStateReplicas];
    const size_t P0 = b->pTopic.size(), R0 = b->rBrokerId.size(), per = (size_t)CCMI_NUM_METRICS * (size_t)W;
    if (P0 + nP > (size_t)INT32_MAX || R0 + nR > (size_t)INT32_MAX)
      throw std::invalid_argument("more than 2^31 - 1 partitions or replicas in one builder");

    ccmi::LoadColumns C{};
    size_t outputBytes = 0;
    ccmi::carve(a->loadOut, [&](Carver& c) {
      c.take(C.pTopic, nP);
      c.take(C.pNumber, nP);
      c.take(C.pEnd, nP);
      c.take(C.rBroker, nR);
      c.take(C.rPartition, nR);
      c.take(C.rLeader, nR);
      c.take(C.rOffline, nR);
      c.take(C.rLogdir, nR);
      c.take(C.load, nR * per);
      outputBytes = c.off;  // what comes back; the descriptors stay on the device
      c.take(C.rDesc, nR);
    });
    char* dOut = (char*)a->loadOut.get();
    C.basePartition = (int32_t)P0;
    C.baseReplica = (int32_t)R0;
    ev.record(kEvWrite, a->st);
    ccmi::loadLaunchColumns(T, Rw, S, C, a->st);
    ev.record(kEvColumns, a->st);
    ccmi::loadLaunchLoads(Rw, C, (long long)nR, a->st);
    hipCheck(hipGetLastError(), "load model write launch");
    ev.record(kEvValues, a->st);

    // One copy out into pinned memory; the columns are appended from there. Room is made first, so that nothing is
    // appended unless everything can be; the sizes go back if anything fails all the same.
    const char* hOut = (const char*)a->pinDown.ensure(outputBytes);
    a->down((void*)hOut, dOut, outputBytes);
    ev.record(kEvCopied, a->st);
    a->sync();
    auto host = [&](const auto* device) { return (decltype(device))(hOut + ((const char*)device - dOut)); };
    auto resizeAll = [&](size_t p, size_t r) {
      b->pTopic.resize(p);
      b->pNumber.resize(p);
      b->pOff.resize(p + 1);
      b->rBrokerId.resize(r);
      b->rPartition.resize(r);
      b->rLeader.resize(r);
      b->rOffline.resize(r);
      b->rLogdir.resize(r);
      b->rLoad.resize(r * per);
    };
    auto grow = [](auto& v, size_t n) {  // room for n more, doubling so that repeated calls stay amortised
      if (v.capacity() < v.size() + n) v.reserve(std::max(v.size() + n, v.capacity() * 2));
    };
    auto append = [](auto& v, const auto* src, size_t n) { v.insert(v.end(), src, src + n); };
    const auto tAppend = std::chrono::steady_clock::now();
    try {
      grow(b->pTopic, nP);
      grow(b->pNumber, nP);
      grow(b->pOff, nP);
      grow(b->rBrokerId, nR);
      grow(b->rPartition, nR);
      grow(b->rLeader, nR);
      grow(b->rOffline, nR);
      grow(b->rLogdir, nR);
      grow(b->rLoad, nR * per);
      // topics in first-appearance order: one look at a name per topic of the topology, none per partition
      const int32_t* topicCol = host(C.pTopic);
      std::vector<int32_t> builderTopic((size_t)t.num_topics, -1);
      for (size_t p = 0; p < nP; ++p) {
        int32_t& bt = builderTopic[(size_t)topicCol[p]];
        if (bt < 0) {
          const std::string name(t.topic_names[topicCol[p]]);
          auto it = b->topicIndex.find(name);
          if (it == b->topicIndex.end()) {
            bt = (int32_t)b->topics.size();
            b->topics.push_back(name);
            b->topicIndex.emplace(name, bt);
          } else {
            bt = it->second;
          }
        }
        b->pTopic.push_back(bt);
      }
      append(b->pNumber, host(C.pNumber), nP);
      append(b->pOff, host(C.pEnd), nP);
      append(b->rBrokerId, host(C.rBroker), nR);
      append(b->rPartition, host(C.rPartition), nR);
      append(b->rLeader, host(C.rLeader), nR);
      append(b->rOffline, host(C.rOffline), nR);
      append(b->rLoad, host(C.load), nR * per);
      b->rLogdir.resize(R0 + nR);
      if (t.replica_logdir) {
        const int32_t* logdirCol = host(C.rLogdir);
        std::vector<std::string> names((size_t)t.num_logdirs);
        for (int i = 0; i < t.num_logdirs; ++i) names[(size_t)i] = t.logdir_names[i];
        for (size_t r = 0; r < nR; ++r)
          if (logdirCol[r] >= 0) b->rLogdir[R0 + r] = names[(size_t)logdirCol[r]];
      }
    } catch (...) {
      resizeAll(P0, R0);
      throw;
    }
    const double appendMs = wallMs(tAppend);
    *num_populated = (int64_t)nP;
    double* tm = a->loadTiming;
    tm[0] = aggregateMs;
    tm[1] = ev.ms(kEvRows, kEvUploaded);
    tm[2] = ev.ms(kEvUploaded, kEvClassified);
    tm[3] = ev.ms(kEvWrite, kEvColumns);
    tm[4] = ev.ms(kEvColumns, kEvValues);
    tm[5] = ev.ms(kEvValues, kEvCopied);
    tm[6] = appendMs + hostCheckMs;
    tm[7] = wallMs(tStart);
    return CCMI_OK;
  });
}

// Diagnostics, outside the ABI (include/ccmi.h does not declare it): the split of the aggregator's last
// ccmi_builder_populate_from_aggregator that populated something, in milliseconds. out[0] the aggregate on the host
// clock (walk, cover, rows enqueued); by HIP events on the aggregator's stream: out[1] the rows kernel's tail and the
// topology upload, out[2] classify and offsets, out[3] columns, out[4] the load values, out[5] the copies back; out[6]
// the host's argument checks and append; out[7] the whole call on the host clock.
extern "C" ccmi_status ccmi_load_model_timing(const ccmi_aggregator* a, double out[8]) {
  if (!a || !out) return CCMI_E_INVALID;
  std::memcpy(out, a->loadTiming, sizeof(a->loadTiming));
  return CCMI_OK;
}
