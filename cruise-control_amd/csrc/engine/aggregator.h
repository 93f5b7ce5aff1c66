// The launchers of K17 (kernels/aggregator.hip) as the host side of ccmi_aggregator (ccmi_aggregator.cpp) calls them.
// Every function only enqueues on `st`; the caller synchronises and reads back. Product only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "devtypes.h"

namespace ccmi {

// The options of one completeness walk as the kernels take them.
struct AggWalkOptions {
  double minEntityRatio, minGroupRatio;
  int32_t maxExtrapolations, groupGranularity;
};

// add_samples: group the accepted samples by entity (runOff[E + 1] and cursor[E] are scratch, order[n] receives the
// batch positions grouped by entity), then replay the batch per entity.
void aggLaunchAddSamples(const AggTables& T, const int32_t* entity, const int64_t* timeMs, const double* values,
                         const uint8_t* accepted, int64_t n, const AggRollEvent* events, int numEvents,
                         long long startOldest, long long windowMs, uint32_t* runOff, uint32_t* cursor, uint32_t* order,
                         hipStream_t st);
// The walk over the windows first, first - 1, .., first - numWindows + 1 (window indices); mask may be null.
void aggLaunchWalk(const AggTables& T, const AggWalk& W, const uint8_t* mask, long long firstWindow, int numWindows,
                   const AggWalkOptions& o, hipStream_t st);
// cover[e] = W.inter[e] (source 0), W.validE[e] (1) or T.present[e] (2); counts the covered entities into
// W.ctr[kAcCovered] and, per tile, into tileOff[tiles + 1] (scanned in place).
void aggLaunchCover(const AggTables& T, const AggWalk& W, int source, uint32_t* tileOff, hipStream_t st);
// The rows of the covered entities whose rank is below capacity: windows[numWindows] are window indices, newest first.
void aggLaunchRows(const AggTables& T, const AggWalk& W, int source, const uint32_t* tileOff, const long long* windows,
                   int numWindows, long long oldest, int maxExtrapolations, int64_t capacity, int32_t* entities,
                   float* values, uint8_t* extrapolations, uint8_t* invalid, hipStream_t st);
// sums[0] = samples in the kept windows, sums[1] = present entities (sums is cleared here)
void aggLaunchStateSums(const AggTables& T, unsigned long long* sums, hipStream_t st);
// clears the state of ids[n] that are present; *removed becomes nonzero if any was (removed is cleared here)
void aggLaunchRemove(const AggTables& T, const int32_t* ids, int64_t n, uint32_t* removed, hipStream_t st);

// ---- K18 (kernels/load_model.hip): MonitorUtils.populatePartitionLoad over the rows aggLaunchRows left on the device,
// as ccmi_builder_populate_from_aggregator (ccmi_load_model.cpp) calls it. All pointers are device memory.
struct LoadTopology {  // ccmi_partition_topology, uploaded; entity e = partition e
  const int32_t* topic;          // [P]
  const int32_t* number;         // [P]
  const int32_t* replicaOffset;  // [P + 1], non-decreasing from 0, at most 8 apart (checked on the host)
  const int32_t* replicaBroker;  // [R] Kafka ids
  const int32_t* leader;         // [P] Kafka id, negative = offline partition
  const uint8_t* offline;        // [R] or null
  const int32_t* logdir;         // [R] or null
  const int32_t* knownBrokers;   // [numKnown] the builder's broker ids, ascending
  int32_t numKnown;
};
struct LoadRows {  // the aggregate's rows: entities ascending, values [k][M][W]
  const int32_t* entities;
  const float* values;
  long long k;
  int32_t M, W;
  int32_t metricOf[6];  // the aggregator metric of each ccmi_metric
};
enum : int { kLoadErrUnknownBroker = 1, kLoadErrDuplicateBroker = 2, kLoadErrLeader = 3 };
enum : int { kLoadStateError = 0, kLoadStatePartitions = 1, kLoadStateReplicas = 2, kLoadStateWords = 4 };
constexpr unsigned long long kLoadNoError = ~0ull;
struct LoadScratch {
  uint32_t* kept;             // [k] replicas of a row's partition when it is populated, else 0
  uint8_t* leaderIdx;         // [k] the leader's position among the replicas
  uint32_t* rank;             // [k] populated partitions before the row
  uint32_t* replicaBase;      // [k] their replicas
  unsigned long long* state;  // [kLoadStateWords]: (entity << 2 | code) of the lowest failing entity or kLoadNoError, the
                              // populated partitions, their replicas
};
struct LoadColumns {  // the builder's columns for this call's partitions [P'] and replicas [R'], in populate order
  int32_t *pTopic, *pNumber, *pEnd;  // topic as the topology numbers it; pEnd = baseReplica + the range's end
  int32_t *rBroker, *rPartition;     // rPartition = basePartition + rank
  uint8_t *rLeader, *rOffline;
  int32_t* rLogdir;                  // index into the topology's logdir names, -1 = none
  unsigned long long* rDesc;         // device only: row << 16 | n << 8 | leaderIdx << 4 | idx
  float* load;                       // [R'][6][W]
  int32_t basePartition, baseReplica;
};
// classify (one lane per row: broker, duplicate and leader checks, the kept replica count, the first error by an
// atomic min) and offsets (exclusive scan of the kept flags and counts); S.state is set here. Enqueues only.
void loadLaunchClassify(const LoadTopology& T, const LoadRows& R, const LoadScratch& S, hipStream_t st);
// the compacted partition and replica columns, one lane per row
void loadLaunchColumns(const LoadTopology& T, const LoadRows& R, const LoadScratch& S, const LoadColumns& C,
                       hipStream_t st);
// C.load through engine/replica_load.h, tiles of whole replicas staged in LDS; numReplicas = state[kLoadStateReplicas]
void loadLaunchLoads(const LoadRows& R, const LoadColumns& C, long long numReplicas, hipStream_t st);

// ---- K19 (kernels/anomaly.hip): the metric anomaly finders over two row sets aggLaunchRows left on the device, as
// ccmi_aggregator_metric_anomalies and ccmi_slow_broker_finder_detect (ccmi_anomaly.cpp) call them. All pointers are
// device memory; the percentile is engine/percentile.h.
struct AnomRows {  // entities ascending, values [k][M][W] (W = 1 for the current rows); k = 0 leaves the pointers unread
  const int32_t* entities;
  const float* values;
  long long k;
  int32_t M, W;
};
struct AnomRecord {  // ccmi_metric_anomaly
  int32_t entity, metric;
  double current, upper, lower;
};
struct AnomPercentile {  // ccmi_metric_anomaly_config
  double upper, lower, upperMargin, lowerMargin;
};
struct AnomSlow {  // ccmi_slow_broker_config as the kernels take it
  double bytesThreshold, flushThreshold, historyPercentile, historyMargin, peerPercentile, peerMargin;
  int32_t demotion, decommission, mFlush, mIn, mRepl;
};
struct AnomSlowRecord {  // ccmi_slow_broker
  int32_t entity, kind, score, reserved;
  long long since;
};
struct AnomSlowScratch {  // one round's per-row scratch over the k current rows
  double* cur;              // [2][k] the current log flush time and per-byte log flush time
  uint8_t* historyHit;      // [2][k]
  uint8_t* skipped;         // [k]
  SortEntry* sortA;         // [2][k] {lo = row, hi = ordered key of cur}; a skipped row and a NaN sort last
  SortEntry* sortB;         // [2][k] the merge passes' other buffer
  unsigned long long* offsets;  // [3] = {0, k, 2k}
  double* base;             // [2] the peer bases (NaN when not evaluated)
  unsigned long long* ctr;  // [kAnomCtrWords]
};
struct AnomScores {  // the finder's state
  int32_t* score;    // [E]
  long long* since;  // [E]
  uint8_t* has;      // [E] a key of _brokerSlownessScore and of _detectedSlowBrokers
};
// rowOf[E] = the row of each entity in `rows`, -1 for none
void anomLaunchRowOf(const AnomRows& rows, int32_t E, int32_t* rowOf, hipStream_t st);
// The percentile finder: one lane per (current row, metric) writes flags[item] and staged[item]; flags is scanned in
// place afterwards (flags[items] = the count).
void anomLaunchPercentile(const AnomRows& history, const AnomRows& current, const int32_t* historyRowOf,
                          const uint8_t* interestedMetrics, const AnomPercentile& p, uint32_t* flags, AnomRecord* staged,
                          hipStream_t st);
// out[rank] = staged[item] for the flagged items whose rank is below capacity
void anomLaunchGather(const uint32_t* flags, const AnomRecord* staged, long long items, long long capacity,
                      AnomRecord* out, hipStream_t st);
// The slow broker finder's round up to the peer bases: per-row currents, filtered history hits, the sort of the active
// currents and the two bases. S.ctr is cleared here.
void anomLaunchSlowRows(const AnomRows& history, const AnomRows& current, const int32_t* historyRowOf,
                        const AnomSlow& p, const AnomSlowScratch& S, hipStream_t st);
// updateBrokerSlownessScore and createSlowBrokerAnomalies, one lane per entity: flags[e] = 1 for a reported broker
// (scanned in place afterwards, flags[E] = the count), kind[e], diag[e], the counters.
void anomLaunchSlowUpdate(const AnomRows& current, const int32_t* currentRowOf, int32_t E, const AnomSlow& p,
                          const AnomSlowScratch& S, const AnomScores& scores, long long timeMs, uint32_t* flags,
                          uint8_t* kind, uint8_t* diag, hipStream_t st);
// flags[e] = has[e], scanned in place (flags[E] = the count); kind[e] = 0
void anomLaunchScoreFlags(const AnomScores& scores, int32_t E, uint32_t* flags, uint8_t* kind, hipStream_t st);
// out[rank] = {e, kind[e], score[e], since[e]} for the flagged entities whose rank is below capacity
void anomLaunchSlowGather(const uint32_t* flags, const uint8_t* kind, const AnomScores& scores, int32_t E,
                          long long capacity, AnomSlowRecord* out, hipStream_t st);

}  // namespace ccmi
