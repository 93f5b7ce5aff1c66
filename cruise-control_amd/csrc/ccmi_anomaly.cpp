// ccmi_aggregator_metric_anomalies and ccmi_slow_broker_finder_* (additive at ABI v13): the two MetricAnomalyFinders of
// MetricAnomalyDetector.run over a broker aggregator's device state (K19, kernels/anomaly.hip). Both compute the
// history rows (an aggregate, left in a.rows) and the current rows (peekCurrentWindow, left in a.rowsCurrent) through
// ccmi_aggregator_impl.h and hand them to the kernels; only the completeness, the counters and the few records come
// back. No exception of the reference is reachable on these inputs: its null checks guard maps that always exist here,
// and a percentile of 0 or 100 makes isDataSufficient false before Percentile.evaluate is reached. A translation unit
// of its own: the test emulation of Device has none of this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <vector>

#include "ccmi.h"
#include "ccmi_aggregator_impl.h"
#include "ccmi_session.h"
#include "engine/aggregator.h"
#include "engine/hip_check.h"
#include "engine/percentile.h"

static_assert(sizeof(ccmi_metric_anomaly_config) == 32 && sizeof(ccmi_metric_anomaly) == 32 &&
                  sizeof(ccmi_slow_broker_config) == 80 && sizeof(ccmi_slow_broker_summary) == 72 &&
                  sizeof(ccmi_slow_broker) == 24,
              "ccmi.h struct sizes");
static_assert(sizeof(ccmi::AnomRecord) == sizeof(ccmi_metric_anomaly) &&
                  sizeof(ccmi::AnomSlowRecord) == sizeof(ccmi_slow_broker),
              "the kernels write the records of ccmi.h");

struct ccmi_slow_broker_finder {
  ccmi_aggregator* a = nullptr;
  ccmi_slow_broker_config cfg{};
  ccmi::DevBuf state;
  ccmi::AnomScores scores{};
  size_t stateBytes = 0;
};

namespace {

using ccmi::AnomRows;
using ccmi::Carver;
using ccmi::hipCheck;

bool within(double v, double lo, double hi) { return v >= lo && v <= hi; }  // false for a NaN

struct RowSets {
  AnomRows history{nullptr, nullptr, 0, 0, 0}, current{nullptr, nullptr, 0, 0, 0};
  std::vector<long long> now;  // the current window, alive until the caller has synchronised (its upload is enqueued)
};

// The shared steps: the aggregate's rows (none when out->failure is set) and the rows of peekCurrentWindow, both left
// on the device and alive together.
RowSets twoRowSets(ccmi_aggregator& a, int64_t fromMs, int64_t toMs, const ccmi_aggregation_options& o,
                   const uint8_t* interested, ccmi_aggregator_completeness* out) {
  RowSets s;
  const int E = a.cfg.num_entities, M = a.cfg.num_metrics;
  ccmi::WalkResult walk;
  s.history.M = s.current.M = M;
  if (ccmi::aggPrepareAggregate(a, fromMs, toMs, o, interested, out, &walk)) {
    if ((int)walk.validWindows.size() > ccmi::kAnomMaxHistory) throw std::logic_error("more than 31 valid windows");
    const ccmi::AggDeviceRows d = ccmi::aggRowsOnDevice(a, o.include_invalid_entities ? 0 : 1, walk.validWindows,
                                                        o.max_allowed_extrapolations_per_entity, E, false);
    s.history = AnomRows{d.entities, d.values, d.k, M, (int32_t)walk.validWindows.size()};
  }
  s.now.assign(1, a.current);
  const ccmi::AggDeviceRows c = ccmi::aggRowsOnDevice(a, 2, s.now, 0, E, false, &a.rowsCurrent);
  s.current = AnomRows{c.entities, c.values, c.k, M, 1};
  return s;
}

void checkSlowConfig(const ccmi_slow_broker_config& c, int M) {
  // the predicates of SlowBrokerFinder.configure; a NaN fails every range
  if (!(c.bytes_in_rate_detection_threshold >= 0.0)) throw std::invalid_argument("bytes_in_rate_detection_threshold < 0");
  if (!(c.log_flush_time_threshold_ms >= 0.0)) throw std::invalid_argument("log_flush_time_threshold_ms < 0");
  if (!within(c.metric_history_percentile, 0.0, 100.0)) throw std::invalid_argument("metric_history_percentile outside [0, 100]");
  if (!(c.metric_history_margin >= 1.0)) throw std::invalid_argument("metric_history_margin < 1");
  if (!within(c.peer_metric_percentile, 0.0, 100.0)) throw std::invalid_argument("peer_metric_percentile outside [0, 100]");
  if (!(c.peer_metric_margin >= 1.0)) throw std::invalid_argument("peer_metric_margin < 1");
  if (c.demotion_score < 0) throw std::invalid_argument("demotion_score < 0");
  if (c.decommission_score < 0) throw std::invalid_argument("decommission_score < 0");
  if (!within(c.self_healing_unfixable_ratio, 0.0, 1.0)) throw std::invalid_argument("self_healing_unfixable_ratio outside [0, 1]");
  for (int m : {c.log_flush_metric, c.leader_bytes_in_metric, c.replication_bytes_in_metric})
    if (m < 0 || m >= M) throw std::invalid_argument("metric index out of range");
}

void layoutScores(ccmi_slow_broker_finder& f, Carver& c) {
  const size_t E = (size_t)f.a->cfg.num_entities;
  c.take(f.scores.since, E);
  c.take(f.scores.score, E);
  c.take(f.scores.has, E);
}

// the flagged entities of flags[E + 1] (scanned) as records, the first `capacity` of them; -> the full count
int64_t slowRecords(ccmi_slow_broker_finder& f, const uint32_t* dFlags, const uint8_t* dKind, ccmi_slow_broker* out,
                    int64_t capacity, uint32_t count) {
  ccmi_aggregator& a = *f.a;
  const int64_t k = std::min<int64_t>(capacity, (int64_t)count);
  if (k <= 0) return (int64_t)count;
  if (!out) throw std::invalid_argument("null record array with capacity > 0");
  ccmi::AnomSlowRecord* dOut = (ccmi::AnomSlowRecord*)a.anomOut.ensure(sizeof(ccmi::AnomSlowRecord) * (size_t)k);
  ccmi::anomLaunchSlowGather(dFlags, dKind, f.scores, a.cfg.num_entities, k, dOut, a.st);
  hipCheck(hipGetLastError(), "slow broker gather launch");
  a.down(out, dOut, sizeof(ccmi::AnomSlowRecord) * (size_t)k);
  a.sync();
  return (int64_t)count;
}

}  // namespace

extern "C" ccmi_status ccmi_aggregator_metric_anomalies(ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
                                                        const ccmi_aggregation_options* options,
                                                        const uint8_t* interested,
                                                        const ccmi_metric_anomaly_config* config,
                                                        const uint8_t* interested_metrics,
                                                        ccmi_aggregator_completeness* out, int64_t* current_window_index,
                                                        ccmi_metric_anomaly* anomalies, int64_t capacity,
                                                        int64_t* num_anomalies) {
  return guarded([&] {
    if (!a || !config || !interested_metrics || !out || !current_window_index || !num_anomalies)
      throw std::invalid_argument("null argument");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    ccmi::aggCheckOptions(options);
    // the ConfigDef ranges of PercentileMetricAnomalyFinderConfig
    if (!within(config->upper_percentile, 0.01, 99.99) || !within(config->lower_percentile, 0.01, 99.99))
      throw std::invalid_argument("a percentile threshold outside [0.01, 99.99]");
    if (!within(config->upper_margin, 0.0, 10.0)) throw std::invalid_argument("upper_margin outside [0, 10]");
    if (!within(config->lower_margin, 0.0, 1.0)) throw std::invalid_argument("lower_margin outside [0, 1]");
    *num_anomalies = 0;
    const ccmi::DeviceGuard dg(a->device);
    const RowSets rows = twoRowSets(*a, from_ms, to_ms, *options, interested, out);
    *current_window_index = a->current;
    if (rows.history.k == 0 || rows.current.k == 0 ||
        !ccmi::pct::isDataSufficient(rows.history.W, config->upper_percentile, config->lower_percentile)) {
      a->sync();  // the rows kernels were only enqueued
      return CCMI_OK;
    }
    const size_t E = (size_t)a->cfg.num_entities, M = (size_t)a->cfg.num_metrics;
    const long long items = rows.current.k * (long long)M;
    if (items >= INT32_MAX) throw std::invalid_argument("more than 2^31 - 1 (entity, metric) pairs");
    int32_t* dRowOf = nullptr;
    uint32_t* dFlags = nullptr;
    ccmi::AnomRecord* dStaged = nullptr;
    uint8_t* dMetrics = nullptr;
    ccmi::carve(a->anom, [&](Carver& c) {
      c.take(dRowOf, E);
      c.take(dFlags, (size_t)items + 1);
      c.take(dStaged, (size_t)items);
      c.take(dMetrics, M);
    });
    a->up(dMetrics, interested_metrics, M);
    ccmi::anomLaunchRowOf(rows.history, (int32_t)E, dRowOf, a->st);
    const ccmi::AnomPercentile p{config->upper_percentile, config->lower_percentile, config->upper_margin,
                                 config->lower_margin};
    ccmi::anomLaunchPercentile(rows.history, rows.current, dRowOf, dMetrics, p, dFlags, dStaged, a->st);
    hipCheck(hipGetLastError(), "metric anomalies launch");
    uint32_t count = 0;
    a->down(&count, dFlags + items, sizeof(count));
    a->sync();
    *num_anomalies = (int64_t)count;
    const int64_t k = std::min<int64_t>(capacity, (int64_t)count);
    if (k <= 0) return CCMI_OK;
    if (!anomalies) throw std::invalid_argument("null record array with capacity > 0");
    ccmi::AnomRecord* dOut = (ccmi::AnomRecord*)a->anomOut.ensure(sizeof(ccmi::AnomRecord) * (size_t)k);
    ccmi::anomLaunchGather(dFlags, dStaged, items, k, dOut, a->st);
    hipCheck(hipGetLastError(), "metric anomalies gather launch");
    a->down(anomalies, dOut, sizeof(ccmi::AnomRecord) * (size_t)k);
    a->sync();
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_slow_broker_finder_create(ccmi_aggregator* a, const ccmi_slow_broker_config* config,
                                                      ccmi_slow_broker_finder** out) {
  return guarded([&] {
    if (!a || !config || !out) throw std::invalid_argument("null argument");
    *out = nullptr;
    checkSlowConfig(*config, a->cfg.num_metrics);
    const ccmi::DeviceGuard dg(a->device);
    std::unique_ptr<ccmi_slow_broker_finder> f(new ccmi_slow_broker_finder);
    f->a = a;
    f->cfg = *config;
    f->stateBytes = ccmi::carve(f->state, [&](Carver& c) { layoutScores(*f, c); });
    hipCheck(hipMemsetAsync(f->state.get(), 0, f->stateBytes, a->st), "hipMemsetAsync (slow broker finder)");
    a->sync();
    *out = f.release();
    return CCMI_OK;
  });
}

extern "C" void ccmi_slow_broker_finder_destroy(ccmi_slow_broker_finder* f) {
  if (!f) return;
  try {
    const ccmi::DeviceGuard dg(f->a->device);
    delete f;
  } catch (...) {
  }
}

extern "C" ccmi_status ccmi_slow_broker_finder_detect(ccmi_slow_broker_finder* f, int64_t from_ms, int64_t to_ms,
                                                      const ccmi_aggregation_options* options,
                                                      const uint8_t* interested, int64_t time_ms,
                                                      ccmi_aggregator_completeness* out,
                                                      ccmi_slow_broker_summary* summary, ccmi_slow_broker* brokers,
                                                      int64_t capacity, int64_t* num_brokers, uint8_t* diagnostics) {
  return guarded([&] {
    if (!f || !out || !summary || !num_brokers) throw std::invalid_argument("null argument");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    if (capacity > 0 && !brokers) throw std::invalid_argument("null record array with capacity > 0");
    ccmi::aggCheckOptions(options);
    *num_brokers = 0;
    ccmi_aggregator& a = *f->a;
    const ccmi::DeviceGuard dg(a.device);
    const RowSets rows = twoRowSets(a, from_ms, to_ms, *options, interested, out);
    const size_t E = (size_t)a.cfg.num_entities, k = (size_t)rows.current.k, k1 = std::max<size_t>(k, 1);
    int32_t *dHistoryRowOf = nullptr, *dCurrentRowOf = nullptr;
    uint32_t* dFlags = nullptr;
    uint8_t *dKind = nullptr, *dDiag = nullptr;
    ccmi::AnomSlowScratch S{};
    ccmi::carve(a.anom, [&](Carver& c) {
      c.take(S.sortA, 2 * k1);
      c.take(S.sortB, 2 * k1);
      c.take(S.cur, 2 * k1);
      c.take(S.offsets, 3);
      c.take(S.base, 2);
      c.take(S.ctr, ccmi::kAnomCtrWords);
      c.take(dHistoryRowOf, E);
      c.take(dCurrentRowOf, E);
      c.take(dFlags, E + 1);
      c.take(S.historyHit, 2 * k1);
      c.take(S.skipped, k1);
      c.take(dKind, E);
      c.take(dDiag, E);
    });
    const unsigned long long offsets[3] = {0ull, (unsigned long long)k, 2ull * k};
    a.up(S.offsets, offsets, sizeof(offsets));
    const ccmi_slow_broker_config& c = f->cfg;
    const ccmi::AnomSlow p{c.bytes_in_rate_detection_threshold, c.log_flush_time_threshold_ms,
                           c.metric_history_percentile, c.metric_history_margin, c.peer_metric_percentile,
                           c.peer_metric_margin, c.demotion_score, c.decommission_score, c.log_flush_metric,
                           c.leader_bytes_in_metric, c.replication_bytes_in_metric};
    ccmi::anomLaunchRowOf(rows.history, (int32_t)E, dHistoryRowOf, a.st);
    ccmi::anomLaunchRowOf(rows.current, (int32_t)E, dCurrentRowOf, a.st);
    ccmi::anomLaunchSlowRows(rows.history, rows.current, dHistoryRowOf, p, S, a.st);
    ccmi::anomLaunchSlowUpdate(rows.current, dCurrentRowOf, (int32_t)E, p, S, f->scores, time_ms, dFlags, dKind, dDiag,
                               a.st);
    hipCheck(hipGetLastError(), "slow broker detect launch");
    unsigned long long ctr[ccmi::kAnomCtrWords];
    double base[2];
    uint32_t count = 0;
    a.down(ctr, S.ctr, sizeof(ctr));
    a.down(base, S.base, sizeof(base));
    a.down(&count, dFlags + E, sizeof(count));
    if (diagnostics) a.down(diagnostics, dDiag, E);
    a.sync();
    const int demotes = (int)ctr[ccmi::kAnDemote], removes = (int)ctr[ccmi::kAnRemove];
    *summary = ccmi_slow_broker_summary{};
    summary->current_window_index = a.current;
    summary->peer_base_log_flush = base[0];
    summary->peer_base_per_byte = base[1];
    summary->num_current = (int32_t)k;
    summary->num_skipped = (int32_t)ctr[ccmi::kAnSkipped];
    summary->num_active = (int32_t)ctr[ccmi::kAnActive];
    summary->cluster_size = (int32_t)rows.history.k;
    summary->num_persistent = removes;
    summary->num_recent = demotes;
    summary->num_suspect = (int32_t)ctr[ccmi::kAnScored] - (demotes + removes);
    summary->num_to_demote = demotes;
    summary->num_to_remove = removes;
    // numBrokersToDemoteOrRemove > clusterSize * _selfHealingUnfixableRatio (an int times a double)
    summary->unfixable = (double)(demotes + removes) > (double)summary->cluster_size * c.self_healing_unfixable_ratio;
    summary->removal_enabled = c.removal_enabled ? 1 : 0;
    *num_brokers = slowRecords(*f, dFlags, dKind, brokers, capacity, count);
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_slow_broker_finder_scores(ccmi_slow_broker_finder* f, ccmi_slow_broker* scored,
                                                      int64_t capacity, int64_t* num_scored) {
  return guarded([&] {
    if (!f || !num_scored) throw std::invalid_argument("null argument");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    *num_scored = 0;
    ccmi_aggregator& a = *f->a;
    const ccmi::DeviceGuard dg(a.device);
    const size_t E = (size_t)a.cfg.num_entities;
    uint32_t* dFlags = nullptr;
    uint8_t* dKind = nullptr;
    ccmi::carve(a.anom, [&](Carver& c) {
      c.take(dFlags, E + 1);
      c.take(dKind, E);
    });
    ccmi::anomLaunchScoreFlags(f->scores, (int32_t)E, dFlags, dKind, a.st);
    hipCheck(hipGetLastError(), "slow broker scores launch");
    uint32_t count = 0;
    a.down(&count, dFlags + E, sizeof(count));
    a.sync();
    *num_scored = slowRecords(*f, dFlags, dKind, scored, capacity, count);
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_slow_broker_finder_reset(ccmi_slow_broker_finder* f) {
  return guarded([&] {
    if (!f) throw std::invalid_argument("null finder");
    ccmi_aggregator& a = *f->a;
    const ccmi::DeviceGuard dg(a.device);
    hipCheck(hipMemsetAsync(f->state.get(), 0, f->stateBytes, a.st), "hipMemsetAsync (slow broker finder)");
    a.sync();
    return CCMI_OK;
  });
}
