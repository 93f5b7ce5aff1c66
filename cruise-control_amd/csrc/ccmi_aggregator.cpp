// ccmi_aggregator (additive at ABI v13): MetricSampleAggregator on the device (K17, kernels/aggregator.hip). An
// aggregator owns its buffers and its stream on one device and needs no session. The host keeps what depends on the
// timestamps alone: the aggregator's window indices and generation, and per batch the accepted flags and the roll-out
// events (MetricSampleAggregator.addSample / maybeRollOutNewWindow); everything per entity, per group and per window
// runs on the device. A translation unit of its own: the test emulation of Device has none of this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ccmi.h"
#include "ccmi_aggregator_impl.h"
#include "ccmi_session.h"
#include "engine/aggregator.h"
#include "engine/aggregator_entity.h"
#include "engine/hip_check.h"

static_assert(sizeof(ccmi_aggregator_config) == 32 && sizeof(ccmi_aggregator_state) == 48 &&
                  sizeof(ccmi_aggregation_options) == 32 && sizeof(ccmi_aggregator_completeness) == 96,
              "ccmi.h struct sizes");

namespace {

using ccmi::AggDeviceRows;
using ccmi::Carver;
using ccmi::hipCheck;
using ccmi::WalkResult;

const float kJavaNaN = [] {  // Float.NaN, the result of Java's 0f / 0
  const uint32_t bits = 0x7fc00000u;
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}();

float ratio(unsigned long long n, unsigned long long total) {  // (float) n / total
  if (total == 0) return n == 0 ? kJavaNaN : 1.0f / 0.0f;
  return (float)n / (float)total;
}

// timeMs / _windowMs + 1 in Java's wrapping long arithmetic
long long windowIndexOf(long long timeMs, long long windowMs) {
  return (long long)((unsigned long long)(timeMs / windowMs) + 1ull);
}

void layoutState(ccmi_aggregator& a, Carver& c, int32_t*& group, uint8_t*& fn) {
  const size_t E = a.cfg.num_entities, M = a.cfg.num_metrics, L = a.L();
  c.take(a.T.counts, L * E);
  c.take(a.T.values, L * M * E);
  c.take(a.T.valid, E);
  c.take(a.T.extrap, E);
  c.take(a.T.present, E);
  c.take(group, E);
  c.take(fn, M);
}

void layoutWalk(ccmi_aggregator& a, Carver& c) {
  const size_t E = a.cfg.num_entities, G = a.cfg.num_groups, L = a.L();
  c.take(a.W.inter, E);
  c.take(a.W.ginter, G);
  c.take(a.W.validE, E);
  c.take(a.W.validG, G);
  c.take(a.W.vfw, E);
  c.take(a.W.gValidW, G);
  c.take(a.W.extrapCnt, E);
  c.take(a.W.gValidCnt, L * G);
  c.take(a.W.gInvalid, L * G);
  c.take(a.W.ctr, ccmi::kAggCtrHead + L * ccmi::kAggCtrPerWindow);
}

void layoutSmall(ccmi_aggregator& a, Carver& c) {
  const size_t E = a.cfg.num_entities, L = a.L();
  c.take(a.S.mask, E);
  c.take(a.S.sums, 2);
  c.take(a.S.tileOff, (E + ccmi::kAggTile - 1) / ccmi::kAggTile + 1);
  c.take(a.S.windows, L);
}

void checkOptions(const ccmi_aggregation_options* o) {
  if (!o) throw std::invalid_argument("null options");
  if (o->min_valid_windows < 1) throw std::invalid_argument("The minimum valid windows must be at least 1");
  if (o->granularity != CCMI_GRANULARITY_ENTITY && o->granularity != CCMI_GRANULARITY_ENTITY_GROUP)
    throw std::invalid_argument("unknown granularity");
}

// MetricSampleAggregator.completeness: clamps the range, runs the walk, fills `out` (and the two masks when given).
WalkResult runCompleteness(ccmi_aggregator& a, int64_t fromMs, int64_t toMs, const ccmi_aggregation_options& o,
                           const uint8_t* interested, ccmi_aggregator_completeness* out, uint8_t* validEntities,
                           uint8_t* validGroups) {
  WalkResult r;
  const int E = a.cfg.num_entities, G = a.cfg.num_groups;
  const long long fromW = std::max(windowIndexOf(fromMs, a.cfg.window_ms), a.oldest);
  const long long toW = std::min(windowIndexOf(toMs, a.cfg.window_ms), a.current - 1);
  out->generation = a.generation;
  out->num_windows = out->num_valid_windows = 0;
  out->failure = CCMI_AGG_FAILURE_NONE;
  out->num_interested_entities = out->num_interested_groups = out->num_valid_entities = out->num_valid_groups = 0;
  out->valid_entity_ratio = out->valid_entity_group_ratio = 0.0f;
  if (fromW > a.current || toW < a.oldest) {  // new MetricSampleCompleteness<>(generation(), _windowMs)
    if (validEntities) std::memset(validEntities, 0, (size_t)E);
    if (validGroups) std::memset(validGroups, 0, (size_t)G);
    return r;
  }
  r.inRange = true;
  r.numWindows = (int)std::max<long long>(0, toW - fromW + 1);
  r.firstWindow = toW;
  if (r.numWindows > out->window_capacity) throw std::invalid_argument("window_capacity is smaller than the range");
  if (r.numWindows > 0 && (!out->window_index || !out->window_included || !out->valid_entity_ratio_by_window ||
                           !out->valid_entity_ratio_with_group_granularity_by_window ||
                           !out->valid_entity_group_ratio_by_window || !out->extrapolated_entity_ratio_by_window))
    throw std::invalid_argument("null per-window array in the completeness struct");
  // an empty interested set means every entity with raw metrics (interpretAggregationOptions)
  bool any = false;
  if (interested)
    for (int e = 0; e < E && !any; ++e) any = interested[e] != 0;
  uint8_t* dMask = any ? a.S.mask : nullptr;
  if (any) a.up(dMask, interested, (size_t)E);
  ccmi::AggWalkOptions wo{o.min_valid_entity_ratio, o.min_valid_entity_group_ratio,
                          o.max_allowed_extrapolations_per_entity, o.granularity == CCMI_GRANULARITY_ENTITY_GROUP};
  ccmi::aggLaunchWalk(a.T, a.W, dMask, r.firstWindow, r.numWindows, wo, a.st);
  r.ctr.resize(ccmi::kAggCtrHead + (size_t)std::max(r.numWindows, 1) * ccmi::kAggCtrPerWindow);
  a.down(r.ctr.data(), a.W.ctr, r.ctr.size() * sizeof(unsigned long long));
  if (validEntities) a.down(validEntities, a.W.validE, (size_t)E);
  if (validGroups) a.down(validGroups, a.W.validG, (size_t)G);
  a.sync();
  const unsigned long long totalE = r.ctr[ccmi::kAcTotalE], totalG = r.ctr[ccmi::kAcTotalG];
  out->num_windows = r.numWindows;
  out->num_interested_entities = (int32_t)totalE;
  out->num_interested_groups = (int32_t)totalG;
  for (int j = 0; j < r.numWindows; ++j) {
    const unsigned long long* c = &r.ctr[ccmi::kAggCtrHead + (size_t)j * ccmi::kAggCtrPerWindow];
    out->window_index[j] = r.firstWindow - j;
    out->window_included[j] = c[ccmi::kAwIncluded] ? 1 : 0;
    out->valid_entity_ratio_by_window[j] = ratio(c[ccmi::kAwValid], totalE);
    out->valid_entity_ratio_with_group_granularity_by_window[j] = ratio(c[ccmi::kAwGroupGran], totalE);
    out->extrapolated_entity_ratio_by_window[j] = ratio(c[ccmi::kAwExtrap], totalE);
    out->valid_entity_group_ratio_by_window[j] = ratio(c[ccmi::kAwGroups], totalG);
    if (c[ccmi::kAwIncluded]) r.validWindows.push_back(r.firstWindow - j);
  }
  out->num_valid_windows = (int32_t)r.validWindows.size();
  out->num_valid_entities = (int32_t)r.ctr[ccmi::kAcValidE];
  out->num_valid_groups = (int32_t)r.ctr[ccmi::kAcValidG];
  out->valid_entity_ratio = ratio(r.ctr[ccmi::kAcValidE], totalE);
  out->valid_entity_group_ratio = ratio(r.ctr[ccmi::kAcValidG], totalG);
  return r;
}

// ccmi_aggregator_impl.h's aggRowsOnDevice, then the rows copied into the caller's arrays.
int64_t runRows(ccmi_aggregator& a, int source, const std::vector<long long>& windows, int maxExtrapolations,
                int64_t capacity, int32_t* entities, float* values, uint8_t* extrapolations, uint8_t* invalid) {
  const int M = a.cfg.num_metrics, Wv = (int)windows.size();
  const AggDeviceRows d = ccmi::aggRowsOnDevice(a, source, windows, maxExtrapolations, capacity, invalid != nullptr);
  const int64_t k = d.k;
  if (k <= 0) return d.covered;
  if (!entities || !values || !extrapolations) throw std::invalid_argument("null row array with capacity > 0");
  a.down(entities, d.entities, sizeof(int32_t) * (size_t)k);
  a.down(values, d.values, sizeof(float) * (size_t)k * M * Wv);
  a.down(extrapolations, d.extrapolations, (size_t)k * Wv);
  if (invalid) a.down(invalid, d.invalid, (size_t)k);
  a.sync();
  return d.covered;
}

}  // namespace

namespace ccmi {

AggDeviceRows aggRowsOnDevice(ccmi_aggregator& a, int source, const std::vector<long long>& windows,
                              int maxExtrapolations, int64_t capacity, bool wantInvalid, DevBuf* target) {
  const int M = a.cfg.num_metrics, Wv = (int)windows.size();
  if (Wv > a.L()) throw std::logic_error("more windows than the aggregator keeps");
  ccmi::aggLaunchCover(a.T, a.W, source, a.S.tileOff, a.st);
  unsigned long long covered = 0;
  a.down(&covered, a.W.ctr + ccmi::kAcCovered, sizeof(covered));
  a.sync();
  AggDeviceRows d;
  d.covered = (int64_t)covered;
  const int64_t k = std::min<int64_t>(capacity, (int64_t)covered);
  if (k <= 0) return d;
  d.k = k;
  ccmi::carve(target ? *target : a.rows, [&](Carver& c) {
    c.take(d.entities, (size_t)k);
    c.take(d.values, (size_t)k * M * Wv);
    c.take(d.extrapolations, (size_t)k * Wv);
    c.take(d.invalid, (size_t)k);
  });
  a.up(a.S.windows, windows.data(), sizeof(long long) * (size_t)Wv);
  ccmi::aggLaunchRows(a.T, a.W, source, a.S.tileOff, a.S.windows, Wv, a.oldest, maxExtrapolations, k, d.entities,
                      d.values, d.extrapolations, wantInvalid ? d.invalid : nullptr, a.st);
  return d;
}

bool aggPrepareAggregate(ccmi_aggregator& a, int64_t fromMs, int64_t toMs, const ccmi_aggregation_options& o,
                         const uint8_t* interested, ccmi_aggregator_completeness* out, WalkResult* walk) {
  *walk = runCompleteness(a, fromMs, toMs, o, interested, out, nullptr, nullptr);
  if (!walk->inRange) {
    out->failure = CCMI_AGG_FAILURE_NO_WINDOW_IN_RANGE;
    return false;
  }
  // validateCompleteness
  if (out->num_valid_windows < o.min_valid_windows) {
    out->failure = CCMI_AGG_FAILURE_NOT_ENOUGH_VALID_WINDOWS;
    return false;
  }
  char msg[256];
  if ((double)out->valid_entity_ratio < o.min_valid_entity_ratio) {
    std::snprintf(msg, sizeof(msg), "The entity coverage %.3f in range [%lld, %lld] does not meet requirement.",
                  (double)out->valid_entity_ratio, (long long)fromMs, (long long)toMs);
    throw ccmi::StateError(msg);
  }
  if ((double)out->valid_entity_group_ratio < o.min_valid_entity_group_ratio) {
    std::snprintf(msg, sizeof(msg), "The entity group coverage %.3f in range [%lld, %lld] does not meet requirement.",
                  (double)out->valid_entity_group_ratio, (long long)fromMs, (long long)toMs);
    throw ccmi::StateError(msg);
  }
  return true;
}

void aggCheckOptions(const ccmi_aggregation_options* o) { checkOptions(o); }

}  // namespace ccmi

extern "C" ccmi_status ccmi_aggregator_create(int32_t device_ordinal, const ccmi_aggregator_config* config,
                                              const uint8_t* metric_function, const int32_t* entity_group,
                                              ccmi_aggregator** out) {
  return guarded([&] {
    if (!config || !metric_function || !entity_group || !out) throw std::invalid_argument("null argument");
    *out = nullptr;
    if (config->num_windows < 1 || config->num_windows + 1 > ccmi::agg::kMaxKeep)
      throw std::invalid_argument("num_windows must be 1..31");
    if (config->window_ms < 1) throw std::invalid_argument("window_ms < 1");
    if (config->min_samples_per_window < 1 || config->min_samples_per_window > 127)
      throw std::invalid_argument("min_samples_per_window must be 1..127");
    if (config->num_metrics < 1 || config->num_entities < 1 || config->num_groups < 1)
      throw std::invalid_argument("num_metrics, num_entities and num_groups must be at least 1");
    for (int m = 0; m < config->num_metrics; ++m)
      if (metric_function[m] > CCMI_AGG_LATEST) throw std::invalid_argument("unknown aggregation function");
    for (int e = 0; e < config->num_entities; ++e)
      if (entity_group[e] < 0 || entity_group[e] >= config->num_groups)
        throw std::invalid_argument("entity group out of range");
    int count = 0;
    hipCheck(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (device_ordinal < 0 || device_ordinal >= count) throw std::invalid_argument("device ordinal out of range");
    const ccmi::DeviceGuard dg(device_ordinal);
    std::unique_ptr<ccmi_aggregator> a(new ccmi_aggregator);
    a->device = device_ordinal;
    a->cfg = *config;
    hipCheck(hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking), "hipStreamCreate (aggregator)");
    int32_t* dGroup = nullptr;
    uint8_t* dFn = nullptr;
    const size_t bytes = ccmi::carve(a->state, [&](Carver& c) { layoutState(*a, c, dGroup, dFn); });
    hipCheck(hipMemsetAsync(a->state.get(), 0, bytes, a->st), "hipMemsetAsync (aggregator)");
    a->up(dGroup, entity_group, sizeof(int32_t) * (size_t)config->num_entities);
    a->up(dFn, metric_function, (size_t)config->num_metrics);
    a->T.group = dGroup;
    a->T.fn = dFn;
    a->T.E = config->num_entities;
    a->T.G = config->num_groups;
    a->T.M = config->num_metrics;
    a->T.L = a->L();
    a->T.minSamples = config->min_samples_per_window;
    a->T.halfMin = ccmi::agg::halfMinRequired(config->min_samples_per_window);
    ccmi::carve(a->walk, [&](Carver& c) { layoutWalk(*a, c); });
    ccmi::carve(a->small, [&](Carver& c) { layoutSmall(*a, c); });
    a->sync();
    *out = a.release();
    return CCMI_OK;
  });
}

extern "C" void ccmi_aggregator_destroy(ccmi_aggregator* a) {
  if (!a) return;
  try {
    const ccmi::DeviceGuard dg(a->device);
    delete a;
  } catch (...) {
  }
}

namespace ccmi {

// The host prologue of add_samples: MetricSampleAggregator.addSample over the timestamps alone gives the accepted
// flags, the roll-outs and the generation. timeMs == nullptr: every sample has the time `sameTimeMs`.
AggAddPlan aggPlanAddSamples(const ccmi_aggregator& a, const int64_t* timeMs, int64_t sameTimeMs, int64_t n) {
  AggAddPlan plan;
  plan.acc.resize((size_t)n);
  plan.cur = a.current;
  plan.oldest = a.oldest;
  plan.gen = a.generation;
  for (int64_t i = 0; i < n; ++i) {
    const long long w = windowIndexOf(timeMs ? timeMs[i] : sameTimeMs, a.cfg.window_ms);
    if (w < plan.oldest) {
      plan.acc[(size_t)i] = 0;
      continue;
    }
    bool rolled = false;
    if (plan.cur < w) {  // maybeRollOutNewWindow
      const long long prevOldest = plan.oldest;
      plan.oldest = std::max<long long>(1, w - a.cfg.num_windows);
      const long long numReset = std::min<long long>(a.L(), plan.oldest - prevOldest);
      if (numReset > 0) plan.events.push_back(ccmi::AggRollEvent{i, plan.oldest, prevOldest, (int32_t)numReset, 0});
      plan.cur = w;
      rolled = true;
    }
    if (rolled || w != plan.cur) plan.gen++;
    plan.acc[(size_t)i] = 1;
    plan.numAccepted++;
  }
  return plan;
}

void AggAddScratch::layout(Carver& c, size_t n, size_t E, size_t numEvents) {
  c.take(acc, n);
  c.take(ord, n);
  c.take(run, E + 1);
  c.take(cur, E);
  c.take(ev, numEvents);
}

// The device body of add_samples over samples that are on the device already; synchronises and commits the plan.
void aggAddSamplesOnDevice(ccmi_aggregator& a, const AggAddPlan& plan, const AggAddScratch& s, const int32_t* dEntity,
                           const int64_t* dTime, const double* dValues, int64_t n) {
  a.up(s.acc, plan.acc.data(), (size_t)n);
  a.up(s.ev, plan.events.data(), sizeof(ccmi::AggRollEvent) * plan.events.size());
  ccmi::aggLaunchAddSamples(a.T, dEntity, dTime, dValues, s.acc, n, s.ev, (int)plan.events.size(), a.oldest,
                            a.cfg.window_ms, s.run, s.cur, s.ord, a.st);
  hipCheck(hipGetLastError(), "add_samples launch");
  a.sync();
  a.current = plan.cur;
  a.oldest = plan.oldest;
  a.generation = plan.gen;
}

}  // namespace ccmi

extern "C" ccmi_status ccmi_aggregator_add_samples(ccmi_aggregator* a, const int32_t* entity, const int64_t* time_ms,
                                                   const double* values, int64_t n, uint8_t* accepted,
                                                   int64_t* num_accepted) {
  return guarded([&] {
    if (!a) throw std::invalid_argument("null aggregator");
    if (n < 0) throw std::invalid_argument("n < 0");
    if (n > INT32_MAX) throw std::invalid_argument("more than 2^31 - 1 samples in one batch");
    if (num_accepted) *num_accepted = 0;
    if (n == 0) return CCMI_OK;
    if (!entity || !time_ms || !values) throw std::invalid_argument("null sample array");
    for (int64_t i = 0; i < n; ++i) {
      if (entity[i] < 0 || entity[i] >= a->cfg.num_entities) throw std::invalid_argument("entity id out of range");
      if (time_ms[i] < 0) throw std::invalid_argument("negative sample time");
    }
    const ccmi::AggAddPlan plan = ccmi::aggPlanAddSamples(*a, time_ms, 0, n);
    const ccmi::DeviceGuard dg(a->device);
    const size_t E = (size_t)a->cfg.num_entities, M = (size_t)a->cfg.num_metrics, N = (size_t)n;
    int32_t* dEnt;
    int64_t* dTime;
    double* dVal;
    ccmi::AggAddScratch scratch;
    ccmi::carve(a->batch, [&](Carver& c) {
      c.take(dEnt, N);
      c.take(dTime, N);
      c.take(dVal, N * M);
      scratch.layout(c, N, E, plan.events.size());
    });
    a->up(dEnt, entity, 4 * N);
    a->up(dTime, time_ms, 8 * N);
    a->up(dVal, values, 8 * N * M);
    ccmi::aggAddSamplesOnDevice(*a, plan, scratch, dEnt, dTime, dVal, n);
    if (accepted) std::memcpy(accepted, plan.acc.data(), N);
    if (num_accepted) *num_accepted = plan.numAccepted;
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_aggregator_state_query(ccmi_aggregator* a, ccmi_aggregator_state* out) {
  return guarded([&] {
    if (!a || !out) throw std::invalid_argument("null argument");
    const ccmi::DeviceGuard dg(a->device);
    ccmi::aggLaunchStateSums(a->T, a->S.sums, a->st);
    unsigned long long sums[2] = {0, 0};
    a->down(sums, a->S.sums, sizeof(sums));
    a->sync();
    *out = ccmi_aggregator_state{};
    out->generation = a->generation;
    out->oldest_window_index = a->oldest;
    out->current_window_index = a->current;
    out->num_samples = (int64_t)sums[0];
    out->num_present_entities = (int64_t)sums[1];
    // numAvailableWindows(-1, Long.MAX_VALUE)
    const long long fromW = std::max(windowIndexOf(-1, a->cfg.window_ms), a->oldest);
    const long long toW = std::min(windowIndexOf(INT64_MAX, a->cfg.window_ms), a->current - 1);
    out->num_available_windows = (int32_t)std::max<long long>(0, toW - fromW + 1);
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_aggregator_completeness_query(ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
                                                          const ccmi_aggregation_options* options,
                                                          const uint8_t* interested, ccmi_aggregator_completeness* out,
                                                          uint8_t* valid_entities, uint8_t* valid_groups) {
  return guarded([&] {
    if (!a || !out) throw std::invalid_argument("null argument");
    checkOptions(options);
    const ccmi::DeviceGuard dg(a->device);
    runCompleteness(*a, from_ms, to_ms, *options, interested, out, valid_entities, valid_groups);
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_aggregator_aggregate(ccmi_aggregator* a, int64_t from_ms, int64_t to_ms,
                                                 const ccmi_aggregation_options* options, const uint8_t* interested,
                                                 ccmi_aggregator_completeness* out, int32_t* entities, float* values,
                                                 uint8_t* extrapolations, uint8_t* invalid, int64_t capacity,
                                                 int64_t* num_entities) {
  return guarded([&] {
    if (!a || !out || !num_entities) throw std::invalid_argument("null argument");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    checkOptions(options);
    *num_entities = 0;
    const ccmi::DeviceGuard dg(a->device);
    WalkResult r;
    if (!ccmi::aggPrepareAggregate(*a, from_ms, to_ms, *options, interested, out, &r)) return CCMI_OK;
    *num_entities = runRows(*a, options->include_invalid_entities ? 0 : 1, r.validWindows,
                            options->max_allowed_extrapolations_per_entity, capacity, entities, values, extrapolations,
                            invalid);
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_aggregator_peek_current_window(ccmi_aggregator* a, int32_t* entities, float* values,
                                                           uint8_t* extrapolations, int64_t capacity,
                                                           int64_t* num_entities) {
  return guarded([&] {
    if (!a || !num_entities) throw std::invalid_argument("null argument");
    if (capacity < 0) throw std::invalid_argument("capacity < 0");
    const ccmi::DeviceGuard dg(a->device);
    *num_entities = runRows(*a, 2, std::vector<long long>{a->current}, 0, capacity, entities, values, extrapolations,
                            nullptr);
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_aggregator_remove_entities(ccmi_aggregator* a, const int32_t* entities, int64_t n) {
  return guarded([&] {
    if (!a) throw std::invalid_argument("null aggregator");
    if (n < 0) throw std::invalid_argument("n < 0");
    if (n == 0) return CCMI_OK;
    if (!entities) throw std::invalid_argument("null entities");
    for (int64_t i = 0; i < n; ++i)
      if (entities[i] < 0 || entities[i] >= a->cfg.num_entities) throw std::invalid_argument("entity id out of range");
    const ccmi::DeviceGuard dg(a->device);
    int32_t* dIds;
    uint32_t* dRemoved;
    ccmi::carve(a->batch, [&](Carver& c) {
      c.take(dIds, (size_t)n);
      c.take(dRemoved, 1);
    });
    a->up(dIds, entities, 4 * (size_t)n);
    ccmi::aggLaunchRemove(a->T, dIds, n, dRemoved, a->st);
    uint32_t removed = 0;
    a->down(&removed, dRemoved, sizeof(removed));
    a->sync();
    if (removed) a->generation++;
    return CCMI_OK;
  });
}

extern "C" ccmi_status ccmi_aggregator_clear(ccmi_aggregator* a) {
  return guarded([&] {
    if (!a) throw std::invalid_argument("null aggregator");
    const ccmi::DeviceGuard dg(a->device);
    const size_t E = (size_t)a->cfg.num_entities;
    hipCheck(hipMemsetAsync(a->T.counts, 0, (size_t)a->L() * E, a->st), "hipMemsetAsync (aggregator)");
    hipCheck(hipMemsetAsync(a->T.valid, 0, sizeof(uint32_t) * E, a->st), "hipMemsetAsync (aggregator)");
    hipCheck(hipMemsetAsync(a->T.extrap, 0, sizeof(uint32_t) * E, a->st), "hipMemsetAsync (aggregator)");
    hipCheck(hipMemsetAsync(a->T.present, 0, E, a->st), "hipMemsetAsync (aggregator)");
    a->sync();
    a->generation++;
    return CCMI_OK;
  });
}
