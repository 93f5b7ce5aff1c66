// What the translation units behind ccmi_aggregator share (ccmi_aggregator.cpp, ccmi_load_model.cpp, ccmi_anomaly.cpp):
// the aggregator object and the two steps of an aggregate that leave their result on the device. Its buffers are the
// DevBuf / PinBuf of engine/devbuf.h, laid out with its Carver. Private to the library; include/ccmi.h only names the
// struct.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ccmi.h"
#include "engine/aggregator.h"
#include "engine/devbuf.h"
#include "engine/hip_check.h"

namespace ccmi {

// The pieces of ccmi_aggregator::small, every size fixed by the config (layoutSmall, ccmi_aggregator.cpp): what the
// host hands a kernel beside the tables and the walk's scratch.
struct AggSmall {
  uint8_t* mask;             // [E] the interested mask of a walk
  unsigned long long* sums;  // [2] ccmi_aggregator_state_query's sums
  uint32_t* tileOff;         // [tiles + 1] the cover pass's tile offsets
  long long* windows;        // [L] the window list of a rows pass: at most L windows can be valid
};

}  // namespace ccmi

struct ccmi_aggregator {
  int device = 0;
  hipStream_t st = nullptr;
  ccmi_aggregator_config cfg{};
  ccmi::AggTables T{};
  ccmi::AggWalk W{};
  long long current = 0, oldest = 0, generation = 0;  // _currentWindowIndex, _oldestWindowIndex, _generation
  ccmi::AggSmall S{};
  ccmi::DevBuf state, walk, small;  // fixed by the config: allocated once, at create
  ccmi::DevBuf batch, rows;         // grow with the batch and with the rows of an aggregate
  ccmi::PinBuf pinUp, pinDown;  // K18: pinned staging of the topology going up and of the columns coming down
  ccmi::DevBuf loadIn, loadOut;  // K18 (ccmi_load_model.cpp): the uploaded topology and per-row scratch, the builder columns
  double loadTiming[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the last bulk load's split (ccmi_load_model_timing)
  ccmi::DevBuf rowsCurrent, anom, anomOut;  // K19 (ccmi_anomaly.cpp): the current rows beside a.rows, the scratch, the records

  ~ccmi_aggregator() {
    if (st) (void)hipStreamDestroy(st);
  }
  int L() const { return cfg.num_windows + 1; }
  void sync() { ccmi::hipCheck(hipStreamSynchronize(st), "hipStreamSynchronize (aggregator)"); }
  void up(void* dst, const void* src, size_t bytes) {
    if (bytes) ccmi::hipCheck(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync (aggregator, up)");
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (bytes) ccmi::hipCheck(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (aggregator, down)");
  }
};

namespace ccmi {

// What a walk left on the device, read back once.
struct WalkResult {
  bool inRange = false;
  int numWindows = 0;
  long long firstWindow = 0;
  std::vector<unsigned long long> ctr;
  std::vector<long long> validWindows;  // newest first
};

// The rows of an aggregate as agg_rows left them in a.rows or the caller's buffer (valid until the aggregator's next call).
struct AggDeviceRows {
  int64_t covered = 0, k = 0;  // the covered entities and how many of them have a row: min(capacity, covered)
  int32_t* entities = nullptr;
  float* values = nullptr;  // [k][M][Wv]
  uint8_t *extrapolations = nullptr, *invalid = nullptr;
};

// ccmi_aggregator_add_samples in two steps, so that samples a kernel left on the device (K20's process_into) take the
// same path as a host batch: the host prologue over the timestamps, then the device body over device pointers.
struct AggAddPlan {
  std::vector<uint8_t> acc;          // accepted flag per sample
  std::vector<AggRollEvent> events;  // the roll-outs, by sample position
  long long cur = 0, oldest = 0, gen = 0;  // the aggregator's counters after the batch
  int64_t numAccepted = 0;
};
struct AggAddScratch {  // pieces of a.batch
  uint8_t* acc = nullptr;
  uint32_t *ord = nullptr, *run = nullptr, *cur = nullptr;
  AggRollEvent* ev = nullptr;
  void layout(Carver& c, size_t n, size_t E, size_t numEvents);
};
AggAddPlan aggPlanAddSamples(const ccmi_aggregator& a, const int64_t* timeMs, int64_t sameTimeMs, int64_t n);
void aggAddSamplesOnDevice(ccmi_aggregator& a, const AggAddPlan& plan, const AggAddScratch& s, const int32_t* dEntity,
                           const int64_t* dTime, const double* dValues, int64_t n);

// checkOptions of the aggregator's calls: std::invalid_argument for a null or malformed options struct
void aggCheckOptions(const ccmi_aggregation_options* o);
// ccmi_aggregator_aggregate up to validateCompleteness: fills `out`; false when out->failure is set (no rows).
bool aggPrepareAggregate(ccmi_aggregator& a, int64_t fromMs, int64_t toMs, const ccmi_aggregation_options& o,
                         const uint8_t* interested, ccmi_aggregator_completeness* out, WalkResult* walk);
// Compacts the covered entities (source: 0 interested, 1 valid, 2 present) and writes the rows below `capacity` into
// a.rows, or into `target` when one is given (K19 keeps two row sets alive). Synchronises once (the covered count); the
// rows kernel is only enqueued.
AggDeviceRows aggRowsOnDevice(ccmi_aggregator& a, int source, const std::vector<long long>& windows,
                              int maxExtrapolations, int64_t capacity, bool wantInvalid, DevBuf* target = nullptr);

}  // namespace ccmi
